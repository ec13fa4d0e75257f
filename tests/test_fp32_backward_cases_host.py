"""CPU: the table of tests/fp32_backward_cases.py against the library's host-side plan query and against the oracle alone.
deepim_conv_wgrad_plan (no context, no device) pins which kernel family, slice plan and reduce pass each row reaches; together the rows
meet every branch of the slice arithmetic, and every branch signature the network's weight gradients take at 480x640, B in {1, 4, 8,
32} (encoder, role-swapped deconvolutions, prediction heads) is carried by a row. The premises of tests/test_gpu_fp32_wgrad_edges.py
hold without the GPU: the exact operands cannot leave fp32's integers, and the module's im2col reference agrees with the oracle."""
import ctypes

import numpy as np
import pytest

import fp32_backward_cases as bc
from mx_deepim_amd.runtime import lib
from mx_deepim_amd.symbols.deepIM_flownet import DECODER, ENCODER
from oracle import net as onet

f32, f64 = np.float32, np.float64
rows = pytest.mark.parametrize("name", bc.NAMES)


def _plan(lds, case):
    B, cin, H, W, cout, k, s, p = case
    plan = (ctypes.c_int * 10)(*[-7] * 10)
    rc = lib.load().deepim_conv_wgrad_plan(lds, B, cin, H, W, cout, k, k, s, p, plan)
    return rc, tuple(plan)


def _hw(case):
    _, _, H, W, _, k, s, p = case
    ho, wo = bc.out_hw(H, W, k, s, p)
    return ho * wo


@rows
def test_row_takes_the_plan_it_is_there_for(name):
    _, case, lds, want = bc.BY_NAME[name]
    assert _plan(lds, case) == (0, want)
    family, bm, mt, kt, units, S, per, last, reduce, ragged = want
    B, cin, _, _, cout, k, _, _ = case
    assert (mt, kt) == (-(-cout // bm), -(-(cin * k * k) // 128))
    if family == bc.FEW:
        assert cout <= 4 and k in (3, 4) and lds == 1
        return
    unit = 16 if family == bc.LDS else 8
    assert units == B * -(-_hw(case) // unit) and ragged == (_hw(case) % unit != 0)
    assert (S - 1) * per < units <= S * per and last == units - (S - 1) * per and 1 <= last <= per
    n = cout * cin * k * k
    if family == bc.LDS:
        assert reduce == (bc.NONE if S == 1 else bc.QUARTERS if S >= 8 and n % 4 == 0 else bc.SCALAR)
        assert S == 1 or per >= 16          # the cost loop keeps slices of at least 16 chunks
    else:
        assert reduce == (bc.QUARTERS if S >= 8 and n % 4 == 0 else bc.SCALAR)          # this kernel always writes slices


def _quarters(S):
    """The slices each of wgrad_reduce4_kernel's four quarters adds: ceil(S / 4) each, the last ones what is left"""
    sq = -(-S // 4)
    return [max(0, min(S, (i + 1) * sq) - i * sq) for i in range(4)]


def test_rows_cover_every_branch_of_the_slice_arithmetic():
    L = [r for r in bc.ROWS if r[3][0] == bc.LDS]
    assert any(r[3][5] == 1 for r in L) and any(r[3][5] > 1 for r in L)
    assert any(r[3][5] > 1 and r[3][7] == r[3][6] for r in L)                 # whole last slice
    assert any(r[3][5] > 1 and r[3][7] < r[3][6] for r in L)                  # short last slice
    assert any(r[3][5] > 1 and r[3][7] < 4 for r in L)                        # shorter than the kernel's three chunks of prefetch
    kinds = {(r[3][8], r[3][5] >= 8) for r in L}
    assert kinds == {(bc.NONE, False), (bc.SCALAR, False), (bc.SCALAR, True), (bc.QUARTERS, True)}
    q = [r[3][5] for r in L if r[3][8] == bc.QUARTERS]
    assert any(s % 4 for s in q)
    lengths = [n for s in q for n in _quarters(s)]
    assert [_quarters(s) for s in (9, 10, 13)] == [[3, 3, 3, 0], [3, 3, 3, 1], [4, 4, 4, 1]] and 9 in q
    assert 0 in lengths                                                       # an empty fourth quarter
    assert any(n >= 4 for n in lengths) and any(n > 4 and n % 4 for n in lengths)      # the four-slice loop, and a remainder after it
    assert any(0 < n < 4 for n in lengths)                                    # the remainder loop alone
    mods = {_hw(r[1]) % 16 for r in L}
    assert mods == {0, 4, 8, 12}
    rc, plan = _plan(1, bc.EXISTING_WHOLE_CHUNK_ROW)                          # % 16 == 0 with S > 1 is an existing test's row
    assert rc == 0 and plan[0] == bc.LDS and plan[5] > 1 and plan[9] == 0
    assert {r[3][1] for r in L} == {64, 128}
    assert any(r[3][2] > 1 and r[1][4] % r[3][1] for r in L)                  # several m-tiles, the last one ragged
    assert any(r[3][3] > 1 and (r[1][1] * r[1][5] ** 2) % 128 for r in L)     # several k-tiles, the last one ragged
    assert any(r[1][1] % 2 for r in L)                                        # odd Cin
    assert any(r[3][9] and r[3][5] > 1 and bc.variants(r[0]) == [1, 3] for r in L) and any(bc.variants(r[0]) == [1] for r in L)
    R = [r for r in bc.ROWS if r[3][0] == bc.REG]
    assert {_hw(r[1]) % 8 for r in R} == {0, 4}
    assert any(r[3][5] == 1 for r in R) and any(r[3][7] < r[3][6] for r in R) and {r[3][8] for r in R} == {bc.SCALAR, bc.QUARTERS}
    F = [r for r in bc.ROWS if r[3][0] == bc.FEW]
    assert {(r[1][4], r[1][5]) for r in F} == {(co, k) for co in (1, 2, 3, 4) for k in (3, 4)}
    assert {r[1][6] for r in F} == {1, 2}
    assert any(_hw(r[1]) < 256 for r in F) and any(_hw(r[1]) > 256 for r in F) and all(_hw(r[1]) % 256 for r in F)
    for r in bc.ROWS:                                                         # "small": below 2 MB of operands
        x, dz = bc.operands(r[0], "exact")
        assert x.nbytes + dz.nbytes < 2 << 20, r[0]


def _signature(case, plan):
    """What decides which code runs: family, tile rows, S class (1, 2 ... 7, 8 and more), a short last slice, the reduce pass, a
    ragged last chunk of a sample"""
    family, bm, _, _, _, S, per, last, reduce, ragged = plan
    if family == bc.FEW:
        return (family, case[4] if case[4] < 3 else 4, case[5])          # the template instantiation
    return (family, bm, 0 if S == 1 else 1 if S < 8 else 2, last < per, reduce, ragged)


def network_weight_gradients(B, cin0, H=480, W=640):
    """(name, (B, Cin, H, W, Cout, k, s, p)) of every fp32 weight gradient of the training graph
    (symbols/deepIM_flownet_train.py): the encoder layers, the decoder's deconvolutions in their role-swapped form (input = the
    un-cropped gradient frame, filters = the layer's input channels, k4 s2 p0), and the 3x3 prediction heads"""
    hh, ww, cin = H, W, cin0
    for name, cout, k, s, p in ENCODER:
        yield name, (B, cin, hh, ww, cout, k, s, p)
        (hh, ww), cin = bc.out_hw(hh, ww, k, s, p), cout
    for l in DECODER.values():
        if l.kind == "deconv":
            yield l.name, (B, l.cout, 2 * l.hw_in[0] + 2, 2 * l.hw_in[1] + 2, l.cin, 4, 2, 0)
        elif l.kind == "pred":
            yield l.name, (B, l.cin, l.hw_in[0], l.hw_in[1], l.cout, 3, 1, 1)


def test_every_weight_gradient_plan_of_the_network_has_a_row():
    tested = {1: {_signature(r[1], r[3]) for r in bc.ROWS if r[2] == 1}, 0: {_signature(r[1], r[3]) for r in bc.ROWS if r[2] == 0}}
    found = {}
    for B in (1, 4, 8, 32):
        for cin0 in (6, 8, 10):          # the network input: 6 or 10 channels, 8 when padded
            layers = list(network_weight_gradients(B, cin0))
            assert len(layers) == 18 and dict(layers)["conv6_1"][1:5] == (1024, 8, 10, 1024) and dict(layers)["deconv4"] == (B, 256, 32, 42, 1026, 4, 2, 0)
            for name, case in layers:
                rc, plan = _plan(1, case)
                assert rc == 0, (name, case)
                found.setdefault(_signature(case, plan), []).append((B, name))
    missing = {s: l for s, l in found.items() if s not in tested[1]}
    assert not missing, missing
    assert {s[0] for s in found} == {bc.FEW, bc.LDS}          # the default option never takes the register-fed kernel below 2 GiB
    assert any(s[0] == bc.LDS and s[5] for s in found)        # the ragged chunk really occurs in training (15 x 20 maps)


def test_exact_operands_stay_inside_fp32_integers():
    for name in bc.NAMES:
        assert bc.exact_sum_limit(name) < 2 ** 24, name
        x, dz = bc.operands(name, "exact")
        assert np.abs(x).max() == 2 and np.abs(dz).max() == 2 and np.array_equal(x, np.rint(x)) and np.array_equal(dz, np.rint(dz))
        dw, db = bc.reference(name, "exact")
        assert dw.dtype == np.int64 and np.abs(dw).max() <= bc.exact_sum_limit(name) and np.count_nonzero(dw) > 0.5 * dw.size
        assert np.array_equal(dw.astype(f32).astype(np.int64), dw) and np.array_equal(db.astype(f32).astype(np.int64), db)
    for shape in bc.WALK_SHAPES:
        assert shape[0] * shape[2] * shape[3] * 8 * 2 ** 27 < 2 ** 53          # the walks' float64 sums are exact


@pytest.mark.parametrize("name", ["ragged-m-k5", "few-co3-k4-s2"])
def test_reference_agrees_with_the_oracle(name):
    """The oracle accumulates in float64 and rounds once: on exact operands it gives the int64 sums themselves, on random ones the
    float64 reference rounded to fp32 (up to the order of its float64 adds: 2^-40 of the sum of magnitudes is generous)."""
    _, (B, cin, H, W, cout, k, s, p), _, _ = bc.BY_NAME[name]
    w0 = np.zeros((cout, cin, k, k), f32)
    x, dz = bc.operands(name, "exact")
    dw, db = bc.reference(name, "exact")
    _, odw, odb = onet.conv2d_backward(x, w0, dz, s, p, need_dx=False)
    np.testing.assert_array_equal(odw.astype(f64), dw.astype(f64))
    np.testing.assert_array_equal(odb.astype(f64), db.astype(f64))
    x, dz = bc.operands(name, "random")
    dw, A, db, Ab = bc.reference(name, "random")
    _, odw, odb = onet.conv2d_backward(x, w0, dz, s, p, need_dx=False)
    assert np.all(np.abs(odw.astype(f64) - dw) <= bc.U * np.abs(dw) + 2.0 ** -40 * A)
    assert np.all(np.abs(odb.astype(f64) - db) <= bc.U * np.abs(db) + 2.0 ** -40 * Ab)
    assert np.all(bc.wgrad_bound(name, A) > 0) and np.all(bc.wgrad_bound(name, A) < 1e-3 * A + 1e-30)


def test_a_correct_fp32_chain_is_inside_the_bound():
    """One fp32 chain in pixel order (rounded products, rounded adds) of the smallest sliced row lies inside the bound the GPU test
    states: the bound is not tighter than fp32 arithmetic itself."""
    name = "short-last"
    _, (B, cin, H, W, cout, k, s, p), _, _ = bc.BY_NAME[name]
    x, dz = bc.operands(name, "random")
    dw, A, _, _ = bc.reference(name, "random")
    cols, rws = bc.im2col(x, k, s, p), bc._rows(dz)
    acc = np.zeros((cout, cin * k * k), f32)
    for i in range(cols.shape[0]):
        acc = (acc + (rws[:, i:i + 1] * cols[i:i + 1, :]).astype(f32)).astype(f32)
    err = np.abs(acc.astype(f64).reshape(dw.shape) - dw)
    assert np.all(err <= bc.wgrad_bound(name, A)) and err.max() > 0


def test_layout_helpers():
    x = np.arange(2 * 16 * 4 * 6, dtype=f32).reshape(2, 16, 4, 6)
    n8, s2 = bc.to_nc8(x), bc.to_nc8_s2d(x)
    assert n8.shape == (2, 2, 4, 6, 8) and s2.shape == (2, 8, 2, 3, 8)
    for (n, c, yy, xx) in ((1, 11, 3, 4), (0, 7, 2, 5), (1, 8, 1, 0)):
        assert n8[n, c // 8, yy, xx, c % 8] == x[n, c, yy, xx]
        c4 = ((yy & 1) * 2 + (xx & 1)) * 16 + c
        assert s2[n, c4 // 8, yy // 2, xx // 2, c4 % 8] == x[n, c, yy, xx]
    dw = np.arange(3 * 8 * 9, dtype=f32).reshape(3, 8, 3, 3)
    assert bc.to_tap_major(dw)[2, 5, 7] == dw[2, 7, 1, 2]


def test_query_refuses_what_the_entries_refuse():
    raw = lib.load().deepim_conv_wgrad_plan
    plan = (ctypes.c_int * 10)()
    for lds in (0, 1):
        for B, cin, H, W, cout, k, s, p in bc.REFUSED:
            plan[:] = [5] * 10
            assert raw(lds, B, cin, H, W, cout, k, k, s, p, plan) != 0, (B, cin, H, W, cout, k, s, p)
            assert list(plan) == [-1] * 10
    assert raw(1, 1, 8, 8, 8, 8, 3, 3, 1, 1, None) != 0
    assert raw(1, 1, 8, 8, 8, 8, 3, 3, 1, 1, plan) == 0 and list(plan) == [bc.LDS, 64, 1, 1, 4, 1, 4, 4, bc.NONE, 0]
    # the family follows the option and the geometry alone: non-square or other kernel sizes never take the few-filter kernel
    assert raw(1, 1, 8, 8, 8, 2, 5, 5, 1, 2, plan) == 0 and plan[0] == bc.LDS
    assert raw(1, 1, 8, 8, 8, 2, 3, 4, 1, 1, plan) == 0 and plan[0] == bc.LDS          # 3 x 4 taps, 8 x 7 output pixels    assert raw(0, 1, 8, 8, 8, 2, 3, 3, 1, 1, plan) == 0 and plan[0] == bc.REG
