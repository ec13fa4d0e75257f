"""CPU: the table of tests/train_half_cases.py against the library's host-side plan queries and against the oracle alone.
deepim_conv_wgrad_half_plan (no context, no device) pins which branch of the weight-gradient kernel each row reaches; together the
rows cover every branch and every combination the nine encoder layers take at 480x640, B in {1, 4, 8, 32}, in both modes; every shape
of tests/golden/make_train_half_digests.py is a row. The data-gradient rows meet every parity-class sub-kernel shape. And the premises
of tests/test_gpu_train_half_edges.py hold without the GPU: the oracle's own accumulation of each exact row's operands equals the
float64 reference bit for bit, the x3 exact operands carry lo halves, and a correct fp32 accumulation of the smallest random row of
each entry lies inside the bound the GPU test states."""
import ctypes

import numpy as np
import pytest

import train_half_cases as tc
from mx_deepim_amd.runtime import lib
from mx_deepim_amd.symbols.deepIM_flownet import ENCODER
from oracle import net as onet

f32, f64 = np.float32, np.float64
wg_cases = pytest.mark.parametrize("rid,mode", tc.WG_CASES, ids=["%s-%s" % c for c in tc.WG_CASES])
dg_cases = pytest.mark.parametrize("rid,mode,ch", tc.DG_CASES, ids=["%s-%s-%dx%d" % ((r, m) + c) for r, m, c in tc.DG_CASES])


def _plan(mode, case):
    B, _, cpad, H, W, cout, k, s, p = case
    plan = (ctypes.c_int * 6)(*[-7] * 6)
    rc = lib.load().deepim_conv_wgrad_half_plan(int(mode == "x3"), B, cpad, H, W, cout, k, s, p, plan)
    return rc, tuple(plan)


def _kind(plan):
    """0: S == 1 with one step; 1: S == 1 with several; 2: S > 1 with one step per slice; 3: S > 1 with several steps per slice"""
    _, _, ksteps, S, sps, _ = plan
    return (0 if ksteps == 1 else 1) if S == 1 else (2 if sps == 1 else 3)


def _combination(case, plan):
    """What decides which code of the kernel runs: the slicing kind, a partial last m-tile, a partial last n-tile, a ragged last k-step"""
    _, _, cpad, _, _, cout, k, _, _ = case
    return (_kind(plan), cout % 128 != 0, (k * k * cpad) % 128 != 0, bool(plan[5]))


@wg_cases
def test_weight_gradient_row_takes_the_plan_it_is_there_for(rid, mode):
    _, _, case, want = tc.WG_BY_ID[rid]
    assert _plan(mode, case) == (0, want)
    m, n, ksteps, S, sps, ragged = want
    assert (m, n) == (-(-case[5] // 128), -(-(case[6] ** 2 * case[2]) // 128)) and ksteps == -(-tc.wg_npix(case) // 32)
    assert (S - 1) * sps < max(ksteps, 1) <= S * sps and ragged == (tc.wg_npix(case) % 32 != 0)


def test_weight_gradient_rows_cover_every_branch():
    for mode in tc.MODES:
        rows = [r for r in tc.WG_ROWS if mode in r[1]]
        assert {_kind(r[3]) for r in rows} == {0, 1, 2, 3}
        assert any(_kind(r[3]) == 3 and r[3][3] * r[3][4] > r[3][2] for r in rows)          # a short last slice
        assert any(_kind(r[3]) == 3 and r[3][3] * r[3][4] == r[3][2] for r in rows)         # and a whole one
        combos = {_combination(r[2], r[3]) for r in rows}
        for axis in (1, 2, 3):
            assert {c[axis] for c in combos} == {False, True}
    f16_rows = [r[2] for r in tc.WG_ROWS]
    assert any(c[1] < c[2] and c[6] == 3 for c in f16_rows) and any(c[5] == 8 for c in f16_rows)
    assert any(c[7] == 2 and c[3] % 2 and c[4] % 2 and c[6] == 5 for c in f16_rows)
    assert any(c[5] % 128 == 16 for c in f16_rows)                                          # the 16-row second m-tile


def _encoder_cases(B, cin=8, H=480, W=640):
    for name, cout, k, s, p in ENCODER:
        yield name, (B, cin, cin, H, W, cout, k, s, p)
        (H, W), cin = tc.out_hw(H, W, k, s, p), cout


def test_every_weight_gradient_plan_of_the_network_has_a_row():
    """flow_conv1's 8 input channels are below a split16 record: the x3 mode takes the fp32 weight gradient there."""
    for mode in tc.MODES:
        tested = {_combination(r[2], r[3]) for r in tc.WG_ROWS if mode in r[1]}
        found = {}
        for B in (1, 4, 8, 32):
            layers = [l for l in _encoder_cases(B) if mode == "f16" or l[1][1] % 16 == 0]
            assert len(layers) == (10 if mode == "f16" else 9) and layers[-1][1][1:6] == (1024, 1024, 8, 10, 1024)
            for name, case in layers:
                rc, plan = _plan(mode, case)
                assert rc == 0
                found.setdefault(_combination(case, plan), []).append((B, name))
        missing = {c: l for c, l in found.items() if c not in tested}
        assert not missing, (mode, missing)
        assert {c[0] for c in found} == {1, 3}          # what the new rows are there for really occurs


def test_every_digest_shape_is_a_row():
    cases = {(r[2], mode) for r in tc.WG_ROWS for mode in r[1]}
    for r in tc.digests.WGRAD:
        for mode in r[9]:
            assert (r[:9], mode) in cases
    assert set(tc.digests.DGRAD) <= set(tc.DG_BY_ID.values())
    for mode in tc.MODES:
        assert tc.digests.DGRAD_CH[mode] in tc.DG_CH[mode]
    assert {c[0] for c in tc.LRELU_CASES} == set(tc.digests.LRELU)
    assert len(tc.LRELU_CASES) == len(tc.digests.LRELU) * 2 * 3


def test_query_refuses_what_the_entries_refuse():
    plan = (ctypes.c_int * 6)()
    raw = lib.load().deepim_conv_wgrad_half_plan
    for args in ((0, 1, 12, 8, 8, 64, 3, 1, 1), (0, 1, 16, 8, 8, 60, 3, 1, 1), (0, 1, 16, 8, 8, 64, 9, 1, 4), (0, 1, 16, 8, 8, 64, 0, 1, 0),
                 (0, 1, 0, 8, 8, 64, 3, 1, 1), (0, 1, 16, 8, 8, 0, 3, 1, 1), (1, 1, 8, 8, 8, 64, 3, 1, 1), (1, 1, 16, 8, 8, 24, 3, 1, 1),
                 (1, 1, 24, 8, 8, 32, 3, 1, 1), (0, 1, 16, 2, 8, 64, 5, 1, 0), (0, 1, 16, 8, 8, 64, 3, 0, 1),
                 (0, 64, 1024, 480, 640, 64, 3, 1, 1), (1, 32, 1024, 480, 640, 64, 3, 1, 1)):
        plan[:] = [5] * 6
        assert raw(*args, plan) != 0, args
        assert list(plan) == [-1] * 6
    assert raw(0, 1, 16, 8, 8, 64, 3, 1, 1, None) != 0
    # the channel rules are each mode's own: a multiple of 8 is enough for fp16 only; twice the elements fit in fp16 only
    assert raw(0, 1, 8, 8, 8, 24, 3, 1, 1, plan) == 0 and list(plan) == [1, 1, 2, 2, 1, 0]
    assert raw(0, 4, 1024, 480, 640, 64, 3, 1, 1, plan) != 0 and raw(0, 3, 1024, 480, 640, 64, 3, 1, 1, plan) == 0
    assert raw(1, 1, 1024, 480, 640, 64, 3, 1, 1, plan) == 0 and raw(1, 3, 1024, 480, 640, 64, 3, 1, 1, plan) != 0


def test_data_gradient_rows_meet_every_sub_kernel_shape():
    assert {g[1:3] for _, g in tc.DG_ROWS if g[4] == 2} >= {(7, 9), (8, 9), (7, 10)}
    assert {(g[3], g[5]) for _, g in tc.DG_ROWS if g[4] == 2} == {(3, 1), (5, 2), (7, 3)}
    assert {g[3] for _, g in tc.DG_ROWS if g[4] == 1} == {1, 3} and any(g[0] == 1 for _, g in tc.DG_ROWS)
    want = {(3, 1): {(1, 1), (1, 2), (2, 1), (2, 2)}, (5, 2): {(3, 3), (3, 2), (2, 3), (2, 2)}, (7, 3): {(3, 3), (3, 4), (4, 3), (4, 4)}}
    for (k, p), shapes in want.items():
        classes = tc.s2_classes(k, p)
        assert len(classes) == 4 and {c[:2] for c in classes.values()} == shapes          # pairwise different, two of them non-square
    assert {c[:2] for k, p in want for c in tc.s2_classes(k, p).values() if c[0] != c[1]} == {(1, 2), (2, 1), (3, 2), (2, 3), (3, 4), (4, 3)}
    assert any(ci > 128 and ci % 64 for ci, _ in tc.DG_CH["f16"]) and any(ci > 128 for ci, _ in tc.DG_CH["x3"])
    # the four class windows of an odd-by-odd frame all differ; an even extent makes two of them equal
    windows = {(h, w): {((h - py + 1) // 2, (w - px + 1) // 2) for py in (0, 1) for px in (0, 1)} for h, w in ((7, 9), (8, 9), (7, 10))}
    assert [len(windows[f]) for f in ((7, 9), (8, 9), (7, 10))] == [4, 2, 2]


# ---- the premises, with the reference alone ------------------------------------------------------------------------------------
@wg_cases
def test_exact_weight_gradient_operands_are_exact_in_the_oracle(rid, mode):
    _, _, _, _, _, _, k, s, p = tc.WG_BY_ID[rid][2]
    (xh, xl), (zh, zl) = tc.wgrad_operands(rid, mode, "exact")
    ref = tc.wgrad_reference(rid, mode, "exact")
    unit = f32(1.0 / (tc.WG_SCALE[mode] * (tc.ACT if mode == "x3" else 1.0)))
    assert np.count_nonzero(ref) > 0.5 * ref.size
    terms = [(xh, zh)] + ([(xh, zl), (xl, zh)] if mode == "x3" else [])
    # the oracle's backward (fp32 in, fp32 out) term by term, and its forward kernel's fp32 fmaf chain over all terms at once
    back = sum(onet.conv2d_backward(x.astype(f32), np.zeros(ref.shape, f32), z.astype(f32), s, p, need_dx=False)[1].astype(f64)
               for x, z in terms)
    np.testing.assert_array_equal((back.astype(f32) * unit).astype(f32), ref.astype(f32))
    chain = tc.wgrad_fp32_chain(np.concatenate([x for x, _ in terms]), np.concatenate([z for _, z in terms]), k, s, p)
    np.testing.assert_array_equal((chain * unit).astype(f32), ref.astype(f32))
    if mode == "x3":
        assert np.count_nonzero(xl) >= 0.25 * xl.size and np.count_nonzero(zl) >= 0.25 * zl.size
        assert np.any(tc.wgrad64(xl, zl, k, s, p))          # the dropped products are not zero: the reference drops them on purpose


@dg_cases
def test_exact_data_gradient_operands_are_exact_in_the_oracle(rid, mode, ch):
    _, Hd, Wd, k, s, p = tc.DG_BY_ID[rid]
    w, sw, (wh, wl), (zh, zl) = tc.dgrad_operands(rid, mode, ch, "exact")
    ref = tc.dgrad_reference(rid, mode, ch, "exact")
    assert np.count_nonzero(ref) > 0.5 * ref.size
    terms = [(wh, zh)] + ([(wh, zl), (wl, zh)] if mode == "x3" else [])
    back = sum(onet.conv2d_backward(np.zeros(ref.shape, f32), a.astype(f32), z.astype(f32), s, p)[0].astype(f64) for a, z in terms)
    np.testing.assert_array_equal((back.astype(f32) / f32(sw)).astype(f32), ref.astype(f32))
    chain = tc.dgrad_fp32_chain(np.concatenate([a for a, _ in terms]), np.concatenate([z for _, z in terms], axis=1), Hd, Wd, s, p)
    np.testing.assert_array_equal((chain / f32(sw)).astype(f32), ref.astype(f32))
    assert tc.dgrad_reached(rid, ch).all()      # (the entry refuses a frame with a row or column no output pixel reaches)
    if mode == "x3":
        assert np.count_nonzero(wl) >= 0.25 * wl.size and np.count_nonzero(zl) >= 0.25 * zl.size


@pytest.mark.parametrize("shape,mode,src", tc.LRELU_CASES, ids=["%s-%s-%dx%dx%dx%d" % ((m, s) + sh) for sh, m, s in tc.LRELU_CASES])
def test_exact_activation_gradient_operands_are_exact(shape, mode, src):
    """Every dz is exact before the output rounding, and a channel's sum is exact in fp32 in any order."""
    (yh, _), d, add, slope = tc.lrelu_operands(shape, mode, src, "exact")
    (hi, lo), db, mag = tc.lrelu_reference(shape, mode, src, "exact")
    e = (0.0 if d is None else d[0] + d[1]) + (0.0 if add is None else tc.LRELU_SCALE * add.astype(f64))
    np.testing.assert_array_equal(hi + lo, np.where(yh > 0, e, e * slope))
    assert np.any(yh == 0) and np.any(yh > 0) and np.any(yh < 0)
    unit = (0.125 if mode == "f16" else 2.0 ** -12) / tc.LRELU_SCALE          # what every dz is a multiple of, over S
    assert np.array_equal(np.rint(mag / unit), mag / unit) and mag.max() / unit < 2 ** 24
    np.testing.assert_array_equal(db.astype(f32).astype(f64), db)
    if mode == "x3" and d is not None:
        assert np.count_nonzero(d[1]) >= 0.25 * d[1].size


def _smallest(cases, cost):
    out = {}
    for c in cases:
        if c[1] not in out or cost(c) < cost(out[c[1]]):
            out[c[1]] = c
    return [out[m] for m in tc.MODES]


def _wg_cost(c):
    case = tc.WG_BY_ID[c[0]][2]
    return tc.wg_npix(case) * case[1] * case[5] * case[6] ** 2


def _dg_cost(c):
    B, Hd, Wd, k, _, _ = tc.DG_BY_ID[c[0]]
    return B * Hd * Wd * k * k * c[2][0] * c[2][1]


@pytest.mark.parametrize("rid,mode", _smallest(tc.WG_CASES, _wg_cost))
def test_a_correct_fp32_weight_gradient_is_inside_the_bound(rid, mode):
    _, _, case, plan = tc.WG_BY_ID[rid]
    (xh, xl), (zh, zl) = tc.wgrad_operands(rid, mode, "random")
    S, A = tc.wgrad_reference(rid, mode, "random")
    terms = [(xh, zh)] + ([(xh, zl), (xl, zh)] if mode == "x3" else [])
    chain = tc.wgrad_fp32_chain(np.concatenate([x for x, _ in terms]), np.concatenate([z for _, z in terms]), *case[6:])
    got = chain.astype(f64) / (tc.WG_SCALE[mode] * (tc.ACT if mode == "x3" else 1.0))
    bound = tc.wgrad_bound(rid, mode, plan, A)
    assert np.all(np.abs(got - S) <= bound) and np.all(bound <= 1e-5 * A)


@pytest.mark.parametrize("rid,mode,ch", _smallest(tc.DG_CASES, _dg_cost))
def test_a_correct_fp32_data_gradient_is_inside_the_bound(rid, mode, ch):
    _, Hd, Wd, k, s, p = tc.DG_BY_ID[rid]
    _, sw, (wh, wl), (zh, zl) = tc.dgrad_operands(rid, mode, ch, "random")
    S, A = tc.dgrad_reference(rid, mode, ch, "random")
    terms = [(wh, zh)] + ([(wh, zl), (wl, zh)] if mode == "x3" else [])
    chain = tc.dgrad_fp32_chain(np.concatenate([a for a, _ in terms]), np.concatenate([z for _, z in terms], axis=1), Hd, Wd, s, p)
    hi, lo = tc.round_to_output(mode, (chain / f32(sw)).astype(f32))
    bound = tc.dgrad_bound(rid, mode, ch, [1] * len(tc.dgrad_convs(rid)), S, A)
    assert np.all(np.abs(hi + lo - S) <= bound)


@pytest.mark.parametrize("mode", tc.MODES)
def test_a_correct_fp32_bias_gradient_is_inside_the_bound(mode):
    """One fp32 chain over a channel's dz values in pixel order, then the multiply by 1 / S."""
    shape = min(tc.digests.LRELU, key=lambda s: s[0] * s[2] * s[3])
    (hi, lo), db_ref, mag = tc.lrelu_reference(shape, mode, "both", "random")
    v = (hi + lo).astype(f32).transpose(1, 0, 2, 3).reshape(shape[1], -1)
    chain = np.zeros(shape[1], f32)
    for i in range(v.shape[1]):
        chain = (chain + v[:, i]).astype(f32)
    got = (chain * f32(1.0 / tc.LRELU_SCALE)).astype(f64)
    assert np.all(np.abs(got - db_ref) <= tc.sum_bound(shape[0] * shape[2] * shape[3] + 2, mag))
