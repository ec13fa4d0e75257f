"""CPU: deepim_deconv_f16_plan and deepim_fewout_f16_plan (host arithmetic, no context, no device; the launchers read the same
functions) pin the launch plan of every row of tests/fp16_decoder_cases.py, the rows together cover what they are there for, every plan
the network's two deconvolutions and three heads take at 480x640 and B in {1, 4, 8, 32} matches a kernel-level row, and the generated
operands and the float64 references are what tests/test_gpu_fp16_decoder_edges.py takes them for."""
import ctypes
import os

import numpy as np
import pytest

import fp16_decoder_cases as dc
from mx_deepim_amd.runtime import lib
from mx_deepim_amd.symbols.deepIM_flownet import DECODER, _pad8
from oracle import net as onet


def _deconv_plan(case):
    B, _, cpad, _, H, W, cout, Ho, Wo = case[:9]
    plan = (ctypes.c_int * 8)(*[-7] * 8)
    lib.deepim_deconv_f16_plan(B, cpad, H, W, cout, Ho, Wo, plan)
    return tuple(plan)


def _fewout_plan(case):
    B, _, cpad, _, H, W = case
    plan = (ctypes.c_int * 4)(*[-7] * 4)
    lib.deepim_fewout_f16_plan(B, H, W, cpad, plan)
    return tuple(plan)


@pytest.mark.parametrize("row", dc.DECONV_ROWS, ids=dc.DECONV_IDS)
def test_deconv_row_takes_the_plan_it_is_there_for(row):
    _, case, want = row
    assert _deconv_plan(case) == want
    B, _, _, _, _, _, cout, Ho, Wo = case[:9]
    assert sum(want[1:5]) == B * Ho * Wo and want[0] == -(-cout // 128) * sum(-(-n // 128) for n in want[1:5])
    assert sum(dc.slice_steps(want)) == want[5] == case[2] // 4 and min(dc.slice_steps(want)) > 0


@pytest.mark.parametrize("row", dc.FEWOUT_ROWS, ids=dc.FEWOUT_IDS)
def test_fewout_row_takes_the_plan_it_is_there_for(row):
    _, case, _, want = row
    assert _fewout_plan(case) == want
    segs = dc.fewout_segments(case, want)
    assert sum(segs) == case[5] and min(segs) > 0 and max(segs) <= 64
    assert want[0] == 64 * want[3] and 64 * (want[3] - 1) < dc.noct(case) <= want[0]


def test_deconv_rows_cover_what_the_issue_lists():
    rows = {rid: (case, plan) for rid, case, plan in dc.DECONV_ROWS}
    combos = {rid: dc.deconv_combination(*cp) for rid, cp in rows.items()}
    assert {p[6] for _, p in rows.values()} == {1, 2, 3, 4, 8}
    assert any(c[0] and c[1] for c in combos.values())                 # a ragged last slice
    assert any(c[0] and c[2] for c in combos.values())                 # a slice that starts mid-tap
    assert {c[3] for c in combos.values()} == {False, True}            # odd and even noct
    assert any(c[0] and c[3] for c in combos.values()) and any(c[4] for c in combos.values())
    assert any(c[5] for c in combos.values()) and any(c[6] for c in combos.values())
    assert any(c[0] and c[6] for c in combos.values())                 # the half-empty M block under split-K too
    # what single rows are there for
    assert rows["one-pixel"][1][:5] == (1, 1, 0, 0, 0) and rows["column"][1][2] == rows["column"][1][4] == 0
    assert dc.slice_steps(rows["three-ragged"][1]) == [17, 17, 16] and dc.slice_steps(rows["four-odd"][1]) == [17, 17, 17, 15]
    assert dc.slice_steps(rows["eight-ragged"][1]) == [17] * 7 + [11]
    case, plan = rows["crop"]
    assert case[7] < 2 * case[4] - 1 and case[8] < 2 * case[5] - 1
    # floor-trim: the tile rule alone asks for 8 slices, 34 steps leave 2 of at least 16
    case, plan = rows["floor-trim"]
    assert min(8, -(-1024 // plan[0])) == 8 and plan[5] // 3 < 16 <= plan[5] // 2 and plan[6] == 2
    # both sides of the 512-tile boundary with the same K
    (c512, p512), (c504, p504) = rows["tiles-512"], rows["tiles-504"]
    assert c512[:7] == c504[:7] and (p512[0], p512[6]) == (512, 1) and (p504[0], p504[6]) == (504, 2) and p512[5] // 2 >= 16
    # the dirty-scratch calls are sliced and cover the scratch of the rows they precede, on another pixel layout
    for rid, (case, plan) in rows.items():
        if plan[6] > 1:
            dirty = dc.dirty_case(rid)
            dplan = _deconv_plan(dirty)
            assert dplan[6] > 1 and dc.scratch_floats(dirty, dplan) >= dc.scratch_floats(case, plan) and dirty[7:9] != case[7:9]


def test_fewout_rows_cover_what_the_issue_lists():
    rows = {rid: (case, plan) for rid, case, _, plan in dc.FEWOUT_ROWS}
    combos = {rid: dc.fewout_combination(*cp) for rid, cp in rows.items()}
    assert {c[0] for c in combos.values()} >= {1, 2, 4}
    assert not combos["full-wave"][1] and dc.noct(rows["full-wave"][0]) == 64          # every lane active
    assert dc.noct(rows["one-lane"][0]) == 65 and dc.noct(rows["four-waves"][0]) == 193 and dc.noct(rows["one-pixel"][0]) == 1
    assert {dc.fewout_nseg_rule(case) for case, _ in rows.values()} == {"width", "rows", "clipped"}
    assert dc.fewout_nseg_rule(rows["clipped"][0]) == "clipped" and dc.fewout_nseg_rule(rows["width-only"][0]) == "width"
    assert dc.fewout_nseg_rule(rows["wide"][0]) == "rows" and dc.fewout_segments(*rows["wide"]) == [18, 18, 18, 16]
    case, plan = rows["1024-rows"]
    assert case[0] * case[4] == 1024 and plan[2] == 1                  # the row count's term at its smallest
    assert dc.fewout_segments(*rows["four-waves"]) == [2, 2, 1]
    assert any(case[4] == 1 for case, _ in rows.values()) and any(case[5] > 64 for case, _ in rows.values())
    assert any(case[2] == 2048 for case, _ in rows.values()) and any(case[3] > case[2] for case, _ in rows.values())
    assert {split for _, _, split, _ in dc.FEWOUT_ROWS} == {(1, 0), (2, 0), (3, 0), (1, 1), (1, 2), (2, 1)}


def test_existing_rows_are_the_ones_the_network_test_runs():
    """The network-shaped rows counted below are the ones tests/test_gpu_fp16_decoder.py parametrises over."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_fp16_decoder.py")).read()
    for shape in dc.EXISTING_DECONV_SHAPES:
        assert repr(shape) in src, shape
    assert "B, Cin, Cin_pad, Hh, Ww, Cout, Ho, Wo = 64, 1026, 1032, 15, 20, 256, 30, 40" in src
    for _, cin, cpad, _, H, W in dc.EXISTING_FEWOUT_CASES:
        assert "(%d, %d, %d, %d, " % (cin, cpad, H, W) in src
    assert '@pytest.mark.parametrize("B", [1, 3])' in src and "    B = 3\n" in src


def test_every_plan_of_the_network_has_a_kernel_level_row():
    tested = {dc.deconv_combination(case, plan) for _, case, plan in dc.DECONV_ROWS}
    tested |= {dc.deconv_combination(case, _deconv_plan(case)) for case in dc.EXISTING_DECONV_CASES}
    tested_few = {dc.fewout_combination(case, plan) for _, case, _, plan in dc.FEWOUT_ROWS}
    tested_few |= {dc.fewout_combination(case, _fewout_plan(case)) for case in dc.EXISTING_FEWOUT_CASES}
    missing, found = [], set()
    for B in (1, 4, 8, 32):
        for name in ("deconv5", "deconv4"):
            l = DECODER[name]
            case = (B, l.cin, _pad8(l.cin), _pad8(l.cin)) + l.hw_in + (l.cout,) + l.hw_out
            combo = dc.deconv_combination(case, _deconv_plan(case))
            found.add(combo)
            if combo not in tested:
                missing.append((B, name, combo))
        for name in ("Convolution1", "Convolution2", "Convolution3"):     # mask_conv3 rides in Convolution3's pass
            l = DECODER[name]
            case = (B, l.cin, _pad8(l.cin), _pad8(l.cin)) + l.hw_in
            combo = dc.fewout_combination(case, _fewout_plan(case))
            if combo not in tested_few:
                missing.append((B, name, combo))
    assert not missing, missing
    # the network takes sliced and unsliced deconvolutions, with slices that start mid-tap and a ragged last one
    assert {c[0] for c in found} == {False, True} and any(c[1] and c[2] for c in found)


def test_queries_refuse_what_the_launchers_refuse():
    raw = lib.load()
    plan = (ctypes.c_int * 8)()
    for args in ((1, 8, 4, 4, 96, 8, 8), (1, 12, 4, 4, 64, 8, 8), (1, 0, 4, 4, 64, 8, 8), (1, 8, 4, 4, 0, 8, 8), (1, 8, 4, 4, 64, 9, 8),
                 (1, 8, 4, 4, 64, 8, 9), (1, 8, 4, 4, 64, 0, 8), (1, 8, 4, 4, 64, 8, 0), (0, 8, 4, 4, 64, 8, 8)):
        assert raw.deepim_deconv_f16_plan(*args, plan) != 0, args
        assert list(plan) == [-1] * 8
    assert raw.deepim_deconv_f16_plan(1, 8, 4, 4, 64, 8, 8, None) != 0
    plan = (ctypes.c_int * 4)()
    for args in ((1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0), (0, 4, 4, 8), (1, 4, 4, 12), (1, 4, 4, 2056)):
        assert raw.deepim_fewout_f16_plan(*args, plan) != 0, args
        assert list(plan) == [-1] * 4
    assert raw.deepim_fewout_f16_plan(1, 4, 4, 8, None) != 0


def _is_fp16_normal_or_zero(a):
    h = a.astype(np.float16)
    return np.array_equal(h.astype(np.float32), a) and not ((a != 0) & (np.abs(a) < dc.F16_MIN_NORMAL)).any() and np.isfinite(a).all()


SMALL_DECONV = [r for r in dc.DECONV_ROWS if not r[0].startswith("tiles-")]


@pytest.mark.parametrize("row", SMALL_DECONV, ids=[r[0] for r in SMALL_DECONV])
def test_deconv_operands_are_what_the_bounds_assume(row):
    _, case, plan = row
    x, w, b = dc.deconv_operands(dc._geometry(case), "exact")
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 4 and set(np.unique(w)) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    assert np.array_equal(b * 4, np.round(b * 4)) and np.abs(b).max() <= 8
    S, A = dc.deconv_reference(case, "exact")
    assert A.max() <= 16 * case[1] + 8 < 2 ** 15 and np.array_equal(S * 4, np.round(S * 4)) and (np.abs(S) <= A).all()
    x, w, b = dc.deconv_operands(dc._geometry(case), "random")
    assert _is_fp16_normal_or_zero(x) and _is_fp16_normal_or_zero(w) and x.any() and w.any()
    S, A = dc.deconv_reference(case, "random")
    assert S.shape == A.shape == (case[0], case[6], case[7], case[8]) and (np.abs(S) <= A).all()
    E = dc.deconv_bound(case, plan, A)
    assert (E > 0).all() and E.max() < 0.1 * np.abs(S).max()           # the bound is well below the values it guards


def test_large_deconv_rows_share_their_operands():
    """tiles-512 and tiles-504 differ in the crop alone: one pair of operands, one uncropped reference (not computed here)."""
    c512, c504 = dc.DECONV_ROWS[dc.DECONV_IDS.index("tiles-512")][1], dc.DECONV_ROWS[dc.DECONV_IDS.index("tiles-504")][1]
    assert dc._geometry(c512) == dc._geometry(c504)
    for kind in ("exact", "random"):
        x, w, b = dc.deconv_operands(dc._geometry(c512), kind)
        assert x.shape == (4, 128, 32, 32) and w.shape == (128, 512, 4, 4) and (kind == "exact" or _is_fp16_normal_or_zero(w))
        assert dc.deconv_operands(dc._geometry(c504), kind)[0] is x


@pytest.mark.parametrize("row", dc.FEWOUT_ROWS, ids=dc.FEWOUT_IDS)
def test_fewout_operands_are_what_the_bounds_assume(row):
    _, case, (n0, n1), plan = row
    x, w, b = dc.fewout_operands(case, n0 + n1, "exact")
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 4 and set(np.unique(w)) <= {-1.0, -0.5, 0.0, 0.5, 1.0}
    S, A = dc.fewout_reference(x, w, b)
    assert A.max() < 2 ** 15 and np.array_equal(S * 4, np.round(S * 4))     # A bounds every partial sum in any order
    x, w, b = dc.fewout_operands(case, n0 + n1, "random")
    assert _is_fp16_normal_or_zero(x) and _is_fp16_normal_or_zero(w) and x.any() and w.any()
    S, A = dc.fewout_reference(x, w, b)
    assert S.shape == (case[0], n0 + n1, case[4], case[5]) and (np.abs(S) <= A).all()
    assert dc.fewout_bound(case, plan, A).max() < 0.1 * np.abs(S).max()     # worst case of 9·2048 terms: a few per cent


def test_flush16_removes_exactly_the_subnormals():
    a = np.array([0.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -15, -2.0 ** -24, 1.5 * 2.0 ** -15, 0.9999 * 2.0 ** -14, 1.0, -65504.0])
    np.testing.assert_array_equal(dc.flush16(a).astype(np.float64), [0, 2.0 ** -14, -2.0 ** -14, 0, 0, 0, 2.0 ** -14, 1, -65504])
    # weights of the widest layer do reach the subnormal range before the flush
    w = np.random.default_rng(0).standard_normal(1 << 20) / np.sqrt(9 * 2048)
    assert ((w.astype(np.float16) != 0) & (np.abs(w.astype(np.float16).astype(np.float64)) < 2.0 ** -14)).any()
    assert _is_fp16_normal_or_zero(dc.flush16(w).astype(np.float32))


def test_nhwc_record_marks_the_channels_nobody_may_read():
    x = np.arange(2 * 5 * 2 * 3, dtype=np.float32).reshape(2, 5, 2, 3)
    rec = dc.nhwc_record(x, 8, 16)
    assert rec.shape == (2, 2, 3, 16) and np.array_equal(rec[..., :5].astype(np.float32), x.transpose(0, 2, 3, 1))
    assert np.isfinite(rec[..., 5:8]).all() and (rec[..., 5:8] != 0).all() and np.isnan(rec[..., 8:]).all()


@pytest.mark.parametrize("rid", ["row", "crop"])
def test_deconv_reference_is_the_oracles_operation(rid):
    """On exact operands the oracle's fp32 sums are exact, so both references must agree to 1e-12 of range."""
    _, case, _ = dc.DECONV_ROWS[dc.DECONV_IDS.index(rid)]
    x, w, b = dc.deconv_operands(dc._geometry(case), "exact")
    S, _ = dc.deconv_reference(case, "exact")
    want = onet.deconv4x4s2_crop(x, w, b, case[7], case[8], (1, 1), 1.0)
    assert np.abs(S - want).max() <= 1e-12 * np.abs(want).max()
    lr = onet.deconv4x4s2_crop(x, w, b, case[7], case[8], (1, 1), dc.SLOPE_EXACT)
    assert np.abs(dc.lrelu(S, dc.SLOPE_EXACT) - lr).max() <= 1e-12 * np.abs(lr).max()


@pytest.mark.parametrize("rid", ["clipped", "wide"])
def test_fewout_reference_is_the_oracles_operation(rid):
    _, case, (n0, n1), _ = dc.FEWOUT_ROWS[dc.FEWOUT_IDS.index(rid)]
    x, w, b = dc.fewout_operands(case, n0 + n1, "exact")
    S, _ = dc.fewout_reference(x, w, b)
    want = onet.conv2d(x, w, b, 1, 1, 1.0)
    assert np.abs(S - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("row", dc.UPSAMPLE_ROWS, ids=[str(r) for r in dc.UPSAMPLE_ROWS])
def test_upsample_operands_keep_the_one_ulp_statement_safe(row):
    flow, w, b = dc.upsample_operands(row, "grid")
    for a in (flow, w, b):
        assert np.array_equal(a * 8, np.round(a * 8))
    S, A = dc.upsample_reference(row, flow, w, b)
    assert A.max() < 2 ** 17 and np.array_equal(S * 64, np.round(S * 64))     # multiples of 1/64 below 2^17: exact in fp32
    flow, w, b = dc.upsample_operands(row, "random")
    S, A = dc.upsample_reference(row, flow, w, b)
    assert S.shape == (row[0], 2, row[3], row[4]) and dc.upsample_margin(S, A).all()
    want = onet.deconv4x4s2_crop(flow, w, b, row[3], row[4], (1, 1), 1.0)
    assert np.abs(S - want).max() <= 1e-5 * np.abs(want).max()            # the same operation as the oracle's fp32 one
