"""deepim_flow_epe on the GPU against its numpy restatement (tests/flow_epe_emulation.py), and through the Python layer
(core/tester.par_generate_gt + calc_EPE_batch) against what the reference's own tester.py gave (tests/golden/flow_epe_golden.npz).

Bars. The counts are exact. Against the restatement the sums are within 1e-10 relative: the per-pixel float64 arithmetic is the
same operation for operation, only the order of the sum over at most 100 233 terms differs (N·2^-53 ≈ 1.1e-11). Against the
reference-run fixture 1e-9 relative, as tests/test_flow_epe_host.py argues."""
import ctypes

import numpy as np
import pytest

import flow_epe_emulation as emu
from flow_epe_emulation import CASES, GOLDEN, check_rows, frames_of, ref_name
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import tester
from mx_deepim_amd.runtime import lib

pytestmark = pytest.mark.gpu
SHAPES = [(1, 5, 7),        # under one wave
          (3, 7, 13),       # 91 pixels: straddles a wave, odd in every way
          (2, 16, 20),      # 320 pixels: more than 256, 80 quads over two waves, H·W % 4 == 0 so no tail
          (2, 33, 65),      # 2 145 pixels: three blocks of 1 024 per pair, misaligned planes, a one-pixel scalar tail
          (1, 301, 333)]    # 100 233 pixels: a lane walks two quads (from 16 384 quads per pair on), 49 blocks, the last one partial,
#                             scalar tail; the largest frame, 480x640 (five quads per lane), runs in test_gpu_tester.py
THRESH = 3e-3


@pytest.fixture(scope="module")
def scenes():
    return {s: emu.scene(*s, seed=100 + i) for i, s in enumerate(SHAPES)}


def run(ctx, s, standard_rep=False, skip=None, totals=None, flow_est=None, **over):
    """deepim_flow_epe on a scene → (B,6) float64 numpy (and `totals`, a device array, accumulated in place)"""
    s = dict(s, **over)
    est = s["flow_est"] if flow_est is None else flow_est
    B, _, H, W = est.shape
    out = ctx.empty((B, 6), dtype=np.float64)
    lib.deepim_flow_epe(ctx.handle, out, totals, ctx.array(est), ctx.array(s["depth_rendered"]), ctx.array(s["depth_observed"]),
                        ctx.array(s["pose_rendered"]), ctx.array(s["pose_observed"]), s["K"],
                        None if skip is None else ctx.array(skip, dtype=np.int32), ctypes.c_float(THRESH),
                        1 if standard_rep else 0, B, H, W)
    return out.asnumpy()


def want(s, standard_rep=False, skip=None, flow_est=None, **over):
    s = dict(s, **over)
    return emu.flow_epe(s["flow_est"] if flow_est is None else flow_est, s["depth_rendered"], s["depth_observed"],
                        s["pose_rendered"], s["pose_observed"], s["K"], skip=skip, thresh=THRESH, standard_rep=standard_rep)


@pytest.mark.parametrize("standard_rep", [False, True], ids=["old_rep", "standard_rep"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_equal_the_restatement(ctx, scenes, shape, standard_rep):
    """skip NULL and totals NULL; every row mixes visible, hidden and background pixels"""
    s = scenes[shape]
    exp = want(s, standard_rep)
    assert (exp[:, 3] > 0).all() and (exp[:, 3] < exp[:, 5]).all() and (exp[:, 5] < exp[:, 1]).all()
    check_rows(run(ctx, s, standard_rep), exp, rel=1e-10)
    if shape == (2, 33, 65):
        assert not np.allclose(exp, want(s, not standard_rep))       # the representation matters for these inputs


def test_pair_without_a_rendered_object_counts_background_only(ctx, scenes):
    s = scenes[(3, 7, 13)]
    dr = s["depth_rendered"].copy()
    dr[1] = 0
    got = run(ctx, s, depth_rendered=dr)
    assert got[1, 3] == 0 and got[1, 2] == 0 and got[1, 5] == 91 and got[1, 4] == got[1, 0]
    check_rows(got, want(s, depth_rendered=dr), rel=1e-10)


def test_pair_with_nothing_visible_because_the_observed_depth_is_zero(ctx, scenes):
    s = scenes[(2, 16, 20)]
    do = s["depth_observed"].copy()
    do[0] = 0
    got = run(ctx, s, depth_observed=do)
    assert got[0, 3] == 0 and got[0, 5] == (s["depth_rendered"][0] == 0).sum() and got[1, 3] > 0
    check_rows(got, want(s, depth_observed=do), rel=1e-10)


def test_skipped_pair_gives_a_zero_row_and_leaves_the_totals_alone(ctx, scenes):
    s = scenes[(3, 7, 13)]
    skip = np.array([0, 1, 0], np.int32)
    totals = ctx.zeros((6,), dtype=np.float64)
    got = run(ctx, s, skip=skip, totals=totals)
    assert (got[1] == 0).all()
    full = run(ctx, s)
    np.testing.assert_array_equal(got[[0, 2]], full[[0, 2]])
    np.testing.assert_array_equal(totals.asnumpy(), (np.zeros(6) + full[0]) + full[2])
    check_rows(got, want(s, skip=skip), rel=1e-10)


def test_prediction_is_rounded_to_fp16_as_numpy_rounds_it(ctx, scenes):
    """a tie (2049 → 2048, 2051 → 2052), values under fp16's smallest subnormal and between two subnormals, a value fp16 holds
    only coarsely (1000.3 → 1000.5); each alone in an otherwise zero prediction over a pair without a rendered object, so that
    epe_all is the rounded value itself"""
    s = scenes[(1, 5, 7)]
    dr = np.zeros_like(s["depth_rendered"])
    for v in (2049.0, 2051.0, -2049.0, 1e-8, 6e-8, 9e-8, 1000.3, 65519.0, 0.33337402):
        est = np.zeros((1, 2, 5, 7), np.float32)
        est[0, 1, 2, 3] = v
        got = run(ctx, s, flow_est=est, depth_rendered=dr)
        assert got[0, 0] == abs(float(np.float32(v).astype(np.float16))), v
        assert got[0, 0] == want(s, flow_est=est, depth_rendered=dr)[0, 0]
    est = s["flow_est"].copy()
    est[0, 0, 0, :3] = [2049.0, 1000.3, 1e-8]
    check_rows(run(ctx, s, flow_est=est), want(s, flow_est=est), rel=1e-10)


def test_prediction_beyond_fp16_gives_inf_as_numpy_does(ctx, scenes):
    s = scenes[(2, 16, 20)]
    est = s["flow_est"].copy()
    bg = np.argwhere(s["depth_rendered"][0] == 0)[0]
    est[0, 0, bg[0], bg[1]] = 7e4                      # a background pixel: epe_all and epe_vizbg overflow, epe_viz does not
    got, exp = run(ctx, s, flow_est=est), want(s, flow_est=est)
    assert np.isposinf(got[0, 0]) and np.isposinf(got[0, 4]) and np.isfinite(got[0, 2])
    assert np.isposinf(exp[0, 0]) and np.isposinf(exp[0, 4])
    np.testing.assert_array_equal(got[:, 1::2], exp[:, 1::2])
    fin = np.isfinite(exp)
    np.testing.assert_allclose(got[fin], exp[fin], rtol=1e-10, atol=0)


def test_num_viz_equals_the_visible_sum_of_calc_flow_forward(ctx, scenes):
    s = scenes[(2, 33, 65)]
    B, H, W = 2, 33, 65
    KT = ctx.empty((B, 3, 4))
    lib.deepim_calc_KT(ctx.handle, KT, ctx.array(s["pose_rendered"]), ctx.array(s["pose_observed"]), s["K"], B)
    np.testing.assert_array_equal(KT.asnumpy(), np.stack([emu.calc_KT(s["pose_rendered"][b], s["pose_observed"][b], s["K"])
                                                          for b in range(B)]))
    flow, vis = ctx.empty((B, H, W, 2)), ctx.empty((B, H, W))
    lib.deepim_calc_flow_forward(ctx.handle, flow, vis, ctx.array(s["depth_rendered"]), ctx.array(s["depth_observed"]), KT,
                                 emu.inv3(s["K"]), ctypes.c_float(THRESH), 0, B, H, W)
    v = vis.asnumpy()
    np.testing.assert_array_equal(run(ctx, s)[:, 3], v.reshape(B, -1).sum(1).astype(np.float64))
    np.testing.assert_array_equal(v == 1, emu.visible(s["depth_rendered"], s["depth_observed"], s["pose_rendered"],
                                                      s["pose_observed"], s["K"], THRESH))


def test_two_calls_give_the_same_bytes_and_totals_add_in_a_fixed_order(ctx, scenes):
    s = scenes[(2, 33, 65)]
    totals = ctx.zeros((6,), dtype=np.float64)
    a = run(ctx, s, totals=totals)
    b = run(ctx, s, totals=totals)
    assert a.tobytes() == b.tobytes()
    t = np.zeros(6)
    for rows in (a, b):
        for row in rows:
            t = t + row
    np.testing.assert_array_equal(totals.asnumpy(), t)


def test_captured_graph_follows_the_prediction_buffer(ctx, scenes):
    s = scenes[(3, 7, 13)]
    B, H, W = 3, 7, 13
    est = ctx.array(s["flow_est"])
    out, totals = ctx.empty((B, 6), dtype=np.float64), ctx.zeros((6,), dtype=np.float64)
    args = (ctx.handle, out, totals, est, ctx.array(s["depth_rendered"]), ctx.array(s["depth_observed"]),
            ctx.array(s["pose_rendered"]), ctx.array(s["pose_observed"]), s["K"], None, ctypes.c_float(THRESH), 0, B, H, W)
    lib.deepim_flow_epe(*args)                     # eagerly once: the scratch grows outside the capture
    first = out.asnumpy()
    gid = ctypes.c_int(-1)
    lib.deepim_graph_begin(ctx.handle)
    try:
        lib.deepim_flow_epe(*args)
    finally:
        lib.deepim_graph_end(ctx.handle, ctypes.byref(gid))
    lib.deepim_graph_launch(ctx.handle, gid.value)
    np.testing.assert_array_equal(out.asnumpy(), first)
    est2 = (s["flow_est"] * np.float32(0.5) + np.float32(0.25)).astype(np.float32)
    est.copyfrom(est2)
    lib.deepim_graph_launch(ctx.handle, gid.value)
    second = out.asnumpy()
    assert not np.array_equal(second, first)
    check_rows(second, want(s, flow_est=est2), rel=1e-10)
    t = np.zeros(6)
    for rows in (first, first, second):            # the eager call and two replays added into the totals
        for row in rows:
            t = t + row
    np.testing.assert_array_equal(totals.asnumpy(), t)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("tag,rep,with_gt", CASES)
def test_python_layer_reproduces_the_reference_run(ctx, gold, tag, rep, with_gt):
    """decoded frames → par_generate_gt (deepim_ingest_depth16 twice) → calc_EPE_batch, against tester.py's own numbers"""
    f = frames_of(gold, tag, with_gt)
    B, H, W = f["depth_rendered"].shape
    cfg = default_config()
    cfg.SCALES = [(H, W)]
    cfg.network.STANDARD_FLOW_REP = rep
    cfg.dataset.INTRINSIC_MATRIX = gold[tag + "_K"]
    frames = {k: v for k, v in f.items() if v is not None and not k.startswith("pose_")}
    gt = tester.par_generate_gt(cfg, frames)
    dr, do = emu.par_generate_gt(f)
    np.testing.assert_array_equal(gt["depth_rendered"].asnumpy()[:, 0], dr)
    np.testing.assert_array_equal(gt["depth_observed"].asnumpy()[:, 0], do)
    est = ctx.array(gold[tag + "_flow_est"])
    rows = tester.calc_EPE_batch(cfg, est, gt, f["pose_rendered"], f["pose_observed"])
    check_rows(rows.asnumpy(), gold[ref_name(tag, rep, with_gt) + "_rows"], rel=1e-9)
    one = tester.calc_EPE_one_pair(cfg, est[0:1], {k: v[0:1] for k, v in gt.items()}, f["pose_rendered"][:1],
                                   f["pose_observed"][:1])
    assert list(one) == list(tester.EPE_KEYS)
    assert [one[k] for k in tester.EPE_KEYS] == rows.asnumpy()[0].tolist()
