"""The pose kernels (csrc/se3.hip) and the small heads (csrc/heads.hip) where the random-pose tests never go: deltas of
the refinement loop's size, half-turns, every threshold of the rotation converters, degenerate quaternions, exp(+-20)
translation deltas, in-place updates, the tile boundaries of the ADI search, batches one past a 64-thread block, the kinks
of the losses.  Groups A-D and F against tests/golden/pose_edges_golden.npz, which the REFERENCE's own Python produced
(tests/golden/make_pose_edges_golden.py); E is bit-identity between launches; G and the point counts against the oracle.

Where each bar comes from:
  A  quaternion / Euler 1e-5, matrix 1e-6, translation rtol 1e-5 / atol 1e-6: test_calc_rt_delta_rot_types_match_reference;
     round trip rtol 1e-4 / atol 1e-5: test_calc_rt_delta
  B  1e-12: the kat_mat2quat_diag check of test_rotation_converters_and_distances_match_reference
  C  1e-12: test_rotation_converters_and_distances_match_reference
  D  fixture rtol 1e-6 / atol 1e-6: test_rt_transform_euler_matches_reference; oracle rtol 1e-6 / atol 1e-7: test_rt_transform
  F  rtol 2e-4 / atol 1e-6 and re < 0.05 degrees at identical poses: test_pose_error_metrics_match_reference; 180 +- 1e-3
     degrees and ADI < 1e-6 m (float32 staging of points 1 m away costs 6e-8): reasoning from the number formats
  G  test_point_matching_loss, test_flow_loss_and_logistic;  point counts: test_transform3d_forward_backward
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import heads as oh
from oracle import se3 as ose3
from mx_deepim_amd.runtime import lib

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
COORDS = {"MODEL": 0, "CAMERA": 1, "CAMERA_NEW": 2, "NAIVE": 3}
ROT_TYPES = {"QUAT": (0, 4, 1e-5), "EULER": (1, 3, 1e-5), "MATRIX": (2, 9, 1e-6)}
F_KINDS = ("perturbed", "equal", "quarter_z", "half_z", "milli", "symmetric")
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "pose_edges_golden.npz"))
MU, SD = G["T_means"].astype(np.float32), G["T_stds"].astype(np.float32)


def _convert(ctx, op, x, width):
    x = np.ascontiguousarray(x, np.float32).reshape(len(x), -1)
    out = ctx.empty((len(x), width), dtype=np.float64)
    lib.deepim_rot_convert(ctx.handle, out, ctx.array(x), op, len(x))
    return out.asnumpy()


def _delta(ctx, src, tgt, coord, rot_type):
    code, width, _ = ROT_TYPES[rot_type]
    rot, trans = ctx.empty((len(src), width)), ctx.empty((len(src), 3))
    lib.deepim_calc_rt_delta_ex(ctx.handle, rot, trans, ctx.array(src), ctx.array(tgt), MU, SD, COORDS[coord], code, len(src))
    return rot.asnumpy(), trans.asnumpy()


# ------------------------------------------------------------------------------------------------------------- A ----
@pytest.mark.parametrize("coord", list(COORDS))
def test_calc_rt_delta_in_the_refinement_regime(ctx, coord):
    """65 pairs whose rotation delta is 0 (target bit-identical to the source), 1e-6 … 0.5 rad and whose translation offset
    is 0 … 2 cm: all three rot types against the reference, then RT_transform(src, delta) gives the target back.  The bars
    are absolute: at 1e-6 rad the float32 matrices carry 6e-8 of noise and the reference's answer is noise-shaped too."""
    src, tgt = G["A_src"], G["A_tgt_right" if coord == "MODEL" else "A_tgt_left"]
    assert len(src) == 65 and np.array_equal(src[0], tgt[0])
    for rot_type, (_, _, tol) in ROT_TYPES.items():
        rot, trans = _delta(ctx, src, tgt, coord, rot_type)
        ref = G["A_%s_%s_r" % (rot_type, "CAMERA" if coord == "CAMERA_NEW" else coord)]    # CAMERA_NEW rotations equal CAMERA's
        np.testing.assert_allclose(rot, ref, rtol=tol, atol=tol)
        np.testing.assert_allclose(trans, G["A_%s_t" % coord], rtol=1e-5, atol=1e-6)
        if rot_type == "QUAT":
            assert (rot[:, 0] > 0.9).all()
            se3 = np.concatenate([rot, trans], 1)
    out = ctx.empty((65, 3, 4))
    lib.deepim_rt_transform(ctx.handle, out, None, ctx.array(src), ctx.array(se3), MU, SD, COORDS[coord], 65)
    np.testing.assert_allclose(out.asnumpy(), tgt, rtol=1e-4, atol=1e-5)
    rotm, t = ctx.empty((65, 3, 3)), ctx.empty((65, 3))
    lib.deepim_calc_se3(ctx.handle, rotm, t, ctx.array(src), ctx.array(G["A_tgt_left"]), 65)      # = the NAIVE delta (RT_transform.py:176-187)
    np.testing.assert_allclose(rotm.asnumpy().reshape(65, 9), G["A_MATRIX_NAIVE_r"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(t.asnumpy(), G["A_NAIVE_t"], rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------- B ----
def test_mat2quat_identity_half_turns_and_tiny_angles(ctx):
    """The Jacobi sweep against LAPACK's eigh on identical float32 matrices, 1e-12: the identity (already diagonal), the six
    half-turns (w ~ 0, where the `q[0] < 0` flip decides the sign), negative traces, angles down to 1e-7 (K nearly
    diagonal), products orthonormal only to 1e-7.  At |w_ref| < 1e-8 the reference's sign is the eigen-solver's choice, so
    those rows compare up to a global sign.  Largest deviation measured: 6e-16."""
    got, ref, half = _convert(ctx, 1, G["B_mat"], 4), G["B_quat"], G["B_half"]
    assert half.sum() == 6 and np.array_equal(np.abs(ref[:, 0]) < 1e-8, half)
    assert (got[:, 0] >= 0).all()
    sign = np.where(half & (np.sum(got * ref, axis=1) < 0), -1.0, 1.0)[:, None]
    print("mat2quat: largest deviation from the reference %.3g" % np.abs(got * sign - ref).max())
    np.testing.assert_allclose(got * sign, ref, rtol=0, atol=1e-12)
    # a half-turn whose eigenvector comes out of the sweep with w < 0 must be flipped: both signs of a 1e-9 residual twist
    for s in (1.0, -1.0):
        m = np.diag([1.0, -1.0, -1.0]) + s * 1e-9 * np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]])
        q = _convert(ctx, 1, m[None], 4)[0]
        assert q[0] >= 0 and abs(abs(q[1]) - 1) < 1e-12
        np.testing.assert_allclose(q, ose3.mat2quat(m.astype(np.float32)), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------- C ----
def test_euler_converters_at_the_gimbal_threshold(ctx):
    """mat2euler at cy = 0 exactly, at cy = 1e-15 (regular branch) and 5e-16 (gimbal branch) either side of 4 eps, on
    euler2mat(0.3, pi/2, -0.2) rounded to float32; euler2mat at 0, +-pi/2, pi and 1e-8; calc_RT_delta EULER at an exact
    quarter-turn about y."""
    got = _convert(ctx, 3, G["C_mat"], 3)
    np.testing.assert_allclose(got, G["C_mat2euler"], rtol=0, atol=1e-12)
    assert (got[[0, 1, 3, 4], 2] == 0).all() and abs(got[2, 0] - got[3, 0]) > 0.5       # the two branches answer differently
    np.testing.assert_allclose(_convert(ctx, 2, G["C_euler"], 9), G["C_euler2mat"].reshape(-1, 9), rtol=0, atol=1e-12)
    for coord in COORDS:
        rot, trans = _delta(ctx, G["C_delta_src"], G["C_delta_tgt_right" if coord == "MODEL" else "C_delta_tgt_left"], coord, "EULER")
        np.testing.assert_allclose(rot, G["C_delta_%s_r" % coord], rtol=0, atol=1e-5)
        np.testing.assert_array_equal(rot, np.float32([[0, np.pi / 2, 0]] * 2))          # exact inputs: float32(pi/2) to the bit
        np.testing.assert_allclose(trans, G["C_delta_%s_t" % coord], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------- D ----
def test_quat2mat_on_both_sides_of_float_eps(ctx):
    """s (.5, .5, .5, .5): float32 Nq = 1.96e-16 < eps gives the identity, 2.56e-16 > eps the 120 degree turn about (1,1,1)."""
    got = _convert(ctx, 0, G["D_quat"], 9).reshape(-1, 3, 3)
    np.testing.assert_allclose(got, G["D_quat2mat"], rtol=1e-6, atol=1e-6)
    assert np.array_equal(got[0], np.eye(3)) and abs(got[1][0, 2] - 1) < 1e-6 and abs(got[2][0, 2] - 1) < 1e-6


@pytest.mark.parametrize("coord", list(COORDS))
def test_rt_transform_edge_rows_and_in_place(ctx, coord):
    """A batch of 65 with (1,0,0,0), the same plus 1e-7 of noise, a norm-1e3 quaternion, components of 1e-20 (squares are
    float32 subnormals: finite in the reference, NaN from a kernel that flushed them), the all-zero quaternion (NaN rotation
    block in the reference, and a finite translation column outside NAIVE) and t_z * std + mean of -20, 0, +20 scattered
    among ordinary rows.  Same NaN mask as the reference, everything else to the bar (so no neighbour of an edge row moves),
    and the in-place update (pose_est = pose_src, what the loop does) equal bit for bit, NaN positions included."""
    src, se3, ref = G["A_src"], G["D_se3"], G["D_rt_%s" % coord]
    B, z = len(se3), int(G["D_zero_row"])
    assert B == 65 and not se3[z, :4].any()
    nan = np.isnan(ref)
    assert nan[z, :, :3].all() and nan.sum() == (12 if coord == "NAIVE" else 9)
    out, out64, dsrc = ctx.empty((B, 3, 4)), ctx.empty((B, 3, 4), dtype=np.float64), ctx.array(src)
    lib.deepim_rt_transform(ctx.handle, out, out64, dsrc, ctx.array(se3), MU, SD, COORDS[coord], B)
    got, got64 = out.asnumpy(), out64.asnumpy()
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(got64), nan)
    assert np.isfinite(got[~nan]).all()
    np.testing.assert_allclose(got64[~nan], ref[~nan], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got[~nan], ref[~nan], rtol=1e-6, atol=1e-6)
    with np.errstate(invalid="ignore"):
        orc = np.stack([ose3.RT_transform(src[b], se3[b, :4], se3[b, 4:], MU, SD, coord) for b in range(B)])
    assert np.array_equal(np.isnan(orc), nan)
    np.testing.assert_allclose(got64[~nan], orc[~nan], rtol=1e-6, atol=1e-7)
    lib.deepim_rt_transform(ctx.handle, dsrc, None, dsrc, ctx.array(se3), MU, SD, COORDS[coord], B)
    np.testing.assert_array_equal(dsrc.asnumpy(), got)
    # Euler rows (quarter / half turns, 1e-8) with the same translation edges, out of place and in place
    e6, refe = G["D_euler_se3"], G["D_rt_euler_%s" % coord]
    Be = len(e6)
    oute, dsrce = ctx.empty((Be, 3, 4)), ctx.array(src[:Be])
    lib.deepim_rt_transform_euler(ctx.handle, oute, None, dsrce, ctx.array(e6), MU, SD, COORDS[coord], Be)
    np.testing.assert_allclose(oute.asnumpy(), refe, rtol=1e-6, atol=1e-6)
    lib.deepim_rt_transform_euler(ctx.handle, dsrce, None, dsrce, ctx.array(e6), MU, SD, COORDS[coord], Be)
    np.testing.assert_array_equal(dsrce.asnumpy(), oute.asnumpy())


# ------------------------------------------------------------------------------------------------------------- E ----
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("row", ["zero", "tiny", "unit"])
def test_fused_pose_tail_on_edge_rows(ctx, B, row):
    """test_fused_pose_tail_is_bit_identical_to_the_separate_launches with an se3 row the network never produces in that
    test: zero rot / trans weights put the row into the biases, whatever fc6 and the zoom factor are.  fc7, se3 and the
    poses equal the three separate launches bit for bit, NaN positions included."""
    rng = np.random.default_rng(7)
    quat = {"zero": [0, 0, 0, 0], "tiny": [1e-20, 1e-20, -1e-20, 1e-20], "unit": [1, 0, 0, 0]}[row]
    b_rot, b_tr = np.array(quat, np.float32), np.array([0.05, -0.03, 0.1], np.float32)
    fc6 = rng.standard_normal((B, 256)).astype(np.float32)
    w7 = (rng.standard_normal((256, 256)) / 16).astype(np.float32)
    b7 = (rng.standard_normal(256) * 0.1).astype(np.float32)
    zf = np.concatenate([rng.uniform(0.3, 0.9, (B, 1)).repeat(2, 1), rng.uniform(-0.2, 0.2, (B, 2))], 1).astype(np.float32)
    d = {k: ctx.array(v) for k, v in dict(fc6=fc6, w7=w7, b7=b7, w_rot=np.zeros((4, 256), np.float32), b_rot=b_rot,
                                         w_tr=np.zeros((3, 256), np.float32), b_tr=b_tr, zf=zf).items()}
    h = ctx.handle
    for rc in range(4):
        src = ctx.array(G["A_src"][:B])
        f7a, se3a, posea = ctx.empty((B, 256)), ctx.empty((B, 7)), ctx.empty((B, 3, 4))
        lib.deepim_fc_forward(h, f7a, d["fc6"], d["w7"], d["b7"], B, 256, 256, cf(0.1))
        lib.deepim_pose_head_forward(h, se3a, f7a, d["w_rot"], d["b_rot"], d["w_tr"], d["b_tr"], d["zf"], B, 256)
        lib.deepim_rt_transform(h, posea, None, src, se3a, MU, SD, rc, B)
        f7b, se3b, poseb = ctx.empty((B, 256)), ctx.empty((B, 7)), ctx.empty((B, 3, 4))
        lib.deepim_pose_tail_forward(h, f7b, se3b, poseb, d["fc6"], d["w7"], d["b7"], d["w_rot"], d["b_rot"], d["w_tr"], d["b_tr"],
                                     d["zf"], src, MU, SD, rc, B, 256, cf(0.1))
        np.testing.assert_array_equal(se3b.asnumpy()[:, :4], np.tile(b_rot, (B, 1)))         # the row under test reached the kernel
        np.testing.assert_array_equal(f7b.asnumpy(), f7a.asnumpy())
        np.testing.assert_array_equal(se3b.asnumpy(), se3a.asnumpy())
        np.testing.assert_array_equal(poseb.asnumpy(), posea.asnumpy())
        nan = np.isnan(poseb.asnumpy())
        if row == "zero":
            assert nan[:, :, :3].all() and nan[:, :, 3].all() == (rc == 3)
        else:
            assert not nan.any()
        lib.deepim_pose_tail_forward(h, f7b, se3b, src, d["fc6"], d["w7"], d["b7"], d["w_rot"], d["b_rot"], d["w_tr"], d["b_tr"],
                                     d["zf"], src, MU, SD, rc, B, 256, cf(0.1))            # in place
        np.testing.assert_array_equal(src.asnumpy(), posea.asnumpy())


# ------------------------------------------------------------------------------------------------------------- F ----
def _points(N):
    """The fixture's N-point set: the centred slice of its 2304-point master (keeps point N-1-i the mirror of point i under
    a half-turn about the model z axis), with the on-axis point in the middle when N is odd."""
    m, h = G["F_points_master"], N // 2
    c = m.shape[1] // 2
    return np.ascontiguousarray(np.concatenate([m[:, c - h:c]] + ([G["F_axis_point"]] if N % 2 else []) + [m[:, c:c + h]], 1))


@pytest.mark.parametrize("N", [1, 255, 1024, 1025, 2304])
def test_pose_error_at_the_tile_boundaries(ctx, N):
    """re / te / ADD / ADI / reprojection error of lib/utils/pose_error.py for 3 pairs at point counts below, at and past
    the 1024-point LDS tile of the ADI search, shared and per-sample point layouts.  Pairs: a small perturbation; est = gt;
    est = gt turned by exactly 90 and 180 degrees (cos exactly 0 and -1 for sample 0) and by 1e-3 rad; and est = gt turned by
    a half-turn about the axis the point set is symmetric about, where the nearest neighbour of point i is point N-1-i — in
    another tile at N = 1025 and 2304 — so ADD is centimetres while ADI is 0: a search that dropped a tile shows as ADI."""
    pts, gt, K = _points(N), G["F_gt"], np.ascontiguousarray(G["F_K"])
    assert pts.shape == (3, N)
    B = len(gt)
    per_sample = np.ascontiguousarray(pts[None] * G["F_scales"][:, None, None])
    out, dgt = ctx.empty((B, 5)), ctx.array(gt)
    for k, kind in enumerate(F_KINDS):
        for layout, dpts in ((0, ctx.array(pts)), (1, ctx.array(per_sample))):
            lib.deepim_pose_error(ctx.handle, out, ctx.array(G["F_est_%s" % kind]), dgt, dpts, 1 - layout, K, B, N)
            got, ref = out.asnumpy(), G["F_metrics_%d" % N][k, layout]
            np.testing.assert_allclose(got[:, 1:], ref[:, 1:], rtol=2e-4, atol=1e-6, err_msg="%s layout %d" % (kind, layout))
            if kind == "equal":
                assert (got[:, 0] < 0.05).all() and got[0, 0] == 0 and np.abs(got[:, 1:]).max() < 1e-6
            else:
                np.testing.assert_allclose(got[:, 0], ref[:, 0], rtol=2e-4, atol=1e-6, err_msg="%s layout %d" % (kind, layout))
            if kind in ("half_z", "symmetric"):
                assert np.abs(got[:, 0] - 180).max() < 1e-3
            if kind == "quarter_z":
                assert got[0, 0] == 90
            if kind == "symmetric":
                assert got[:, 3].max() < 1e-6, got[:, 3]
                assert N == 1 or got[:, 2].min() > 1e-2


# ------------------------------------------------------------------------------------------------------------- G ----
@pytest.mark.parametrize("N", [1, 85, 86, 257])
def test_point_matching_loss_at_its_kinks(ctx, N):
    """3N = 3, 255, 258, 771 elements.  L1 with est == gt at every third element: gradient 0 there, not +-1.  smooth_L1 with
    sigma = 2 at residuals of exactly +-0.25 (the first value of the linear branch), 0 and +-0.25 (1 +- 2^-20).  All-zero
    weights: sum and gradient exactly 0."""
    rng = np.random.default_rng(N)
    n = 3 * N
    gt = (rng.standard_normal((1, 3, N)) * 0.1).astype(np.float32)
    est = (gt + rng.standard_normal((1, 3, N)).astype(np.float32) * 0.1).astype(np.float32)
    same = (np.arange(n) % 3 == 0).reshape(1, 3, N)
    est[same] = gt[same]
    w = np.ones((1, 3, N), np.float32)
    u = 2.0 ** -20
    kinks = np.array([0.25, -0.25, 0, 0.25 * (1 + u), 0.25 * (1 - u), -0.25 * (1 + u), -0.25 * (1 - u)], np.float32)
    res = kinks[np.arange(n) % 7].reshape(1, 3, N)
    zero = np.zeros((1, 3, N), np.float32)
    for name, code, sigma, e, g_, wt, norm in (("L1", 0, 1.5, est, gt, w, 0.1), ("smooth_L1", 2, 2.0, res, zero, w, 1.0),
                                               ("L1", 0, 1.5, est, gt, zero, 0.1), ("smooth_L1", 2, 2.0, res, zero, zero, 1.0)):
        rl, rs, rg = oh.point_matching_loss(e, g_, wt, norm, name, sigma, 0.1)
        loss, s, g = ctx.empty(e.shape), ctx.empty((1,)), ctx.empty(e.shape)
        lib.deepim_point_matching_loss(ctx.handle, loss, s, g, ctx.array(e), ctx.array(g_), ctx.array(wt), cf(norm), code, cf(sigma),
                                       cf(0.1), 1, N)
        np.testing.assert_allclose(loss.asnumpy(), rl, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(g.asnumpy(), rg, rtol=1e-6, atol=1e-9)
        if wt.any():
            assert abs(float(s.asnumpy()[0]) - rs) / rs < 1e-5
        else:
            assert float(s.asnumpy()[0]) == 0 and not g.asnumpy().any() and not loss.asnumpy().any()
        if name == "L1" and wt.any():
            assert not g.asnumpy()[same].any() and (np.abs(g.asnumpy()[~same]) == 1).all()
        if name == "smooth_L1" and wt.any():
            at = np.abs(res) == 0.25        # |x| = 1 / sigma^2 exactly: the linear branch, |x| - 0.5 / sigma^2 = 0.125, slope +-1
            np.testing.assert_array_equal(loss.asnumpy()[at], np.float32(0.125))
            np.testing.assert_array_equal(g.asnumpy()[at], np.float32(0.1) * np.sign(res[at]))


@pytest.mark.parametrize("n", [1, 255, 257])
def test_flow_loss_and_logistic_at_saturation(ctx, n):
    """Flow loss with all-zero weights and with est == gt / normalize; the mask logistic at logits where expf overflows
    (+-90, +-100): probabilities finite and exactly 0 or 1 where float32 says so, gradient (p - label) * scale, no NaN."""
    rng = np.random.default_rng(n)
    gt = (rng.standard_normal(n) * 20).astype(np.float32)
    est = rng.standard_normal(n).astype(np.float32)
    est[::3] = gt[::3] / np.float32(20.0)
    for w in (np.ones(n, np.float32), np.zeros(n, np.float32)):
        rl, rs, rg = oh.flow_loss(est, gt, w, 20.0, 0.25)
        loss, s, g = ctx.empty((n,)), ctx.empty((1,)), ctx.empty((n,))
        lib.deepim_flow_loss(ctx.handle, loss, s, g, ctx.array(est), ctx.array(gt), ctx.array(w), cf(20.0), cf(0.25), n)
        np.testing.assert_allclose(loss.asnumpy(), rl, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(g.asnumpy(), rg, rtol=1e-6, atol=1e-12)
        assert not g.asnumpy()[::3].any()
        if w.any() and rs > 0:
            assert abs(float(s.asnumpy()[0]) - rs) / rs < 1e-5
        else:
            assert float(s.asnumpy()[0]) == rs == 0
    logits = np.array([-100, -90, 0, 90, 100], np.float32)[(np.arange(n) + n) % 5]
    lab = (np.arange(n) % 2).astype(np.float32)
    with np.errstate(over="ignore"):
        rp, rgl = oh.mask_logistic(logits, lab, 0.03)
    p, gl = ctx.empty((n,)), ctx.empty((n,))
    lib.deepim_mask_logistic(ctx.handle, p, gl, ctx.array(logits), ctx.array(lab), cf(0.03), n)
    p, gl = p.asnumpy(), gl.asnumpy()
    assert np.isfinite(p).all() and np.isfinite(gl).all()
    np.testing.assert_array_equal(p[logits <= -90], 0)
    np.testing.assert_array_equal(p[logits >= 90], 1)
    np.testing.assert_array_equal(p[logits == 0], 0.5)
    np.testing.assert_allclose(p, rp, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gl, rgl, rtol=1e-5, atol=1e-8)
    np.testing.assert_array_equal(gl, (p - lab) * np.float32(0.03))


# -------------------------------------------------------------------------------------------------- point counts ----
@pytest.mark.parametrize("N", [1, 63, 256, 257])
def test_transform3d_and_points_transform_point_counts(ctx, N):
    """One point, one short of a wavefront, exactly one 256-thread block and one past it."""
    rng = np.random.default_rng(100 + N)
    B = 3
    pts = (rng.standard_normal((B, 3, N)) * 0.05).astype(np.float32)
    q = rng.standard_normal((B, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = (rng.standard_normal((B, 3)) * 0.05).astype(np.float32)
    src = np.ascontiguousarray(G["A_src"][:B])
    og = rng.standard_normal((B, 3, N)).astype(np.float32)
    mu, sd = np.zeros(3, np.float32), np.ones(3, np.float32)
    dp, dq_, dt_, dsrc = ctx.array(pts), ctx.array(q), ctx.array(t), ctx.array(src)
    for coord, rc in COORDS.items():
        out = ctx.empty((B, 3, N))
        lib.deepim_transform3d_forward(ctx.handle, out, dp, dq_, dt_, dsrc, mu, sd, rc, B, N)
        np.testing.assert_allclose(out.asnumpy(), ose3.transform3d_forward(pts, q, t, src, mu, sd, coord), rtol=1e-6, atol=1e-7)
        rq, rt = ose3.transform3d_backward(og, pts, q, t, src, mu, sd, coord)
        gq, gt = ctx.empty((B, 4)), ctx.empty((B, 3))
        lib.deepim_transform3d_backward(ctx.handle, gq, gt, ctx.array(og), dp, dq_, dt_, dsrc, mu, sd, rc, B, N)
        assert np.abs(gq.asnumpy() - rq).max() / (np.abs(rq).max() + 1e-6) < 1e-4
        assert np.abs(gt.asnumpy() - rt).max() / (np.abs(rt).max() + 1e-6) < 1e-4
    out = ctx.empty((B, 3, N))
    lib.deepim_points_transform(ctx.handle, out, dp, dsrc, B, N)
    R, X = src.astype(np.float64), pts.astype(np.float64)
    want = ((R[:, :, 0:1] * X[:, None, 0] + R[:, :, 1:2] * X[:, None, 1]) + R[:, :, 2:3] * X[:, None, 2]) + R[:, :, 3:4]
    np.testing.assert_array_equal(out.asnumpy(), want.astype(np.float32))        # float64 R X + T, rounded once
