"""Pin the CPU oracle (oracle/se3.py) against the reference's own Python at the edges of the pose arithmetic
(tests/golden/pose_edges_golden.npz, written by tests/golden/make_pose_edges_golden.py): refinement-sized deltas,
half-turns, the gimbal / identity thresholds, degenerate quaternions and exp(+-20) translation deltas.  Same rows and same
bars as tests/test_gpu_pose_edges.py, so the oracle the other GPU tests lean on is right here too.

Bars: quaternion / Euler 1e-5, matrix 1e-6, translation rtol 1e-5 / atol 1e-6 (test_calc_rt_delta_rot_types_match_reference),
mat2quat 1e-12 (kat_mat2quat_diag), Euler converters 1e-12 (test_rotation_converters_and_distances_match_reference),
RT_transform rtol 1e-6 / atol 1e-6 (test_rt_transform_euler_matches_reference), rotation / translation distance
rtol 1e-6 / atol 1e-6 (test_mat2quat_dist_ttransform)."""
import os

import numpy as np
import pytest

from oracle import se3 as ose3

COORDS = ("MODEL", "CAMERA", "CAMERA_NEW", "NAIVE")
F_KINDS = ("perturbed", "equal", "quarter_z", "half_z", "milli", "symmetric")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "pose_edges_golden.npz"))


def _rot_key(rot_type, coord):
    return "A_%s_%s_r" % (rot_type, "CAMERA" if coord == "CAMERA_NEW" else coord)    # CAMERA_NEW rotations equal CAMERA's


@pytest.mark.parametrize("coord", COORDS)
def test_calc_rt_delta_small_deltas(g, coord):
    src, tgt = g["A_src"], g["A_tgt_right" if coord == "MODEL" else "A_tgt_left"]
    for rot_type, tol in (("QUAT", 1e-5), ("EULER", 1e-5), ("MATRIX", 1e-6)):
        rt = [ose3.calc_RT_delta(src[b], tgt[b], g["T_means"], g["T_stds"], coord, rot_type) for b in range(len(src))]
        r = np.stack([np.asarray(a, np.float64).reshape(-1) for a, _ in rt])
        np.testing.assert_allclose(r, g[_rot_key(rot_type, coord)], rtol=tol, atol=tol)
        np.testing.assert_allclose(np.stack([b for _, b in rt]), g["A_%s_t" % coord], rtol=1e-5, atol=1e-6)
    rot0, _ = ose3.calc_RT_delta(src[0], tgt[0], g["T_means"], g["T_stds"], coord, "QUAT")
    assert np.array_equal(tgt[0], src[0]) and abs(rot0[0] - 1) < 1e-6      # identical poses: the identity quaternion


def test_calc_se3_small_deltas(g):
    for b in range(len(g["A_src"])):
        rotm, t = ose3.calc_se3(g["A_src"][b], g["A_tgt_left"][b])
        np.testing.assert_allclose(rotm.reshape(-1), g["A_MATRIX_NAIVE_r"][b], rtol=0, atol=1e-6)
        np.testing.assert_allclose(t, g["A_NAIVE_t"][b], rtol=0, atol=1e-6)


def test_mat2quat_edges(g):
    got = np.stack([ose3.mat2quat(m) for m in g["B_mat"]])
    ref, half = g["B_quat"], g["B_half"]
    assert (got[:, 0] >= 0).all()
    assert half.sum() == 6 and np.array_equal(np.abs(ref[:, 0]) < 1e-8, half)
    sign = np.where(half & (np.sum(got * ref, axis=1) < 0), -1.0, 1.0)[:, None]   # w ~ 0: the sign is the eigen-solver's choice
    np.testing.assert_allclose(got * sign, ref, rtol=0, atol=1e-12)


def test_euler_converters_edges(g):
    for m, ref in zip(g["C_mat"], g["C_mat2euler"]):
        np.testing.assert_allclose(ose3.mat2euler(m), ref, rtol=0, atol=1e-12)
    for e, ref in zip(g["C_euler"], g["C_euler2mat"]):
        np.testing.assert_allclose(ose3.euler2mat(*e), ref, rtol=0, atol=1e-12)
    for coord in COORDS:
        tgt = g["C_delta_tgt_right" if coord == "MODEL" else "C_delta_tgt_left"]
        for b in range(2):
            r, t = ose3.calc_RT_delta(g["C_delta_src"][b], tgt[b], g["T_means"], g["T_stds"], coord, "EULER")
            np.testing.assert_allclose(r, g["C_delta_%s_r" % coord][b], rtol=0, atol=1e-12)
            np.testing.assert_allclose(t, g["C_delta_%s_t" % coord][b], rtol=1e-5, atol=1e-6)


def test_quat2mat_on_both_sides_of_eps(g):
    got = np.stack([ose3.quat2mat(q) for q in g["D_quat"]])
    np.testing.assert_allclose(got, g["D_quat2mat"], rtol=1e-6, atol=1e-6)
    assert np.array_equal(got[0], np.eye(3)) and abs(got[1][0, 2] - 1) < 1e-6      # identity below eps, a 120 degree turn above


@pytest.mark.parametrize("coord", COORDS)
def test_rt_transform_edge_rows(g, coord):
    src, se3, ref = g["A_src"], g["D_se3"], g["D_rt_%s" % coord]
    with np.errstate(invalid="ignore"):             # 0 / 0 of the all-zero quaternion, as in the reference
        got = np.stack([ose3.RT_transform(src[b], se3[b, :4], se3[b, 4:], g["T_means"], g["T_stds"], coord) for b in range(len(se3))])
    nan = np.isnan(ref)
    z = int(g["D_zero_row"])
    assert nan[z, :, :3].all() and nan.sum() == (12 if coord == "NAIVE" else 9)
    assert np.array_equal(np.isnan(got), nan)
    np.testing.assert_allclose(got[~nan], ref[~nan], rtol=1e-6, atol=1e-6)
    e6, refe = g["D_euler_se3"], g["D_rt_euler_%s" % coord]
    gote = np.stack([ose3.RT_transform(src[b], e6[b, :3], e6[b, 3:], g["T_means"], g["T_stds"], coord) for b in range(len(e6))])
    np.testing.assert_allclose(gote, refe, rtol=1e-6, atol=1e-6)


def test_rt_dist_at_zero_quarter_half_and_milliradian_turns(g):
    """calc_rt_dist_m = (re, te) of lib/utils/pose_error.py.  The identical-pose rows keep the 0.05 degree bar of
    test_pose_error_metrics_match_reference: the reference's logm sees the float32 rotations' 1e-7 of non-orthonormality
    there (2e-6 degrees), the oracle sees a zero antisymmetric part."""
    gt = g["F_gt"]
    for k, kind in enumerate(F_KINDS):
        est, ref = g["F_est_%s" % kind], g["F_metrics_1025"][k, 0]
        for b in range(len(gt)):
            rd, td = ose3.calc_rt_dist_m(est[b], gt[b])
            if kind == "equal":
                assert 0 <= rd < 0.05 and td == 0
            else:
                np.testing.assert_allclose([rd, td], ref[b, :2], rtol=1e-6, atol=1e-6)
            if kind in ("half_z", "symmetric"):
                assert abs(rd - 180) < 1e-3
