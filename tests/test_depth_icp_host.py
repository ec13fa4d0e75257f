"""The depth ICP's numpy restatement (tests/depth_icp_emulation.py) on its own: ten Gauss-Newton steps from one rendered depth
pull a perturbed ellipsoid back onto the observed one, and the two degenerate systems are reported instead of solved.

An ellipsoid with three different axes, not a sphere: a sphere's rotation is unobservable from depth (cond ≈ 2e7, ADD does not
fall)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_icp_emulation as emu  # noqa: E402

from mx_deepim_amd import synthetic  # noqa: E402

H, W = 96, 128
K = np.array([[286.2, 0, 63.5], [0, 286.8, 47.5], [0, 0, 1]], np.float32)
AXES = (0.05, 0.08, 0.11)
SEEDS = [int(s) for s in np.random.default_rng(2333).integers(0, 2 ** 31, 4)]


def scene(seed):
    """(pose_gt, pose_init, depth_init, depth_observed, points (500,3))"""
    rng = np.random.default_rng(seed)
    R = synthetic.random_rotation(rng)
    t = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.7, 0.9)])
    gt = np.concatenate([R, t[:, None]], 1).astype(np.float32)
    Rs = synthetic.euler_to_mat(*np.deg2rad(rng.normal(0, 3.0, 3))) @ R
    ts = t + rng.normal(0, 1, 3) * np.array([0.004, 0.004, 0.008])
    init = np.concatenate([Rs, ts[:, None]], 1).astype(np.float32)
    points = synthetic.sample_model_points(rng, AXES, 500).T.astype(np.float64)
    return (gt, init, synthetic.raycast_ellipsoid(init, AXES, K, H, W)[1], synthetic.raycast_ellipsoid(gt, AXES, K, H, W)[1],
            points)


@pytest.mark.parametrize("seed", SEEDS)
def test_ten_steps_cut_add_twentyfold(seed):
    gt, init, d_src, d_tgt, points = scene(seed)
    Kb = K[None]
    normals, _ = emu.depth_normals(d_tgt[None], Kb, 0.01)
    T = emu.identity(1)
    for _ in range(10):
        T, sys_, status, info = emu.icp_step(T, d_src[None], d_tgt[None], normals, Kb)
        assert status[0] == 0
        assert info["cond"][0] <= 1e6
        assert sys_[0, 27] > 100
    add0 = emu.add_metric(init, gt, points)
    add1 = emu.add_metric(emu.icp_apply(T, init[None])[0], gt, points)
    print("seed %d: ADD %.3f mm -> %.4f mm, cond %.3g" % (seed, add0 * 1e3, add1 * 1e3, info["cond"][0]))
    assert add1 <= add0 / 20


def test_fronto_parallel_plane_is_rank_deficient():
    """constant depth: n = (0,0,-1) everywhere, so the ω_z, t_x and t_y columns of J are exactly zero → status 2, T unchanged"""
    d = np.full((1, H, W), 0.8, np.float32)
    normals, _ = emu.depth_normals(d, K[None], 0.01)
    assert (normals[0, :, 1:-1, 1:-1] == np.array([0, 0, -1], np.float32)[:, None, None]).all()
    assert (normals[0, :, 0] == 0).all() and (normals[0, :, :, -1] == 0).all()
    T0 = emu.identity(1)
    T0[0, 2, 3] = 0.003
    T, sys_, status, _ = emu.icp_step(T0, d, d, normals, K[None])
    assert status[0] == 2
    assert sys_[0, 27] > 1000
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(emu.IU):
        A[i, j] = A[j, i] = sys_[0, k]
    assert (A[[2, 3, 4]] == 0).all()
    np.testing.assert_array_equal(T.view(np.uint32), T0.view(np.uint32))


def test_empty_source_has_too_few_pairs():
    d = np.full((1, H, W), 0.8, np.float32)
    normals, _ = emu.depth_normals(d, K[None], 0.01)
    T0 = emu.identity(1)
    T, sys_, status, _ = emu.icp_step(T0, np.zeros_like(d), d, normals, K[None])
    assert status[0] == 1 and (sys_[0] == 0).all()
    np.testing.assert_array_equal(T, T0)


# ----------------------------------------------------- the scenes of tests/test_gpu_depth_icp_paths.py, judged without a GPU --
import depth_icp_scenes as scenes  # noqa: E402


@pytest.fixture(scope="module")
def gates():
    return scenes.gates_case()


def test_gates_scene_rejects_pixels_at_every_gate(gates):
    scenes.check_gates(gates)


def test_without_max_step_only_the_holes_take_normals_away(gates):
    scenes.check_wide_normals(gates)


def test_half_turn_puts_every_source_point_behind_the_camera(gates):
    scenes.check_behind(gates)


def test_converged_input_stays_put_and_a_tiny_pose_takes_the_series(gates):
    scenes.check_converged(gates)


def test_rim_scene_uses_the_frames_rim_the_ragged_quad_and_the_skew(gates):
    scenes.check_rim(gates)


def test_rcond_and_min_pairs_are_decided_on_both_sides(gates):
    scenes.check_thresholds(gates)


@pytest.mark.parametrize("seed", scenes.CHAIN_SEEDS)
def test_chains_scene_fills_163_blocks(seed):
    scenes.check_chains(scenes.chains_case(seed))


def test_the_outcome_counts_leave_the_arithmetic_alone(gates):
    """the step's reports are by-products: with and without its z′ > 0 test it gives the same bytes on a scene all in front"""
    c = gates
    a, b = scenes.step(c), scenes.step(c, foil="no_behind")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))
    assert (a[3]["counts"]["behind"] == 0).all()


def test_frames_without_an_interior_have_no_normals():
    for H, W in ((2, 9), (1, 1)):
        n, m = emu.depth_normals(np.full((2, H, W), 0.8, np.float32), np.stack([K, K]), 0.01)
        assert n.shape == (2, 3, H, W) and (n == 0).all() and m == np.inf
