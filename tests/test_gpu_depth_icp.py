"""csrc/icp.hip against its numpy restatement (tests/depth_icp_emulation.py), and DepthICP.refine end to end.

Kernel parity at B = 3 with three different per-pair cameras read through the bound table, at 40x56 (W no multiple of 64 or 4,
three blocks of 1024 pixels per pair) and 5x7 (a 3x5 interior and little else). Pair 1's target stands in front of a wall (a depth
discontinuity for max_step), row 2 is set in `skip`. The seeds were picked on the CPU so that no decision of the emulation sits
within 1e-9 of its threshold and cond(ΣJJᵀ) <= 1e6; both are asserted.

Bounds: the normals and T are float32 values of magnitude <= 1, compared within 2 ulp of 1 (2.4e-7) — a solve error of
cond · 1e-12 lies below one ulp under the cond cap. A sum has <= 4096 terms with about ten roundings each at 1.1e-16 behind it:
1e-11 of its Σ|term|."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_icp_emulation as emu  # noqa: E402

from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.runtime import lib  # noqa: E402

pytestmark = pytest.mark.gpu
AXES = (0.05, 0.08, 0.11)
ULP2 = 2.4e-7
DIST_MAX, MAX_STEP, RCOND = 0.02, 0.01, 1e-9        # MAX_STEP: the degenerate case's; the parity cases carry their own
# (H, W, focal length, min_pairs, max_step, seed). 5x7: the object has to fill the frame, so a pixel is 2 cm of it and the depth
# steps between neighbours are larger; 15 interior pixels support few pairs. Seeds: see the module docstring.
SHAPES = {"40x56": (40, 56, 125.0, 12, 0.01, 5), "5x7": (5, 7, 35.0, 6, 0.04, 33)}


def small_pose(rng, deg, mm):
    R = synthetic.euler_to_mat(*np.deg2rad(rng.normal(0, deg, 3)))
    return np.concatenate([R, (rng.normal(0, 1, 3) * mm * 1e-3)[:, None]], 1).astype(np.float32)


def build_case(H, W, f, min_pairs, max_step, seed):
    """the inputs of one parity case and what the emulation makes of them"""
    rng = np.random.default_rng(seed)
    c = type("Case", (), {})()
    c.H, c.W, c.min_pairs, c.max_step = H, W, min_pairs, max_step
    c.K = np.stack([np.array([[f * s, 0, (W - 1) / 2 + dx], [0, f * s * 1.002, (H - 1) / 2 + dy], [0, 0, 1]], np.float32)
                    for s, dx, dy in ((1.0, 0.0, 0.0), (1.04, 0.3, -0.2), (0.97, -0.4, 0.25))])
    src, tgt = [], []
    for b in range(3):
        R = synthetic.random_rotation(rng)
        t = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.7, 0.9)])
        gt = np.concatenate([R, t[:, None]], 1).astype(np.float32)
        Rs = synthetic.euler_to_mat(*np.deg2rad(rng.normal(0, 3.0, 3))) @ R
        init = np.concatenate([Rs, (t + rng.normal(0, 1, 3) * np.array([0.004, 0.004, 0.008]))[:, None]], 1).astype(np.float32)
        src.append(synthetic.raycast_ellipsoid(init, AXES, c.K[b], H, W)[1])
        d = synthetic.raycast_ellipsoid(gt, AXES, c.K[b], H, W)[1]
        if b == 1:
            d = np.where(d > 0, d, np.float32(t[2] + 0.25)).astype(np.float32)       # a wall behind the object
        tgt.append(d)
    c.src, c.tgt = np.stack(src), np.stack(tgt)
    c.T0 = np.stack([small_pose(rng, 0.3, 1.0) for _ in range(3)])
    c.skip = np.array([0, 0, 1], np.int32)
    c.normals, c.m_step = emu.depth_normals(c.tgt, c.K, max_step)
    c.T1, c.sys, c.status, c.info = emu.icp_step(c.T0, c.src, c.tgt, c.normals, c.K, c.skip, DIST_MAX, min_pairs, RCOND)
    return c


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request, ctx):
    c = build_case(*SHAPES[request.param])
    B, H, W = 3, c.H, c.W
    c.ctx = ctx
    c.K_d = ctx.array(c.K)
    c.src_d, c.tgt_d = ctx.array(c.src.reshape(B, 1, H, W)), ctx.array(c.tgt.reshape(B, 1, H, W))
    c.nrm_d = ctx.array(c.normals)            # the step is fed the emulation's normals: the two passes are judged apart
    c.skip_d = ctx.array(c.skip, dtype=np.int32)
    return c


def run_normals(c, K_host=None, b=None):
    ctx, H, W = c.ctx, c.H, c.W
    depth = c.tgt_d if b is None else c.tgt_d[b:b + 1]
    out = ctx.zeros((depth.shape[0], 3, H, W))
    if K_host is None:
        ctx.bind_cameras(c.K_d)
    lib.deepim_depth_normals(ctx.handle, out, depth, K_host, ctypes.c_float(c.max_step), depth.shape[0], H, W)
    return out.asnumpy()


def run_step(c, K_host=None, b=None):
    ctx, H, W = c.ctx, c.H, c.W
    sl = slice(0, 3) if b is None else slice(b, b + 1)
    n = sl.stop - sl.start
    T = ctx.array(c.T0[sl])
    sys_d, st = ctx.zeros((n, 30), dtype=np.float64), ctx.zeros((n,), dtype=np.int32)
    if K_host is None:
        ctx.bind_cameras(c.K_d)
    lib.deepim_icp_step(ctx.handle, T, sys_d, st, c.src_d[sl], c.tgt_d[sl], c.nrm_d[sl], K_host, c.skip_d[sl],
                        ctypes.c_float(DIST_MAX), c.min_pairs, ctypes.c_double(RCOND), n, H, W)
    return T.asnumpy(), sys_d.asnumpy(), st.asnumpy()


def test_the_scene_sits_away_from_every_threshold(case):
    c = case
    m = dict(c.info["margin"], step=c.m_step)
    print("margins", m, "cond", c.info["cond"], "count", c.sys[:, 27], "status", c.status)
    assert min(m.values()) > 1e-9
    assert (c.info["cond"] <= 1e6).all()
    assert (c.status == 0).all() and (c.sys[:, 27] >= c.min_pairs).all()
    assert not np.array_equal(c.T1[0], c.T0[0]) and not np.array_equal(c.T1[1], c.T0[1])
    zero = (c.normals == 0).all(1)
    assert zero[:, 0].all() and zero[:, :, -1].all() and not zero[:, 1:-1, 1:-1].all()
    if c.H > 5:
        assert zero[1, 1:-1, 1:-1].any()                   # the wall's edge: max_step at work


def test_normals_match_the_emulation(case):
    c = case
    got = run_normals(c)
    print("max |normal error|", np.abs(got.astype(np.float64) - c.normals).max())
    np.testing.assert_array_equal((got == 0).all(1), (c.normals == 0).all(1))
    assert np.abs(got.astype(np.float64) - c.normals).max() <= ULP2
    np.testing.assert_array_equal(got.view(np.uint32), run_normals(c).view(np.uint32))
    for b in range(3):
        np.testing.assert_array_equal(run_normals(c, np.ascontiguousarray(c.K[b]), b)[0].view(np.uint32), got[b].view(np.uint32))


def test_step_matches_the_emulation(case):
    c = case
    T, sys_, st = run_step(c)
    np.testing.assert_array_equal(st, c.status)
    np.testing.assert_array_equal(sys_[:, 27], c.sys[:, 27])
    err = np.abs(sys_ - c.sys)
    print("max sys error / Σ|term|", (err / np.maximum(c.info["abs"], 1e-300)).max(), "max |T error|", np.abs(T - c.T1).max())
    assert (err <= 1e-11 * c.info["abs"]).all()
    assert (sys_[:, 29] == 0).all()
    assert np.abs(T.astype(np.float64) - c.T1).max() <= ULP2
    np.testing.assert_array_equal(T[2].view(np.uint32), c.T0[2].view(np.uint32))          # the skipped row
    T2, sys2, st2 = run_step(c)
    assert T.tobytes() == T2.tobytes() and sys_.tobytes() == sys2.tobytes() and st.tobytes() == st2.tobytes()
    for b in range(3):
        Tb, sysb, stb = run_step(c, np.ascontiguousarray(c.K[b]), b)
        assert Tb[0].tobytes() == T[b].tobytes() and sysb[0].tobytes() == sys_[b].tobytes() and stb[0] == st[b]


def test_apply_matches_the_emulation(case):
    c = case
    out = c.ctx.zeros((3, 3, 4))
    poses = np.stack([small_pose(np.random.default_rng(3 + b), 40.0, 300.0) for b in range(3)])
    lib.deepim_icp_apply(c.ctx.handle, out, c.ctx.array(c.T1), c.ctx.array(poses), 3)
    np.testing.assert_array_equal(out.asnumpy().view(np.uint32), emu.icp_apply(c.T1, poses).view(np.uint32))


def test_degenerate_systems_are_reported_not_solved(ctx):
    """pair 0: a fronto-parallel plane (the ω_z, t_x, t_y pivots are exact zeros in double) → 2; pair 1: an empty source → 1"""
    H, W = 24, 40
    K = np.array([[125.0, 0, 19.5], [0, 125.2, 11.5], [0, 0, 1]], np.float32)
    tgt = np.full((2, 1, H, W), 0.8, np.float32)
    src = tgt.copy()
    src[1] = 0
    T0 = emu.identity(2)
    T0[:, 2, 3] = 0.003
    nrm, T = ctx.zeros((2, 3, H, W)), ctx.array(T0)
    sys_d, st = ctx.zeros((2, 30), dtype=np.float64), ctx.zeros((2,), dtype=np.int32)
    tgt_d = ctx.array(tgt)
    lib.deepim_depth_normals(ctx.handle, nrm, tgt_d, K, ctypes.c_float(MAX_STEP), 2, H, W)
    lib.deepim_icp_step(ctx.handle, T, sys_d, st, ctx.array(src), tgt_d, nrm, K, None, ctypes.c_float(DIST_MAX), 12,
                        ctypes.c_double(RCOND), 2, H, W)
    n = nrm.asnumpy()
    assert (n[:, :, 1:-1, 1:-1] == np.array([0, 0, -1], np.float32)[None, :, None, None]).all()
    e_n, _ = emu.depth_normals(tgt[:, 0], np.stack([K, K]), MAX_STEP)
    e_T, e_sys, e_st, _ = emu.icp_step(T0, src[:, 0], tgt[:, 0], e_n, np.stack([K, K]), None, DIST_MAX, 12, RCOND)
    assert e_st.tolist() == [2, 1]
    np.testing.assert_array_equal(st.asnumpy(), e_st)
    s = sys_d.asnumpy()
    assert s[0, 27] == e_sys[0, 27] > 500 and (s[1] == 0).all()
    assert (s[0, [emu.IU.index((2, 2)), emu.IU.index((3, 3)), emu.IU.index((4, 4))]] == 0).all()
    np.testing.assert_array_equal(T.asnumpy().view(np.uint32), T0.view(np.uint32))


# ------------------------------------------------------------------------------------------------------ DepthICP.refine --
RH, RW = 96, 128
RK = np.array([[286.2, 0, 63.5], [0, 286.8, 47.5], [0, 0, 1]], np.float32)


def test_refine_pulls_rasterised_ellipsoids_onto_their_depth(ctx):
    from mx_deepim_amd.config import default_config
    from mx_deepim_amd.lib.pair_matching.depth_icp import DepthICP
    from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py

    classes = ["a", "b"]
    axes = {"a": np.array(AXES), "b": np.array(AXES)[[1, 2, 0]] * 0.9}
    meshes = {}
    for cname in classes:
        m = synthetic.ellipsoid_mesh(axes[cname])
        m.pop("uv")
        meshes[cname] = m
    rm = Render_Py("unused", classes, RK, RW, RH, meshes=meshes, ctx=ctx, pixel_means=np.zeros(3, np.float32))
    rng = np.random.default_rng(2333)
    gt, init = [], []
    for b in range(2):
        R = synthetic.random_rotation(rng)
        t = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.7, 0.9)])
        gt.append(np.concatenate([R, t[:, None]], 1))
        Rs = synthetic.euler_to_mat(*np.deg2rad(rng.normal(0, 3.0, 3))) @ R
        init.append(np.concatenate([Rs, (t + rng.normal(0, 1, 3) * np.array([0.004, 0.004, 0.008]))[:, None]], 1))
    gt, init = np.stack(gt).astype(np.float32), np.stack(init).astype(np.float32)
    ids = ctx.array(np.array([0, 1], np.int32), dtype=np.int32)
    image, depth_tgt, scratch_depth = ctx.empty((2, 3, RH, RW)), ctx.empty((2, 1, RH, RW)), ctx.empty((2, 1, RH, RW))
    gt_d, init_d = ctx.array(gt), ctx.array(init)
    rm.render_classes_into(image, depth_tgt, ids, gt_d)
    points = np.stack([synthetic.sample_model_points(rng, axes[cname], 500) for cname in classes])        # (2,3,500)
    points_d = ctx.array(points)

    def add_of(poses_d):
        out = ctx.empty((2, 5))
        lib.deepim_pose_error(ctx.handle, out, poses_d, gt_d, points_d, 0, RK, 2, 500)
        return out.asnumpy()[:, 2].astype(np.float64)

    icp = DepthICP(rm, default_config())
    refined, status = icp.refine(init_d, ids, depth_tgt)
    add0, add1 = add_of(init_d), add_of(refined)

    def render(poses):
        rm.render_classes_into(image, scratch_depth, ids, ctx.array(poses))
        return scratch_depth.asnumpy()[:, 0]

    Kb = np.stack([RK, RK])
    e_poses, e_status, infos = emu.refine(init, render, depth_tgt.asnumpy()[:, 0], Kb)
    e_add = np.array([emu.add_metric(e_poses[b], gt[b], points[b].T.astype(np.float64)) for b in range(2)])
    print("ADD initial", add0, "device", add1, "emulation", e_add, "status", status.asnumpy(), e_status)
    assert (e_status == 0).all() and (e_add <= add0 / 20).all()        # the scene: a failure below is the kernels'
    assert (status.asnumpy() == 0).all()
    assert (add1 <= add0 / 20).all()
    # a device (B,3,3) K and the host K give the same poses
    same, _ = icp.refine(init_d, ids, depth_tgt, K=ctx.array(Kb))
    np.testing.assert_array_equal(same.asnumpy().view(np.uint32), refined.asnumpy().view(np.uint32))
