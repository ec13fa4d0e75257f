#!/usr/bin/env python
"""Golden vectors for the rendered-pose rule of csrc/sample.hip (deepim_pose_perturb), produced by the REFERENCE's own Python:
lib/pair_matching/RT_transform.py's mat2euler, euler2mat and calc_rt_dist_m, imported UNMODIFIED through the shims of
tests/golden/make_golden.py and make_pose_edges_golden.py, and the accept expression of
toolkit/LM6d_1_gen_rendered_pose.py:86-97 written out on them.

Runs only where the reference checkout of tests/golden/make_golden.py is present:  python tests/golden/make_pose_sampler_golden.py
(`--check` regenerates and compares every key with the committed file instead of writing it.)
Writes tests/golden/pose_sampler_golden.npz (committed).  TEST INFRASTRUCTURE ONLY.

Inputs, stored in the types the device entry takes: src (n,3,4) float32, normals (n,6) float64, K (3,3) float32, noise (2,5)
float32 = the toolkit's constants at angle_max 45 and 20, cfg (n) = which row of noise a case uses, width, height, border.
Outputs: pose (n,3,4) float64 = the candidate, r_dist (n) degrees, cx, cy (n), accept (n) bool under OUR rule (the toolkit's
expression and tgt_trans.z > 0; accept_toolkit keeps the toolkit's own flag), and rdist_formula_gap.

Cases: 200 random ones (a quarter with wide translations, so the border rejects some) and constructed ones: gimbal-lock
sources (aj = +-pi/2, both exact matrices and rounded euler2mat), the identity, candidates on both sides of angle_max (both
values) and of each of the four border limits, and a candidate behind the camera (z < 0) that the toolkit's expression accepts.
Every case is asserted to lie at least 1e-3 degrees and 1e-3 px from every threshold, so no flag can flip on rounding.
"""
import os
import sys
import warnings
from math import pi

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
import make_pose_edges_golden as pe  # noqa: E402
import pose_sampler_emulation as emu  # noqa: E402

f32, f64 = np.float32, np.float64
K32 = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], f32)
NOISE = np.array([[15.0, 45.0, 0.01, 0.01, 0.05], [15.0, 20.0, 0.01, 0.01, 0.05]], f32)
WIDTH, HEIGHT, BORDER = 640, 480, 16.0
N_RANDOM = 200


def reference_candidate(RT, src, z, noise):
    """LM6d_1_gen_rendered_pose.py:80-97 for one candidate, the normals handed in where the file draws them."""
    angle_std, angle_max, x_std, y_std, z_std = [f64(v) for v in noise]
    K = K32.astype(f64)
    src_pose_m = src.astype(f64)
    src_euler = np.squeeze(RT.mat2euler(src_pose_m[:3, :3]))
    src_trans = src_pose_m[:, 3]
    tgt_euler = src_euler + z[0:3] * (angle_std / 180 * pi)
    tgt_trans = src_trans + np.array([z[3] * x_std, z[4] * y_std, z[5] * z_std])
    tgt_pose_m = np.hstack((RT.euler2mat(tgt_euler[0], tgt_euler[1], tgt_euler[2]), tgt_trans.reshape((3, 1))))
    r_dist, _t = RT.calc_rt_dist_m(tgt_pose_m, src_pose_m)
    r_dist = float(np.real(r_dist))
    transform = np.matmul(K, tgt_trans.reshape(3, 1))
    center_x = float(transform[0, 0] / transform[2, 0])
    center_y = float(transform[1, 0] / transform[2, 0])
    rejected = r_dist > angle_max or not (BORDER < center_x < (WIDTH - BORDER) and BORDER < center_y < (HEIGHT - BORDER))
    return tgt_pose_m, r_dist, center_x, center_y, (not rejected)


def with_translation(src, t):
    out = np.array(src, f32)
    out[:, 3] = np.asarray(t, f64).astype(f32)
    return out


def build():
    RT, _, _ = mg.load_reference()
    RT.np = pe._Np1Array()
    rng = np.random.default_rng(9024)
    cases = []          # (src float32, normals float64, cfg, tag)

    for i in range(N_RANDOM):
        src = mg.rand_pose(rng).astype(f32)
        if i % 4 == 3:
            src = with_translation(src, [rng.uniform(-0.6, 0.6), rng.uniform(-0.45, 0.45), rng.uniform(0.6, 1.2)])
        cases.append((src, rng.standard_normal(6), i % 2, "random"))

    # gimbal-lock sources: exact matrices with cy = 0, and euler2mat(., +-pi/2, .) rounded to float32 (cy ~ 6e-17 <= 4 eps)
    gimbal = [np.array([[0, .6, .8], [0, .8, -.6], [-1, 0, 0]], f64), np.array([[0, .6, .8], [0, -.8, .6], [1, 0, 0]], f64),
              RT.euler2mat(0.3, pi / 2, -0.2), RT.euler2mat(-1.1, -pi / 2, 0.7)]
    for g, R in enumerate(gimbal):
        src = np.zeros((3, 4), f32)
        src[:, :3] = np.asarray(R, f64).astype(f32)
        src[:, 3] = [0.02, -0.03, 0.9]
        M = src[:, :3].astype(f64)
        assert np.sqrt(M[0, 0] ** 2 + M[1, 0] ** 2) <= 4 * np.finfo(f64).eps, g
        for cfg in (0, 1):
            cases.append((src, rng.standard_normal(6) * 0.6, cfg, "gimbal"))

    ident = np.zeros((3, 4), f32)
    ident[:, :3] = np.eye(3)
    ident[:, 3] = [0.0, 0.0, 1.0]
    for cfg in (0, 1):
        cases.append((ident, rng.standard_normal(6), cfg, "identity"))

    # both sides of angle_max: scale a direction of the Euler noise until r_dist crosses the limit (bisection), then 1e-3 off
    for cfg in (0, 1):
        for _ in range(3):
            src = mg.rand_pose(rng).astype(f32)
            d = rng.standard_normal(3)
            d /= np.linalg.norm(d)
            tail = rng.standard_normal(3) * 0.3

            def r_at(s):
                return reference_candidate(RT, src, np.concatenate([d * s, tail]), NOISE[cfg])[1]
            lo, hi = 0.0, 8.0
            assert r_at(hi) > NOISE[cfg][1]
            for _it in range(60):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if r_at(mid) <= NOISE[cfg][1] else (lo, mid)
            for s in (lo * (1 - 1e-3), lo * (1 + 1e-3)):
                cases.append((src, np.concatenate([d * s, tail]), cfg, "angle_max"))

    # both sides of each border limit: the candidate's centre 0.01 px inside / outside
    fx, fy, px, py = f64(K32[0, 0]), f64(K32[1, 1]), f64(K32[0, 2]), f64(K32[1, 2])
    for axis, limit in ((0, BORDER), (0, WIDTH - BORDER), (1, BORDER), (1, HEIGHT - BORDER)):
        for off in (-0.01, 0.01):
            src = mg.rand_pose(rng).astype(f32)
            z = rng.standard_normal(6) * 0.3
            tz = 0.9
            c = [px + 20.0, py - 15.0]
            c[axis] = limit + off
            tgt = np.array([(c[0] - px) * tz / fx, (c[1] - py) * tz / fy, tz])
            src = with_translation(src, tgt - z[3:] * NOISE[0, 2:].astype(f64))
            cases.append((src, z, 0, "border"))

    # behind the camera: the toolkit's expression accepts (centre in the frame, small angle), ours does not
    src = with_translation(mg.rand_pose(rng).astype(f32), [0.0, 0.0, 0.02])
    cases.append((src, np.array([0.1, -0.2, 0.1, 0.0, 0.0, -1.0]), 0, "behind"))

    n = len(cases)
    out = dict(src=np.stack([c[0] for c in cases]), normals=np.stack([c[1] for c in cases]).astype(f64),
               cfg=np.array([c[2] for c in cases], np.int32), tag=np.array([c[3] for c in cases]), K=K32, noise=NOISE,
               width=np.array(WIDTH), height=np.array(HEIGHT), border=np.array(BORDER, f32))
    pose, r_dist, cx, cy = np.zeros((n, 3, 4)), np.zeros(n), np.zeros(n), np.zeros(n)
    accept, toolkit = np.zeros(n, bool), np.zeros(n, bool)
    gap = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (src, z, cfg, tag) in enumerate(cases):
            pose[i], r_dist[i], cx[i], cy[i], toolkit[i] = reference_candidate(RT, src, z, NOISE[cfg])
            accept[i] = toolkit[i] and pose[i, 2, 3] > 0
            # no flag can flip on rounding
            assert abs(r_dist[i] - NOISE[cfg][1]) >= 1e-3, (i, tag, r_dist[i])
            for v, hi in ((cx[i], WIDTH), (cy[i], HEIGHT)):
                assert min(abs(v - BORDER), abs(v - (hi - BORDER))) >= 1e-3, (i, tag, v)
            assert abs(pose[i, 2, 3]) >= 1e-3, (i, tag)
            gap = max(gap, abs(emu.angle_deg(src[:, :3].astype(f64), pose[i, :, :3]) - r_dist[i]))
    assert gap <= 1e-6, gap
    tags = out["tag"]
    for cfg in (0, 1):          # the constructed pairs really straddle their thresholds
        sel = (tags == "angle_max") & (out["cfg"] == cfg)
        assert sel.sum() == 6 and list(accept[sel]) == [True, False] * 3, accept[sel]
    sel = tags == "border"
    assert list(accept[sel]) == [False, True, True, False, False, True, True, False], accept[sel]
    sel = tags == "behind"
    assert toolkit[sel].all() and not accept[sel].any() and (pose[sel, 2, 3] < 0).all()
    rnd = tags == "random"
    assert 0.2 < accept[rnd].mean() < 0.95 and (~toolkit[rnd] & (r_dist[rnd] < 20)).any()       # both reasons reject
    out.update(pose=pose, r_dist=r_dist, cx=cx, cy=cy, accept=accept, accept_toolkit=toolkit, rdist_formula_gap=np.array(gap))
    return out


def main():
    out = build()
    path = os.path.join(HERE, "pose_sampler_golden.npz")
    if "--check" in sys.argv:
        old = np.load(path)
        assert sorted(old.files) == sorted(out)
        for k in out:
            assert np.array_equal(old[k], np.asarray(out[k])), k
        print("pose_sampler_golden.npz reproduced: %d keys equal" % len(out))
        return
    np.savez_compressed(path, **out)
    print("wrote pose_sampler_golden.npz: %d keys, %d cases, %d bytes, accepted %d, rdist_formula_gap %.3g deg"
          % (len(out), len(out["src"]), os.path.getsize(path), int(out["accept"].sum()), float(out["rdist_formula_gap"])))


if __name__ == "__main__":
    main()
