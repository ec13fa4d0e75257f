#!/usr/bin/env python
"""Golden vectors for the observed-pose rule of csrc/sample.hip (deepim_observed_pose_candidate) and for
lib/pair_matching/pose_sampler.observed_pose_stats, produced by the REFERENCE's own Python: lib/pair_matching/RT_transform.py's
quat2mat and mat2quat, imported UNMODIFIED through the shims of tests/golden/make_golden.py, with the expressions of
toolkit/LM6d_ds_0_gen_observed_poses.py written out on them: angle() (:74-78), the candidate (:203-220) and the arithmetic of
stat_poses() (:81-145). The toolkit file itself cannot be imported: it creates directories when it is.

Runs only where the reference checkout of tests/golden/make_golden.py is present:  python tests/golden/make_observed_pose_golden.py
(`--check` regenerates and compares every key with the committed file instead of writing it.)
Writes tests/golden/observed_pose_golden.npz (committed, data only).  TEST INFRASTRUCTURE ONLY.

Statistics: train_poses (2, 40, 3, 4) float64, two classes' training poses -> trans_mean, trans_std, pz_mean, pz_std (2,3),
angles (2,40) degrees, angle_max (2), closest (2) = the index of the training pose whose R e_z is closest to pz_mean (ours: the
fallback), quat (2,40,4) = mat2quat of the rotations as stat_poses stores them, and table (2,22) float64 = the device table.
Candidates, in the types the device entry takes: cls (n) int32, normals (n,7) float64, K (3,3) float32, width, height, border.
Outputs: pose (n,3,4) float64, deg, cx, cy (n), accept (n) bool under OUR rule (the toolkit's expression and tgt_trans.z > 0;
accept_toolkit keeps the toolkit's own flag).

Cases: 200 random ones (half with wide translations, so the border rejects some) and constructed ones: both sides of
angle_max for both classes, both sides of each of the four border limits, and one behind the camera (z < 0) that the toolkit's
expression accepts. Every case is asserted to lie at least 1e-3 degrees and 1e-3 px from every threshold, so no flag can flip
on rounding.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

f32, f64 = np.float32, np.float64
K32 = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], f32)
WIDTH, HEIGHT, BORDER = 640, 480, 48.0
N_RANDOM, N_TRAIN = 200, 40


def angle(u, v):
    """LM6d_ds_0_gen_observed_poses.py:74-78."""
    c = np.dot(u, v) / (np.linalg.norm(u) * np.linalg.norm(v))  # -> cosine of the angle
    rad = np.arccos(np.clip(c, -1, 1))
    deg = rad / np.pi * 180
    return deg


def stat_poses(RT, poses):
    """The arithmetic of stat_poses() (:81-145) for one class whose pose files hold `poses`."""
    pz = np.array([0, 0, 1])
    num_observed = len(poses)
    pose_dict = np.zeros((num_observed, 7))
    new_pz_list = []
    for observed_i, pose in enumerate(poses):
        rot = pose[:3, :3]
        quat = np.squeeze(RT.mat2quat(rot))
        src_trans = pose[:3, 3]
        pose_dict[observed_i, :4] = quat
        pose_dict[observed_i, 4:] = src_trans
        new_pz = np.dot(rot, pz.reshape((-1, 1))).reshape((3,))
        new_pz_list.append(new_pz)
    new_pz_arr = np.array(new_pz_list)
    pz_mean = np.mean(new_pz_arr, 0)
    pz_std = np.std(new_pz_arr, 0)
    trans_mean = np.mean(pose_dict[:, 4:], 0)
    trans_std = np.std(pose_dict[:, 4:], 0)
    angles = []
    for p_i in range(new_pz_arr.shape[0]):
        deg = angle(pz_mean, new_pz_arr[p_i, :])
        angles.append(deg)
    angles = np.array(angles)
    return dict(trans_mean=trans_mean, trans_std=trans_std, pz_mean=pz_mean, pz_std=pz_std, angles=angles, angle_max=np.max(angles),
                quat=pose_dict[:, :4])


def reference_candidate(RT, z, trans_mean, trans_std, pz_mean, deg_max):
    """LM6d_ds_0_gen_observed_poses.py:203-220 for one candidate, the normals handed in where the file draws them."""
    pz = np.array([0, 0, 1])
    K = K32.astype(f64)
    tgt_quat = np.array(z[:4], f64)
    tgt_quat = tgt_quat / np.linalg.norm(tgt_quat)
    if tgt_quat[0] < 0:
        tgt_quat *= -1
    tgt_trans = trans_mean + trans_std * z[4:7]            # np.random.normal(src_trans_mean, src_trans_std)
    tgt_rot_m = RT.quat2mat(tgt_quat)
    new_pz = np.dot(tgt_rot_m, pz.reshape((-1, 1))).reshape((3,))
    deg = angle(new_pz, pz_mean)
    transform = np.matmul(K, tgt_trans.reshape(3, 1))
    center_x = float(transform[0, 0] / transform[2, 0])
    center_y = float(transform[1, 0] / transform[2, 0])
    rejected = deg > deg_max or not (48 < center_x < (640 - 48) and 48 < center_y < (480 - 48))
    return np.hstack((tgt_rot_m, tgt_trans.reshape(3, 1))), float(deg), center_x, center_y, (not rejected)


def cone_poses(rng, axis, half_angle_deg, n, t_mean, t_std):
    """n training poses whose R e_z lies within half_angle_deg of `axis`, with a random spin about it."""
    axis = np.asarray(axis, f64) / np.linalg.norm(axis)
    out = np.zeros((n, 3, 4))
    for i in range(n):
        while True:
            R = mg.rand_pose(rng)[:, :3]
            if angle(R[:, 2], axis) <= half_angle_deg:
                break
        out[i, :, :3] = R
        out[i, :, 3] = t_mean + t_std * rng.standard_normal(3)
    return out


def quat_taking_ez_to(d):
    """The shortest-arc unit quaternion (w >= 0) that takes e_z to the unit vector d."""
    ez = np.array([0.0, 0.0, 1.0])
    q = np.concatenate([[1.0 + ez.dot(d)], np.cross(ez, d)])
    return q / np.linalg.norm(q)


def build():
    RT, _, _ = mg.load_reference()
    rng = np.random.default_rng(2333)
    train = np.stack([cone_poses(rng, [0.2, -0.3, 1.0], 65.0, N_TRAIN, np.array([0.0, -0.02, 0.9]), np.array([0.11, 0.08, 0.15])),
                      cone_poses(rng, [-0.5, 0.1, 0.8], 50.0, N_TRAIN, np.array([0.03, 0.0, 1.0]), np.array([0.09, 0.07, 0.12]))])
    st = [stat_poses(RT, train[c]) for c in (0, 1)]
    closest = np.array([int(np.argmin(s["angles"])) for s in st])
    table = np.stack([np.concatenate([s["trans_mean"], s["trans_std"], s["pz_mean"], [s["angle_max"]],
                                      train[c][closest[c]].astype(f32).astype(f64).reshape(12)]) for c, s in enumerate(st)])
    cases = []          # (cls, normals (7), tag)
    for i in range(N_RANDOM):
        z = rng.standard_normal(7)
        if i % 4 >= 2:                      # half with wide translations, so the border rejects some
            z[4:6] *= 3.0
        cases.append((i % 2, z, "random"))

    # both sides of angle_max: R e_z at angle_max -+ 0.01 degrees from pz_mean, the quaternion scaled like a draw of four normals
    for c in (0, 1):
        u = st[c]["pz_mean"] / np.linalg.norm(st[c]["pz_mean"])
        for k in range(3):
            perp = np.cross(u, rng.standard_normal(3))
            perp /= np.linalg.norm(perp)
            for off in (-0.01, 0.01):
                th = (st[c]["angle_max"] + off) / 180.0 * np.pi
                q = quat_taking_ez_to(np.cos(th) * u + np.sin(th) * perp) * rng.uniform(0.5, 2.5) * (1 if k % 2 == 0 else -1)
                cases.append((c, np.concatenate([q, rng.standard_normal(3) * 0.3]), "angle_max"))

    # both sides of each border limit: the centre 0.01 px inside / outside, a rotation well inside the cone
    fx, fy, px, py = f64(K32[0, 0]), f64(K32[1, 1]), f64(K32[0, 2]), f64(K32[1, 2])
    for axis, limit in ((0, BORDER), (0, WIDTH - BORDER), (1, BORDER), (1, HEIGHT - BORDER)):
        for off in (-0.01, 0.01):
            c = 0
            u = st[c]["pz_mean"] / np.linalg.norm(st[c]["pz_mean"])
            q = quat_taking_ez_to(u) * 1.3
            tz = 0.9
            ctr = [px + 20.0, py - 15.0]
            ctr[axis] = limit + off
            t = np.array([(ctr[0] - px) * tz / fx, (ctr[1] - py) * tz / fy, tz])
            cases.append((c, np.concatenate([q, (t - st[c]["trans_mean"]) / st[c]["trans_std"]]), "border"))

    # behind the camera: the toolkit's expression accepts (centre in the frame, R e_z on pz_mean), ours does not
    u = st[1]["pz_mean"] / np.linalg.norm(st[1]["pz_mean"])
    t = np.array([0.01, -0.02, -0.5])
    cases.append((1, np.concatenate([quat_taking_ez_to(u) * 0.8, (t - st[1]["trans_mean"]) / st[1]["trans_std"]]), "behind"))

    n = len(cases)
    out = dict(train_poses=train, table=table, closest=closest, K=K32, width=np.array(WIDTH), height=np.array(HEIGHT),
               border=np.array(BORDER, f32), cls=np.array([c[0] for c in cases], np.int32),
               normals=np.stack([c[1] for c in cases]).astype(f64), tag=np.array([c[2] for c in cases]))
    for key in ("trans_mean", "trans_std", "pz_mean", "pz_std", "angles", "angle_max", "quat"):
        out[key] = np.stack([np.asarray(s[key], f64) for s in st])
    pose, deg, cx, cy = np.zeros((n, 3, 4)), np.zeros(n), np.zeros(n), np.zeros(n)
    accept, toolkit = np.zeros(n, bool), np.zeros(n, bool)
    for i, (c, z, tag) in enumerate(cases):
        s = st[c]
        pose[i], deg[i], cx[i], cy[i], toolkit[i] = reference_candidate(RT, z, s["trans_mean"], s["trans_std"], s["pz_mean"], s["angle_max"])
        accept[i] = toolkit[i] and pose[i, 2, 3] > 0
        # no flag can flip on rounding
        assert abs(deg[i] - s["angle_max"]) >= 1e-3, (i, tag, deg[i])
        for v, hi in ((cx[i], WIDTH), (cy[i], HEIGHT)):
            assert min(abs(v - BORDER), abs(v - (hi - BORDER))) >= 1e-3, (i, tag, v)
        assert abs(pose[i, 2, 3]) >= 1e-3, (i, tag)
    tags = out["tag"]
    sel = tags == "angle_max"               # the constructed pairs really straddle their thresholds
    assert sel.sum() == 12 and list(accept[sel]) == [True, False] * 6, accept[sel]
    sel = tags == "border"
    assert list(accept[sel]) == [False, True, True, False, False, True, True, False], accept[sel]
    sel = tags == "behind"
    assert toolkit[sel].all() and not accept[sel].any() and (pose[sel, 2, 3] < 0).all()
    rnd = tags == "random"
    assert 0.1 < accept[rnd].mean() < 0.6, accept[rnd].mean()
    assert (~toolkit[rnd] & (deg[rnd] < out["angle_max"][out["cls"][rnd]])).any()          # both reasons reject
    assert (deg[rnd] > out["angle_max"][out["cls"][rnd]]).any()
    out.update(pose=pose, deg=deg, cx=cx, cy=cy, accept=accept, accept_toolkit=toolkit)
    return out


def main():
    out = build()
    path = os.path.join(HERE, "observed_pose_golden.npz")
    if "--check" in sys.argv:
        old = np.load(path)
        assert sorted(old.files) == sorted(out)
        for k in out:
            assert np.array_equal(old[k], np.asarray(out[k])), k
        print("observed_pose_golden.npz reproduced: %d keys equal" % len(out))
        return
    np.savez_compressed(path, **out)
    print("wrote observed_pose_golden.npz: %d keys, %d cases, %d bytes, accepted %d, angle_max %s"
          % (len(out), len(out["cls"]), os.path.getsize(path), int(out["accept"].sum()), out["angle_max"]))


if __name__ == "__main__":
    main()
