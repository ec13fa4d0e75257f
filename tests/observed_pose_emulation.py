"""numpy emulation of the synthetic-observed draws of csrc/sample.hip: the observed-pose rule of
toolkit/LM6d_ds_0_gen_observed_poses.py:200-250 with its bounded attempt loop (deepim_sample_observed_poses) and the light
draws of toolkit/LM6d_ds_1_gen_observed.py:116-144 (deepim_sample_lights), float64 numpy over pose_sampler_emulation's
Philox, uniform, box_muller and below.  TEST INFRASTRUCTURE ONLY.

Counter layout as in pose_sampler_emulation; stream 4 is the quaternion block of an observed-pose candidate (four normals),
stream 5 its translation block (three normals, the fourth discarded), stream 6 the light draw."""
import numpy as np

import pose_sampler_emulation as emu

FLOAT_EPS = np.finfo(np.float64).eps
LIGHT_POSITIONS = np.array([[1, 0, 1], [1, 1, 1], [0, 1, 1], [-1, 1, 1], [-1, 0, 1], [0, 0, 1]], np.float64)      # ds_1:117-128
LIGHT_COLORS = np.array([[0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]], np.float64)  # ds_1:138
BRIGHTNESS_RATIOS = (0.2, 0.25, 0.3, 0.35, 0.4)                                                                    # ds_1:86
TABLE_COLUMNS = 22          # trans_mean[3], trans_std[3], pz_mean[3], angle_max, fallback pose [12]


def normals7(seed, ids, attempt):
    """(n,7) float64: stream 4 gives z0..z3 (the quaternion), stream 5 z4..z6 (the translation)."""
    a, b = emu.draw(seed, ids, attempt, 4), emu.draw(seed, ids, attempt, 5)
    z0, z1 = emu.box_muller(a[:, 0], a[:, 1])
    z2, z3 = emu.box_muller(a[:, 2], a[:, 3])
    z4, z5 = emu.box_muller(b[:, 0], b[:, 1])
    z6, _ = emu.box_muller(b[:, 2], b[:, 3])
    return np.stack([z0, z1, z2, z3, z4, z5, z6], 1)


def quat2mat(q):
    """RT_transform.quat2mat, expression by expression."""
    w, x, y, z = q
    Nq = w * w + x * x + y * y + z * z
    if Nq < FLOAT_EPS:
        return np.eye(3)
    s = 2.0 / Nq
    X, Y, Z = x * s, y * s, z * s
    wX, wY, wZ = w * X, w * Y, w * Z
    xX, xY, xZ = x * X, x * Y, x * Z
    yY, yZ, zZ = y * Y, y * Z, z * Z
    return np.array([[1.0 - (yY + zZ), xY - wZ, xZ + wY], [xY + wZ, 1.0 - (xX + zZ), yZ - wX], [xZ - wY, yZ + wX, 1.0 - (xX + yY)]])


def angle(u, v):
    """ds_0:74-78 with the sums in the device's order."""
    dot = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    nu = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    nv = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.float64(dot) / (nu * nv)
    return float(np.arccos(np.clip(c, -1.0, 1.0)) / np.pi * 180.0)


def candidate(row, z, K, width, height, border):
    """One candidate: row (22) float64 of the class table, z (7) float64, K (3,3) float32 ->
    (pose (3,4) float64, deg, cx, cy, accept)."""
    row, z = np.asarray(row, np.float64), np.asarray(z, np.float64)
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    n = np.sqrt(((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]) + z[3] * z[3])
    q = z[:4] / n
    if q[0] < 0:
        q = -q
    R = quat2mat(q)
    t = row[0:3] + z[4:7] * row[3:6]
    deg = angle(R[:, 2], row[6:9])
    p = [(K[i, 0] * t[0] + K[i, 1] * t[1]) + K[i, 2] * t[2] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        cx, cy = float(np.float64(p[0]) / np.float64(p[2])), float(np.float64(p[1]) / np.float64(p[2]))
    lo = float(np.float32(border))
    accept = bool(deg <= row[9] and lo < cx < width - lo and lo < cy < height - lo and t[2] > 0.0)
    return np.concatenate([R, t.reshape(3, 1)], 1), deg, cx, cy, accept


def margin(deg, cx, cy, angle_max, width, height, border):
    """(degrees from angle_max, pixels from the nearest border limit)."""
    lo = float(np.float32(border))
    return abs(deg - angle_max), min(abs(cx - lo), abs(cx - (width - lo)), abs(cy - lo), abs(cy - (height - lo)))


def sample(class_index, table, K, width, height, border, max_attempts, seed, ids):
    """The attempt loop -> (pose (B,3,4) float32, attempts (B) int32, normals (B,7), stat (B,4), borderline (B) bool).
    Exhausted: the class's fallback pose, attempts 0. Class id outside the table: zero pose, attempts -1. A pair is borderline
    when some candidate up to its acceptance lies within 1e-3 degrees of angle_max or 1e-3 px of a border limit."""
    table = np.asarray(table, np.float64).reshape(-1, TABLE_COLUMNS)
    cls = np.asarray(class_index, np.int64)
    B = len(cls)
    ids = np.asarray(ids, np.uint64).reshape(B)
    pose, attempts = np.zeros((B, 3, 4), np.float32), np.zeros(B, np.int32)
    zs, stat, borderline = np.zeros((B, 7)), np.zeros((B, 4)), np.zeros(B, bool)
    ok_cls = (cls >= 0) & (cls < len(table))
    attempts[~ok_cls] = -1
    for b in np.nonzero(ok_cls)[0]:
        pose[b] = table[cls[b], 10:22].reshape(3, 4).astype(np.float32)
    open_ = ok_cls.copy()
    for a in range(int(max_attempts)):
        idx = np.nonzero(open_)[0]
        if idx.size == 0:
            break
        z = normals7(seed, ids[idx], a)
        for j, b in enumerate(idx):
            row = table[cls[b]]
            P, deg, cx, cy, ok = candidate(row, z[j], K, width, height, border)
            dr, dp = margin(deg, cx, cy, row[9], width, height, border)
            if dr < 1e-3 or dp < 1e-3:
                borderline[b] = True
            if ok:
                pose[b], attempts[b], zs[b], open_[b] = P.astype(np.float32), a + 1, z[j], False
                stat[b] = [deg, cx, cy, 1.0]
    return pose, attempts, zs, stat, borderline


def lights(seed, ids, ratios=BRIGHTNESS_RATIOS):
    """-> (light_offset (n,3), light_intensity (n,3), brightness_ratio (n)) float32, and (position, colour, ratio) indices."""
    ids = np.asarray(ids, np.uint64).reshape(-1)
    c0, c1 = emu.draw(seed, ids, 0, 6), emu.draw(seed, ids, 1, 6)
    pos = (ids % np.uint64(6)).astype(np.int64)
    offset = (0.5 * LIGHT_POSITIONS[pos]).astype(np.float32)
    intensity = 0.9 + 0.2 * emu.uniform(c0[:, :3])
    colour = emu.below(c0[:, 3], 7)
    ratio = emu.below(c1[:, 0], len(ratios))
    return (offset, (LIGHT_COLORS[colour] * intensity).astype(np.float32), np.asarray(ratios, np.float32)[ratio],
            (pos, colour, ratio))


def observed_pose_stats(poses):
    """stat_poses() of ds_0:81-180 for one class, straight numpy: poses (n,3,4) -> the 22 floats of a table row."""
    poses = np.asarray(poses, np.float64)
    pz = poses[:, :, 2]
    pz_mean = np.mean(pz, 0)
    degs = np.array([angle(pz_mean, p) for p in pz])
    k = int(np.argmin(degs))
    return np.concatenate([np.mean(poses[:, :, 3], 0), np.std(poses[:, :, 3], 0), pz_mean, [degs.max()],
                           poses[k].astype(np.float32).astype(np.float64).reshape(12)])


# ---- the scenario shared by tests/test_synthetic_observed_host.py (its premises, on the CPU) and the GPU test
K_SMALL = (np.diag([0.1, 0.1, 1.0]) @ emu.LM_K.astype(np.float64)).astype(np.float32)
_CACHE = {}


def class_table(angle_max=(70.0, 60.0)):
    """Two classes for 48x64 frames under K_SMALL. With a uniform rotation the angle of R e_z to any axis is below a with
    probability (1 - cos a)/2: 33 % at 70 degrees, 25 % at 60, and the border rule takes a little more."""
    rows = []
    for c, amax in enumerate(angle_max):
        pz = np.array([0.2, -0.1, 1.0]) if c == 0 else np.array([-0.3, 0.2, 0.9])
        pz /= np.linalg.norm(pz)
        fallback = np.zeros((3, 4))
        fallback[:, :3] = np.eye(3)
        fallback[:, 3] = [0.01 * c, -0.01, 0.6]
        rows.append(np.concatenate([[0.0, 0.0, 0.6 + 0.05 * c], [0.03, 0.02, 0.05], pz * 0.8, [amax],
                                    fallback.astype(np.float32).reshape(12)]))
    return np.stack(rows)


SCENARIO_SEED, SCENARIO_B, SCENARIO_BASE, SCENARIO_BORDER, SCENARIO_ATTEMPTS = 2333, 257, 5, 4.8, 100


def block_scenario():
    """B = 257 pairs of mixed classes, draw_base 5, emulated once."""
    if "block" not in _CACHE:
        cls = (np.random.default_rng(3).integers(0, 2, SCENARIO_B)).astype(np.int32)
        table = class_table()
        ids = SCENARIO_BASE + np.arange(SCENARIO_B, dtype=np.uint64)
        pose, attempts, zs, stat, borderline = sample(cls, table, K_SMALL, 64, 48, SCENARIO_BORDER, SCENARIO_ATTEMPTS, SCENARIO_SEED, ids)
        _CACHE["block"] = dict(cls=cls, table=table, ids=ids, pose=pose, attempts=attempts, normals=zs, stat=stat,
                               borderline=borderline)
    return _CACHE["block"]
