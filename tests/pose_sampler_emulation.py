"""numpy emulation of csrc/sample.hip: Philox4x32-10, the uniforms and Box-Muller normals, the rendered-pose rule of
toolkit/LM6d_1_gen_rendered_pose.py:80-107 on oracle.se3's euler2mat / mat2euler with the device's angle formula, the bounded
attempt loop and the mask-dilate draw.  TEST INFRASTRUCTURE ONLY.

Counter layout (include/deepim_hip.h, R-group): key = (seed lo, seed hi), counter = (draw id lo, draw id hi, attempt, stream);
streams 0 and 1 are the two blocks of a pose draw, stream 2 is the mask-dilate draw."""
import math

import numpy as np

from oracle import se3 as ose3

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
SKIPPED = ((0, 1, 4), (1, 2, 5), (2, 3, 6), (0, 3, 7))      # lib/utils/mask_dilate._SKIPPED

KNOWN_ANSWERS = (       # (counter, key, output): the three vectors of the issue, checked against this implementation
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(ctr, key):
    """ctr (...,4), key (...,2) of 32-bit words -> (...,4) uint32. Vectorised over the leading axes."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] & np.uint64(MASK32) for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & np.uint64(MASK32) for i in range(2)]
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return np.stack(c, axis=-1).astype(np.uint32)


def draw(seed, ids, attempt, stream):
    """The four words of (seed, id, attempt, stream) for every id -> (n,4) uint32."""
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
    n = ids.size
    ctr = np.stack([ids & np.uint64(MASK32), ids >> np.uint64(32), np.full(n, attempt, np.uint64), np.full(n, stream, np.uint64)], 1)
    seed = int(seed)
    key = np.broadcast_to(np.array([seed & MASK32, (seed >> 32) & MASK32], np.uint64), (n, 2))
    return philox4x32_10(ctr, key)


def uniform(words):
    return (np.asarray(words, np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


def box_muller(a, b):
    r = np.sqrt(-2.0 * np.log(uniform(a)))
    t = 6.283185307179586 * uniform(b)
    return r * np.cos(t), r * np.sin(t)


def normals(seed, ids, attempt):
    """(n,6) float64: block 0 gives z0..z3, block 1 z4, z5."""
    a, b = draw(seed, ids, attempt, 0), draw(seed, ids, attempt, 1)
    z0, z1 = box_muller(a[:, 0], a[:, 1])
    z2, z3 = box_muller(a[:, 2], a[:, 3])
    z4, z5 = box_muller(b[:, 0], b[:, 1])
    return np.stack([z0, z1, z2, z3, z4, z5], 1)


def angle_deg(R_src, R_tgt):
    """The device's r_dist: the angle of R_src^T R_tgt from the antisymmetric part and the trace (oracle.se3.calc_rt_dist_m)."""
    src = np.zeros((3, 4))
    tgt = np.zeros((3, 4))
    src[:, :3], tgt[:, :3] = R_src, R_tgt
    return ose3.calc_rt_dist_m(src, tgt)[0]


def perturb(src, z, K, noise, width, height, border):
    """One candidate: src (3,4) float32, z (6) float64, K (3,3) float32, noise = (angle_std, angle_max, x_std, y_std, z_std)
    float32 -> (pose (3,4) float64, r_dist, cx, cy, accept)."""
    src = np.asarray(src, np.float32).astype(np.float64)
    z = np.asarray(z, np.float64)
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    angle_std, angle_max, x_std, y_std, z_std = [float(np.float32(v)) for v in noise]
    e = ose3.mat2euler(src[:, :3])
    scale = angle_std / 180.0 * math.pi
    Rt = ose3.euler2mat(e[0] + z[0] * scale, e[1] + z[1] * scale, e[2] + z[2] * scale)
    t = np.array([src[0, 3] + z[3] * x_std, src[1, 3] + z[4] * y_std, src[2, 3] + z[5] * z_std])
    pose = np.concatenate([Rt, t.reshape(3, 1)], 1)
    r_dist = angle_deg(src[:, :3], Rt)
    p = [(K[i, 0] * t[0] + K[i, 1] * t[1]) + K[i, 2] * t[2] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        cx, cy = np.float64(p[0]) / np.float64(p[2]), np.float64(p[1]) / np.float64(p[2])
    lo = float(np.float32(border))
    accept = bool(r_dist <= angle_max and lo < cx < width - lo and lo < cy < height - lo and t[2] > 0.0)
    return pose, r_dist, float(cx), float(cy), accept


def margin(r_dist, cx, cy, noise, width, height, border):
    """How far a candidate is from a threshold of the rule: (degrees from angle_max, pixels from the nearest border limit)."""
    lo = float(np.float32(border))
    return abs(r_dist - float(np.float32(noise[1]))), min(abs(cx - lo), abs(cx - (width - lo)), abs(cy - lo), abs(cy - (height - lo)))


def sample(pose_src, K, noise, width, height, border, max_attempts, seed, ids):
    """The attempt loop for every pair -> (pose_out (B,3,4) float32, attempts (B) int32, normals (B,6), borderline (B) bool):
    a pair is borderline when some attempt up to its acceptance lies within 1e-4 degrees of angle_max or 1e-4 px of a border
    limit."""
    pose_src = np.asarray(pose_src, np.float32)
    B = len(pose_src)
    ids = np.asarray(ids, np.uint64).reshape(B)
    out, attempts = pose_src.copy(), np.zeros(B, np.int32)
    zs, borderline, open_ = np.zeros((B, 6)), np.zeros(B, bool), np.ones(B, bool)
    for a in range(int(max_attempts)):
        idx = np.nonzero(open_)[0]
        if idx.size == 0:
            break
        z = normals(seed, ids[idx], a)
        for j, b in enumerate(idx):
            pose, r_dist, cx, cy, ok = perturb(pose_src[b], z[j], K, noise, width, height, border)
            dr, dp = margin(r_dist, cx, cy, noise, width, height, border)
            if dr < 1e-4 or dp < 1e-4:
                borderline[b] = True
            if ok:
                out[b], attempts[b], zs[b], open_[b] = pose.astype(np.float32), a + 1, z[j], False
    return out, attempts, zs, borderline


def below(words, n):
    return ((np.asarray(words, np.uint32).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def mask_dilate(seed, ids, max_thickness=10):
    """-> (thickness (n,4) int32, direction (n))."""
    c0, c1 = draw(seed, ids, 0, 2), draw(seed, ids, 1, 2)
    direction = below(c0[:, 0], 10)
    sides = np.stack([c0[:, 1], c0[:, 2], c0[:, 3], c1[:, 0]], 1)
    out = (below(sides, max_thickness) + 1).astype(np.int32)
    for k, skipped in enumerate(SKIPPED):
        out[np.isin(direction, skipped), k] = 0
    return out, direction


def random_poses(rng, n, z_lo=0.6, z_hi=1.2):
    """n float32 poses with uniform random rotations (QR of a Gaussian matrix), the object near the optical axis."""
    out = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out[i, :, :3] = q
        out[i, :, 3] = [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(z_lo, z_hi)]
    return out


LM_K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], np.float32)
TOOLKIT_NOISE = np.array([15.0, 45.0, 0.01, 0.01, 0.05], np.float32)


# ---- scenarios shared by tests/test_pose_sampler_host.py (their premises, on the CPU) and tests/test_gpu_pose_sampler.py
_CACHE = {}


def rejection_scenario():
    """B = 256 random poses at 0.6-1.2 m, angle_max 20, at most 64 attempts, seed 2333: the rule rejects often.
    -> dict(src, noise, seed, max_attempts, ids, pose, attempts, normals, borderline), the last four emulated once."""
    if "rej" not in _CACHE:
        src = random_poses(np.random.default_rng(2333), 256)
        noise = TOOLKIT_NOISE.copy()
        noise[1] = 20.0
        ids = np.arange(256, dtype=np.uint64)
        pose, attempts, zs, borderline = sample(src, LM_K, noise, 640, 480, 16.0, 64, 2333, ids)
        _CACHE["rej"] = dict(src=src, noise=noise, seed=2333, max_attempts=64, ids=ids, pose=pose, attempts=attempts, normals=zs,
                             borderline=borderline)
    return _CACHE["rej"]


STAT_SEED, STAT_B = 77, 4096


def stat_normals():
    """The first candidate's normals of draw ids 0 .. 4095 under STAT_SEED."""
    if "stat" not in _CACHE:
        _CACHE["stat"] = normals(STAT_SEED, np.arange(STAT_B, dtype=np.uint64), 0)
    return _CACHE["stat"]


def normal_statistics(z):
    """-> (largest |mean|, largest |std - 1|, largest |pairwise correlation|) of the columns of z."""
    c = np.corrcoef(z.T)
    return np.abs(z.mean(0)).max(), np.abs(z.std(0) - 1).max(), np.abs(c - np.eye(z.shape[1])).max()
