"""Shared by tests/test_cameras_host.py and tests/test_gpu_cameras.py: the three cameras and the B = 5 table [K0, K1, K0, K2, K1]
(repeats, and runs of length 1), and small scenes whose pairs are sane under every one of them.

K0 is the config matrix scaled to the test frame; K1 and K2 multiply fx, fy by 0.93 / 1.08 and shift cx, cy by +3.5 / -2.25 px:
non-dyadic factors, so the rounding of the inverse intrinsics is exercised, and close enough that a pose that is in frame under
one camera is in frame under all."""
import numpy as np

import flow_epe_emulation as emu
from mx_deepim_amd import synthetic
from oracle import zoom as ozoom

f32 = np.float32
ROWS = np.array([0, 1, 0, 2, 1])
B = len(ROWS)
MEANS = synthetic.PIXEL_MEANS[::-1].copy()


def cameras(H, W, K_config=synthetic.K_LINEMOD):
    """[K0, K1, K2] float32 for an H x W frame (the config matrix is a 480 x 640 camera)."""
    K0 = np.array(K_config, f32).reshape(3, 3).copy()
    K0[0] *= f32(W / 640.0)
    K0[1] *= f32(H / 480.0)
    out = [K0]
    for scale, shift in ((0.93, 3.5), (1.08, -2.25)):
        K = K0.copy()
        K[0, 0], K[1, 1] = K0[0, 0] * f32(scale), K0[1, 1] * f32(scale)
        K[0, 2], K[1, 2] = K0[0, 2] + f32(shift), K0[1, 2] + f32(shift)
        out.append(K)
    return out


def table(H, W, K_config=synthetic.K_LINEMOD):
    """(5,3,3) float32, C-contiguous: rows [K0, K1, K0, K2, K1]"""
    cams = cameras(H, W, K_config)
    return np.ascontiguousarray(np.stack([cams[c] for c in ROWS]), f32)


def _disc(H, W, cx, cy, r):
    y, x = np.mgrid[0:H, 0:W]
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r


def zoom_scene(H, W, seed, empty_rendered=3):
    """Inputs of the zoom front ends for B = 5 pairs: observed / rendered discs around the projected centre (black outside, so
    the mask-less ZoomImage boxes are the discs too), depths, poses about 1 m away. Pair `empty_rendered` has no rendered object
    (the rend[1] < 0 branch). → dict of float32 arrays."""
    rng = np.random.default_rng(seed)
    K0 = cameras(H, W)[0]
    s = {k: np.zeros((B, c, H, W), f32) for k, c in (("image_observed", 3), ("image_rendered", 3), ("mask_observed", 1),
                                                    ("mask_rendered", 1), ("depth_observed", 1), ("depth_rendered", 1))}
    s["src_pose"] = np.zeros((B, 3, 4), f32)
    for b in range(B):
        t = np.array([rng.uniform(-0.06, 0.06), rng.uniform(-0.05, 0.05), rng.uniform(0.8, 1.2)])
        s["src_pose"][b] = np.concatenate([synthetic.random_rotation(rng), t[:, None]], 1)
        c = K0.astype(np.float64) @ t
        cx, cy = c[0] / c[2], c[1] / c[2]
        for kind, dx, r in (("observed", rng.uniform(-3, 3), H / 5.0), ("rendered", rng.uniform(-3, 3), H / 6.0)):
            m = _disc(H, W, cx + dx, cy - dx, r)
            if kind == "rendered" and b == empty_rendered:
                m[:] = False
            s["mask_" + kind][b, 0] = m
            s["depth_" + kind][b, 0] = m * rng.uniform(0.7, 1.3, (H, W))
            s["image_" + kind][b] = m[None] * np.floor(rng.uniform(1, 256, (3, H, W)))
    for kind in ("observed", "rendered"):
        s["image_" + kind] = (s["image_" + kind] - MEANS.reshape(1, 3, 1, 1)).astype(f32)
    return s


def zoom_factors_oracle(s, K):
    """oracle/zoom.zoom_factor_from_valid for every pair of a zoom scene under one camera (raises on an empty observed box)"""
    _, _, H, W = s["mask_observed"].shape
    return np.stack([ozoom.zoom_factor_from_valid(s["mask_observed"][b, 0] > 0.3, s["mask_rendered"][b, 0] > 0.3, s["src_pose"][b],
                                                  K, H, W) for b in range(B)])


def flow_scene(H, W, seed, rows=None):
    """tests/flow_epe_emulation.scene with a camera per pair: pair b's observed depth is its rendered blob projected by ITS camera
    (so most of it is visible under that camera), `rows` = the (5,3,3) table (default: table(H, W))."""
    rows = table(H, W) if rows is None else rows
    s = emu.scene(B, H, W, seed)
    rng = np.random.default_rng(seed + 1)
    do = np.zeros((B, H, W), f32)
    for b in range(B):
        dr = s["depth_rendered"][b]
        pw, ph, pz, _, _ = emu.project(dr, emu.calc_KT(s["pose_rendered"][b], s["pose_observed"][b], rows[b]), emu.inv3(rows[b]))
        xr, yr = np.rint(pw), np.rint(ph)
        ok = (dr != 0) & (xr >= 0) & (xr < W) & (yr >= 0) & (yr < H)
        do[b][yr[ok].astype(int), xr[ok].astype(int)] = pz[ok]
        r = rng.uniform(size=(H, W))
        do[b][r < 0.1] += f32(0.01)
        do[b][r > 0.92] = 0
    s["depth_observed"] = do
    del s["K"]
    return s


def box_mesh(half=(0.05, 0.04, 0.03)):
    """An axis-aligned box: 8 vertices, 12 triangles (both windings appear on no face twice), vertex colours, uv and unit
    normals along the diagonals."""
    sx, sy, sz = half
    v = np.array([[x, y, z] for x in (-sx, sx) for y in (-sy, sy) for z in (-sz, sz)], f32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    colors = np.floor(255 * (0.5 + v / (2 * np.abs(v).max(0)))).astype(f32)
    uv = (0.5 + v[:, :2] / (2 * np.abs(v[:, :2]).max(0))).astype(f32)
    return {"vertices": v, "faces": faces, "colors": colors, "uv": uv,
            "normals": (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)}


def ellipsoid(axes=(0.05, 0.04, 0.035), n_lat=8, n_lon=16):
    m = synthetic.ellipsoid_mesh(np.asarray(axes), n_lat, n_lon)
    n = m["vertices"] / (np.asarray(axes, f32) ** 2)
    m["normals"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    return m


def poses(n, H, W, seed):
    """(tgt, src) (n,3,4) float32 pose pairs in frame under K0 (synthetic.sample_pose_pair keeps the centre 16 px inside)"""
    rng = np.random.default_rng(seed)
    K0 = cameras(H, W)[0]
    pairs = [synthetic.sample_pose_pair(rng, K0, H, W) for _ in range(n)]
    return np.stack([p[0] for p in pairs]).astype(f32), np.stack([p[1] for p in pairs]).astype(f32)


def arp_2d(pose_est, pose_gt, pts, K):
    """Average re-projection error in pixels, float64: mean_i |proj(K, R_e p_i + t_e) - proj(K, R_g p_i + t_g)|; pts (N,3)."""
    K = np.asarray(K, np.float64)

    def proj(P):
        q = (np.asarray(P[:, :3], np.float64) @ np.asarray(pts, np.float64).T + np.asarray(P[:, 3:], np.float64))
        q = K @ q
        return (q[:2] / q[2]).T
    return float(np.mean(np.linalg.norm(proj(pose_est) - proj(pose_gt), axis=1)))
