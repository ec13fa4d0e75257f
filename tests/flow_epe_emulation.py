"""numpy restatement of deepim_flow_epe (csrc/flow.hip: calc_KT_kernel, inv3d, calc_flow_core, flow_epe_partial_kernel): the
same float32 / float64 operations in the same order per pixel, without fused multiply-adds (numpy's elementwise arithmetic has
none; the library is built with -ffp-contract=off). Only the order of the SUMS differs (numpy's pairwise sum here, lane → wave →
block → partials on the device): the counts are exact, the sums agree to about N·2^-53 relative.

TEST INFRASTRUCTURE ONLY — the product never imports it."""
import os

import numpy as np

f32, f64 = np.float32, np.float64
KEYS = ("epe_all", "num_all", "epe_viz", "num_viz", "epe_vizbg", "num_vizbg")


def calc_KT(pose_src, pose_tgt, K):
    """calc_KT_kernel: se3_inverse(src), se3_mul(tgt, inv), K·M — float32, left to right."""
    S, T, K = np.asarray(pose_src, f32), np.asarray(pose_tgt, f32), np.asarray(K, f32).reshape(3, 3)
    Ri = np.zeros((3, 3), f32)
    ti = np.zeros(3, f32)
    for i in range(3):
        for j in range(3):
            Ri[i, j] = S[j, i]
    for i in range(3):
        ti[i] = f32(-1.0) * f32(f32(f32(Ri[i, 0] * S[0, 3]) + f32(Ri[i, 1] * S[1, 3])) + f32(Ri[i, 2] * S[2, 3]))
    M = np.zeros((3, 4), f32)
    for i in range(3):
        for j in range(3):
            M[i, j] = f32(f32(f32(T[i, 0] * Ri[0, j]) + f32(T[i, 1] * Ri[1, j])) + f32(T[i, 2] * Ri[2, j]))
        M[i, 3] = f32(f32(f32(f32(T[i, 0] * ti[0]) + f32(T[i, 1] * ti[1])) + f32(T[i, 2] * ti[2])) + T[i, 3])
    O = np.zeros((3, 4), f32)
    for i in range(3):
        for j in range(4):
            O[i, j] = f32(f32(f32(K[i, 0] * M[0, j]) + f32(K[i, 1] * M[1, j])) + f32(K[i, 2] * M[2, j]))
    return O


def inv3(K):
    """inv3d: adjugate in double, then float32 (np.linalg.inv of a float32 K gives float32)."""
    a, b, c, d, e, f, g, h, i = [float(v) for v in np.asarray(K, f32).reshape(9)]
    A, Bc, C = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * Bc + c * C
    o = [A / det, -(b * i - c * h) / det, (b * f - c * e) / det, Bc / det, (a * i - c * g) / det, -(a * f - c * d) / det,
         C / det, -(a * h - b * g) / det, (a * e - b * d) / det]
    return np.array(o, f64).astype(f32).reshape(3, 3)


def project(depth_src, KT, Kinv):
    """the float64 projection of calc_flow_core for every pixel → (pw, ph, pz, w, h), each (H,W) float64"""
    ds = np.asarray(depth_src, f32)
    H, W = ds.shape
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    h, w = h.astype(f64), w.astype(f64)
    Ki, T = np.asarray(Kinv, f32).astype(f64).reshape(9), np.asarray(KT, f32).astype(f64).reshape(12)
    d = ds.astype(f64)
    rx = Ki[0] * w + Ki[1] * h + Ki[2]
    ry = Ki[3] * w + Ki[4] * h + Ki[5]
    rz = Ki[6] * w + Ki[7] * h + Ki[8]
    X, Y, Z = d * rx, d * ry, d * rz
    xp = T[0] * X + T[1] * Y + T[2] * Z + T[3]
    yp = T[4] * X + T[5] * Y + T[6] * Z + T[7]
    zp = T[8] * X + T[9] * Y + T[10] * Z + T[11]
    pz = zp + 1e-15
    with np.errstate(divide="ignore", invalid="ignore"):
        pw, ph = xp / pz, yp / pz
    return pw, ph, pz, w, h


def calc_flow_core(depth_src, depth_tgt, KT, Kinv, thresh):
    """calc_flow_core for one pair → (dw, dh, vis): float64 (H,W) pw − w and ph − h (zero where not visible), bool (H,W)."""
    ds = np.asarray(depth_src, f32)
    dt_map = np.asarray(depth_tgt, f32)
    H, W = ds.shape
    pw, ph, pz, w, h = project(ds, KT, Kinv)
    nz = ds != 0
    pwr = np.where(nz, np.rint(pw), 0).astype(np.int64)
    phr = np.where(nz, np.rint(ph), 0).astype(np.int64)
    within = (pwr >= 0) & (pwr < W) & (phr >= 0) & (phr < H)
    pwc, phc = np.clip(pwr, 0, W - 1), np.clip(phr, 0, H - 1)
    dt = dt_map[phc, pwc].astype(f64)
    vis = nz & within & (np.abs(dt - pz) < f64(f32(thresh))) & (np.abs(dt) > 1e-10)
    return np.where(vis, pw - w, 0.0), np.where(vis, ph - h, 0.0), vis


def point_diff(flow_est, depth_src, depth_tgt, KT, Kinv, thresh, standard_rep):
    """flow_epe_partial_kernel per pixel of one pair → (point_diff float64 (H,W), vis, vizbg)."""
    dw, dh, vis = calc_flow_core(depth_src, depth_tgt, KT, Kinv, thresh)
    g0, g1 = (dw, dh) if standard_rep else (dh, dw)
    with np.errstate(over="ignore"):
        est = np.asarray(flow_est, f32).astype(np.float16).astype(f64)      # tester.py:350-352
    dx, dy = g0 - est[0], g1 - est[1]
    with np.errstate(over="ignore", invalid="ignore"):
        diff = np.sqrt(dx * dx + dy * dy)
    return diff, vis, vis | (np.asarray(depth_src, f32) == 0)


def flow_epe(flow_est, depth_rendered, depth_observed, pose_rendered, pose_observed, K, skip=None, thresh=3e-3,
             standard_rep=False):
    """deepim_flow_epe → (B,6) float64 rows {epe_all, num_all, epe_viz, num_viz, epe_vizbg, num_vizbg}."""
    B = len(flow_est)
    Kinv = inv3(K)
    out = np.zeros((B, 6), f64)
    for b in range(B):
        if skip is not None and skip[b] != 0:
            continue
        KT = calc_KT(pose_rendered[b], pose_observed[b], K)
        diff, vis, vizbg = point_diff(flow_est[b], depth_rendered[b], depth_observed[b], KT, Kinv, thresh, standard_rep)
        with np.errstate(invalid="ignore"):
            out[b] = [diff.sum(), diff.size, diff[vis].sum(), vis.sum(), diff[vizbg].sum(), vizbg.sum()]
    return out


def visible(depth_rendered, depth_observed, pose_rendered, pose_observed, K, thresh=3e-3):
    """(B,H,W) bool visibility of the batch."""
    Kinv = inv3(K)
    return np.stack([calc_flow_core(depth_rendered[b], depth_observed[b], calc_KT(pose_rendered[b], pose_observed[b], K), Kinv,
                                    thresh)[2] for b in range(len(depth_rendered))])


def par_generate_gt(frames, depth_factor=1000):
    """tester.py:530-557 on decoded frames → (depth_rendered, depth_observed) float32 (B,H,W): uint16 / DEPTH_FACTOR in float32
    (deepim_ingest_depth16's correctly rounded division), depth_gt_observed when the frames carry it, else depth_observed,
    zeroed where mask_gt_observed != mask_idx."""
    dr = np.asarray(frames["depth_rendered"]).astype(f32) / f32(depth_factor)
    key = "depth_gt_observed" if frames.get("depth_gt_observed") is not None else "depth_observed"
    do = np.asarray(frames[key]).astype(f32) / f32(depth_factor)
    idx = np.asarray(frames["mask_idx"]).reshape(-1, 1, 1)
    do[np.asarray(frames["mask_gt_observed"]) != idx] = 0
    return dr, do


def scene(B, H, W, seed):
    """A small synthetic batch for the kernel tests: K, float32 poses (a few degrees and a pixel or two apart), a rendered depth
    blob around 1 m with holes, and an observed depth built from the blob's own projection (so most of it is visible), then pushed
    out of the threshold or zeroed on some pixels; a random fp32 prediction. → dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    f = float(max(H, W))
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], f32)
    Kinv = inv3(K)

    def rot(a):
        a = np.deg2rad(a)
        cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
        return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    src, tgt = np.zeros((B, 3, 4), f32), np.zeros((B, 3, 4), f32)
    dr, do = np.zeros((B, H, W), f32), np.zeros((B, H, W), f32)
    for b in range(B):
        Rs = rot(rng.uniform(-20, 20, 3))
        ts = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 1.0])
        src[b] = np.concatenate([Rs, ts[:, None]], 1)
        tgt[b] = np.concatenate([rot(rng.uniform(-2, 2, 3)) @ Rs, (ts + rng.uniform(-1.5, 1.5, 3) / f)[:, None]], 1)
        dr[b, 1:H - 1, 1:W - 1] = rng.uniform(0.9, 1.1, (H - 2, W - 2))
        dr[b][rng.uniform(size=(H, W)) < 0.15] = 0
        pw, ph, pz, _, _ = project(dr[b], calc_KT(src[b], tgt[b], K), Kinv)
        xr, yr = np.rint(pw), np.rint(ph)
        ok = (dr[b] != 0) & (xr >= 0) & (xr < W) & (yr >= 0) & (yr < H)
        do[b][yr[ok].astype(int), xr[ok].astype(int)] = pz[ok]      # where two pixels land on one, the last one stays visible
        r = rng.uniform(size=(H, W))
        do[b][r < 0.1] += f32(0.01)
        do[b][r > 0.92] = 0
    est = (rng.standard_normal((B, 2, H, W)) * 2).astype(f32)
    return {"K": K, "pose_rendered": src, "pose_observed": tgt, "depth_rendered": dr, "depth_observed": do, "flow_est": est}


# ---- the reference-run fixture (tests/golden/flow_epe_golden.npz) and the comparison both test files use
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_epe_golden.npz")
FRAME_KEYS = ("depth_rendered", "depth_gt_observed", "depth_observed", "mask_gt_observed", "mask_idx", "pose_rendered",
              "pose_observed")
CASES = [(t, r, g) for t in ("a", "b") for r in (False, True) for g in (True, False)]


def frames_of(gold, tag, with_gt_depth=True):
    f = {k: gold["%s_%s" % (tag, k)] for k in FRAME_KEYS}
    if not with_gt_depth:
        f["depth_gt_observed"] = None
    return f


def ref_name(tag, rep, with_gt):
    return "%s_ref_%s_%s" % (tag, "std" if rep else "old", "gt" if with_gt else "nogt")


def check_rows(got, want, rel=1e-9):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got[:, 1::2], want[:, 1::2])                 # num_all, num_viz, num_vizbg
    np.testing.assert_allclose(got[:, 0::2], want[:, 0::2], rtol=rel, atol=0)   # epe_all, epe_viz, epe_vizbg
