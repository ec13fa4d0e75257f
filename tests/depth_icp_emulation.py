"""A numpy float64 restatement of csrc/icp.hip: deepim_depth_normals, deepim_icp_step and deepim_icp_apply.

Every per-pixel quantity is computed with the device's operations in the device's order (IEEE double +, -, *, /, sqrt and rint,
no fused multiply-add), from the same fp32 inputs, so every accept / reject decision is the device's as long as no value sits on
a threshold; the normals and `T` are rounded to fp32 where the device stores them. Two things are not bit-for-bit: the order in
which the accepted pixels' terms are added (numpy's pairwise sum here, lane → wave → block → finish on the device; the tests
bound that by 1e-11 · Σ|term|), and sin / cos of the Rodrigues exponential (each library's own, an ulp apart at most).

Besides the results the step reports what the tests need to know about the scene: cond(ΣJJᵀ), Σ|term| of every sum, and the
smallest distance of any decision to its threshold (`margin`): the rounding tie of the projected pixel (pixels), the frame edge
(pixels), dist_max (metres) and, from the normal pass, max_step (metres). It also reports what it decided, so that a test can
assert that its scene takes the paths it is about: how many source pixels of every pair met each outcome (`counts`), how many
1024-pixel blocks of a pair hold a source pixel and how many hold none (`blocks`), θ² of the solved twist (`theta2`: the
Rodrigues branch) and how far the Cholesky pivots stayed from rcond · max diag (`pivot`, `rho`).
"""
import numpy as np

IU = [(i, j) for i in range(6) for j in range(i, 6)]       # the 21 upper entries of ΣJJᵀ, row by row


def inv3d(K):
    """csrc/common.h inv3d: the adjugate inverse in double of a float32 K, operation for operation"""
    a, b, c, d, e, f, g, h, i = [np.float64(v) for v in np.asarray(K, np.float32).reshape(9)]
    A, Bc, C = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * Bc + c * C
    return np.array([A / det, -(b * i - c * h) / det, (b * f - c * e) / det,
                     Bc / det, (a * i - c * g) / det, -(a * f - c * d) / det,
                     C / det, -(a * h - b * g) / det, (a * e - b * d) / det])


def _vertex(kinv, x, y, d):
    """depth · K⁻¹ · (x, y, 1): ((k0·x + k1·y) + k2) · d per row"""
    return [((kinv[3 * r] * x + kinv[3 * r + 1] * y) + kinv[3 * r + 2]) * d for r in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def depth_normals(depth, K, max_step):
    """depth (B,H,W) float32 metres, K (B,3,3) float32 → (normals (B,3,H,W) float32, margin): the smallest
    | |d_neighbour − d_centre| − max_step | over the interior pixels whose five depths are positive (inf when there is none)"""
    depth = np.asarray(depth, np.float32)
    B, H, W = depth.shape
    ms = np.float64(np.float32(max_step))
    out = np.zeros((B, 3, H, W), np.float32)
    margin = np.inf
    if H < 3 or W < 3:
        return out, margin
    x, y = np.meshgrid(np.arange(1, W - 1, dtype=np.float64), np.arange(1, H - 1, dtype=np.float64))
    for b in range(B):
        kinv = inv3d(K[b])
        d = depth[b].astype(np.float64)
        dc, dl, dr, du, dd = d[1:-1, 1:-1], d[1:-1, :-2], d[1:-1, 2:], d[:-2, 1:-1], d[2:, 1:-1]
        ok = (dc > 0) & (dl > 0) & (dr > 0) & (du > 0) & (dd > 0)
        steps = np.stack([np.abs(n - dc) for n in (dl, dr, du, dd)])
        if ok.any():
            margin = min(margin, float(np.min(np.abs(steps[:, ok] - ms))))
        ok &= ~(steps > ms).any(0)
        vc = _vertex(kinv, x, y, dc)
        vl, vr = _vertex(kinv, x - 1, y, dl), _vertex(kinv, x + 1, y, dr)
        vu, vd = _vertex(kinv, x, y - 1, du), _vertex(kinv, x, y + 1, dd)
        c = _cross([vr[i] - vl[i] for i in range(3)], [vd[i] - vu[i] for i in range(3)])
        n2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        ok &= n2 > 0
        ln = np.sqrt(np.where(ok, n2, 1.0))
        n = [ci / ln for ci in c]
        flip = _dot(n, vc) > 0
        for i in range(3):
            out[b, i, 1:-1, 1:-1] = np.where(ok, np.where(flip, -n[i], n[i]), 0.0).astype(np.float32)
    return out, margin


BLOCK_PIX = 1024                                            # the pixel kernel's block: 256 lanes x 4 consecutive source pixels
FOILS = (None, "no_behind", "no_skew")
OUTCOMES = ("src", "behind", "outside", "hole", "no_normal", "far", "used")


def cholesky_solve(A, g, rcond, pivots=None):
    """The finish's solve: A (6,6) symmetric (upper entries used), g (6). → (xi or None when a pivot ≤ rcond · max diag).
    `pivots`, a list, receives (v_j, max diag) of every pivot that was compared with rcond · max diag, the refused one included."""
    L = np.zeros((6, 6))
    maxdiag = max(A[i, i] for i in range(6))
    lim = rcond * maxdiag
    for j in range(6):
        s = A[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        if pivots is not None:
            pivots.append((s, maxdiag))
        if not s > lim:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            s = A[j, i]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    yv = np.zeros(6)
    for i in range(6):
        s = g[i]
        for k in range(i):
            s = s - L[i, k] * yv[k]
        yv[i] = s / L[i, i]
    xi = np.zeros(6)
    for i in range(5, -1, -1):
        s = yv[i]
        for k in range(i + 1, 6):
            s = s - L[k, i] * xi[k]
        xi[i] = s / L[i, i]
    return xi


def theta2(xi):
    """θ² of the twist as the finish computes it"""
    w = xi[:3]
    return (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]


def se3_exp(xi):
    """(R, t) of exp(ξ̂), ξ = (ω, v): Rodrigues with its V matrix; the series below θ² = 1e-8"""
    w, v = xi[:3], xi[3:]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if th2 < 1e-8:
        a, bb, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        th = np.sqrt(th2)
        sh = np.sin(0.5 * th)
        a, bb, c = np.sin(th) / th, 2.0 * sh * sh / th2, (th - np.sin(th)) / (th2 * th)
    Wm = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    W2 = np.array([[-(w[1] * w[1] + w[2] * w[2]), w[0] * w[1], w[0] * w[2]],
                   [w[0] * w[1], -(w[0] * w[0] + w[2] * w[2]), w[1] * w[2]],
                   [w[0] * w[2], w[1] * w[2], -(w[0] * w[0] + w[1] * w[1])]])
    eye = np.eye(3)
    R = (eye + a * Wm) + bb * W2
    V = (eye + bb * Wm) + c * W2
    t = np.array([(V[i, 0] * v[0] + V[i, 1] * v[1]) + V[i, 2] * v[2] for i in range(3)])
    return R, t


def _compose(Ra, ta, Rb, tb):
    """[Ra·Rb | Ra·tb + ta] with the device's operation order"""
    R = np.array([[(Ra[i, 0] * Rb[0, j] + Ra[i, 1] * Rb[1, j]) + Ra[i, 2] * Rb[2, j] for j in range(3)] for i in range(3)])
    t = np.array([((Ra[i, 0] * tb[0] + Ra[i, 1] * tb[1]) + Ra[i, 2] * tb[2]) + ta[i] for i in range(3)])
    return R, t


def icp_step(T, depth_src, depth_tgt, normals_tgt, K, skip=None, dist_max=0.02, min_pairs=12, rcond=1e-9, foil=None):
    """One deepim_icp_step. T (B,3,4) float32, depths (B,H,W) float32, normals (B,3,H,W) float32, K (B,3,3) float32.
    → (T_new (B,3,4) float32, sys (B,30) float64, status (B) int32, info) with info = {"cond": (B), "abs": (B,30) Σ|term| of
    every sys entry, "margin": {"tie", "edge", "dist"}, "counts": {outcome: (B) int64} for the OUTCOMES (src = behind + outside +
    hole + no_normal + far + used; a pixel counts for the first gate that rejects it, in the kernel's order), "nblk": blocks per
    pair, "blocks": {"with", "without": (B)} blocks with and without a source pixel, "theta2": (B) θ² of the solved twist (nan
    where none was solved), "rho": (B) smallest compared pivot / max diag, "pivot": (B) smallest |v_j − rcond · max diag| /
    max diag over the compared pivots (inf where the count stopped the pair before the solve), "rim": {"left", "right", "top",
    "bottom": (B)} the used pixels whose target pixel lies in the frame's first or last column or row, "tail": (B) the used
    source pixels of a ragged last quad (H·W no multiple of 4)}.
    `foil` names one way of being wrong, for a test to assert that its scene would notice it: "no_behind" is the step without
    its z′ > 0 test, "no_skew" projects without K[0][1]. The default, None, is the device's arithmetic."""
    assert foil in FOILS
    T = np.asarray(T, np.float32)
    depth_src, depth_tgt = np.asarray(depth_src, np.float32), np.asarray(depth_tgt, np.float32)
    normals_tgt = np.asarray(normals_tgt, np.float32)
    B, H, W = depth_src.shape
    dm = np.float64(np.float32(dist_max))
    dm2 = dm * dm
    T_new, sys_ = T.copy(), np.zeros((B, 30))
    abs_ = np.zeros((B, 30))
    status = np.zeros(B, np.int32)
    cond = np.full(B, np.inf)
    margin = {"tie": np.inf, "edge": np.inf, "dist": np.inf}
    counts = {k: np.zeros(B, np.int64) for k in OUTCOMES}
    nblk = -(-(H * W) // BLOCK_PIX)
    blocks = {"with": np.zeros(B, np.int64), "without": np.zeros(B, np.int64)}
    th2, rho, pivot = np.full(B, np.nan), np.full(B, np.inf), np.full(B, np.inf)
    rim = {k: np.zeros(B, np.int64) for k in ("left", "right", "top", "bottom")}
    tail = np.zeros(B, np.int64)
    xg, yg = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for b in range(B):
        Kd = np.asarray(K[b], np.float32).astype(np.float64).reshape(9)
        kinv = inv3d(K[b])
        Td = T[b].astype(np.float64)
        ds = depth_src[b].astype(np.float64)
        sel = ds > 0
        blocks["with"][b] = len(np.unique(np.flatnonzero(sel.reshape(-1)) // BLOCK_PIX))
        blocks["without"][b] = nblk - blocks["with"][b]
        counts["src"][b] = int(sel.sum())
        x, y, d = xg[sel], yg[sel], ds[sel]
        in_tail = (y * W + x) >= (H * W) // 4 * 4
        p = _vertex(kinv, x, y, d)
        pp = [((Td[i, 0] * p[0] + Td[i, 1] * p[1]) + Td[i, 2] * p[2]) + Td[i, 3] for i in range(3)]
        keep = pp[2] > 0 if foil != "no_behind" else np.ones(len(d), bool)
        counts["behind"][b] = int((~keep).sum())
        pp, in_tail = [v[keep] for v in pp], in_tail[keep]
        if foil == "no_skew":
            Kd[1] = 0.0
        uz = (Kd[6] * pp[0] + Kd[7] * pp[1]) + Kd[8] * pp[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = ((Kd[0] * pp[0] + Kd[1] * pp[1]) + Kd[2] * pp[2]) / uz
            v = ((Kd[3] * pp[0] + Kd[4] * pp[1]) + Kd[5] * pp[2]) / uz
        px, py = np.rint(u), np.rint(v)
        if len(u):
            fin = np.isfinite(u) & np.isfinite(v)
            for c, r in ((u[fin], px[fin]), (v[fin], py[fin])):
                if len(c):
                    margin["tie"] = min(margin["tie"], float(np.min(np.abs(np.abs(c - r) - 0.5))))
            for c, n in ((u[fin], W), (v[fin], H)):
                if len(c):
                    margin["edge"] = min(margin["edge"], float(np.min(np.minimum(np.abs(c + 0.5), np.abs(c - (n - 0.5))))))
        inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        counts["outside"][b] = int((~inside).sum())
        pp, in_tail = [v[inside] for v in pp], in_tail[inside]
        ix, iy = px[inside].astype(np.int64), py[inside].astype(np.int64)
        dt = depth_tgt[b][iy, ix].astype(np.float64)
        n = [normals_tgt[b, i][iy, ix].astype(np.float64) for i in range(3)]
        ok = (dt > 0) & ~((n[0] == 0) & (n[1] == 0) & (n[2] == 0))
        counts["hole"][b] = int((~(dt > 0)).sum())
        counts["no_normal"][b] = int(((dt > 0) & ~ok).sum())
        q = _vertex(kinv, px[inside], py[inside], dt)
        e = [pp[i] - q[i] for i in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        if ok.any():
            margin["dist"] = min(margin["dist"], float(np.min(np.abs(np.sqrt(d2[ok]) - dm))))
        counts["far"][b] = int((ok & (d2 > dm2)).sum())
        ok &= ~(d2 > dm2)
        counts["used"][b] = int(ok.sum())
        for k, hit in (("left", ix == 0), ("right", ix == W - 1), ("top", iy == 0), ("bottom", iy == H - 1)):
            rim[k][b] = int((ok & hit).sum())
        tail[b] = int((ok & in_tail).sum())
        pp, n, e = [v[ok] for v in pp], [v[ok] for v in n], [v[ok] for v in e]
        r = _dot(n, e)
        J = _cross(pp, n) + n
        terms = [J[i] * J[j] for i, j in IU] + [-(J[i] * r) for i in range(6)] + [np.ones_like(r), r * r]
        for k, t in enumerate(terms):
            sys_[b, k] = np.sum(t)
            abs_[b, k] = np.sum(np.abs(t))
        A = np.zeros((6, 6))
        for k, (i, j) in enumerate(IU):
            A[i, j] = A[j, i] = sys_[b, k]
        if sys_[b, 27] < min_pairs:
            status[b] = 1
            continue
        cond[b] = np.linalg.cond(A)
        pv = []
        xi = cholesky_solve(A, sys_[b, 21:27], rcond, pv)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho[b] = min(v / m for v, m in pv)
            pivot[b] = min(abs(v - rcond * m) / m for v, m in pv)
        if xi is None:
            status[b] = 2
            continue
        if skip is not None and skip[b]:
            continue
        th2[b] = theta2(xi)
        Re, te = se3_exp(xi)
        Rn, tn = _compose(Re, te, Td[:, :3], Td[:, 3])
        T_new[b] = np.concatenate([Rn, tn[:, None]], 1).astype(np.float32)
    return T_new, sys_, status, {"cond": cond, "abs": abs_, "margin": margin, "counts": counts, "nblk": nblk, "blocks": blocks,
                                 "theta2": th2, "rho": rho, "pivot": pivot, "rim": rim, "tail": tail}


def icp_apply(T, pose):
    """deepim_icp_apply: [R_T·R | R_T·t + t_T], float32 (B,3,4)"""
    T, pose = np.asarray(T, np.float32).astype(np.float64), np.asarray(pose, np.float32).astype(np.float64)
    out = np.zeros(T.shape, np.float32)
    for b in range(len(T)):
        R, t = _compose(T[b, :, :3], T[b, :, 3], pose[b, :, :3], pose[b, :, 3])
        out[b] = np.concatenate([R, t[:, None]], 1).astype(np.float32)
    return out


def identity(B):
    return np.tile(np.eye(3, 4, dtype=np.float32), (B, 1, 1))


def refine(poses, render, depth_tgt, K, skip=None, dist_max=0.02, max_step=0.01, min_pairs=12, rcond=1e-9, outer=2, inner=5):
    """DepthICP.refine with `render(poses) -> (B,H,W) float32 depth` in the rasteriser's place.
    → (poses (B,3,4) float32, status (B) of the last step, infos of every step)"""
    poses = np.asarray(poses, np.float32).copy()
    normals, m = depth_normals(depth_tgt, K, max_step)
    infos, status = [], None
    for _ in range(outer):
        src = render(poses)
        T = identity(len(poses))
        for _ in range(inner):
            T, _, status, info = icp_step(T, src, depth_tgt, normals, K, skip, dist_max, min_pairs, rcond)
            infos.append(info)
        poses = icp_apply(T, poses)
    return poses, status, infos


def add_metric(pose_a, pose_b, points):
    """mean distance of the (N,3) model points under the two (3,4) poses"""
    pa = points @ pose_a[:, :3].astype(np.float64).T + pose_a[:, 3]
    pb = points @ pose_b[:, :3].astype(np.float64).T + pose_b[:, 3]
    return float(np.mean(np.linalg.norm(pa - pb, axis=1)))
