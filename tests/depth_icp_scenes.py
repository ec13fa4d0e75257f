"""The scenes of tests/test_gpu_depth_icp_paths.py, built on the host from the restatement (tests/depth_icp_emulation.py), and the
conditions each of them has to meet before a device result is judged on it. tests/test_depth_icp_host.py asserts the same
conditions without a GPU, so a failure on the device is the kernel's and not the scene's.

Every `check_*` prints what it measured and then asserts; the seeds were searched on the CPU with these very functions."""
import numpy as np

import depth_icp_emulation as emu

from mx_deepim_amd import synthetic

AXES = (0.05, 0.08, 0.11)
RCOND = 1e-9
MARGIN, COND_MAX, MAX_TERMS = 1e-9, 1e6, 60000      # the existing parity caps; the 1e-11 · Σ|term| bound holds up to 60 000 terms
GATES_SEED, CHAIN_SEEDS = 0, (1, 2, 3)


class Case:
    pass


def small_pose(rng, deg, mm):
    R = synthetic.euler_to_mat(*np.deg2rad(rng.normal(0, deg, 3)))
    return np.concatenate([R, (rng.normal(0, 1, 3) * mm * 1e-3)[:, None]], 1).astype(np.float32)


def cameras(f, H, W, n):
    return np.stack([np.array([[f * s, 0, (W - 1) / 2 + dx], [0, f * s * 1.002, (H - 1) / 2 + dy], [0, 0, 1]], np.float32)
                     for s, dx, dy in ((1.0, 0.0, 0.0), (1.04, 0.3, -0.2), (0.97, -0.4, 0.25))[:n]])


def step(c, T0=None, src=None, normals=None, **kw):
    """the restatement's step on the case's targets and normals → (T, sys, status, info)"""
    args = dict(skip=None, dist_max=c.dist_max, min_pairs=c.min_pairs, rcond=RCOND)
    args.update(kw)
    return emu.icp_step(c.T0 if T0 is None else T0, c.src if src is None else src, c.tgt, c.normals if normals is None else normals,
                        c.K, **args)


def rim_filled(normals):
    """the normals with the frame's first and last rows and columns, which the normal pass leaves zero, copied from their
    neighbours: the step takes any normals, and only with these can a pixel that lands on the rim be used"""
    n = normals.copy()
    n[:, :, 0, :], n[:, :, -1, :] = n[:, :, 1, :], n[:, :, -2, :]
    n[:, :, :, 0], n[:, :, :, -1] = n[:, :, :, 1], n[:, :, :, -2]
    return n


def margins(info, m_step=np.inf):
    return min(min(info["margin"].values()), m_step)


# ------------------------------------------------------------------------------------------------- 1. every gate rejects --
def gates_case(seed=GATES_SEED):
    """37x59, B = 3: an odd plane of 2183 pixels (three blocks, a ragged last quad, unaligned bases of pairs 1 and 2). Camera 1
    has skew; pair 0's object crosses the right edge of the frame; pair 1 stands before a wall and starts far enough off for
    source pixels to land on the wall; pair 2's target has holes; dist_max is tight enough to reject."""
    H, W, f = 37, 59, 125.0
    rng = np.random.default_rng(seed)
    c = Case()
    c.H, c.W, c.B, c.min_pairs, c.max_step, c.dist_max = H, W, 3, 12, 0.01, 0.012
    c.K = cameras(f, H, W, 3)
    c.K[1][0][1] = 0.8
    src, tgt = [], []
    for b in range(3):
        R = synthetic.random_rotation(rng)
        t = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.7, 0.9)])
        if b == 0:
            t[0] = 0.13 * t[2] / 0.8
        gt = np.concatenate([R, t[:, None]], 1).astype(np.float32)
        Rs = synthetic.euler_to_mat(*np.deg2rad(rng.normal(0, 3.0, 3))) @ R
        sig = np.array([0.012, 0.012, 0.008]) if b == 1 else np.array([0.004, 0.004, 0.008])
        init = np.concatenate([Rs, (t + rng.normal(0, 1, 3) * sig)[:, None]], 1).astype(np.float32)
        src.append(synthetic.raycast_ellipsoid(init, AXES, c.K[b], H, W)[1])
        d = synthetic.raycast_ellipsoid(gt, AXES, c.K[b], H, W)[1]
        if b == 1:
            d = np.where(d > 0, d, np.float32(t[2] + 0.25)).astype(np.float32)       # a wall behind the object
        if b == 2:
            d[rng.random((H, W)) < 0.04] = 0                                         # holes in the measurement
        tgt.append(d)
    c.src, c.tgt = np.stack(src), np.stack(tgt)
    c.T0 = np.stack([small_pose(rng, 0.3, 1.0) for _ in range(3)])
    c.T0[0, 0, 3] += np.float32(0.012)
    c.normals, c.m_step = emu.depth_normals(c.tgt, c.K, c.max_step)
    c.T1, c.sys, c.status, c.info = step(c)
    # with max_step out of the way a hole's neighbours are without a normal because of the hole alone, not because of the jump to it
    c.wide_step = 10.0
    c.normals_wide, c.m_wide = emu.depth_normals(c.tgt, c.K, c.wide_step)
    # 2. every source point behind the camera: a half turn about y
    c.T_behind = np.tile(np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0]], np.float32), (3, 1, 1))
    c.behind = step(c, c.T_behind, dist_max=10.0)
    c.behind_foil = step(c, c.T_behind, dist_max=10.0, foil="no_behind")
    # 4. converged input: (a) the target against itself from the identity, (b) from a pose so small that θ² < 1e-8
    c.T_id = emu.identity(3)
    c.conv_a = step(c, c.T_id, c.tgt)
    c.T_tiny = np.stack([small_pose(rng, 1e-3, 0.01) for _ in range(3)])
    c.conv_b = step(c, c.T_tiny, c.tgt)
    # the frame's rim, the ragged last quad and the skew: the target against itself, 0.45 px to the right at the wall's depth so
    # that the skew's share of u (up to 0.11 px) decides roundings, with normals on the rim
    c.normals_rim = rim_filled(c.normals)
    c.T_shift = emu.identity(3)
    c.T_shift[:, 0, 3] = 0.0036
    c.rim = step(c, c.T_shift, c.tgt, c.normals_rim)
    c.rim_foil = step(c, c.T_shift, c.tgt, c.normals_rim, foil="no_skew")
    # 5. rcond on either side of the worst pair's smallest pivot; min_pairs met exactly and missed by one
    c.rho = step(c, rcond=0.0)[3]["rho"]
    c.worst = int(np.argmin(c.rho))
    c.rcond_lo, c.rcond_hi = float(c.rho.min()) / 2, float(c.rho.min()) * 2
    c.skip_worst = np.zeros(3, np.int32)
    c.skip_worst[c.worst] = 1
    c.solve_lo = step(c, rcond=c.rcond_lo)
    c.solve_hi = step(c, rcond=c.rcond_hi, skip=c.skip_worst)
    c.fewest = int(np.argmin(c.sys[:, 27]))
    c.count_fewest = int(c.sys[c.fewest, 27])
    c.pairs_met = step(c, min_pairs=c.count_fewest)
    c.pairs_missed = step(c, min_pairs=c.count_fewest + 1)
    return c


def check_parity_caps(name, res, m_step=np.inf, solved=None):
    """what the ULP2 and 1e-11 · Σ|term| bounds rest on; `solved`: the rows whose T is compared (default: those of status 0)"""
    _, sys_, status, info = res
    rows = status == 0 if solved is None else solved
    print(name, "margins", info["margin"], "step", m_step, "cond", info["cond"], "count", sys_[:, 27], "status", status,
          "theta2", info["theta2"], "pivot", info["pivot"])
    assert margins(info, m_step) > MARGIN
    assert (info["cond"][rows] <= COND_MAX).all()
    assert (sys_[:, 27] <= MAX_TERMS).all()


def check_gates(c):
    n = c.info["counts"]
    print("gates", {k: v.tolist() for k, v in n.items()}, "blocks", c.info["blocks"], "nblk", c.info["nblk"])
    check_parity_caps("gates", (c.T1, c.sys, c.status, c.info), c.m_step)
    assert c.H * c.W == 2183 and c.info["nblk"] == 3 and (c.info["blocks"]["with"] >= 2).all()
    assert (c.status == 0).all()
    assert n["outside"][0] >= 5
    assert n["far"].sum() >= 20
    assert n["hole"][2] >= 5
    assert (n["used"] >= 100).all()
    assert (n["no_normal"] > 0).all() and (n["behind"] == 0).all()
    assert (n["src"] == sum(n[k] for k in emu.OUTCOMES[1:])).all() and (n["used"] == c.sys[:, 27]).all()
    assert c.K[1][0][1] != 0
    assert all(not np.array_equal(c.T1[b], c.T0[b]) for b in range(3))
    holes = c.tgt == 0
    zero = (c.normals == 0).all(1)
    assert holes[2].sum() >= 40 and zero[2][holes[2]].all() and not zero[:, 1:-1, 1:-1].all()


def check_wide_normals(c):
    beside = (c.tgt[2, 1:-1, 1:-1] > 0) & (c.normals_wide[2, :, 1:-1, 1:-1] == 0).all(0)
    print("normals with max_step", c.wide_step, "margin", c.m_wide, "measured pixels without a normal beside a hole", beside.sum())
    assert c.m_wide > MARGIN
    assert beside.sum() >= 40
    assert (c.normals_wide[1, :, 1:-1, 1:-1] != 0).any(0).all()         # the wall pair: every jump is taken now


def check_behind(c):
    _, sys_, status, info = c.behind
    foil = c.behind_foil[3]["counts"]["used"]
    print("behind", info["counts"]["behind"], "a step without the gate would use", foil)
    assert (info["counts"]["behind"] == info["counts"]["src"]).all() and (info["counts"]["src"] > 0).all()
    assert (sys_ == 0).all() and (status == 1).all()
    np.testing.assert_array_equal(c.behind[0].view(np.uint32), c.T_behind.view(np.uint32))
    assert (foil >= 100).all()


def check_converged(c):
    T, sys_, status, info = c.conv_a
    print("converged (a) count", sys_[:, 27], "theta2", info["theta2"])
    assert (status == 0).all() and (sys_[:, 27] >= 100).all() and (sys_[:, 27] <= MAX_TERMS).all()
    assert (sys_[:, 21:27] == 0).all() and (sys_[:, 28] == 0).all()
    assert (info["theta2"] == 0).all()
    assert margins(info) > MARGIN
    np.testing.assert_array_equal(T.view(np.uint32), c.T_id.view(np.uint32))
    check_parity_caps("converged (b)", c.conv_b)
    T, sys_, status, info = c.conv_b
    assert (status == 0).all()
    assert (info["theta2"] < 1e-8).all() and (info["theta2"] > 0).all()
    assert all(not np.array_equal(T[b], c.T_tiny[b]) for b in range(3))


def check_rim(c):
    T, sys_, status, info = c.rim
    n, rim = info["counts"], info["rim"]
    skew = (np.abs(sys_ - c.rim_foil[1]) / np.maximum(info["abs"], 1e-300)).max(1)
    print("rim", {k: v.tolist() for k, v in n.items()}, {k: v.tolist() for k, v in rim.items()}, "tail", info["tail"],
          "a projection without skew moves the sums by", skew, "of their Σ|term|")
    check_parity_caps("rim", c.rim)
    assert (status == 0).all()
    assert all(rim[k][1] >= 30 for k in rim)                   # the wall pair uses all four sides of the rim,
    assert rim["right"][0] >= 5 and n["outside"][0] >= 5         # pair 0 the last column, next to pixels that leave the frame,
    assert (c.H * c.W) % 4 == 3 and info["tail"][1] == 3         # and the wall pair the three pixels of the ragged last quad
    assert c.K[1][0][1] != 0 and skew[1] >= 1e-3


def check_thresholds(c):
    print("rho", c.rho, "worst", c.worst, "rcond", c.rcond_lo, c.rcond_hi)
    check_parity_caps("rcond below", c.solve_lo, c.m_step)
    check_parity_caps("rcond above", c.solve_hi, c.m_step)
    assert (c.solve_lo[2] == 0).all()
    assert c.solve_hi[2][c.worst] == 2 and set(c.solve_hi[2].tolist()) <= {0, 2}
    assert c.solve_lo[3]["pivot"].min() >= 1e-6 and c.solve_hi[3]["pivot"].min() >= 1e-6
    for b in np.flatnonzero(c.solve_hi[2] == 2):
        np.testing.assert_array_equal(c.solve_hi[0][b].view(np.uint32), c.T0[b].view(np.uint32))
    b = c.fewest
    assert c.count_fewest >= 100 and (np.delete(c.sys[:, 27], b) > c.count_fewest).all()
    assert c.pairs_met[2].tolist() == [0, 0, 0]
    assert c.pairs_missed[2].tolist() == [int(i == b) for i in range(3)]
    np.testing.assert_array_equal(c.pairs_missed[0][b].view(np.uint32), c.T0[b].view(np.uint32))


# ------------------------------------------------------------------------------------------------- 3. long finish chains --
def chains_case(seed):
    """346x482, B = 2, two cameras, no wall: 163 blocks per pair, so the finish's 32 chains hold 5 or 6 partials each (the
    unroll-4 body and its remainder at both lengths), and the ellipsoid leaves whole blocks without a source pixel."""
    H, W, f = 346, 482, 1000.0
    rng = np.random.default_rng(seed)
    c = Case()
    c.H, c.W, c.B, c.min_pairs, c.max_step, c.dist_max = H, W, 2, 12, 0.01, 0.02
    c.K = cameras(f, H, W, 2)
    src, tgt = [], []
    for b in range(2):
        R = synthetic.random_rotation(rng)
        t = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.7, 0.9)])
        gt = np.concatenate([R, t[:, None]], 1).astype(np.float32)
        Rs = synthetic.euler_to_mat(*np.deg2rad(rng.normal(0, 3.0, 3))) @ R
        init = np.concatenate([Rs, (t + rng.normal(0, 1, 3) * np.array([0.004, 0.004, 0.008]))[:, None]], 1).astype(np.float32)
        src.append(synthetic.raycast_ellipsoid(init, AXES, c.K[b], H, W)[1])
        tgt.append(synthetic.raycast_ellipsoid(gt, AXES, c.K[b], H, W)[1])
    c.src, c.tgt = np.stack(src), np.stack(tgt)
    c.T0 = np.stack([small_pose(rng, 0.3, 1.0) for _ in range(2)])
    c.normals, c.m_step = emu.depth_normals(c.tgt, c.K, c.max_step)
    c.T1, c.sys, c.status, c.info = step(c)
    return c


def check_chains(c):
    print("chains", {k: v.tolist() for k, v in c.info["counts"].items()}, "blocks", c.info["blocks"], "nblk", c.info["nblk"])
    check_parity_caps("chains", (c.T1, c.sys, c.status, c.info), c.m_step)
    assert c.info["nblk"] == 163
    assert (c.info["blocks"]["with"] >= 64).all() and (c.info["blocks"]["without"] >= 16).all()
    assert (c.status == 0).all() and (c.sys[:, 27] >= 10000).all()
    assert all(not np.array_equal(c.T1[b], c.T0[b]) for b in range(2))


def table_rows(name, c, res):
    """one row of the coverage table of test_gpu_depth_icp_paths.py's docstring"""
    info = res[3]
    n = info["counts"]
    col = lambda v: " / ".join(str(int(x)) for x in v)          # noqa: E731
    th = " / ".join("%.1e" % x if np.isfinite(x) else "-" for x in info["theta2"])
    return "| %s | %d (%s empty) | %s | %s | %s | %s | %s | %s | %s | %s |" % (
        name, info["nblk"], col(info["blocks"]["without"]), col(n["src"]), col(n["behind"]), col(n["outside"]), col(n["hole"]),
        col(n["no_normal"]), col(n["far"]), col(n["used"]), th)
