"""csrc/icp.hip on the paths that the parity scenes of test_gpu_depth_icp.py leave untaken: every pixel gate rejecting, finish
chains of more than one partial, the Rodrigues series branch, rcond and min_pairs decided on both sides, and the entries' refusals.

The scenes are built by tests/depth_icp_scenes.py from the restatement (tests/depth_icp_emulation.py), which reports what it
decided; every test asserts its scene's conditions (scenes.check_*) before it judges a device result, and
tests/test_depth_icp_host.py asserts the same conditions without a GPU. What the restatement decides on them (per pair):

| case | blocks per pair | source pixels | behind camera | outside frame | target hole | zero normal | beyond dist_max | used | θ² of the step |
|---|---|---|---|---|---|---|---|---|---|
| gates 37x59 | 3 (1 / 1 / 1 empty) | 443 / 476 / 605 | 0 / 0 / 0 | 29 / 0 / 4 | 21 / 0 / 46 | 147 / 102 / 166 | 91 / 168 / 87 | 155 / 206 / 302 | 9.2e-3 / 2.3e-2 / 2.1e-3 |
| behind camera | 3 (1 / 1 / 1 empty) | 443 / 476 / 605 | 443 / 476 / 605 | 0 / 0 / 0 | 0 / 0 / 0 | 0 / 0 / 0 | 0 / 0 / 0 | 0 / 0 / 0 | none: status 1 |
| converged (a) | 3 (1 / 0 / 0 empty) | 409 / 2183 / 598 | 0 / 0 / 0 | 0 / 0 / 0 | 0 / 0 / 0 | 155 / 426 / 208 | 0 / 0 / 0 | 254 / 1757 / 390 | 0 / 0 / 0 |
| converged (b) | 3 (1 / 0 / 0 empty) | 409 / 2183 / 598 | 0 / 0 / 0 | 0 / 0 / 0 | 0 / 0 / 0 | 155 / 426 / 208 | 0 / 0 / 0 | 254 / 1757 / 390 | 2.4e-9 / 2.6e-9 / 1.5e-9 |
| rim | 3 (1 / 0 / 0 empty) | 409 / 2183 / 598 | 0 / 0 / 0 | 18 / 0 / 0 | 7 / 0 / 57 | 113 / 238 / 148 | 0 / 0 / 0 | 271 / 1945 / 393 | 5.9e-5 / 8.8e-7 / 9.1e-4 |
| chains 346x482, seed 1 | 163 (63 / 87 empty) | 35020 / 29980 | 0 / 0 | 0 / 0 | 1730 / 5415 | 311 / 311 | 7 / 9618 | 32972 / 14636 | 5.7e-4 / 5.4e-2 |
| chains 346x482, seed 2 | 163 (55 / 66 empty) | 31389 / 32990 | 0 / 0 | 0 / 0 | 2363 / 2919 | 305 / 288 | 756 / 4981 | 27965 / 24802 | 8.1e-3 / 1.1e-2 |
| chains 346x482, seed 3 | 163 (36 / 26 empty) | 27989 / 46467 | 0 / 0 | 0 / 0 | 3140 / 2655 | 251 / 430 | 1515 / 333 | 23083 / 43049 | 2.4e-2 / 7.9e-3 |

The gates scene's smallest pivot / max diag is 1.6e-5 / 5.5e-5 / 1.4e-4: rcond = 7.8e-6 solves all three pairs, rcond = 3.1e-5 refuses
pair 0, and every compared pivot stays >= 7.8e-6 · max diag from the limit. Pair 0's count of 155 is the min_pairs that is met and missed.

(gates: 37x59, an odd plane of 2183 pixels — pairs 1 and 2 start at addresses that are no multiple of 16 bytes and block 2 ends in
a ragged quad; camera 1 has skew, pair 0 leaves the frame on the right, pair 1 stands before a wall, pair 2's target has holes.
rim: the gates scene's targets against themselves, started 0.45 px to the right, with normals copied onto the frame's first and last
rows and columns, which the normal pass leaves zero and which therefore hide the frame gate's last column and row in every other
case: pair 1 uses 37 / 37 / 59 / 59 pixels of the left / right / top / bottom rim and the three pixels of the ragged last quad, pair
0 uses 17 pixels of the last column beside 18 that leave the frame, and a projection without K[0][1] would move pair 1's sums by
8e-3 of their Σ|term|. chains: 346x482, 163 blocks per pair, so each of the finish's 32 chains adds 5 or 6 partials.)

Bounds, as in test_gpu_depth_icp.py: normals and T within 2 ulp of 1 (2.4e-7) under cond <= 1e6 and every decision farther than
1e-9 from its threshold; a sum within 1e-11 of its Σ|term| — (n − 1) · 1.1e-16 for the order of n <= 60 000 terms plus about ten
roundings per term stays under 7e-12; counts and statuses exact; the same call twice gives the same bytes; a single-pair call
with K_host = K[b] gives the bytes of row b of the batched call through the bound table."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_icp_emulation as emu  # noqa: E402
import depth_icp_scenes as scenes  # noqa: E402

from mx_deepim_amd.runtime import lib  # noqa: E402

pytestmark = pytest.mark.gpu
ULP2 = 2.4e-7
RCOND = scenes.RCOND


def upload(c, ctx):
    B, H, W = c.B, c.H, c.W
    c.ctx = ctx
    c.K_d = ctx.array(c.K)
    c.src_d, c.tgt_d = ctx.array(c.src.reshape(B, 1, H, W)), ctx.array(c.tgt.reshape(B, 1, H, W))
    c.nrm_d = ctx.array(c.normals)            # the step is fed the restatement's normals: the two passes are judged apart
    return c


@pytest.fixture(scope="module")
def gates(ctx):
    return upload(scenes.gates_case(), ctx)


@pytest.fixture(scope="module", params=scenes.CHAIN_SEEDS)
def chains(request, ctx):
    return upload(scenes.chains_case(request.param), ctx)


def run_step(c, T0=None, src_d=None, nrm_d=None, dist_max=None, min_pairs=None, rcond=RCOND, skip=None, K_host=None, b=None,
             with_sys=True):
    """one deepim_icp_step on the case's targets and normals → (T, sys or None, status) on the host"""
    ctx, H, W = c.ctx, c.H, c.W
    sl = slice(0, c.B) if b is None else slice(b, b + 1)
    n = sl.stop - sl.start
    T = ctx.array((c.T0 if T0 is None else T0)[sl])
    sys_d = ctx.zeros((n, 30), dtype=np.float64) if with_sys else None
    st = ctx.array(np.full(n, -1, np.int32), dtype=np.int32)
    skip_d = None if skip is None else ctx.array(skip[sl], dtype=np.int32)
    if K_host is None:
        ctx.bind_cameras(c.K_d)
    lib.deepim_icp_step(ctx.handle, T, sys_d, st, (c.src_d if src_d is None else src_d)[sl], c.tgt_d[sl],
                        (c.nrm_d if nrm_d is None else nrm_d)[sl], K_host, skip_d,
                        ctypes.c_float(c.dist_max if dist_max is None else dist_max),
                        c.min_pairs if min_pairs is None else min_pairs, ctypes.c_double(rcond), n, H, W)
    return T.asnumpy(), sys_d.asnumpy() if with_sys else None, st.asnumpy()


def judge(name, got, want):
    """a device step against the restatement's: statuses and counts exact, sums within 1e-11 · Σ|term|, T within ULP2"""
    (T, sys_, st), (e_T, e_sys, e_st, info) = got, want
    assert (e_sys[:, 27] <= scenes.MAX_TERMS).all()
    err = np.abs(sys_ - e_sys)
    print(name, "status", st, "count", sys_[:, 27], "max sys error / Σ|term|", (err / np.maximum(info["abs"], 1e-300)).max(),
          "max |T error|", np.abs(T.astype(np.float64) - e_T).max())
    np.testing.assert_array_equal(st, e_st)
    np.testing.assert_array_equal(sys_[:, 27], e_sys[:, 27])
    assert (err <= 1e-11 * info["abs"]).all()
    assert (sys_[:, 29] == 0).all()
    assert np.isfinite(T).all()
    assert np.abs(T.astype(np.float64) - e_T).max() <= ULP2


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def repeatable_and_row_for_row(c, got, **kw):
    """the same call again gives the same bytes, and so does every pair alone with its camera passed from the host"""
    assert same_bytes(got, run_step(c, **kw))
    skip = kw.pop("skip", None)
    for b in range(c.B):
        one = run_step(c, K_host=np.ascontiguousarray(c.K[b]), b=b, skip=skip, **kw)
        assert one[0][0].tobytes() == got[0][b].tobytes() and one[1][0].tobytes() == got[1][b].tobytes() and one[2][0] == got[2][b]


def run_normals(c, K_host=None, b=None, max_step=None):
    ctx, H, W = c.ctx, c.H, c.W
    depth = c.tgt_d if b is None else c.tgt_d[b:b + 1]
    out = ctx.array(np.full((depth.shape[0], 3, H, W), 7.0, np.float32))
    if K_host is None:
        ctx.bind_cameras(c.K_d)
    lib.deepim_depth_normals(ctx.handle, out, depth, K_host, ctypes.c_float(c.max_step if max_step is None else max_step),
                             depth.shape[0], H, W)
    return out.asnumpy()


# ------------------------------------------------------------------------------------------------- 1. every gate rejects --
def test_step_with_every_gate_rejecting(gates):
    c = gates
    scenes.check_gates(c)
    got = run_step(c)
    judge("gates", got, (c.T1, c.sys, c.status, c.info))
    repeatable_and_row_for_row(c, got)


def test_normals_over_holes_and_under_a_skewed_camera(gates):
    c = gates
    scenes.check_gates(c)
    got = run_normals(c)
    print("max |normal error|", np.abs(got.astype(np.float64) - c.normals).max())
    np.testing.assert_array_equal((got == 0).all(1), (c.normals == 0).all(1))
    assert np.abs(got.astype(np.float64) - c.normals).max() <= ULP2
    np.testing.assert_array_equal(got.view(np.uint32), run_normals(c).view(np.uint32))
    for b in range(c.B):
        np.testing.assert_array_equal(run_normals(c, np.ascontiguousarray(c.K[b]), b)[0].view(np.uint32), got[b].view(np.uint32))


def test_normals_beside_holes_without_the_help_of_max_step(gates):
    """a hole's neighbours also fail the max_step test (a step of the whole depth); with max_step = 10 m the > 0 tests stand alone"""
    c = gates
    scenes.check_wide_normals(c)
    got = run_normals(c, max_step=c.wide_step)
    print("max |normal error|", np.abs(got.astype(np.float64) - c.normals_wide).max())
    np.testing.assert_array_equal((got == 0).all(1), (c.normals_wide == 0).all(1))
    assert np.abs(got.astype(np.float64) - c.normals_wide).max() <= ULP2
    for b in range(c.B):
        one = run_normals(c, np.ascontiguousarray(c.K[b]), b, max_step=c.wide_step)
        np.testing.assert_array_equal(one[0].view(np.uint32), got[b].view(np.uint32))


@pytest.mark.parametrize("H,W", [(2, 9), (1, 1)])
def test_normals_of_a_frame_without_an_interior_are_zeros(ctx, gates, H, W):
    depth = np.full((2, 1, H, W), 0.8, np.float32)
    e_n, _ = emu.depth_normals(depth[:, 0], gates.K[:2], 0.01)
    assert (e_n == 0).all()
    for K_host in (None, np.ascontiguousarray(gates.K[1])):
        out = ctx.array(np.full((2, 3, H, W), 7.0, np.float32))
        if K_host is None:
            ctx.bind_cameras(gates.K_d)
        lib.deepim_depth_normals(ctx.handle, out, ctx.array(depth), K_host, ctypes.c_float(0.01), 2, H, W)
        np.testing.assert_array_equal(out.asnumpy().view(np.uint32), e_n.view(np.uint32))


def test_rim_ragged_quad_and_skew_decide_pixels(gates):
    """the frame gate at its last column and row, the last quad of an odd plane and K[0][1] in the projection: the normal pass
    leaves the rim without normals, so only a step fed normals there can show an off-by-one of the frame gate"""
    c = gates
    scenes.check_rim(c)
    nrm_d = c.ctx.array(c.normals_rim)
    got = run_step(c, T0=c.T_shift, src_d=c.tgt_d, nrm_d=nrm_d)
    judge("rim", got, c.rim)
    repeatable_and_row_for_row(c, got, T0=c.T_shift, src_d=c.tgt_d, nrm_d=nrm_d)


# ------------------------------------------------------------------------------------------------- 2. behind the camera --
def test_points_behind_the_camera_are_not_paired(gates):
    c = gates
    scenes.check_behind(c)
    T, sys_, st = got = run_step(c, T0=c.T_behind, dist_max=10.0)
    print("behind: count", sys_[:, 27], "status", st)
    assert (sys_ == 0).all()
    assert st.tolist() == [1, 1, 1]
    np.testing.assert_array_equal(T.view(np.uint32), c.T_behind.view(np.uint32))
    judge("behind", got, c.behind)
    repeatable_and_row_for_row(c, got, T0=c.T_behind, dist_max=10.0)


# ------------------------------------------------------------------------------------------------- 3. long finish chains --
def test_finish_adds_chains_of_five_and_six_partials(chains):
    c = chains
    scenes.check_chains(c)
    got = run_step(c)
    judge("chains", got, (c.T1, c.sys, c.status, c.info))
    repeatable_and_row_for_row(c, got)


# ------------------------------------------------------------------------------------------------------- 4. converged --
def test_converged_input_leaves_T_bit_for_bit(gates):
    c = gates
    scenes.check_converged(c)
    T, sys_, st = got = run_step(c, T0=c.T_id, src_d=c.tgt_d)
    judge("converged (a)", got, c.conv_a)
    assert st.tolist() == [0, 0, 0]
    assert (sys_[:, 21:27] == 0).all() and (sys_[:, 28] == 0).all()
    assert np.isfinite(T).all()
    np.testing.assert_array_equal(T.view(np.uint32), c.T_id.view(np.uint32))


def test_tiny_step_takes_the_series_branch(gates):
    c = gates
    scenes.check_converged(c)
    got = run_step(c, T0=c.T_tiny, src_d=c.tgt_d)
    judge("converged (b)", got, c.conv_b)
    repeatable_and_row_for_row(c, got, T0=c.T_tiny, src_d=c.tgt_d)


# ------------------------------------------------------------------------------------------------------ 5. thresholds --
def test_rcond_is_decided_on_both_sides_and_skip_keeps_the_status(gates):
    c = gates
    scenes.check_thresholds(c)
    lo = run_step(c, rcond=c.rcond_lo)
    judge("rcond below", lo, c.solve_lo)
    assert lo[2].tolist() == [0, 0, 0]
    hi = run_step(c, rcond=c.rcond_hi, skip=c.skip_worst)          # the skipped row is the refused one: its status is still 2
    judge("rcond above", hi, c.solve_hi)
    assert hi[2][c.worst] == 2
    for b in np.flatnonzero(hi[2] == 2):
        np.testing.assert_array_equal(hi[0][b].view(np.uint32), c.T0[b].view(np.uint32))
    assert hi[1][c.worst].tobytes() == lo[1][c.worst].tobytes()          # refused, yet its sums are written: the same pixels' sums
    plain = run_step(c, rcond=c.rcond_hi)                               # without skip: the same bytes, the refusal alone holds T
    assert same_bytes(hi, plain)
    repeatable_and_row_for_row(c, hi, rcond=c.rcond_hi, skip=c.skip_worst)


def test_min_pairs_is_met_exactly_and_missed_by_one(gates):
    c = gates
    scenes.check_thresholds(c)
    b = c.fewest
    met = run_step(c, min_pairs=c.count_fewest)
    judge("min_pairs = count", met, c.pairs_met)
    assert met[2].tolist() == [0, 0, 0] and met[1][b, 27] == c.count_fewest
    missed = run_step(c, min_pairs=c.count_fewest + 1)
    judge("min_pairs = count + 1", missed, c.pairs_missed)
    assert missed[2].tolist() == [int(i == b) for i in range(3)]
    np.testing.assert_array_equal(missed[0][b].view(np.uint32), c.T0[b].view(np.uint32))
    assert missed[1].tobytes() == met[1].tobytes()


# --------------------------------------------------------------------------------------------------- 6. host contract --
def test_the_entries_refuse_bad_arguments_and_write_nothing(gates):
    c = gates
    ctx, H, W = c.ctx, c.H, c.W
    K0 = np.ascontiguousarray(c.K[0])
    sys0, st0, n0 = np.full((3, 30), 7.0), np.full(3, 9, np.int32), np.full((3, 3, H, W), 7.0, np.float32)
    T, sys_d, st, nrm = ctx.array(c.T0), ctx.array(sys0, dtype=np.float64), ctx.array(st0, dtype=np.int32), ctx.array(n0)
    pose = ctx.array(c.T1)

    def untouched():
        return (T.asnumpy().tobytes() == c.T0.tobytes() and sys_d.asnumpy().tobytes() == sys0.tobytes()
                and st.asnumpy().tobytes() == st0.tobytes() and nrm.asnumpy().tobytes() == n0.tobytes()
                and pose.asnumpy().tobytes() == c.T1.tobytes())

    def step(K_host=K0, dist_max=0.012, rcond=RCOND, B=3, H=H, W=W, sys_=sys_d):
        return lib.deepim_icp_step(ctx.handle, T, sys_, st, c.src_d, c.tgt_d, c.nrm_d, K_host, None, ctypes.c_float(dist_max), 12,
                                   ctypes.c_double(rcond), B, H, W)

    def normals(K_host=K0, B=3, H=H, W=W):
        return lib.deepim_depth_normals(ctx.handle, nrm, c.tgt_d, K_host, ctypes.c_float(0.01), B, H, W)

    ctx.bind_cameras(None)
    for kw in (dict(H=0), dict(B=65536), dict(dist_max=-1e-3), dict(rcond=-1e-12), dict(K_host=None)):
        with pytest.raises(RuntimeError, match="deepim_icp_step failed"):
            step(**kw)
        assert untouched(), kw
    with pytest.raises(RuntimeError, match="deepim_icp_step: K_host is NULL and no camera table is bound"):
        step(K_host=None)
    for kw in (dict(H=0), dict(B=65536), dict(K_host=None)):
        with pytest.raises(RuntimeError, match="deepim_depth_normals failed"):
            normals(**kw)
        assert untouched(), kw
    with pytest.raises(RuntimeError, match="deepim_depth_normals: K_host is NULL and no camera table is bound"):
        normals(K_host=None)
    with pytest.raises(RuntimeError, match="deepim_icp_apply failed"):
        lib.deepim_icp_apply(ctx.handle, pose, T, pose, -1)
    assert untouched()
    # B = 0: nothing to do, nothing written, no camera asked for
    assert step(B=0) == 0 and step(B=0, K_host=None) == 0
    assert normals(B=0) == 0 and normals(B=0, K_host=None) == 0
    assert lib.deepim_icp_apply(ctx.handle, pose, T, pose, 0) == 0
    assert untouched()
    # sys = NULL: the same T and status
    ctx.bind_cameras(c.K_d)
    with_sys, without = run_step(c), run_step(c, with_sys=False)
    assert without[1] is None
    assert with_sys[0].tobytes() == without[0].tobytes() and with_sys[2].tobytes() == without[2].tobytes()
    assert with_sys[2].tolist() == [0, 0, 0] and not np.array_equal(with_sys[0], c.T0)
