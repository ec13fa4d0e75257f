#!/usr/bin/env python
"""Golden vectors for the pose kernels (csrc/se3.hip) in the regimes the random-pose fixtures never reach: refinement-sized
deltas, half-turns, the gimbal / identity / sign-flip thresholds of the rotation converters, degenerate quaternions, large
translation deltas and the tile boundaries of the ADI search.  Produced by the REFERENCE's own Python.

Runs only where the reference checkout of tests/golden/make_golden.py is present:  python tests/golden/make_pose_edges_golden.py
(`--check` regenerates and compares every key with the committed file instead of writing it.)
Writes tests/golden/pose_edges_golden.npz (committed).  TEST INFRASTRUCTURE ONLY.

lib/pair_matching/RT_transform.py, lib/utils/projection.py and lib/utils/pose_error.py are imported UNMODIFIED, with the
NumPy-2 names tests/golden/make_golden.py injects (np.float, np.int, np.maximum_sctype) and the `copy=False` module shim
of se3_extra_golden().  Every input is stored as float32, the type the device entries take; the reference runs on exactly
those float32 values (under this container's NumPy-2 promotion, hence the 1e-6 bars of the tests that read this file).
Every constructed case asserts the regime it was built for, so a case that lands on the wrong side of a threshold fails
here and not on the GPU.

Groups (key prefix):
  A_  calc_RT_delta at rotation deltas of 0 … 0.5 rad and translation offsets of 0 … 2 cm, B = 65
  B_  mat2quat: identity, half-turns, negative trace, tiny angles, products only orthonormal to 1e-7
  C_  mat2euler at cy = 0 and on both sides of 4 eps, euler2mat at quarter / half turns, calc_RT_delta EULER at a
      quarter-turn about y
  D_  quat2mat on both sides of Nq = eps; RT_transform rows with unit / huge / denormal-squared / zero quaternions and
      exp(+-20) translation deltas scattered in a batch of 65
  F_  re / te / add / adi / arp_2d at N = 1, 255, 1024, 1025, 2304 on a mirror-symmetric point set
"""
import os
import sys
import warnings
from math import cos, pi, sin

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

f32, f64 = np.float32, np.float64
COORDS = ("MODEL", "CAMERA", "CAMERA_NEW", "NAIVE")
EPS = np.finfo(np.float64).eps
MU, SD = np.array([0.01, -0.02, 0.03]), np.array([0.9, 1.1, 1.2])
A_ANGLES = (0.0, 1e-6, 1e-4, 1e-2, 0.1, 0.5)
A_OFFSETS = (0.0, 1e-5, 1e-3, 2e-2)
F_SIZES = (1, 255, 1024, 1025, 2304)
F_MASTER = 2304
F_KINDS = ("perturbed", "equal", "quarter_z", "half_z", "milli", "symmetric")
F_SCALES = (1.0, 0.5, 2.0)          # per-sample point layout: sample b holds the shared set times F_SCALES[b] (exact in float32)


class _Np1Array(object):
    """mat2euler calls np.array(mat, dtype=float64, copy=False) (:347), which NumPy 1.x reads as "copy only if needed"."""
    def __getattr__(self, name):
        return getattr(np, name)

    def array(self, *a, **k):
        if k.get("copy") is False:
            k["copy"] = None
        return np.array(*a, **k)


def axis_angle(axis, angle):
    """Rodrigues, float64.  angle = 0 gives the identity exactly."""
    n = np.asarray(axis, f64) / np.linalg.norm(axis)
    Kx = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + sin(angle) * Kx + (1 - cos(angle)) * (Kx @ Kx)


def rot_z(a):
    return np.array([[cos(a), -sin(a), 0], [sin(a), cos(a), 0], [0, 0, 1]])


def rot_y(a):
    return np.array([[cos(a), 0, sin(a)], [0, 1, 0], [-sin(a), 0, cos(a)]])


def rand_pose(rng):
    return mg.rand_pose(rng).astype(f32)


def turned(pose, Rd, side):
    """pose with the float64 rotation Rd applied on the left (camera coords) or right (MODEL), rounded once to float32."""
    out = pose.copy()
    R = pose[:, :3].astype(f64)
    out[:, :3] = ((Rd @ R) if side == "left" else (R @ Rd)).astype(f32)
    return out


def group_a(RT, rng, out):
    B = 65
    src = np.stack([rand_pose(rng) for _ in range(B)])
    angle = np.array([A_ANGLES[b % 6] for b in range(B)])
    off = np.zeros((B, 3))
    for b in range(B):
        if b < 24:                      # every (angle, offset) pair once, the offset the same on all three axes
            off[b] = A_OFFSETS[b // 6]
        else:
            off[b] = rng.choice(A_OFFSETS, 3) * rng.choice([-1.0, 1.0], 3)
    tgt = {}
    for side in ("left", "right"):
        tgt[side] = np.stack([turned(src[b], axis_angle(rng.standard_normal(3), angle[b]), side) for b in range(B)])
        tgt[side][:, :, 3] = (src[:, :, 3].astype(f64) + off).astype(f32)
    for b in np.nonzero(angle == 0)[0]:
        assert np.array_equal(tgt["left"][b, :, :3], src[b, :, :3]) and np.array_equal(tgt["right"][b, :, :3], src[b, :, :3])
    assert np.array_equal(tgt["left"][0], src[0])                     # row 0: target bit-identical to the source
    for side in ("left", "right"):                                     # the rotation that was applied survives the rounding
        for b in range(B):
            Rd = tgt[side][b, :, :3].astype(f64) @ src[b, :, :3].astype(f64).T if side == "left" else \
                src[b, :, :3].astype(f64).T @ tgt[side][b, :, :3].astype(f64)
            got = np.arccos(np.clip((np.trace(Rd) - 1) / 2, -1, 1))
            assert abs(got - angle[b]) < 1e-3 * angle[b] + 1e-3, (b, got, angle[b])
    out.update(A_src=src, A_tgt_left=tgt["left"], A_tgt_right=tgt["right"], A_angle=angle.astype(f32))
    for coord in COORDS:
        t_ = tgt["right"] if coord == "MODEL" else tgt["left"]
        for rtype in ("QUAT", "EULER", "MATRIX"):
            rt = [RT.calc_RT_delta(src[i], t_[i], MU, SD, coord, rtype) for i in range(B)]
            r = np.stack([np.asarray(a).reshape(-1) for a, _ in rt])
            r = r if rtype == "MATRIX" else r.astype(f64)
            if coord == "CAMERA_NEW":   # the same R_inv_transform branch as CAMERA (:67-68): stored once
                assert np.array_equal(r, out["A_%s_CAMERA_r" % rtype])
            else:
                out["A_%s_%s_r" % (rtype, coord)] = r
            tr = np.stack([np.asarray(b_, f64) for _, b_ in rt])
            if rtype == "QUAT":
                out["A_%s_t" % coord] = tr
            else:
                assert np.array_equal(tr, out["A_%s_t" % coord])
    for i in range(B):                  # calc_se3 (:176-187) is the NAIVE delta under another name: no keys of its own
        rotm, t = RT.calc_se3(src[i], tgt["left"][i])
        assert np.array_equal(rotm.reshape(-1), out["A_MATRIX_NAIVE_r"][i]) and np.array_equal(t, out["A_NAIVE_t"][i])
    for coord in ("MODEL", "CAMERA", "NAIVE"):
        assert out["A_MATRIX_%s_r" % coord].dtype == f32
        assert np.isfinite(out["A_QUAT_%s_r" % coord]).all() and (out["A_QUAT_%s_r" % coord][:, 0] > 0.9).all()


def group_b(RT, rng, out):
    mats, half = [], []

    def add(M, is_half=False):
        half.append(is_half)
        mats.append(np.asarray(M, f64).astype(f32))

    add(np.eye(3))
    for d in ([1, -1, -1], [-1, 1, -1], [-1, -1, 1]):
        add(np.diag(d), True)
    for ax in ([1, 2, 3], [1, 1, 0], [0, 0, 1]):
        add(axis_angle(ax, pi), True)
    add(axis_angle([0.3, -0.5, 0.8], pi - 1e-3))
    for a in (2.2, 2.5, 2.8, 3.1):
        add(axis_angle(rng.standard_normal(3), a))
        assert np.trace(mats[-1]) < 0
    for a in (1e-7, 1e-5, 1e-3, 3e-2):
        add(axis_angle(rng.standard_normal(3), a))
    for _ in range(3):                  # float32 product of two float32 rotations
        P = rand_pose(rng)[:, :3] @ rand_pose(rng)[:, :3]
        assert P.dtype == f32
        dev = np.abs(P.astype(f64) @ P.astype(f64).T - np.eye(3)).max()
        assert 1e-9 < dev < 1e-6, dev
        add(P)
    mats = np.stack(mats)
    ref = np.stack([RT.mat2quat(m) for m in mats])
    assert ref.dtype == f64 and (ref[:, 0] >= 0).all()
    assert np.array_equal(np.abs(ref[:, 0]) < 1e-8, np.array(half)), ref[:, 0]      # exactly the six half-turns
    assert np.abs(np.linalg.norm(ref, axis=1) - 1).max() < 1e-12
    out.update(B_mat=mats, B_quat=ref, B_half=np.array(half))


def group_c(RT, rng, out):
    mats = [[[0, .6, .8], [0, .8, -.6], [-1, 0, 0]], [[0, .6, .8], [0, -.8, .6], [1, 0, 0]],
            [[1e-15, .6, .8], [0, .8, -.6], [-1, 0, 0]], [[5e-16, .6, .8], [0, .8, -.6], [-1, 0, 0]],
            RT.euler2mat(0.3, pi / 2, -0.2)]
    mats = np.stack([np.asarray(m, f64).astype(f32) for m in mats])
    cy = np.sqrt(mats[:, 0, 0].astype(f64) ** 2 + mats[:, 1, 0].astype(f64) ** 2)
    assert cy[0] == 0 and cy[1] == 0 and cy[2] > 4 * EPS and 0 < cy[3] <= 4 * EPS and 0 < cy[4] <= 4 * EPS, cy
    ref = np.stack([np.array(RT.mat2euler(m)) for m in mats])
    assert (ref[[0, 1, 3, 4], 2] == 0).all() and ref[2, 2] == 0 and abs(ref[2, 0] - ref[3, 0]) > 0.5   # the branches differ
    out.update(C_mat=mats, C_mat2euler=ref)
    vals = (0.0, pi / 2, -pi / 2, pi, 1e-8)
    eul = np.array([[a, b, c] for a in vals for b in vals for c in vals] + [[0.3, pi / 2, -0.2]]).astype(f32)
    out.update(C_euler=eul, C_euler2mat=np.stack([RT.euler2mat(e[0], e[1], e[2]) for e in eul]))
    # calc_RT_delta EULER at a quarter-turn about y: exact source rotations, so the delta is exact and cy = 0
    src = np.stack([rand_pose(rng) for _ in range(2)])
    src[0, :, :3] = np.eye(3)
    src[1, :, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]
    Ry = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], f64)
    tl = np.stack([turned(s, Ry, "left") for s in src])
    tr = np.stack([turned(s, Ry, "right") for s in src])
    for t_ in (tl, tr):
        t_[:, :, 3] += np.array([0.01, -0.005, 0.02], f32)
    out.update(C_delta_src=src, C_delta_tgt_left=tl, C_delta_tgt_right=tr)
    for coord in COORDS:
        t_ = tr if coord == "MODEL" else tl
        rt = [RT.calc_RT_delta(src[i], t_[i], MU, SD, coord, "EULER") for i in range(2)]
        r = np.stack([np.asarray(a, f64) for a, _ in rt])
        np.testing.assert_allclose(r, [[0, pi / 2, 0]] * 2, atol=1e-12)
        out["C_delta_%s_r" % coord] = r
        out["C_delta_%s_t" % coord] = np.stack([np.asarray(b, f64) for _, b in rt])


def group_d(RT, rng, out):
    q = np.array([[.5, .5, .5, .5]]) * np.array([[1.4e-8], [1.6e-8], [1.0]])
    q = q.astype(f32)
    Nq = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    assert Nq.dtype == f32 and Nq[0] < EPS < Nq[1], Nq
    ref = np.stack([np.asarray(RT.quat2mat(v), f64) for v in q])
    turn = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], f64)             # 120 degrees about (1,1,1)
    assert np.array_equal(ref[0], np.eye(3)) and np.abs(ref[1] - turn).max() < 1e-6 and np.abs(ref[2] - turn).max() < 1e-6
    out.update(D_quat=q, D_quat2mat=ref)

    B = 65
    src = out["A_src"]                  # the 65 source poses of group A
    se3 = np.concatenate([rng.standard_normal((B, 4)) * 0.3 + [1, 0, 0, 0], rng.standard_normal((B, 3)) * 0.1], 1)
    unit = rng.standard_normal(4)
    unit /= np.linalg.norm(unit)
    rows = {"unit": 3, "unit_noise": 17, "huge": 31, "tiny": 40, "zero": 52, "tiny_last": 64}
    se3[rows["unit"], :4] = [1, 0, 0, 0]
    se3[rows["unit_noise"], :4] = np.array([1, 0, 0, 0]) + rng.standard_normal(4) * 1e-7
    se3[rows["huge"], :4] = unit * 1e3
    se3[rows["tiny"], :4] = [1e-20, 1e-20, -1e-20, 1e-20]
    se3[rows["zero"], :4] = 0
    se3[rows["tiny_last"], :4] = [1e-20, -1e-20, 1e-20, 1e-20]
    zrows = {8: -20.0, 24: 0.0, 47: 20.0}
    for b, v in zrows.items():
        se3[b, 6] = (v - MU[2]) / SD[2]
    se3 = se3.astype(f32)
    sq = se3[rows["tiny"], :4] * se3[rows["tiny"], :4]
    assert sq.dtype == f32 and (sq > 0).all() and (sq < np.finfo(f32).tiny).all()       # squares are float32 subnormals
    assert abs(np.linalg.norm(se3[rows["huge"], :4].astype(f64)) - 1e3) < 1e-3
    for b, v in zrows.items():
        assert abs(f64(se3[b, 6]) * SD[2] + MU[2] - v) < 1e-5
    out.update(D_se3=se3, D_rows=np.array(sorted(rows.values())), D_zero_row=np.array(rows["zero"]),
               D_z_rows=np.array(sorted(zrows)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # 0 / 0 of the all-zero quaternion
        for coord in COORDS:
            ref = np.stack([np.asarray(RT.RT_transform(src[i], se3[i, :4], se3[i, 4:], MU, SD, coord), f64) for i in range(B)])
            nan = np.isnan(ref)
            want = np.zeros((B, 3, 4), bool)
            want[rows["zero"], :, :3] = True
            if coord == "NAIVE":
                want[rows["zero"], :, 3] = True
            assert np.array_equal(nan, want), coord                       # NaN exactly in the zero row's rotation block
            assert np.isfinite(ref[~nan]).all()
            out["D_rt_%s" % coord] = ref
    # Euler rows: quarter / half turns and 1e-8 among ordinary angles, the same translation edges
    Be = 17
    eul = (rng.standard_normal((Be, 3)) * 0.4)
    eul[2], eul[9], eul[13], eul[16] = [0, pi / 2, 0], [pi / 2, -pi / 2, pi], [1e-8, 1e-8, -1e-8], [pi, 0, -pi / 2]
    e6 = np.concatenate([eul, se3[:Be, 4:]], 1).astype(f32)
    out.update(D_euler_se3=e6)
    for coord in COORDS:
        out["D_rt_euler_%s" % coord] = np.stack(
            [np.asarray(RT.RT_transform(src[i], e6[i, :3], e6[i, 3:], MU, SD, coord), f64) for i in range(Be)])
        assert np.isfinite(out["D_rt_euler_%s" % coord]).all()


def symmetric_master(rng):
    """(3, 2304) float32 on a 2^-11 m grid, point 2303-i the mirror of point i under a half-turn about the model z axis,
    and one point on that axis."""
    g = 2.0 ** -11
    p = np.clip(np.round(rng.standard_normal((3, F_MASTER // 2)) * 0.04 / g), -250, 250)
    p[0][(p[0] == 0) & (p[1] == 0)] = 1
    p *= g
    mirror = (p * np.array([[-1.0], [-1.0], [1.0]]))[:, ::-1]
    axis_point = np.array([[0.0], [0.0], [np.round(rng.standard_normal() * 0.04 / g) * g]])
    return np.concatenate([p, mirror], 1).astype(f32), axis_point.astype(f32)


def symmetric_points(master, axis_point, N):
    """The N-point set of the fixture: the centred slice of the master, which keeps point N-1-i the mirror of point i, with
    the on-axis point in the middle when N is odd.  tests/test_gpu_pose_edges.py cuts the same slices."""
    h, c = N // 2, F_MASTER // 2
    pts = np.concatenate([master[:, c - h:c]] + ([axis_point] if N % 2 else []) + [master[:, c:c + h]], 1)
    assert pts.shape == (3, N) and pts.dtype == f32
    assert np.array_equal(pts[:, ::-1] * np.array([[-1], [-1], [1]], f32), pts)
    return pts


def group_f(PE, rng, out):
    K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])
    B = 3
    gt = np.stack([rand_pose(rng) for _ in range(B)])
    gt[0, :, :3] = [[0, -1, 0], [0, 0, -1], [1, 0, 0]]                 # exact rotation: cos of the 0 / 90 / 180 degree rows is exactly 1 / 0 / -1
    est = {}
    e = gt.copy()
    for b in range(B):
        a = rng.normal(0, 0.1, 3)
        e[b, :, :3] = (rot_z(a[2]) @ rot_y(a[1]) @ gt[b, :, :3].astype(f64)).astype(f32)
        e[b, :, 3] += rng.normal(0, 0.01, 3).astype(f32)
    est["perturbed"] = e
    est["equal"] = gt.copy()
    Rq, Rh = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), np.diag([-1.0, -1.0, 1.0])
    est["quarter_z"] = np.stack([turned(g_, Rq, "left") for g_ in gt])
    est["half_z"] = np.stack([turned(g_, Rh, "left") for g_ in gt])
    est["milli"] = np.stack([turned(g_, rot_z(1e-3), "left") for g_ in gt])
    est["symmetric"] = np.stack([turned(g_, Rh, "right") for g_ in gt])     # half-turn about the model's symmetry axis
    for b in range(B):                  # exact: rows / columns permuted and negated
        assert np.array_equal(est["half_z"][b, :2, :3], -gt[b, :2, :3]) and np.array_equal(est["symmetric"][b, :, :2], -gt[b, :, :2])
    c = lambda E, G: (np.trace(E[:, :3].astype(f64).T @ G[:, :3].astype(f64)) - 1) / 2   # noqa: E731
    assert c(est["equal"][0], gt[0]) == 1 and c(est["quarter_z"][0], gt[0]) == 0 and c(est["half_z"][0], gt[0]) == -1
    out.update(F_K=K.astype(f32), F_gt=gt, F_scales=np.array(F_SCALES, f32))
    K = K.astype(f32).astype(f64)
    for kind in F_KINDS:
        out["F_est_%s" % kind] = est[kind]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # logm at an exact half-turn warns about its own accuracy
        master, axis_point = symmetric_master(rng)
        out.update(F_points_master=master, F_axis_point=axis_point)
        for N in F_SIZES:
            pts = symmetric_points(master, axis_point, N)
            m = np.zeros((len(F_KINDS), 2, B, 5))
            for k, kind in enumerate(F_KINDS):
                for lay in range(2):
                    for b in range(B):
                        P = (pts * (f32(F_SCALES[b]) if lay else f32(1))).astype(f64).T
                        Re, te = est[kind][b, :, :3].astype(f64), est[kind][b, :, 3].astype(f64)
                        Rg, tg = gt[b, :, :3].astype(f64), gt[b, :, 3].astype(f64)
                        m[k, lay, b] = [np.real(PE.re(Re, Rg)), PE.te(te, tg), PE.add(Re, te, Rg, tg, P), PE.adi(Re, te, Rg, tg, P),
                                        PE.arp_2d(Re, te, Rg, tg, P, K)]
            assert np.isfinite(m).all()
            s = F_KINDS.index("symmetric")
            assert (m[s, :, :, 3] < 1e-7).all(), m[s, :, :, 3]
            if N > 1:                   # the single point of N = 1 lies on the axis: ADD = 0 there
                assert (m[s, :, :, 2] > 1e-2).all(), m[s, :, :, 2]
            assert np.abs(m[F_KINDS.index("half_z"), :, :, 0] - 180).max() < 1e-3
            assert np.abs(m[F_KINDS.index("quarter_z"), :, :, 0] - 90).max() < 1e-3
            assert m[F_KINDS.index("equal"), :, :, 0].max() < 0.05 and np.abs(m[F_KINDS.index("equal"), :, :, 1:]).max() == 0
            out["F_metrics_%d" % N] = m


def build():
    RT, _, _ = mg.load_reference()
    RT.np = _Np1Array()
    sys.path.insert(0, mg.REF)
    from lib.utils import pose_error as PE
    out = dict(T_means=MU, T_stds=SD)
    group_a(RT, np.random.default_rng(9001), out)
    group_b(RT, np.random.default_rng(9002), out)
    group_c(RT, np.random.default_rng(9003), out)
    group_d(RT, np.random.default_rng(9004), out)
    group_f(PE, np.random.default_rng(9006), out)
    return out


def main():
    out = build()
    path = os.path.join(HERE, "pose_edges_golden.npz")
    if "--check" in sys.argv:
        old = np.load(path)
        assert sorted(old.files) == sorted(out)
        for k in out:
            assert np.array_equal(old[k], np.asarray(out[k]), equal_nan=True), k
        print("pose_edges_golden.npz reproduced: %d keys equal" % len(out))
        return
    np.savez_compressed(path, **out)
    print("wrote pose_edges_golden.npz: %d keys, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
