"""Synthetic observed scenes with occluders on the GPU: deepim_render_scene_forward against the observed entry (S = 1, byte for
byte) and against a composition of single-object draws made on the host (S = 3, hand-placed poses checked with oracle/render.py),
the exact-tie rule, deepim_sample_occluders against the numpy emulation bit for bit, deepim_occlusion_gate on crafted counts,
SyntheticObserved(occluders=...) against the chain written out by hand, and core/loader.TrainDataLoader with occluded synthetic
pairs over a host set and a resident one. The meshes and sizes of tests/test_gpu_synthetic_observed.py: 48x64 on the
four-pixel store path, 45x61 on the single-pixel one; B = 4, S = 3. One train step at full size."""
import ctypes

import numpy as np
import pytest

import observed_pose_emulation as oemu
import occluder_emulation as occ
import test_gpu_fit as tf
import test_gpu_loader as tl
import test_gpu_synthetic_observed as tso
from mx_deepim_amd import synthetic
from mx_deepim_amd.core.loader import ResidentObserved, TrainDataLoader
from mx_deepim_amd.lib.pair_matching.pose_sampler import sample_lights, sample_observed_poses, sample_occluders
from mx_deepim_amd.lib.render_glumpy.render_py_light import Render_Py_Light
from mx_deepim_amd.lib.utils import image as dimage
from mx_deepim_amd.lib.utils.synthetic_observed import OccluderSpec, SyntheticObserved
from mx_deepim_amd.runtime import lib
from oracle import render as orender

pytestmark = pytest.mark.gpu
H, W, K_SMALL, ZN, ZF = tso.H, tso.W, tso.K_SMALL, tso.ZN, tso.ZF
cf, u64 = ctypes.c_float, ctypes.c_ulonglong
world = tl.world                 # the loader tests' module fixture, built once for this module too
B, S = 4, 3
DIAMETERS = {0: 0.10, 1: 0.12}    # the two ellipsoids' longest axes, in metres
SIZES = [(48, 64), (45, 61)]
CHAIN_SEED = 402                  # see test_full_chain: picked with the emulation and the CPU oracle


def _scene(ctx, rm, cls, poses, off, inten, ratio, rows=None, N=None, label_value=None, fill=None, visible=True):
    """deepim_render_scene_forward -> (image (N,h,w,3), depth (N,h,w), label (N,h,w), visible (B,S)) on the host."""
    cls, poses = np.asarray(cls, np.int32), np.asarray(poses, np.float32)
    nB, nS = cls.shape
    h, w = rm.height, rm.width
    N = nB if N is None else N
    out = [ctx.empty((N, h, w, 3), np.uint8), ctx.empty((N, h, w), np.uint16), ctx.empty((N, h, w), np.uint8)]
    if fill is not None:
        for a in out:
            lib.deepim_memset(ctx.handle, a, fill, a.nbytes)
    vis = ctx.array(np.full((nB, nS), -7, np.int32), dtype=np.int32) if visible else None       # the call writes it, whatever it held
    t = rm.mesh_table()
    lib.deepim_render_scene_forward(ctx.handle, out[0], out[1], out[2], vis, None if rows is None else ctx.array(rows, dtype=np.int32), N,
                                    None if label_value is None else ctx.array(label_value, dtype=np.int32), cf(1000.0),
                                    ctx.array(cls, dtype=np.int32), t.mesh_desc, t.n_classes, t.max_V, t.max_F, t.vertices,
                                    t.vertex_attr, t.normals, t.faces, t.textures, ctx.array(poses), K_SMALL, ctx.array(off),
                                    ctx.array(inten), ctx.array(ratio), nB, nS, h, w, cf(ZN), cf(ZF))
    return [a.asnumpy() for a in out] + [vis.asnumpy() if visible else None]


def _pose(t, seed):
    p = np.zeros((3, 4), np.float32)
    p[:, :3] = synthetic.random_rotation(np.random.default_rng(seed))
    p[:, 3] = t
    return p


def _hand_scenes():
    """Four frames of three slots. Frame 0: slot 1 in front of the target and partly over it, slot 2 behind it and overlapping.
    Frame 1: slot 1 empty (class -1). Frames 2, 3: two more of the first kind (frame 2 is the one the test leaves unstored)."""
    zero = np.zeros((3, 4), np.float32)
    frames = [([0, 1, 0], [_pose([0.0, 0.0, 0.6], 1), _pose([0.035, 0.01, 0.5], 2), _pose([-0.03, 0.015, 0.75], 3)]),
              ([1, -1, 0], [_pose([0.01, -0.01, 0.65], 4), zero, _pose([0.03, -0.03, 0.52], 5)]),
              ([0, 1, 1], [_pose([-0.02, 0.01, 0.55], 6), _pose([-0.05, 0.0, 0.45], 7), _pose([0.0, 0.04, 0.7], 8)]),
              ([1, 0, 0], [_pose([0.02, 0.0, 0.6], 9), _pose([0.02, 0.045, 0.5], 10), _pose([0.06, 0.0, 0.8], 11)])]
    return np.array([c for c, _p in frames], np.int32), np.stack([np.stack(p) for _c, p in frames])


def _oracle_counts(cls, poses, h, w):
    """(visible (S), full (S)) pixel counts of one frame's slots from oracle/render.py depths composed on the CPU."""
    d = np.full((len(cls), h, w), np.inf, np.float32)
    for s, c in enumerate(cls):
        if c >= 0:
            m = tso._lit_meshes()[int(c)]
            dep = orender.render(m["vertices"], m["uv"], m["faces"], poses[s], K_SMALL, h, w, texture=m["texture"])[1]
            d[s] = np.where(dep > 0, dep, np.inf)
    win, hit = np.argmin(d, 0), np.isfinite(d.min(0))
    return (np.array([np.count_nonzero(hit & (win == s)) for s in range(len(cls))]),
            np.array([np.count_nonzero(np.isfinite(d[s])) for s in range(len(cls))]))


def _lights4():
    _ids, _cls, _poses, off, inten, ratio = tso._six()
    return off[:B], inten[:B], ratio[:B]


# ------------------------------------------------------------------------------------------------------------ a. S = 1 --
@pytest.mark.parametrize("h,w", SIZES)
def test_one_slot_equals_the_observed_entry(ctx, h, w):
    rm = tso._machine(ctx, h, w)
    _ids, cls, poses, off, inten, ratio = tso._six()
    label_value = np.array([1, 2, 3, 1, 200, 255], np.int32)
    want = tso._frames(ctx, rm, cls, poses, off, inten, ratio, label_value=label_value)
    got = _scene(ctx, rm, cls[:, None], poses[:, None], off, inten, ratio, label_value=label_value[:, None])
    assert want[0].any() and want[1].any()
    for g, x in zip(got[:3], want):
        np.testing.assert_array_equal(g, x)
    np.testing.assert_array_equal(got[3][:, 0], np.count_nonzero(want[1].reshape(6, -1), axis=1))
    assert (got[3] > 20).all()
    # NULL label_value = s + 1 = 1, NULL visible, rows as in the observed entry
    rows = np.array([7, 0, 3, 5, 9, 1], np.int32)
    want = tso._frames(ctx, rm, cls, poses, off, inten, ratio, rows=rows, N=9, fill=0xAB)
    got = _scene(ctx, rm, cls[:, None], poses[:, None], off, inten, ratio, rows=rows, N=9, fill=0xAB, visible=False)
    for g, x in zip(got[:3], want):
        np.testing.assert_array_equal(g, x)


def test_scene_refusals(ctx):
    rm = tso._machine(ctx)
    off, inten, ratio = _lights4()
    cls, poses = _hand_scenes()
    with pytest.raises(RuntimeError, match="1..8"):
        _scene(ctx, rm, np.zeros((1, 9), np.int32), np.zeros((1, 9, 3, 4), np.float32), off[:1], inten[:1], ratio[:1])
    with pytest.raises(RuntimeError, match="N >= B"):
        _scene(ctx, rm, cls, poses, off, inten, ratio, N=3)
    t = rm.mesh_table()
    a = ctx.empty((1,), np.int32)
    for kw, match in ((dict(B=8192, S=8), "B \\* S"), (dict(max_F=(1 << 24) + 1), "2\\^24"), (dict(zfar=66.0), "65536")):
        with pytest.raises(RuntimeError, match=match):
            lib.deepim_render_scene_forward(ctx.handle, a, a, a, None, None, 10000, None, cf(1000.0), a, t.mesh_desc, t.n_classes, t.max_V,
                                            kw.get("max_F", t.max_F), t.vertices, t.vertex_attr, t.normals, t.faces, t.textures, a, K_SMALL,
                                            a, a, a, kw.get("B", 1), kw.get("S", 1), H, W, cf(ZN), cf(kw.get("zfar", ZF)))


# ------------------------------------------------------------------------------------------------------ b. composition --
@pytest.mark.parametrize("h,w", SIZES)
def test_scene_equals_the_composition_of_single_object_draws(ctx, h, w):
    rm = tso._machine(ctx, h, w)
    cls, poses = _hand_scenes()
    off, inten, ratio = _lights4()
    assert len(set(map(tuple, off.tolist()))) == B
    # the premise, on the CPU: every live slot wins some pixels and the target keeps strictly between 0.2 and 0.9 of its own
    for f in range(B):
        vis, full = _oracle_counts(cls[f], poses[f], h, w)
        assert ((vis > 0) == (cls[f] >= 0)).all() and 0.2 < vis[0] / full[0] < 0.9, (f, vis, full)
    label_value = np.array([[1, 2, 3], [1, 2, 3], [9, 200, 255], [1, 2, 3]], np.int32)
    flat = lambda a: np.repeat(a, S, axis=0)                                       # noqa: E731  (a frame's light for each of its slots)
    before = tso._frames(ctx, rm, cls.reshape(-1), poses.reshape(-1, 3, 4), flat(off), flat(inten), flat(ratio), label_value=label_value.reshape(-1))
    alone = [a.reshape((B, S) + a.shape[1:]) for a in before]
    z = np.full((B, S, h, w), np.inf, np.float32)
    for f in range(B):
        for s in range(S):
            if cls[f, s] >= 0:
                dep = tso._lit_one(ctx, rm, int(cls[f, s]), poses[f, s], off[f], inten[f], ratio[f])[1]
                z[f, s] = np.where(dep != 0, dep, np.inf)
    win = np.argmin(z, 1)                                                          # the smallest float depth, the lowest slot on ties
    want = [np.take_along_axis(a, win.reshape((B, 1, h, w) + (1,) * (a.ndim - 4)), 1)[:, 0] for a in alone]
    counts = np.array([[np.count_nonzero((win[f] == s) & (want[1][f] != 0)) for s in range(S)] for f in range(B)])
    rows, N = np.array([5, 0, 9, 2], np.int32), 7                                  # frame 2's row is outside [0, N)
    got = _scene(ctx, rm, cls, poses, off, inten, ratio, rows=rows, N=N, label_value=label_value, fill=0xAB)
    stored = [0, 1, 3]
    for g, x in zip(got[:3], want):
        np.testing.assert_array_equal(g[rows[stored]], x[stored])
        assert (g[[1, 3, 4, 6]].view(np.uint8) == 0xAB).all()                      # rows not named keep the pattern
    np.testing.assert_array_equal(got[3], counts)                                  # the unstored frame's pixels are still counted
    assert (counts[cls >= 0] > 0).all() and (counts[cls < 0] == 0).all()
    assert all(0.2 < counts[f, 0] / np.count_nonzero(alone[1][f, 0]) < 0.9 for f in range(B))
    for f in stored:                                                               # every label of the frame's live slots is on the map
        assert set(np.unique(got[2][rows[f]]).tolist()) == {0} | set(label_value[f][cls[f] >= 0].tolist())
    # the z-buffer was left all-ones: an ordinary draw gives the bytes it gave before
    after = tso._frames(ctx, rm, cls.reshape(-1), poses.reshape(-1, 3, 4), flat(off), flat(inten), flat(ratio), label_value=label_value.reshape(-1))
    for a, b in zip(after, before):
        np.testing.assert_array_equal(a, b)


# ----------------------------------------------------------------------------------------------------------- c. the tie --
@pytest.mark.parametrize("h,w", SIZES)
def test_an_exact_tie_goes_to_the_lower_slot(ctx, h, w):
    rm = tso._machine(ctx, h, w)
    cls, poses = _hand_scenes()
    off, inten, ratio = _lights4()
    cls = np.stack([cls[:, 0], cls[:, 0], np.full(B, -1, np.int32)], 1)
    poses = np.stack([poses[:, 0], poses[:, 0], poses[:, 2]], 1)
    image, depth, label, visible = _scene(ctx, rm, cls, poses, off, inten, ratio)
    one = _scene(ctx, rm, cls[:, :1], poses[:, :1], off, inten, ratio)
    np.testing.assert_array_equal(image, one[0])
    np.testing.assert_array_equal(depth, one[1])
    np.testing.assert_array_equal(label, (depth != 0).astype(np.uint8))            # slot 0's label, 1, on every covered pixel
    np.testing.assert_array_equal(visible, np.stack([one[3][:, 0], np.zeros(B, np.int32), np.zeros(B, np.int32)], 1))
    assert (visible[:, 0] > 20).all()
    # the higher slot wins where it is alone in front: the same two objects, the second one nearer
    poses[:, 1, 2, 3] -= 0.1
    _i, _d, label, visible = _scene(ctx, rm, cls, poses, off, inten, ratio)
    assert (visible[:, 1] > 20).all() and set(np.unique(label).tolist()) <= {0, 1, 2} and (label == 2).any()


# ------------------------------------------------------------------------------------------------------- d. the sampler --
def _targets(n):
    rng = np.random.default_rng(8)
    import pose_sampler_emulation as emu
    return (np.arange(n) % 2).astype(np.int32), emu.random_poses(rng, n, 0.5, 0.7)


def test_sampler_equals_the_emulation(ctx):
    n, seed, base = 300, 17, (1 << 33) + 5            # more than one block; ids beyond 32 bits
    cls_t, pose_t = _targets(n)
    table = np.array([DIAMETERS[0], DIAMETERS[1]], np.float32)
    dev = (ctx.array(cls_t, dtype=np.int32), ctx.array(pose_t), ctx.array([1, 0, 1], dtype=np.int32), ctx.array(table))
    kw = dict(min_occluders=1, max_occluders=3, lateral=(0.1, 0.7), toward=(-0.3, 1.2))
    ids = base + np.arange(n, dtype=np.uint64)
    want = occ.occluders(seed, ids, cls_t, pose_t, [1, 0, 1], table, **kw)
    assert set(want[3].tolist()) == {1, 2, 3} and (want[0][:, 1:] == -1).any()
    perm = np.random.default_rng(4).permutation(n)
    for got, order in ((sample_occluders(*dev, seed, draw_base=base, **kw), np.arange(n)),
                       (sample_occluders(ctx.array(cls_t[perm], dtype=np.int32), ctx.array(pose_t[perm]), dev[2], dev[3], seed, draw_base=3,
                                         draw_ids=ids[perm], **kw), perm)):
        c, p, lab = (a.asnumpy() for a in got)
        assert c.dtype == np.int32 and p.dtype == np.float32 and p.shape == (n, 4, 3, 4)
        np.testing.assert_array_equal(c, want[0][order])
        np.testing.assert_array_equal(p.view(np.uint32), want[1][order].view(np.uint32))
        np.testing.assert_array_equal(lab, want[2][order])
    # near the camera every occluder falls behind it: empty slots; no occluders: one slot, the target
    near = pose_t.copy()
    near[:, 2, 3] = 0.05
    c, p, _l = (a.asnumpy() for a in sample_occluders(dev[0], ctx.array(near), dev[2], dev[3], seed, min_occluders=2, max_occluders=2))
    assert (c[:, 1:] == -1).all() and not p[:, 1:].any()
    c, p, lab = (a.asnumpy() for a in sample_occluders(dev[0], dev[1], dev[2], dev[3], seed, max_occluders=0))
    np.testing.assert_array_equal(c[:, 0], cls_t)
    np.testing.assert_array_equal(p[:, 0].view(np.uint32), pose_t.view(np.uint32))
    assert c.shape == (n, 1) and (lab == 1).all()
    with pytest.raises(RuntimeError, match="max_occluders <= 7"):
        sample_occluders(*dev, seed, max_occluders=8)


# ---------------------------------------------------------------------------------------------------------- e. the gate --
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("with_depth_observed", [True, False])
def test_gate_on_crafted_counts(ctx, h, w, with_depth_observed):
    rng = np.random.default_rng(h)
    N, rows = 6, np.array([2, 0, 3, 1, 9], np.int32)          # five pairs; the last one's row is outside [0, N)
    nB = len(rows)
    visible = np.array([[5, 3, 0], [4, 9, 9], [5, 0, 0], [7, 1, 1], [10, 0, 0]], np.int32)
    full = np.array([10, 10, 0, 10, 10], np.int32)
    slot_class = np.array([[0, 1, -1], [1, 0, 0], [0, -1, -1], [1, -1, 1], [0, 1, 1]], np.int32)
    want_kept = np.array([1, 0, 0, 1, 1], np.int32)            # 5 >= 0.5 * 10; 4 < 5; full = 0; 7 >= 5; 10 >= 5
    shapes = [((h, w, 3), np.uint8), ((h, w), np.uint16), ((h, w), np.uint8), ((h, w), np.uint16)]
    scene = [rng.integers(0, np.iinfo(dt).max, (N,) + s, dtype=dt, endpoint=True) for s, dt in shapes]
    alone = [rng.integers(0, np.iinfo(dt).max, (nB,) + s, dtype=dt, endpoint=True) for s, dt in shapes[:3]]
    dev = [ctx.array(a, dtype=a.dtype) for a in scene]
    kept, totals = ctx.array(np.full(nB, -3, np.int32), dtype=np.int32), ctx.zeros((3,), np.uint64)

    def run():
        lib.deepim_occlusion_gate(ctx.handle, dev[0], dev[1], dev[2], dev[3] if with_depth_observed else None, kept, totals,
                                  ctx.array(rows, dtype=np.int32), N, *[ctx.array(a, dtype=a.dtype) for a in alone],
                                  ctx.array(visible, dtype=np.int32), ctx.array(full, dtype=np.int32), ctx.array(slot_class, dtype=np.int32),
                                  cf(0.5), nB, 3, h, w)

    run()
    got = [a.asnumpy() for a in dev]
    np.testing.assert_array_equal(kept.asnumpy(), want_kept)
    for b in range(4):
        r = rows[b]
        np.testing.assert_array_equal(got[1][r], alone[1][b])                      # depth_gt_observed: the alone depth in all rows
        if want_kept[b]:
            for k in (0, 2, 3):
                np.testing.assert_array_equal(got[k][r], scene[k][r])              # kept rows keep their scene bytes
        else:
            np.testing.assert_array_equal(got[0][r], alone[0][b])
            np.testing.assert_array_equal(got[2][r], alone[2][b])
            np.testing.assert_array_equal(got[3][r], alone[1][b] if with_depth_observed else scene[3][r])
    for k in range(4):
        np.testing.assert_array_equal(got[k][[4, 5]], scene[k][[4, 5]])            # rows not named are not touched
    assert totals.asnumpy().tolist() == [5, 3, 6]
    run()                                                                          # the totals are running ones
    assert totals.asnumpy().tolist() == [10, 6, 12]


# ----------------------------------------------------------------------------------------------------- f. the full chain --
@pytest.fixture(scope="module")
def lit(ctx):
    return tso._machine(ctx)


def _spec(**kw):
    args = dict(classes=[0, 1], diameters=DIAMETERS, min_occluders=1, max_occluders=2)
    args.update(kw)
    return OccluderSpec(**args)


def _generator(lit, seed=CHAIN_SEED, **kw):
    return SyntheticObserved(lit, tso._stats(), K_SMALL, seed, border=oemu.SCENARIO_BORDER, **kw)


FRAME_KEYS = ("image_observed", "depth_gt_observed", "mask_gt_observed")


def test_full_chain(ctx, lit):
    """CHAIN_SEED with draw ids 50..53 and classes 0, 1, 1, 0: on the CPU (tests/observed_pose_emulation.py for the poses,
    tests/occluder_emulation.py for the occluders, oracle/render.py for the depths) the targets keep 0.95, 0.00, 0.22 and 0.91 of
    their pixels, so two pairs are kept with visible < full and two fall back, all at least 0.18 away from min_visible = 0.4."""
    cls_t, ids = np.array([0, 1, 1, 0], np.int32), 50 + np.arange(B, dtype=np.uint64)
    spec = _spec()
    gen = _generator(lit, occluders=spec)
    totals = ctx.zeros((3,), np.uint64)
    out = gen.frames(cls_t, ids, totals=totals)
    assert set(out) >= set(FRAME_KEYS) | {"pose_observed", "attempts", "light_offset", "light_intensity", "brightness_ratio", "class_index",
                                          "depth_observed", "kept", "visible", "occluder_class"}
    # by hand: sampler -> S = 1 draw -> scene -> gate
    dcls, dids = ctx.array(cls_t, dtype=np.int32), ctx.array(ids, dtype=np.uint64)
    pose, _attempts = sample_observed_poses(dcls, gen.pose_table, K_SMALL, W, H, CHAIN_SEED, draw_ids=dids, border=oemu.SCENARIO_BORDER)
    off, inten, ratio = (a.asnumpy() for a in sample_lights(ctx, B, CHAIN_SEED, draw_ids=dids, brightness_ratios=gen.brightness_ratios))
    ocls, oposes, olabel = (a.asnumpy() for a in sample_occluders(dcls, pose, ctx.array(spec.classes, dtype=np.int32),
                                                                  ctx.array(spec.diameter_table(2)), CHAIN_SEED, draw_ids=dids,
                                                                  min_occluders=1, max_occluders=2))
    pose = pose.asnumpy()
    want_cls, want_poses, _l, n = occ.occluders(CHAIN_SEED, ids, cls_t, pose, spec.classes, spec.diameter_table(2), 1, 2)
    np.testing.assert_array_equal(ocls, want_cls)
    assert (n >= 1).all() and (ocls[:, 1] >= 0).all()
    alone = _scene(ctx, lit, cls_t[:, None], pose[:, None], off, inten, ratio)
    scene = _scene(ctx, lit, ocls, oposes, off, inten, ratio, label_value=olabel)
    full, visible = alone[3][:, 0], scene[3]
    kept = (full > 0) & (visible[:, 0].astype(np.float64) >= np.float64(np.float32(0.4)) * full)
    print("visible", visible[:, 0], "full", full, "kept", kept)
    assert (kept & (visible[:, 0] < full)).any() and (~kept).any()                # a pair kept though partly hidden, and a fallback
    np.testing.assert_array_equal(out["kept"].asnumpy(), kept.astype(np.int32))
    np.testing.assert_array_equal(out["visible"].asnumpy(), visible)
    np.testing.assert_array_equal(out["occluder_class"].asnumpy(), ocls)
    np.testing.assert_array_equal(out["pose_observed"].asnumpy().view(np.uint32), pose.view(np.uint32))
    pick = lambda k: np.where(kept.reshape((B,) + (1,) * (scene[k].ndim - 1)), scene[k], alone[k])      # noqa: E731
    np.testing.assert_array_equal(out["image_observed"].asnumpy(), pick(0))
    np.testing.assert_array_equal(out["depth_observed"].asnumpy(), pick(1))       # the scene's depth, occluders included
    np.testing.assert_array_equal(out["mask_gt_observed"].asnumpy(), pick(2))
    np.testing.assert_array_equal(out["depth_gt_observed"].asnumpy(), alone[1])   # the target alone, kept or not
    b = int(np.nonzero(kept & (visible[:, 0] < full))[0][0])
    label = out["mask_gt_observed"].asnumpy()[b]
    assert np.count_nonzero(label == 1) == visible[b, 0] and (label > 1).any()    # label 1 = the visible part of the target only
    assert totals.asnumpy().tolist() == [B, int(kept.sum()), int((ocls[:, 1:] >= 0).sum())]
    # the host dict follows suit
    host = gen.to_host(cls_t, ids)
    np.testing.assert_array_equal(host["depth_observed"], pick(1))
    np.testing.assert_array_equal(host["depth_gt_observed"], alone[1])
    assert host["mask_idx"].tolist() == [1] * B
    # rows of a batch's own arrays, without a depth_observed: the other rows are not touched
    rows = np.array([5, 0, 3, 2])
    own = {k: ctx.empty((6, H, W) + inner, dt) for k, dt, inner in (("image_observed", np.uint8, (3,)), ("depth_gt_observed", np.uint16, ()),
                                                                    ("mask_gt_observed", np.uint8, ()))}
    for a in own.values():
        lib.deepim_memset(ctx.handle, a, 0xAB, a.nbytes)
    placed = gen.frames(cls_t, ids, out=own, rows=rows)
    assert placed["depth_observed"] is None
    for k in FRAME_KEYS:
        np.testing.assert_array_equal(own[k].asnumpy()[rows], out[k].asnumpy(), err_msg=k)
        assert (own[k].asnumpy()[[1, 4]].view(np.uint8) == 0xAB).all()


def test_no_occluders_gives_the_bytes_of_the_plain_generator(ctx, lit):
    cls_t, ids = np.array([0, 1, 1, 0, 1, 0], np.int32), 1000 + np.arange(6, dtype=np.uint64)
    plain = _generator(lit).frames(cls_t, ids)
    none = _generator(lit, occluders=_spec(min_occluders=0, max_occluders=0)).frames(cls_t, ids)
    for k in FRAME_KEYS + ("pose_observed", "attempts", "light_offset", "light_intensity", "brightness_ratio"):
        np.testing.assert_array_equal(none[k].asnumpy().view(np.uint8), plain[k].asnumpy().view(np.uint8), err_msg=k)
    np.testing.assert_array_equal(none["depth_observed"].asnumpy(), plain["depth_gt_observed"].asnumpy())
    assert none["kept"].asnumpy().tolist() == [1] * 6 and none["visible"].shape == (6, 1)
    assert plain["image_observed"].asnumpy().any() and "kept" not in plain
    with pytest.raises(KeyError, match="class ids"):
        _generator(lit, occluders=_spec(classes=[0, 2], diameters={0: 0.1, 2: 0.1}))
    with pytest.raises(KeyError, match="class ids"):
        _generator(lit, occluders=_spec(classes=[0], diameters={0: 0.1})).check_classes([0, 1])      # a target without a diameter


# ------------------------------------------------------------------------------------------------------------ g. loader --
N_SYN = 5


def test_loader_over_a_host_set_and_a_resident_one(ctx, world, lit):
    cfg0, rm, observed, points = world
    assert cfg0.network.INPUT_DEPTH
    kw = dict(num_synthetic=N_SYN, synthetic_classes=[0, 1], shuffle=True)
    args = dict(batch_size=tl.BS, seed=tl.SEED, num_rendered_per_observed=tl.R, points=points, noise=tl.NOISE)
    gen, plain_gen = _generator(lit, occluders=_spec()), _generator(lit)
    host = TrainDataLoader(observed, cfg0, rm, synthetic=gen, **args, **kw)
    resident = TrainDataLoader(ResidentObserved(observed, ctx, spare_rows=tl.BS, points=points), cfg0, rm, synthetic=gen, **args, **kw)
    plain = TrainDataLoader(observed, cfg0, rm, synthetic=plain_gen, **args, **kw)
    np.testing.assert_array_equal(host.pairs, plain.pairs)                         # the plan and the draw ids do not change
    np.testing.assert_array_equal(host.draw_ids, plain.draw_ids)
    changed = scene_depth = 0
    for pairs, ids, (d0, l0), (d1, l1), (dp, lp) in zip(host.pairs.copy(), host.draw_ids.copy(), host, resident, plain):
        d0, l0, dp, lp = tl._host(d0), tl._host(l0), tl._host(dp), tl._host(lp)
        tl._same(tl._host(d1), d0)                                                 # both sets: the same batches byte for byte
        tl._same(tl._host(l1), l0)
        is_syn = pairs >= tl.M * tl.R
        for d, p in ((d0, dp), (l0, lp)):
            for k in d:
                np.testing.assert_array_equal(d[k][~is_syn], p[k][~is_syn], err_msg=k)      # real rows: the loader without occluders
        if is_syn.any():
            drawn = gen.frames(host.synthetic_classes[(pairs[is_syn] - tl.M * tl.R) % 2], ids[is_syn])
            seen, alone = drawn["depth_observed"].asnumpy(), drawn["depth_gt_observed"].asnumpy()
            for k in ("depth_observed", "depth_gt_observed"):                      # the scene's depth in; the target alone for the labels
                np.testing.assert_array_equal(d0[k][is_syn], dimage._depth(ctx, {k: drawn[k]}, k, cfg0).asnumpy(), err_msg=k)
            np.testing.assert_array_equal(d0["depth_gt_observed"][is_syn], dp["depth_gt_observed"][is_syn])
            scene_depth += int(np.count_nonzero(seen != alone))
            changed += int(any(not np.array_equal(d0["image_observed"][b], dp["image_observed"][b]) for b in np.nonzero(is_syn)[0]))
    assert changed > 0 and scene_depth > 0                                         # occluders were drawn and the camera's depth holds them
    st = host.stats()
    assert st == resident.stats() and st["occluded_pairs"] == st["observed_pairs"] == N_SYN
    assert 0 <= st["occluded_kept"] <= N_SYN and N_SYN <= st["occluder_slots"] <= 2 * N_SYN
    assert "occluded_pairs" not in plain.stats()


def test_one_train_step_on_an_occluded_batch_at_full_size(ctx):
    """fc6 fixes 480x640: one batch of two occluded synthetic pairs, TRAIN_ITER_SIZE = 1."""
    cfg, net, params, _batches, upd = tf._world(ctx, False, iters=1, n_batches=1)
    rm = upd.render_machine
    FH, FW, K = 480, 640, synthetic.K_LINEMOD
    axes = [0.05, 0.04, 0.035]
    rng = np.random.default_rng(5)
    poses = np.stack([synthetic.sample_pose_pair(rng)[0] for _ in range(2)])
    observed = tl._observed_from_renders(ctx, rm, poses, np.zeros(2, np.int32))
    points = {0: (synthetic.sample_model_points(rng, axes, 3000), np.ones((3, 3000), np.float32))}
    m = synthetic.ellipsoid_mesh(axes, 12, 24)
    m.pop("colors")
    nrm = m["vertices"] / (np.asarray(axes, np.float32) ** 2)
    m["normals"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    m["texture"] = synthetic.procedural_texture()
    light = Render_Py_Light("unused", K, FW, FH, ZN, ZF, list(oemu.BRIGHTNESS_RATIOS), meshes=[m], ctx=ctx)
    fallback = np.concatenate([np.eye(3), [[0.0], [0.0], [0.9]]], 1)
    stats = {0: dict(trans_mean=[0.0, 0.0, 0.9], trans_std=[0.05, 0.04, 0.1], pz_mean=[0.1, -0.2, 0.9], angle_max=70.0, fallback=fallback)}
    gen = SyntheticObserved(light, stats, K, seed=12, occluders=OccluderSpec([0], {0: 0.1}, min_occluders=1, max_occluders=2))
    loader = TrainDataLoader(observed, cfg, rm, batch_size=2, seed=9, points=points, synthetic=gen, num_synthetic=2)
    assert [int((p >= 2).sum()) for p in loader.pairs] == [0, 2]
    data, label = loader.make_batch(loader.pairs[1], loader.draw_ids[1])
    assert np.isfinite(data["image_observed"].asnumpy()).all() and data["mask_observed"].asnumpy().any()
    net.bind_train(ctx, 2, params, num_points=3000)
    net.train_step(data, label, upd, iters=1, lr=tf.LR, wd=cfg.TRAIN.wd, momentum=cfg.TRAIN.momentum)
    sums = {k: v.asnumpy() for k, v in net.act.items() if k.endswith("_loss_sum")}
    print({k: float(v[0]) for k, v in sums.items()}, loader.stats())
    assert sums and all(np.isfinite(v).all() for v in sums.values())
    assert all(np.isfinite(v).all() for v in tf._state(net).values())
    assert loader.stats()["occluded_pairs"] == 2
