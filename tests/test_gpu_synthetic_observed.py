"""Synthetic lit observed frames on the GPU: deepim_sample_observed_poses / deepim_observed_pose_candidate against the reference-run
golden file and the numpy emulation (tests/observed_pose_emulation.py), deepim_sample_lights against the emulation bit for bit,
deepim_render_observed_forward against the existing lit draw with no tolerance (48x64 on the four-pixel store path, 45x61 on the
single-pixel one) and once against oracle/render.py, Render_Py_Light, and core/loader.TrainDataLoader with synthetic pairs
against the chain written out by hand (the world of tests/test_gpu_loader.py). One test at full size."""
import ctypes
import os

import numpy as np
import pytest

import observed_pose_emulation as oemu
import test_gpu_fit as tf
import test_gpu_loader as tl
from mx_deepim_amd import synthetic
from mx_deepim_amd.core.loader import TrainDataLoader
from mx_deepim_amd.core.module import MutableModule
from mx_deepim_amd.lib.pair_matching import data_pair
from mx_deepim_amd.lib.pair_matching.pose_sampler import (pack_observed_table, sample_lights, sample_observed_poses,
                                                          sample_rendered_poses)
from mx_deepim_amd.lib.render_glumpy.render_py_light import Render_Py_Light
from mx_deepim_amd.lib.render_glumpy.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi
from mx_deepim_amd.lib.utils import image as dimage
from mx_deepim_amd.lib.utils.background import BackgroundPool, background_draws_device
from mx_deepim_amd.lib.utils.synthetic_observed import SyntheticObserved
from mx_deepim_amd.runtime import DeviceArray, lib
from oracle import render as orender

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observed_pose_golden.npz")
H, W, K_SMALL = tl.H, tl.W, tl.K_SMALL
ZN, ZF = 0.25, 6.0
cf = ctypes.c_float
u64 = ctypes.c_ulonglong
world = tl.world                 # the loader tests' module fixture, built once for this module too
SYN_SEED, S = 404, 5


def _lit_meshes():
    """Two ellipsoids (12 x 24) with analytic normals and the procedural texture."""
    out = []
    for axes in tl.AXES:
        m = synthetic.ellipsoid_mesh(axes, 12, 24)
        m.pop("colors")
        n = m["vertices"] / (np.asarray(axes, np.float32) ** 2)
        m["normals"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        m["texture"] = synthetic.procedural_texture()
        out.append(m)
    return out


def _machine(ctx, h=H, w=W):
    return Render_Py_Light_ModelNet_Multi(["a", "b"], None, K_SMALL, w, h, ZN, ZF, brightness_ratios=[0.7], meshes=_lit_meshes(), ctx=ctx)


@pytest.fixture(scope="module")
def lit(ctx):
    return _machine(ctx)


def _stats():
    t = oemu.class_table()
    return {c: dict(trans_mean=t[c, 0:3], trans_std=t[c, 3:6], pz_mean=t[c, 6:9], angle_max=t[c, 9], fallback=t[c, 10:22].reshape(3, 4))
            for c in (0, 1)}


@pytest.fixture(scope="module")
def syn(ctx, lit):
    return SyntheticObserved(lit, _stats(), K_SMALL, SYN_SEED, border=oemu.SCENARIO_BORDER)


def _candidate(ctx, cls, table, normals, K, width, height, border):
    B = len(cls)
    pose, stat = ctx.empty((B, 3, 4)), ctx.empty((B, 4), np.float64)
    lib.deepim_observed_pose_candidate(ctx.handle, pose, stat, ctx.array(cls, dtype=np.int32), ctx.array(table, dtype=np.float64),
                                       len(table), ctx.array(normals, dtype=np.float64), np.ascontiguousarray(K, np.float32), width,
                                       height, cf(border), B)
    return pose.asnumpy(), stat.asnumpy()


def _sample(ctx, cls, table, max_attempts, seed, draw_base=0, draw_ids=None, border=oemu.SCENARIO_BORDER):
    """deepim_sample_observed_poses at 48x64 -> (pose, attempts, normals, stat) on the host."""
    B = len(cls)
    pose, attempts = ctx.empty((B, 3, 4)), ctx.empty((B,), np.int32)
    normals, stat = ctx.empty((B, 7), np.float64), ctx.empty((B, 4), np.float64)
    ids = None if draw_ids is None else ctx.array(draw_ids, dtype=np.uint64)
    lib.deepim_sample_observed_poses(ctx.handle, pose, attempts, normals, stat, ctx.array(cls, dtype=np.int32),
                                     ctx.array(table, dtype=np.float64), len(table), K_SMALL, W, H, cf(border), max_attempts, u64(seed),
                                     u64(draw_base), ids, B)
    return pose.asnumpy(), attempts.asnumpy(), normals.asnumpy(), stat.asnumpy()


def _lights(ctx, B, seed, draw_base=0, draw_ids=None, ratios=oemu.BRIGHTNESS_RATIOS):
    off, inten, ratio = sample_lights(ctx, B, seed, draw_base=draw_base, draw_ids=draw_ids, brightness_ratios=ratios)
    return off.asnumpy(), inten.asnumpy(), ratio.asnumpy()


def _frames(ctx, rm, cls, poses, off, inten, ratio, rows=None, N=None, label_value=None, fill=None, depth_factor=1000.0):
    """deepim_render_observed_forward -> (image (N,h,w,3) uint8, depth (N,h,w) uint16, label (N,h,w) uint8) on the host."""
    B, h, w = len(cls), rm.height, rm.width
    N = B if N is None else N
    out = [ctx.empty((N, h, w, 3), np.uint8), ctx.empty((N, h, w), np.uint16), ctx.empty((N, h, w), np.uint8)]
    if fill is not None:
        for a in out:
            lib.deepim_memset(ctx.handle, a, fill, a.nbytes)
    t = rm.mesh_table()
    lib.deepim_render_observed_forward(ctx.handle, out[0], out[1], out[2], None if rows is None else ctx.array(rows, dtype=np.int32), N,
                                       None if label_value is None else ctx.array(label_value, dtype=np.int32), cf(depth_factor),
                                       ctx.array(cls, dtype=np.int32), t.mesh_desc, t.n_classes, t.max_V, t.max_F, t.vertices,
                                       t.vertex_attr, t.normals, t.faces, t.textures, ctx.array(poses), K_SMALL, ctx.array(off),
                                       ctx.array(inten), ctx.array(ratio), B, h, w, cf(ZN), cf(ZF))
    return [a.asnumpy() for a in out]


def _lit_one(ctx, rm, cls, pose, off, inten, ratio):
    """The existing lit draw, B = 1, pixel_means NULL -> (levels (3,h,w) RGB, depth (h,w)) float32."""
    h, w = rm.height, rm.width
    image, depth = ctx.empty((1, 3, h, w)), ctx.empty((1, 1, h, w))
    t = rm.mesh_table()
    lib.deepim_render_classes_forward(ctx.handle, image, depth, None, None, cf(0.0), ctx.array([cls], dtype=np.int32), t.mesh_desc,
                                      t.n_classes, t.max_V, t.max_F, t.vertices, t.vertex_attr, t.normals, t.faces, t.textures,
                                      ctx.array(pose[None]), K_SMALL, None, np.ascontiguousarray(off, np.float32),
                                      ctx.array(inten[None]), cf(float(ratio)), 1, h, w, cf(ZN), cf(ZF))
    return image.asnumpy()[0], depth.asnumpy()[0, 0]


def _six(seed=SYN_SEED):
    """Six consecutive draw ids (all six light positions) whose lights include a colour row with a zero channel and at least
    three distinct ratios, found with the emulation; poses in front of the camera, two classes."""
    for base in range(0, 6000, 6):
        ids = base + np.arange(6, dtype=np.uint64)
        off, inten, ratio, (pos, colour, k) = oemu.lights(seed, ids)
        if len(set(k.tolist())) >= 3 and (inten == 0).any() and (colour == 6).any():
            break
    rng = np.random.default_rng(5)
    poses = np.zeros((6, 3, 4), np.float32)
    for i in range(6):
        poses[i, :, :3] = synthetic.random_rotation(rng)
        poses[i, :, 3] = [rng.uniform(-0.05, 0.05), rng.uniform(-0.04, 0.04), rng.uniform(0.45, 0.7)]
    return ids, np.array([0, 1, 1, 0, 1, 0], np.int32), poses, off, inten, ratio


# ------------------------------------------------------------------------------------------------------ the pose sampler --
def test_candidates_match_the_reference_run_golden(ctx):
    g = np.load(GOLDEN)
    pose, stat = _candidate(ctx, g["cls"], g["table"], g["normals"], g["K"], int(g["width"]), int(g["height"]), float(g["border"]))
    want = g["pose"]
    rot = np.abs(pose[:, :, :3] - want[:, :, :3]).max()
    dt, at = np.abs(pose[:, :, 3] - want[:, :, 3]), np.abs(want[:, :, 3])
    deg = np.abs(stat[:, 0] - g["deg"]).max()
    cxy = max((np.abs(stat[:, 1] - g["cx"]) / np.abs(g["cx"])).max(), (np.abs(stat[:, 2] - g["cy"]) / np.abs(g["cy"])).max())
    print("rotation %.3e (2.4e-7), translation rel %.3e (2.4e-7), deg %.3e (1e-5), centre rel %.3e (1e-9)"
          % (rot, (dt[at > 0] / at[at > 0]).max(), deg, cxy))
    assert rot <= 2.4e-7 and (dt <= 2.4e-7 * at).all()
    assert deg <= 1e-5 and cxy <= 1e-9
    np.testing.assert_array_equal(stat[:, 3] != 0, g["accept"])
    assert set(np.unique(stat[:, 3])) <= {0.0, 1.0}


def test_sampler_across_a_block_matches_the_emulation(ctx):
    s = oemu.block_scenario()
    B = oemu.SCENARIO_B
    pose, attempts, normals, stat = _sample(ctx, s["cls"], s["table"], oemu.SCENARIO_ATTEMPTS, oemu.SCENARIO_SEED,
                                            draw_base=oemu.SCENARIO_BASE)
    keep = ~s["borderline"]
    assert B == 257 and (~keep).mean() <= 0.01
    print("%.0f %% of pairs retried, mean %.2f attempts, max %d" % (100 * (attempts > 1).mean(), attempts.mean(), attempts.max()))
    np.testing.assert_array_equal(attempts[keep], s["attempts"][keep])
    assert (attempts > 1).mean() >= 0.3             # a kernel that never retries cannot pass
    print("normals: %.3e from the emulation (bar 1e-12)" % np.abs(normals - s["normals"])[keep].max())
    assert np.abs(normals - s["normals"])[keep].max() <= 1e-12
    assert np.abs(pose - s["pose"])[keep].max() <= 2.4e-7 * max(1.0, np.abs(s["pose"]).max())
    assert np.abs(stat - s["stat"])[keep].max() <= 1e-5 and (stat[:, 3] == 1).all()
    # the accepted normals replay to the same pose through the normals-in entry
    again, st2 = _candidate(ctx, s["cls"], s["table"], normals, K_SMALL, W, H, oemu.SCENARIO_BORDER)
    np.testing.assert_array_equal(pose.view(np.uint32), again.view(np.uint32))
    assert (st2[:, 3] == 1).all()
    # the Python entry: the same arrays
    p2, a2, z2, s2 = sample_observed_poses(ctx.array(s["cls"], dtype=np.int32), ctx.array(s["table"], dtype=np.float64), K_SMALL, W, H,
                                           oemu.SCENARIO_SEED, draw_base=oemu.SCENARIO_BASE, border=oemu.SCENARIO_BORDER,
                                           with_normals=True, with_stat=True)
    for got, want in zip((p2, a2, z2, s2), (pose, attempts, normals, stat)):
        np.testing.assert_array_equal(got.asnumpy(), want)


def test_sampler_bounds(ctx):
    table = oemu.class_table(angle_max=(0.0, 0.0))
    cls = np.array([0, 1, -1, 2, 1] * 14, np.int32)
    pose, attempts, normals, stat = _sample(ctx, cls, table, 1, 3)
    ok = (cls >= 0) & (cls < 2)
    np.testing.assert_array_equal(attempts, np.where(ok, 0, -1))
    np.testing.assert_array_equal(pose[ok].reshape(-1, 12).view(np.uint32), table[cls[ok], 10:].astype(np.float32).view(np.uint32))
    assert not pose[~ok].any() and not normals.any() and not stat.any()
    with pytest.raises(RuntimeError, match="max_attempts"):
        _sample(ctx, cls, table, 0, 3)
    with pytest.raises(RuntimeError, match="ratios"):
        _lights(ctx, 4, 1, ratios=np.arange(9) / 10.0)
    assert _sample(ctx, cls[:0], table, 3, 1)[0].shape == (0, 3, 4)
    assert _lights(ctx, 0, 1)[0].shape == (0, 3)


def test_light_draws_equal_the_emulation(ctx):
    B, seed, base = 512, 17, (1 << 33) + 5          # ids beyond 32 bits: the high counter word is used
    got = _lights(ctx, B, seed, draw_base=base)
    want = oemu.lights(seed, base + np.arange(B, dtype=np.uint64))
    for g, w in zip(got, want[:3]):
        assert g.dtype == np.float32
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))
    three = _lights(ctx, 64, seed, draw_base=base, ratios=(0.1, 0.5, 0.9))
    np.testing.assert_array_equal(three[2], oemu.lights(seed, base + np.arange(64, dtype=np.uint64), ratios=(0.1, 0.5, 0.9))[2])


def test_a_pairs_draw_does_not_depend_on_its_placement(ctx, syn):
    B, base = 16, 1000
    cls = (np.arange(B) % 2).astype(np.int32)
    keys = ("pose_observed", "attempts", "light_offset", "light_intensity", "brightness_ratio", "image_observed",
            "depth_gt_observed", "mask_gt_observed")

    def run(c, ids):
        out = syn.frames(c, ids)
        return [out[k].asnumpy() for k in keys]

    whole = run(cls, base + np.arange(B))
    halves = [run(cls[i:i + 8], base + i + np.arange(8)) for i in (0, 8)]
    perm = np.random.default_rng(2).permutation(B)
    permuted = run(cls[perm], base + perm)
    assert (whole[1] > 1).any() and whole[5].any()
    for k in range(len(keys)):
        np.testing.assert_array_equal(np.concatenate([halves[0][k], halves[1][k]]).view(np.uint8), whole[k].view(np.uint8), err_msg=keys[k])
        np.testing.assert_array_equal(permuted[k].view(np.uint8), whole[k][perm].view(np.uint8), err_msg=keys[k])
    # draw_ids against draw_base at the entries themselves
    t = ctx.array(oemu.class_table(), dtype=np.float64)
    a = sample_observed_poses(ctx.array(cls, dtype=np.int32), t, K_SMALL, W, H, SYN_SEED, draw_base=base, border=oemu.SCENARIO_BORDER)
    b = sample_observed_poses(ctx.array(cls, dtype=np.int32), t, K_SMALL, W, H, SYN_SEED, draw_base=77, draw_ids=base + np.arange(B),
                              border=oemu.SCENARIO_BORDER)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.asnumpy().view(np.uint8), y.asnumpy().view(np.uint8))
    np.testing.assert_array_equal(a[0].asnumpy().view(np.uint32), whole[0].view(np.uint32))
    for x, y in zip(_lights(ctx, B, SYN_SEED, draw_base=base), _lights(ctx, B, SYN_SEED, draw_base=3, draw_ids=base + np.arange(B))):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------- the draw --
@pytest.mark.parametrize("h,w", [(48, 64), (45, 61)])
def test_frames_equal_the_existing_lit_draw(ctx, h, w):
    """(48, 64): the four-pixels-per-lane store path; (45, 61): 2745 pixels, not a multiple of 4, the single-pixel path with a
    partial last block."""
    rm = _machine(ctx, h, w)
    _ids, cls, poses, off, inten, ratio = _six()
    assert len(set(map(tuple, off.tolist()))) == 6 and len(set(ratio.tolist())) >= 3 and (inten == 0).any()
    label_value = np.array([1, 2, 3, 1, 200, 255], np.int32)
    image, depth, label = _frames(ctx, rm, cls, poses, off, inten, ratio, label_value=label_value)
    differ = 0
    for b in range(6):
        levels, dep = _lit_one(ctx, rm, int(cls[b]), poses[b], off[b], inten[b], ratio[b])
        assert np.count_nonzero(dep) > 20, b
        np.testing.assert_array_equal(image[b].astype(np.float32), levels[::-1].transpose(1, 2, 0), err_msg=str(b))
        prod = dep.astype(np.float32) * np.float32(1000)
        assert prod.dtype == np.float32
        np.testing.assert_array_equal(depth[b], prod.astype(np.uint16), err_msg=str(b))
        np.testing.assert_array_equal(label[b], (label_value[b] * (dep != 0)).astype(np.uint8), err_msg=str(b))
        differ += int(np.count_nonzero(np.rint(prod) != np.floor(prod)))
        zero = np.nonzero(inten[b] == 0)[0]         # a colour row's zero channel is black in the frame (BGR)
        for c in zero:
            assert not image[b][:, :, 2 - c].any()
    assert differ > 0                               # truncation and rint differ here: a rounding kernel fails
    # NULL label_value = 1
    _i, _d, ones = _frames(ctx, rm, cls, poses, off, inten, ratio)
    np.testing.assert_array_equal(ones, (label != 0).astype(np.uint8))
    # a class id outside the table: an empty frame, the others unaffected
    bad = cls.copy()
    bad[2] = 2
    i2, d2, l2 = _frames(ctx, rm, bad, poses, off, inten, ratio, label_value=label_value)
    assert not i2[2].any() and not d2[2].any() and not l2[2].any()
    keep = [0, 1, 3, 4, 5]
    np.testing.assert_array_equal(i2[keep], image[keep])
    np.testing.assert_array_equal(d2[keep], depth[keep])


@pytest.mark.parametrize("h,w", [(48, 64), (45, 61)])
def test_destination_rows(ctx, h, w):
    rm = _machine(ctx, h, w)
    _ids, cls, poses, off, inten, ratio = _six()
    sel, rows = slice(0, 4), np.array([7, 0, 3, 5], np.int32)
    ident = _frames(ctx, rm, cls[sel], poses[sel], off[sel], inten[sel], ratio[sel])
    got = _frames(ctx, rm, cls[sel], poses[sel], off[sel], inten[sel], ratio[sel], rows=rows, N=9, fill=0xAB)
    others = [r for r in range(9) if r not in rows.tolist()]
    for g, want in zip(got, ident):
        np.testing.assert_array_equal(g[rows], want)
        assert (g[others].view(np.uint8) == 0xAB).all()
    assert ident[0].any()
    # a row outside [0, N) is not written, and the z-buffer is still put back: the next draw is the identity draw again
    off_rows = rows.copy()
    off_rows[1] = 9
    got = _frames(ctx, rm, cls[sel], poses[sel], off[sel], inten[sel], ratio[sel], rows=off_rows, N=9, fill=0xAB)
    assert (got[0][[0, 9 - 1]].view(np.uint8) == 0xAB).all()
    again = _frames(ctx, rm, cls[sel], poses[sel], off[sel], inten[sel], ratio[sel])
    for a, b in zip(again, ident):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(RuntimeError, match="N >= B"):
        _frames(ctx, rm, cls[sel], poses[sel], off[sel], inten[sel], ratio[sel], N=3)


def test_one_frame_against_the_oracle(ctx, lit):
    """Depth frame exact; levels within 1 on fewer than 1 % of the frame's values, the bar of test_gpu_render.py:316, which the
    parent's float lit draw is held to on the same input in this test."""
    _ids, cls, poses, off, inten, ratio = _six()
    b = int(np.nonzero((inten != 0).all(1))[0][0])                     # the white row: every channel lit
    m = _lit_meshes()[int(cls[b])]
    ri, rd = orender.render(m["vertices"], m["uv"], m["faces"], poses[b], K_SMALL, H, W, texture=m["texture"], normals=m["normals"],
                            light_offset=off[b], light_intensity=inten[b], brightness_ratio=float(ratio[b]))
    levels, dep = _lit_one(ctx, lit, int(cls[b]), poses[b], off[b], inten[b], ratio[b])
    np.testing.assert_array_equal(dep, rd)
    parent = np.abs(levels - ri)
    assert parent.max() <= 1.0 and np.mean(parent > 0) < 0.01, (parent.max(), np.mean(parent > 0))
    image, depth, _label = _frames(ctx, lit, cls[b:b + 1], poses[b:b + 1], off[b:b + 1], inten[b:b + 1], ratio[b:b + 1])
    np.testing.assert_array_equal(depth[0], (rd.astype(np.float32) * np.float32(1000)).astype(np.uint16))
    d = np.abs(image[0].astype(np.float32) - ri[::-1].transpose(1, 2, 0))
    print("levels: %.4f %% of the values differ from the oracle (parent %.4f %%), max %g" % (100 * np.mean(d > 0), 100 * np.mean(parent > 0), d.max()))
    assert d.max() <= 1.0 and np.mean(d > 0) < 0.01 and np.count_nonzero(rd) > 20


def test_render_py_light_returns_the_generators_bytes(ctx):
    m = _lit_meshes()[0]
    ratios = [0.2, 0.25, 0.3, 0.35, 0.4]
    rm = Render_Py_Light("unused", K_SMALL, W, H, ZN, ZF, ratios, meshes=[m], ctx=ctx)
    stats = {0: _stats()[0]}
    gen = SyntheticObserved(rm, stats, K_SMALL, SYN_SEED, border=oemu.SCENARIO_BORDER, brightness_ratios=ratios)
    out = gen.frames(np.zeros(4, np.int32), 50 + np.arange(4))
    poses, off, inten, ratio = (out[k].asnumpy() for k in ("pose_observed", "light_offset", "light_intensity", "brightness_ratio"))
    image, depth = out["image_observed"].asnumpy(), out["depth_gt_observed"].asnumpy()
    assert len(set(ratio.tolist())) >= 2
    for b in range(4):
        t = poses[b][:, 3]
        k = int(np.argmin(np.abs(np.asarray(ratios, np.float32) - ratio[b])))
        light_position = off[b].astype(np.float64) + np.array([t[0], -t[1], -t[2]], np.float64)       # ds_1:131-135
        bgr, dep = rm.render(poses[b][:, :3], t, light_position, inten[b], brightness_k=k, r_type="mat")
        assert bgr.dtype == np.uint8 and bgr.shape == (H, W, 3) and np.count_nonzero(dep) > 20
        np.testing.assert_array_equal(bgr, image[b])
        np.testing.assert_array_equal((dep * np.float32(1000)).astype(np.uint16), depth[b])
        other, _d = rm.render(poses[b][:, :3], t, light_position, inten[b], brightness_k=(k + 2) % 5, r_type="mat")
        assert not np.array_equal(other, bgr)                                                       # brightness_k selects the ratio
    host = gen.to_host(np.zeros(4, np.int32), 50 + np.arange(4))
    np.testing.assert_array_equal(host["image_observed"], image)
    np.testing.assert_array_equal(host["depth_observed"], depth)
    assert host["mask_idx"].tolist() == [1] * 4 and host["depth_observed"] is not host["depth_gt_observed"]
    assert set(host) == {"image_observed", "depth_gt_observed", "depth_observed", "mask_gt_observed", "mask_idx", "pose_observed", "class_index"}


# ----------------------------------------------------------------------------------------------------------- the loader --
def test_loader_without_synthetic_pairs_is_unchanged(ctx, world, syn):
    plain = tl._epochs(tl._loader(world), 1)[0]
    for loader in (tl._loader(world, synthetic=None), tl._loader(world, synthetic=syn, num_synthetic=0)):
        got = tl._epochs(loader, 1)[0]
        assert len(got) == len(plain) == 3
        for (d0, l0), (d1, l1) in zip(got, plain):
            tl._same(d0, d1)
            tl._same(l0, l1)
    with pytest.raises(ValueError, match="synthetic="):
        tl._loader(world, num_synthetic=3)
    with pytest.raises(KeyError, match="class ids"):
        tl._loader(world, synthetic=syn, num_synthetic=3, synthetic_classes=[0, 2])


def _hand_mixed_batch(ctx, world, syn, cfg, pairs, ids, pool=None):
    """The chain the loader is specified as with synthetic pairs, written out: -> (data, label, attempts, observed attempts,
    use_bg)."""
    _cfg, rm, obs, points = world
    pairs, ids = np.asarray(pairs), np.asarray(ids)
    real = pairs < tl.M * tl.R
    m = np.where(real, pairs // tl.R, 0)
    B = len(pairs)
    host = {k: obs[k][m].copy() for k in ("image_observed", "depth_gt_observed", "depth_observed", "mask_gt_observed")}
    mask_idx, cls, pose = obs["mask_idx"][m].copy(), obs["class_index"][m].copy(), obs["pose_observed"][m].copy()
    rows = np.nonzero(~real)[0]
    observed_attempts = np.zeros(0, np.int32)
    if rows.size:
        cls_syn = np.array([0, 1], np.int32)[(pairs[rows] - tl.M * tl.R) % 2]
        drawn = syn.frames(cls_syn, ids[rows])
        for k in ("image_observed", "depth_gt_observed", "mask_gt_observed"):
            host[k][rows] = drawn[k].asnumpy()
        host["depth_observed"][rows] = host["depth_gt_observed"][rows]
        mask_idx[rows], cls[rows], pose[rows] = 1, cls_syn, drawn["pose_observed"].asnumpy()
        observed_attempts = drawn["attempts"].asnumpy()
    frames = {"depth_gt_observed": host["depth_gt_observed"], "depth_observed": host["depth_observed"],
              "mask_gt_observed": host["mask_gt_observed"], "mask_idx": mask_idx}
    use = None
    if pool is None:
        image = dimage.transform_batch(ctx, ctx.array(host["image_observed"], dtype=np.uint8), dimage._means_rgb(cfg))
    else:
        use, idx = background_draws_device(ctx, B, tl.SEED, ids.astype(np.uint64), float(cfg.TRAIN.REPLACE_OBSERVED_BG_RATIO), len(pool),
                                           always=~real)
        image = dimage.transform_batch_pool(ctx, ctx.array(host["image_observed"], dtype=np.uint8), dimage._means_rgb(cfg),
                                            ctx.array(host["mask_gt_observed"], dtype=np.uint8), use, idx, pool)
        use = use.asnumpy()
    batch = {"image_observed": image, "depth_gt_observed": dimage._depth(ctx, frames, "depth_gt_observed", cfg),
             "depth_observed": dimage._depth(ctx, frames, "depth_observed", cfg),
             "mask_gt_observed": dimage.label_mask(ctx, frames, "mask_gt_observed"),
             "pose_observed": ctx.array(pose), "class_index": ctx.array(cls, dtype=np.int32)}
    batch["pose_rendered"], attempts = sample_rendered_poses(batch["pose_observed"], K_SMALL, W, H, tl.SEED, draw_ids=ids, noise=tl.NOISE)
    batch["image_rendered"], batch["depth_rendered"] = rm.render_batch(batch["class_index"], batch["pose_rendered"])
    batch["point_cloud_model"] = ctx.array(np.stack([points[int(c)][0] for c in cls]))
    batch["point_cloud_weights"] = ctx.array(np.stack([points[int(c)][1] for c in cls]))
    out = data_pair.get_data_pair_train_batch(batch, cfg)
    return out["data"], out["label"], attempts.asnumpy(), observed_attempts, use, host


def test_mixed_batches_equal_the_hand_written_chain(ctx, world, syn):
    cfg = world[0]
    loader = tl._loader(world, shuffle=True, synthetic=syn, num_synthetic=S, synthetic_classes=[0, 1])
    assert len(loader) == 5 and loader.dropped == 0
    attempts, observed, first_syn_poses = [], [], {}
    for e in range(2):
        order = loader.pairs.reshape(-1)
        assert sorted(order.tolist()) == list(range(20)) and order.tolist() != list(range(20))
        np.testing.assert_array_equal(loader.draw_ids, (loader.pairs + e * 20).astype(np.uint64))
        mixed = 0
        for pairs, ids, (data, label) in zip(loader.pairs.copy(), loader.draw_ids.copy(), loader):
            want_data, want_label, a, oa, _use, _host = _hand_mixed_batch(ctx, world, syn, cfg, pairs, ids)
            data = tl._host(data)
            tl._same(data, tl._host(want_data))
            tl._same(tl._host(label), tl._host(want_label))
            attempts.append(a)
            observed.append(oa)
            is_syn = pairs >= tl.M * tl.R
            mixed += int(0 < is_syn.sum() < tl.BS)
            for b in np.nonzero(is_syn)[0]:
                assert np.count_nonzero(data["depth_gt_observed"][b]) > 0 and data["mask_observed"][b].any()
                np.testing.assert_array_equal(data["depth_observed"][b], data["depth_gt_observed"][b])
                if e == 0:
                    first_syn_poses[int(pairs[b])] = data["tgt_pose"][b]
                else:
                    assert not np.array_equal(first_syn_poses[int(pairs[b])], data["tgt_pose"][b])      # fresh poses after reset()
        assert mixed > 0                             # real and synthetic rows share batches
        loader.reset()
    attempts, observed = np.concatenate(attempts), np.concatenate(observed)
    stats = loader.stats()
    assert stats == {"pairs": 40, "attempts": int(attempts.sum()), "exhausted": int((attempts == 0).sum()),
                     "observed_pairs": 2 * S, "observed_attempts": int(observed.sum()), "observed_exhausted": int((observed == 0).sum())}
    assert stats["observed_attempts"] >= 2 * S - stats["observed_exhausted"] and len(first_syn_poses) == S


def test_synthetic_rows_always_take_a_pool_background(ctx, world, syn):
    import background_emulation as bemu
    pool = BackgroundPool(ctx, [bemu.background_image(bh, bw) for bh, bw in bemu.SMALL_BACKGROUNDS] + [bemu.background_image(H, W)], H, W)
    cfg = tl._config()
    cfg.TRAIN.REPLACE_OBSERVED_BG_RATIO = 0.0
    loader = tl._loader(world, cfg=cfg, shuffle=True, backgrounds=pool, synthetic=syn, num_synthetic=S, synthetic_classes=[0, 1])
    plain = tl._loader(world, cfg=cfg, shuffle=True, synthetic=syn, num_synthetic=S, synthetic_classes=[0, 1])
    np.testing.assert_array_equal(loader.pairs, plain.pairs)
    seen = 0
    for pairs, ids, (data, _l), (pdata, _pl) in zip(loader.pairs.copy(), loader.draw_ids.copy(), loader, plain):
        want_data, _wl, _a, _oa, use, host = _hand_mixed_batch(ctx, world, syn, cfg, pairs, ids, pool=pool)
        is_syn = pairs >= tl.M * tl.R
        np.testing.assert_array_equal(use, is_syn.astype(np.int32))
        got, without = data["image_observed"].asnumpy(), pdata["image_observed"].asnumpy()
        np.testing.assert_array_equal(got, want_data["image_observed"].asnumpy())
        for b in range(tl.BS):
            off_label = np.repeat((host["mask_gt_observed"][b] == 0)[None], 3, 0)
            np.testing.assert_array_equal(got[b][~off_label], without[b][~off_label])
            if is_syn[b]:                    # pool pixels outside the label, where the frame was black
                assert np.count_nonzero(got[b][off_label] != without[b][off_label]) > 0
                seen += 1
            else:
                np.testing.assert_array_equal(got[b], without[b])
    assert seen == S


def test_nothing_is_read_back_with_synthetic_pairs(ctx, world, syn, monkeypatch):
    loader = tl._loader(world, shuffle=True, synthetic=syn, num_synthetic=S, synthetic_classes=[0, 1])
    reads = []
    real = DeviceArray.asnumpy
    monkeypatch.setattr(DeviceArray, "asnumpy", lambda self: (reads.append(self.nbytes), real(self))[1])
    assert sum(1 for _ in loader) == 5 and reads == []
    assert loader.stats()["observed_pairs"] == S and reads == [48]          # one read-back, on demand


def test_fit_over_mixed_batches_equals_the_hand_loop_at_full_size(ctx):
    """fc6 fixes 480x640: batches of 2 with one real and one synthetic pair each, TRAIN_ITER_SIZE = 1, one epoch of two batches."""
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
    n = m["vertices"] / (np.asarray(axes, np.float32) ** 2)
    m["normals"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    m["texture"] = synthetic.procedural_texture()
    light = Render_Py_Light("unused", K, FW, FH, ZN, ZF, list(oemu.BRIGHTNESS_RATIOS), meshes=[m], ctx=ctx)
    fallback = np.concatenate([np.eye(3), [[0.0], [0.0], [0.9]]], 1)
    stats = {0: dict(trans_mean=[0.0, 0.0, 0.9], trans_std=[0.05, 0.04, 0.1], pz_mean=[0.1, -0.2, 0.9], angle_max=70.0, fallback=fallback)}
    gen = SyntheticObserved(light, stats, K, seed=12)

    def loader():
        return TrainDataLoader(observed, cfg, rm, batch_size=2, seed=9, points=points, synthetic=gen, num_synthetic=2)

    first = loader()
    assert len(first) == 2 and [int((p >= 2).sum()) for p in first.pairs] == [0, 2]
    first = TrainDataLoader(observed, cfg, rm, batch_size=2, seed=9, points=points, synthetic=gen, num_synthetic=2, shuffle=True)
    # seed 9's permutation of the four pairs puts one synthetic pair into each batch
    assert [int((p >= 2).sum()) for p in first.pairs] == [1, 1]
    net.bind_train(ctx, 2, params, num_points=3000)
    sink = []
    MutableModule(cfg, net, logger=tf._logger("test_gpu_synthetic_observed.fit", sink)).fit(
        first, eval_metric=tf._metrics(cfg), optimizer_params={"learning_rate": tf.LR, "momentum": cfg.TRAIN.momentum, "wd": cfg.TRAIN.wd},
        begin_epoch=0, num_epoch=1, prefix="unused", updater=upd)
    after_fit = tf._state(net)
    st = first.stats()
    assert first.epoch == 1 and st["pairs"] == 4 and st["observed_pairs"] == 2
    assert all(np.isfinite(v).all() for v in after_fit.values())
    assert sink and not any("nan" in str(line).lower() or "inf" in str(line).lower().replace("info", "") for line in sink)
    net.bind_train(ctx, 2, params, num_points=3000)
    second = TrainDataLoader(observed, cfg, rm, batch_size=2, seed=9, points=points, synthetic=gen, num_synthetic=2, shuffle=True)
    for data, label in second:
        assert np.isfinite(data["image_observed"].asnumpy()).all()
        net.train_step(data, label, upd, iters=1, lr=tf.LR, wd=cfg.TRAIN.wd, momentum=cfg.TRAIN.momentum)
    tf._assert_same_bytes(after_fit, tf._state(net))
    moved = [k for k, v in params.items() if not np.array_equal(np.asarray(v, np.float32), after_fit["w:" + k])]
    assert moved                                # the two steps really trained
