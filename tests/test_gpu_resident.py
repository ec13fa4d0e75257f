"""Device-resident observed sets on the GPU. Kernel level, straight through the ABI: deepim_ingest_bgr8_frames / _pool_frames
against the per-sample entries on host-gathered frames and against the numpy formula (frames of 6x10 and of 5x7 = 35 pixels,
where lanes straddle two pairs whose frames differ and frames start at odd bytes; bases dword-aligned and offset by one byte),
an index outside the set, deepim_gather_rows, and offsets past 2^31 in a 4 700-frame allocation. Loader level, on the 48x64
world of test_gpu_loader.py: every batch of TrainDataLoader / TestDataLoader over a ResidentObserved equals the host-set
loader's bit for bit, what a batch uploads, pred_eval, and fit at full size."""
import ctypes

import numpy as np
import pytest

import background_emulation as bemu
import test_gpu_fit as tf
import test_gpu_loader as tl
import test_gpu_synthetic_observed as tso
import test_gpu_test_loader as ttl
import test_gpu_tester as tt
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import loader as L
from mx_deepim_amd.core import tester
from mx_deepim_amd.core.module import MutableModule
from mx_deepim_amd.core.resident import ResidentObserved
from mx_deepim_amd.lib.dataset.LM6D_REFINE import LM6D_REFINE
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
from mx_deepim_amd.lib.utils.background import BackgroundPool
from mx_deepim_amd.lib.utils.synthetic_observed import SyntheticObserved
from mx_deepim_amd.runtime import Context, DeviceArray, lib
from mx_deepim_amd.symbols import deepIM_flownet

pytestmark = pytest.mark.gpu
FRAME_RANGE = 16                 # bit 4 of the status word
MEANS = np.array([1.5, 120.25, 7.0], np.float32)
world = tl.world                 # the loader tests' module fixture, built once for this module too


def u8(ctx, a):
    return ctx.array(a, dtype=np.uint8)


def i32(ctx, a):
    return ctx.array(a, dtype=np.int32)


def status(ctx):
    st = ctypes.c_int(-1)
    lib.deepim_zoom_status(ctx.handle, ctypes.byref(st))
    return st.value


def at_offset(ctx, a, off):
    """`a` on the device, flat, `off` bytes behind a fresh allocation's start: off = 0 is dword-aligned, 1 is not."""
    return u8(ctx, np.concatenate([np.zeros(off, np.uint8), a.reshape(-1)]))[off:]


def formula(frames, means):
    """out[b,i,y,x] = float(frames[b,y,x,2-i]) - means[i], one fp32 subtraction"""
    return frames[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32) - np.asarray(means, np.float32).reshape(1, 3, 1, 1)


def per_sample(ctx, frames, means):
    B, H, W, _ = frames.shape
    out = ctx.empty((B, 3, H, W))
    lib.deepim_ingest_bgr8(ctx.handle, out, u8(ctx, frames), None, None, None, means, B, H, W)
    return out.asnumpy()


def through_index(ctx, frames_dev, index, N, means, H, W):
    B = len(index)
    out = ctx.empty((B, 3, H, W))
    out.copyfrom(np.float32(-7.0))
    lib.deepim_ingest_bgr8_frames(ctx.handle, out, frames_dev, i32(ctx, index), N, means, B, H, W)
    return out.asnumpy()


# ---------------------------------------------------------------------------------------------------------- the kernels --
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("H,W", [(6, 10), (5, 7)])
def test_bgr_entries_equal_the_per_sample_entries_on_gathered_frames(ctx, H, W, off):
    N, index = 7, np.array([6, 0, 0, 3, 6], np.int32)
    B = len(index)
    rng = np.random.default_rng(H * 10 + W + off)
    frames = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    status(ctx)                                                                   # reading clears the sticky word
    for means in (MEANS, None):
        got = through_index(ctx, at_offset(ctx, frames, off), index, N, means, H, W)
        np.testing.assert_array_equal(got.view(np.uint32), per_sample(ctx, frames[index], means).view(np.uint32))
        np.testing.assert_array_equal(got.view(np.uint32), formula(frames[index], MEANS if means is not None else np.zeros(3)).view(np.uint32))
    # the pool variant: a two-image pool, use_bg mixing 0 and 1, both label values in every frame
    images = [bemu.background_image(bh, bw) for bh, bw in bemu.SMALL_BACKGROUNDS[2:4]]
    pool = BackgroundPool(ctx, images, H, W)
    fg = (rng.integers(0, 2, (N, H, W)) * 5).astype(np.uint8)
    fg[:, 0, 0], fg[:, 0, 1] = 0, 5
    use_bg, bg_index = np.array([1, 0, 1, 1, 0], np.int32), np.array([0, 1, 1, 0, 1], np.int32)
    want = ctx.empty((B, 3, H, W))
    lib.deepim_ingest_bgr8_pool(ctx.handle, want, u8(ctx, frames[index]), u8(ctx, fg[index]), i32(ctx, use_bg), i32(ctx, bg_index),
                                pool.pixels, pool.desc, pool.xtab, pool.ytab, len(pool), MEANS, B, H, W)
    got = ctx.empty((B, 3, H, W))
    got.copyfrom(np.float32(-7.0))
    lib.deepim_ingest_bgr8_pool_frames(ctx.handle, got, at_offset(ctx, frames, off), at_offset(ctx, fg, off), i32(ctx, index), N,
                                       i32(ctx, use_bg), i32(ctx, bg_index), pool.pixels, pool.desc, pool.xtab, pool.ytab, len(pool),
                                       MEANS, B, H, W)
    np.testing.assert_array_equal(got.asnumpy().view(np.uint32), want.asnumpy().view(np.uint32))
    np.testing.assert_array_equal(got.asnumpy().view(np.uint32),
                                  bemu.ingest_pool(frames[index], fg[index], use_bg, bg_index, images, MEANS).view(np.uint32))
    assert not np.array_equal(got.asnumpy(), formula(frames[index], MEANS))          # backgrounds were composited
    assert status(ctx) == 0


@pytest.mark.parametrize("H,W", [(6, 10), (5, 7)])
def test_an_index_outside_the_set_is_an_empty_frame(ctx, H, W):
    N, index = 7, np.array([0, 7, -1, 2], np.int32)
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    status(ctx)                                                                   # reading clears the sticky word
    got = through_index(ctx, u8(ctx, frames), index, N, MEANS, H, W)
    empty = np.broadcast_to((np.float32(0) - MEANS).reshape(3, 1, 1), (3, H, W))
    np.testing.assert_array_equal(got[1], empty)
    np.testing.assert_array_equal(got[2], empty)
    np.testing.assert_array_equal(got[[0, 3]], per_sample(ctx, frames[[0, 2]], MEANS))
    assert status(ctx) & FRAME_RANGE
    good = through_index(ctx, u8(ctx, frames), np.array([0, 6, 1, 2], np.int32), N, MEANS, H, W)
    np.testing.assert_array_equal(good, formula(frames[[0, 6, 1, 2]], MEANS))
    assert status(ctx) == 0                                                       # clear after a clean call
    # the pool variant: no background for the pair without a frame
    images = [bemu.background_image(bh, bw) for bh, bw in bemu.SMALL_BACKGROUNDS[2:4]]
    pool = BackgroundPool(ctx, images, H, W)
    fg = np.zeros((N, H, W), np.uint8)                                            # every pixel would take the background
    out = ctx.empty((4, 3, H, W))
    lib.deepim_ingest_bgr8_pool_frames(ctx.handle, out, u8(ctx, frames), u8(ctx, fg), i32(ctx, index), N, None, i32(ctx, [0, 1, 0, 1]),
                                       pool.pixels, pool.desc, pool.xtab, pool.ytab, len(pool), MEANS, 4, H, W)
    out = out.asnumpy()
    np.testing.assert_array_equal(out[1], empty)
    np.testing.assert_array_equal(out[2], empty)
    np.testing.assert_array_equal(out[[0, 3]], bemu.ingest_pool(frames[[0, 2]], fg[[0, 2]], None, np.array([0, 1]), images, MEANS))
    assert status(ctx) == FRAME_RANGE


@pytest.mark.parametrize("words,off_words", [(1, 0), (12, 0), (37, 0), (16, 0), (16, 1)])
def test_gather_rows(ctx, words, off_words):
    """1, 12 and 37 words; 37 is the word path, 16 the 16-byte path — on an aligned out and on one a word off, the word path again"""
    n_rows, index = 9, np.array([8, 0, 3, 3, 9, 8, -2, 1], np.int32)
    B = len(index)
    rng = np.random.default_rng(words)
    table = rng.integers(1, 2 ** 32, (n_rows, words), dtype=np.uint32)
    whole = ctx.empty((off_words + B * words,), np.uint32)
    whole.copyfrom(np.uint32(0xdeadbeef))
    out = whole[off_words:]
    status(ctx)
    lib.deepim_gather_rows(ctx.handle, out, ctx.array(table, dtype=np.uint32), i32(ctx, index), n_rows, words, B)
    ok = (index >= 0) & (index < n_rows)
    want = np.where(ok[:, None], table[np.where(ok, index, 0)], 0).astype(np.uint32)
    np.testing.assert_array_equal(out.asnumpy().reshape(B, words), want)
    assert status(ctx) == FRAME_RANGE
    lib.deepim_gather_rows(ctx.handle, out, ctx.array(table, dtype=np.uint32), i32(ctx, index[:4]), n_rows, words, 4)
    np.testing.assert_array_equal(out.asnumpy().reshape(B, words)[:4], table[index[:4]])
    assert status(ctx) == 0


def test_offsets_past_2_31(ctx):
    """N = 4 700 frames of 480x640: frame 2 400 of the BGR array starts at byte 2.2e9, frame 4 699 at 4.3e9. The arrays are
    not initialised; three frames are written."""
    N, H, W = 4700, 480, 640
    try:
        image, depth, labels = ctx.empty((N, H, W, 3), np.uint8), ctx.empty((N, H, W), np.uint16), ctx.empty((N, H, W), np.uint8)
    except RuntimeError as e:
        pytest.skip("the device refused the 8.7 GB of the three arrays: %s" % e)
    assert image.nbytes > 2 ** 32
    index = np.array([4699, 0, 2400], np.int32)
    rng = np.random.default_rng(64)
    bgr = rng.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    d16 = rng.integers(0, 65536, (3, H, W)).astype(np.uint16)
    lab = rng.integers(0, 3, (3, H, W)).astype(np.uint8)
    for j, f in enumerate(index):
        image[int(f)].copyfrom(bgr[j])
        depth[int(f)].copyfrom(d16[j])
        labels[int(f)].copyfrom(lab[j])
    fi, mask_idx = i32(ctx, index), np.array([1, 2, 1], np.int32)
    status(ctx)
    out = ctx.empty((3, 3, H, W))
    lib.deepim_ingest_bgr8_frames(ctx.handle, out, image, fi, N, MEANS, 3, H, W)
    np.testing.assert_array_equal(out.asnumpy(), formula(bgr, MEANS))
    out = ctx.empty((3, 1, H, W))
    lib.deepim_ingest_depth16_frames(ctx.handle, out, depth, labels, fi, i32(ctx, mask_idx), ctypes.c_float(1000.0), N, 3, H, W)
    want = np.where(lab == mask_idx[:, None, None], d16.astype(np.float32) / np.float32(1000.0), np.float32(0))
    np.testing.assert_array_equal(out.asnumpy()[:, 0], want)
    lib.deepim_ingest_label_mask_frames(ctx.handle, out, labels, fi, i32(ctx, mask_idx), N, 3, H, W)
    np.testing.assert_array_equal(out.asnumpy()[:, 0], (lab == mask_idx[:, None, None]).astype(np.float32))
    rows = ctx.empty((3, H, W, 3), np.uint8)
    lib.deepim_gather_rows(ctx.handle, rows, image, fi, N, H * W * 3 // 4, 3)
    np.testing.assert_array_equal(rows.asnumpy(), bgr)
    assert status(ctx) == 0


# ----------------------------------------------------------------------------------------------------- the training loader --
@pytest.fixture(scope="module")
def syn(ctx):
    return SyntheticObserved(tso._machine(ctx), tso._stats(), tl.K_SMALL, tso.SYN_SEED, border=tso.oemu.SCENARIO_BORDER)


@pytest.fixture(scope="module")
def pool(ctx):
    return BackgroundPool(ctx, [bemu.background_image(bh, bw) for bh, bw in bemu.SMALL_BACKGROUNDS] + [bemu.background_image(tl.H, tl.W)],
                          tl.H, tl.W)


def _pair_of_loaders(ctx, world, cfg=None, shuffle=True, **kw):
    """(the host-set loader, the loader over a resident set built from the same dict) with the same arguments"""
    cfg0, rm, observed, points = world
    res = ResidentObserved(observed, ctx, spare_rows=tl.BS, points=points)
    assert res.M == tl.M and res.nbytes == ResidentObserved.nbytes_of(observed, spare_rows=tl.BS)
    args = dict(batch_size=tl.BS, seed=tl.SEED, num_rendered_per_observed=tl.R, points=points, noise=tl.NOISE, shuffle=shuffle)
    args.update(kw)
    return L.TrainDataLoader(observed, cfg or cfg0, rm, **args), L.TrainDataLoader(res, cfg or cfg0, rm, **args)


def _assert_two_equal_epochs(host, resident):
    np.testing.assert_array_equal(host.pairs, resident.pairs)
    want, got = tl._epochs(host, 2), tl._epochs(resident, 2)
    n = 0
    for e in range(2):
        assert len(got[e]) == len(want[e]) > 0
        for (d0, l0), (d1, l1) in zip(want[e], got[e]):
            tl._same(d1, d0)
            tl._same(l1, l0)
            n += 1
    assert host.stats() == resident.stats() and host.stats()["pairs"] == n * tl.BS
    return got


def _mask_inputs():
    cfg = tl._config()
    cfg.network.MASK_INPUTS = True
    return cfg


@pytest.mark.parametrize("cfg", [None, tl._config(mask_dilate=True), _mask_inputs()], ids=["plain", "mask_dilate", "depth_mask_inputs"])
def test_training_batches_equal_the_host_loader(ctx, world, cfg):
    assert (cfg or world[0]).network.INPUT_DEPTH
    _assert_two_equal_epochs(*_pair_of_loaders(ctx, world, cfg))


def test_training_batches_with_backgrounds_equal_the_host_loader(ctx, world, pool):
    cfg = tl._config()
    cfg.TRAIN.REPLACE_OBSERVED_BG_RATIO = 0.5
    flags = np.array([True, False, False, True, False])
    host, resident = _pair_of_loaders(ctx, world, cfg, backgrounds=pool, data_syn=flags)
    got = _assert_two_equal_epochs(host, resident)
    plain = tl._epochs(_pair_of_loaders(ctx, world, cfg)[1], 1)
    assert any(not np.array_equal(d["image_observed"], p["image_observed"]) for (d, _l), (p, _pl) in zip(got[0], plain[0]))


@pytest.mark.parametrize("shuffle", [False, True])
def test_training_batches_with_synthetic_pairs_equal_the_host_loader(ctx, world, syn, pool, shuffle):
    S = 5                      # 15 real + 5 synthetic pairs in batches of 4; in order: batch 3 mixes them, batch 4 is all synthetic
    kw = dict(synthetic=syn, num_synthetic=S, synthetic_classes=[0, 1])
    host, resident = _pair_of_loaders(ctx, world, shuffle=shuffle, **kw)
    is_syn = (resident.pairs >= tl.M * tl.R).sum(1)
    if not shuffle:
        assert is_syn.tolist() == [0, 0, 0, 1, 4]
    got = _assert_two_equal_epochs(host, resident)
    assert all(np.count_nonzero(d["depth_gt_observed"][b]) > 0 for d, _l in got[0] for b in range(tl.BS))
    with pytest.raises(ValueError, match="claimed"):           # the spare rows belong to `resident` for as long as it lives
        L.TrainDataLoader(resident.resident, world[0], world[1], batch_size=tl.BS, seed=tl.SEED, num_rendered_per_observed=tl.R,
                          points=world[3], noise=tl.NOISE, **kw)
    with pytest.raises(ValueError, match="spare"):
        L.TrainDataLoader(ResidentObserved(world[2], ctx, spare_rows=tl.BS - 1), world[0], world[1], batch_size=tl.BS, seed=tl.SEED,
                          num_rendered_per_observed=tl.R, points=world[3], noise=tl.NOISE, **kw)
    # with a pool: the synthetic rows always take a background, the flags come from the resident table
    cfg = tl._config()
    cfg.TRAIN.REPLACE_OBSERVED_BG_RATIO = 0.5
    del host, resident
    _assert_two_equal_epochs(*_pair_of_loaders(ctx, world, cfg, shuffle=shuffle, backgrounds=pool, **kw))


def test_a_resident_batch_uploads_ids_alone(ctx, world, syn, pool, monkeypatch):
    """frame_index (4 B), the draw ids (8 B) and, with synthetic pairs, their positions (4 B each): at most 16 B per pair, plus
    the synthetic class ids. Nothing is read back."""
    cfg = tl._config(mask_dilate=True)
    cfg.TRAIN.REPLACE_OBSERVED_BG_RATIO = 0.5
    _host, loader = _pair_of_loaders(ctx, world, cfg, shuffle=False, backgrounds=pool, synthetic=syn, num_synthetic=5,
                                     synthetic_classes=[0, 1])
    ups, reads = [], []
    real_array, real_copyfrom, real_asnumpy = Context.array, DeviceArray.copyfrom, DeviceArray.asnumpy

    def array(self, host, dtype=np.float32):
        a = real_array(self, host, dtype)
        ups.append(a.nbytes)
        return a

    def copyfrom(self, src):
        if not isinstance(src, DeviceArray):
            ups.append(self.nbytes)
        return real_copyfrom(self, src)

    monkeypatch.setattr(Context, "array", array)
    monkeypatch.setattr(DeviceArray, "copyfrom", copyfrom)
    monkeypatch.setattr(DeviceArray, "asnumpy", lambda self: (reads.append(self.nbytes), real_asnumpy(self))[1])
    per_batch = []
    for pairs, ids in zip(loader.pairs, loader.draw_ids):
        del ups[:]
        loader.make_batch(pairs, ids)
        per_batch.append(sum(ups))
    monkeypatch.undo()
    n_syn = (loader.pairs >= tl.M * tl.R).sum(1)
    assert n_syn.tolist() == [0, 0, 0, 1, 4] and reads == []
    for up, s in zip(per_batch, n_syn):
        assert 12 * tl.BS <= up <= 16 * tl.BS + 4 * s, (per_batch, n_syn)


# --------------------------------------------------------------------------------------------------------- the test loader --
frames_world = ttl.world         # the test-loader tests' module fixture


@pytest.mark.parametrize("shared", [True, False])
def test_test_loader_over_a_resident_set_equals_the_host_loader(ctx, frames_world, shared):
    rm, observed, pairdb = frames_world
    cfg = ttl._config(INIT_MASK="mask_gt_observed", MASK_DILATE=True)
    cfg.network.INPUT_DEPTH = True
    observed = dict(observed, depth_observed=observed["depth_gt_observed"][::-1].copy())
    res = ResidentObserved(observed, ctx)
    host = L.TestDataLoader(observed, pairdb, cfg, rm, batch_size=ttl.B, seed=ttl.SEED, shared_frames=shared)
    resident = L.TestDataLoader(res, pairdb, cfg, rm, batch_size=ttl.B, seed=ttl.SEED, shared_frames=shared)
    assert len(resident) == len(host) == 3 and resident.getpad() == host.getpad() == 1 and resident.keys == host.keys
    for (d0, f0, r0), (d1, f1, r1) in zip(host, resident):
        assert set(d0) == set(d1) and [bool(r.get("pad")) for r in r0] == [bool(r.get("pad")) for r in r1]
        assert ("frame_index" in f1) == shared
        for k in sorted(d0):
            if k == "observed_frames":           # the frames themselves: the resident arrays, named through frame_index
                assert shared and d1[k].image is res.arrays["image_observed"] and f1["image_observed"] is res.arrays["image_observed"]
                assert d1[k].n_frames == ttl.F and f1["depth_observed"] is res.arrays["depth_observed"]
                np.testing.assert_array_equal(d1[k].image.asnumpy()[f1["frame_index"].asnumpy()],
                                              d0[k].image.asnumpy()[f0["frame_index"].asnumpy()])
                continue
            a, b = d0[k].asnumpy(), d1[k].asnumpy()
            assert a.dtype == b.dtype and a.shape == b.shape, k
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=k)
        if not shared:
            for k in resident.keys:
                np.testing.assert_array_equal(f1[k].asnumpy(), f0[k].asnumpy(), err_msg=k)


def test_per_pair_rows_need_whole_words(ctx):
    H, W = 5, 7
    cfg = default_config()
    cfg.SCALES = [(H, W)]
    observed = {"image_observed": np.zeros((2, H, W, 3), np.uint8), "mask_gt_observed": np.zeros((2, H, W), np.uint8),
                "depth_gt_observed": np.zeros((2, H, W), np.uint16)}

    class Machine(object):
        classes, height, width = ["a"], H, W
    Machine.ctx = ctx
    pose = np.concatenate([np.eye(3), [[0.0], [0.0], [0.6]]], 1).astype(np.float32)
    pairdb = [{"frame": 1, "gt_class": "a", "mask_idx": 1, "pose_observed": pose, "pose_rendered": pose}]
    res = ResidentObserved(observed, ctx)
    assert L.TestDataLoader(res, pairdb, cfg, Machine(), shared_frames=True).F == 2
    with pytest.raises(ValueError, match="multiple of 4 bytes"):
        L.TestDataLoader(res, pairdb, cfg, Machine(), shared_frames=False)


# ----------------------------------------------------------------------------------------------- pred_eval and fit, full size --
def _same_containers(a, b, path=""):
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same_containers(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_containers(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray) and a.dtype == object:
        assert b.dtype == object and a.shape == b.shape, path
        _same_containers(a.tolist(), b.tolist(), path)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, path
        np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8), err_msg=path)
    else:
        assert a == b or (a != a and b != b), path


def test_pred_eval_over_a_resident_set_equals_the_host_loader(ctx, small_batch, tmp_path):
    d = small_batch
    cfg = default_config()
    cfg.network.PIXEL_MEANS = tt.MEANS_BGR.astype(np.float32)
    cfg.TEST.test_iter, cfg.TEST.FAST_TEST = 2, False
    cfg.dataset.class_name = list(tt.CLASSES)
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=20)
    params["trans_weight"] = params["trans_weight"] * np.float32(0.02)
    params["trans_bias"] = params["trans_bias"] * np.float32(0.02)
    net.bind(ctx, 2, params)
    meshes = {}
    for i, c in enumerate(tt.CLASSES):
        m = synthetic.ellipsoid_mesh(np.array([0.05, 0.04, 0.035]) * (1.0 + 0.2 * i), 12, 24)
        m.pop("uv")
        meshes[c] = m
    rm = Render_Py("unused", tt.CLASSES, cfg.dataset.INTRINSIC_MATRIX, ttl.FW, ttl.FH, meshes=meshes, ctx=ctx,
                   pixel_means=tt.MEANS_BGR[::-1].astype(np.float32))
    points = {c: meshes[c]["vertices"][::7] for c in tt.CLASSES}
    diameters = {c: 0.1 + 0.02 * i for i, c in enumerate(tt.CLASSES)}
    dep = d["depth_gt_observed"][:, 0]
    observed = {"image_observed": tt.to_bgr8(d["image_observed"]), "depth_gt_observed": np.rint(dep * 1000).astype(np.uint16),
                "mask_gt_observed": ((dep > 0) * 3).astype(np.uint8)}
    third = d["src_pose"][0][1].copy()
    third[:, 3] += np.array([0.004, -0.003, 0.01], np.float32)
    initial = [d["src_pose"][0][0].copy(), d["src_pose"][0][1].copy(), third]
    pairdb = [{"frame": f, "gt_class": c, "mask_idx": 3, "pose_observed": d["pose_tgt"][f].copy(), "pose_rendered": p}
              for f, c, p in zip([0, 1, 1], ["ape", "cat", "cat"], initial)]

    def run(test_data, name):
        log = tt.ListLogger()
        imdb = LM6D_REFINE(tt.CLASSES, points, diameters, ctx=ctx, logger=log, name=name, result_path=str(tmp_path / name))
        return tester.pred_eval(cfg, tester.Predictor(cfg, net), test_data, imdb, logger=log, render_machine=rm)

    want = run(L.TestDataLoader(observed, pairdb, cfg, rm, batch_size=2), "host")
    res = ResidentObserved(observed, ctx)
    got = run(L.TestDataLoader(res, pairdb, cfg, rm, batch_size=2), "resident")
    assert [len(got["all_poses_est"][c][0]) for c in (0, 1)] == [1, 2] and got["num_inst"].tolist() == [1, 2, 3]
    assert got["epe"]["num_all"] == 3 * ttl.FH * ttl.FW
    for c, n in ((0, 1), (1, 2)):
        for it in range(2):
            for k in range(n):
                a, b = got["all_poses_est"][c][it][k], want["all_poses_est"][c][it][k]
                assert np.isfinite(a).all()
                np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg="class %d iter %d pair %d" % (c, it, k))
    _same_containers(got, want)


def test_fit_over_a_resident_loader_equals_fit_over_the_host_loader_at_full_size(ctx):
    """fc6 fixes 480x640: B = 1, M = 2, TRAIN_ITER_SIZE = 1, one epoch of two batches."""
    cfg, net, params, _batches, upd = tf._world(ctx, False, iters=1, n_batches=1)
    rm = upd.render_machine
    rng = np.random.default_rng(5)
    poses = np.stack([synthetic.sample_pose_pair(rng)[0] for _ in range(2)])
    observed = tl._observed_from_renders(ctx, rm, poses, np.zeros(2, np.int32))
    points = {0: (synthetic.sample_model_points(rng, [0.05, 0.04, 0.035], 3000), np.ones((3, 3000), np.float32))}

    def fit(obs, name):
        net.bind_train(ctx, 1, params, num_points=3000)
        loader = L.TrainDataLoader(obs, cfg, rm, batch_size=1, seed=9, points=points)
        MutableModule(cfg, net, logger=tf._logger(name, [])).fit(
            loader, eval_metric=tf._metrics(cfg), optimizer_params={"learning_rate": tf.LR, "momentum": cfg.TRAIN.momentum, "wd": cfg.TRAIN.wd},
            begin_epoch=0, num_epoch=1, prefix="unused", updater=upd)
        assert loader.epoch == 1 and loader.stats()["pairs"] == 2
        return tf._state(net)

    after_host = fit(observed, "test_gpu_resident.fit.host")
    after_resident = fit(ResidentObserved(observed, ctx, points=points), "test_gpu_resident.fit.resident")
    tf._assert_same_bytes(after_host, after_resident)
    assert [k for k, v in params.items() if not np.array_equal(np.asarray(v, np.float32), after_resident["w:" + k])]      # it trained
