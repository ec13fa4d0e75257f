"""The device background path on the GPU: deepim_ingest_bgr8_pool and deepim_sample_backgrounds against
tests/background_emulation.py bit for bit, get_pair_image with a bg_pool against the reference-run fixture
tests/golden/background_golden.npz, the equivalence with deepim_ingest_bgr8 fed a materialised background, the range guard of
bg_index, one full-size case, and TrainDataLoader with a pool against the chain written out by hand (the world of
tests/test_gpu_loader.py, 48x64)."""
import ctypes
import os

import numpy as np
import pytest

import background_emulation as bemu
import ingest_emulation as iemu
import pose_sampler_emulation as pemu
import test_gpu_loader as tl
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core.loader import TrainDataLoader
from mx_deepim_amd.lib.utils import image as dimage
from mx_deepim_amd.lib.utils.background import BackgroundPool, background_draws_device
from mx_deepim_amd.runtime import DeviceArray, lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "background_golden.npz")
BG_RANGE = 32                    # bit 5 of the status word
MEANS = np.array([1.5, 120.25, 7.0])
world = tl.world                 # the loader tests' module fixture, built once for this module too


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def small_images():
    return [bemu.background_image(bh, bw) for bh, bw in bemu.SMALL_BACKGROUNDS]


def u8(ctx, a):
    return ctx.array(a, dtype=np.uint8)


def i32(ctx, a):
    return ctx.array(a, dtype=np.int32)


def status(ctx):
    st = ctypes.c_int(-1)
    lib.deepim_zoom_status(ctx.handle, ctypes.byref(st))
    return st.value


def pool_ingest(ctx, pool, frames, labels, use_bg, bg_index, means=None):
    B, H, W, _ = frames.shape
    out = ctx.empty((B, 3, H, W))
    out.copyfrom(np.float32(-7.0))
    lib.deepim_ingest_bgr8_pool(ctx.handle, out, u8(ctx, frames), u8(ctx, labels), None if use_bg is None else i32(ctx, use_bg),
                                i32(ctx, bg_index), pool.pixels, pool.desc, pool.xtab, pool.ytab, len(pool),
                                None if means is None else np.ascontiguousarray(means, np.float32), B, H, W)
    return out.asnumpy()


def label_maps(rng, B, H, W):
    """random 0 / 100 / 200 maps (`!= 0`, not `== mask_idx`), then one all zero, one all non-zero, one with two objects' labels"""
    fg = (rng.integers(0, 3, (B, H, W)) * rng.integers(0, 2, (B, H, W)) * 100).astype(np.uint8)
    fg[1] = 0
    fg[2] = 3
    fg[3] = 0
    fg[3, 1:H // 2, 1:W // 2] = 2
    fg[3, H // 2:, W // 2:] = 9
    return fg


# ------------------------------------------------------------------------------------------------------------- the kernel --
@pytest.mark.parametrize("H,W", [(30, 44), (9, 13)])       # float4 stores; H·W % 4 != 0: scalar stores, odd row and sample starts
def test_pool_kernel_is_the_emulation(ctx, small_images, H, W):
    B = 5
    rng = np.random.default_rng(H * 100 + W)
    pool = BackgroundPool(ctx, small_images, H, W)
    assert len(pool) == 5 and pool.nbytes > sum(im.size for im in small_images)
    for (ch, cw, s, oh, ow), im in zip(pool.geometry, small_images):
        assert (ch, cw) == bemu.crop_size(im.shape[0], im.shape[1], H, W) and (s, oh, ow) == bemu.resized_size(ch, cw, H, W)
    if (H, W) == (30, 44):
        assert any(g[3] < H for g in pool.geometry) and any(g[4] < W for g in pool.geometry)  # black strips on either side
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    fg = label_maps(rng, B, H, W)
    idx = np.array([3, 0, 4, 1, 2], np.int32)
    for use_bg in (np.array([1, 7, 1, 1, 0], np.int32), np.array([0, 1, 0, 1, 1], np.int32), None, np.zeros(B, np.int32)):
        for means in (MEANS, None):
            want = bemu.ingest_pool(frames, fg, use_bg, idx, small_images, means)
            got = pool_ingest(ctx, pool, frames, fg, use_bg, idx, means)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # use_bg == 0 everywhere: the bits of deepim_ingest_bgr8 without a background
    plain = ctx.empty((B, 3, H, W))
    lib.deepim_ingest_bgr8(ctx.handle, plain, u8(ctx, frames), None, None, None, np.ascontiguousarray(MEANS, np.float32), B, H, W)
    np.testing.assert_array_equal(pool_ingest(ctx, pool, frames, fg, np.zeros(B, np.int32), idx, MEANS), plain.asnumpy())
    assert status(ctx) == 0
    # every image of the pool in every slot
    for shift in range(1, 5):
        k = (idx + shift) % 5
        np.testing.assert_array_equal(pool_ingest(ctx, pool, frames, fg, None, k, MEANS), bemu.ingest_pool(frames, fg, None, k, small_images, MEANS))


def test_pool_kernel_unaligned_frames(ctx, small_images):
    """frames and labels at odd addresses take the byte-load variant; the pool's windows stay aligned"""
    B, H, W = 2, 9, 13
    rng = np.random.default_rng(5)
    pool = BackgroundPool(ctx, small_images, H, W)
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    fg = (rng.integers(0, 2, (B, H, W)) * 5).astype(np.uint8)
    idx = np.array([2, 3], np.int32)
    flat_f, flat_l = u8(ctx, np.concatenate([[0], frames.reshape(-1)])), u8(ctx, np.concatenate([[0, 0, 0], fg.reshape(-1)]))
    out = ctx.empty((B, 3, H, W))
    lib.deepim_ingest_bgr8_pool(ctx.handle, out, flat_f[1:], flat_l[3:], None, i32(ctx, idx), pool.pixels, pool.desc, pool.xtab,
                                pool.ytab, len(pool), None, B, H, W)
    np.testing.assert_array_equal(out.asnumpy(), bemu.ingest_pool(frames, fg, None, idx, small_images))


@pytest.mark.parametrize("H,W", [(30, 44), (9, 13)])
def test_equivalence_with_a_materialised_background(ctx, small_images, H, W):
    B = 5
    rng = np.random.default_rng(H + W)
    pool = BackgroundPool(ctx, small_images, H, W)
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    fg = label_maps(rng, B, H, W)
    idx, use_bg = np.array([4, 3, 2, 1, 0], np.int32), np.array([1, 0, 1, 1, 1], np.int32)
    bg = bemu.background_frames(small_images, idx, H, W)
    assert bg.any()
    old = ctx.empty((B, 3, H, W))
    means = np.ascontiguousarray(MEANS, np.float32)
    lib.deepim_ingest_bgr8(ctx.handle, old, u8(ctx, frames), u8(ctx, bg), u8(ctx, fg), i32(ctx, use_bg), means, B, H, W)
    assert np.array_equal(pool_ingest(ctx, pool, frames, fg, use_bg, idx, MEANS), old.asnumpy())


def test_bg_index_out_of_range(ctx, small_images):
    B, H, W = 5, 30, 44
    rng = np.random.default_rng(8)
    pool = BackgroundPool(ctx, small_images, H, W)
    P = len(pool)
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    fg = label_maps(rng, B, H, W)
    fg[0, 0, 0] = 1                                   # the pair's first pixel keeps the frame and still reports
    good = np.array([0, 1, 2, 3, 4], np.int32)
    status(ctx)
    want_good = pool_ingest(ctx, pool, frames, fg, None, good, MEANS)
    assert status(ctx) == 0
    for bad_value in (-1, P, 2 ** 31 - 1, -2 ** 31):
        idx = good.copy()
        idx[0] = idx[3] = bad_value
        got = pool_ingest(ctx, pool, frames, fg, None, idx, MEANS)
        assert status(ctx) == BG_RANGE and status(ctx) == 0          # set, and cleared by the read
        black = iemu.transform_f32(iemu.composite(frames, np.zeros_like(frames), fg), MEANS)
        for b in range(B):
            np.testing.assert_array_equal(got[b], black[b] if b in (0, 3) else want_good[b])
        # a pair that composites nothing does not consult its index
        use = np.array([0, 1, 1, 0, 1], np.int32)
        got = pool_ingest(ctx, pool, frames, fg, use, idx, MEANS)
        assert status(ctx) == 0
        np.testing.assert_array_equal(got, bemu.ingest_pool(frames, fg, use, idx, small_images, MEANS))


def test_full_size(ctx):
    H, W, B = 480, 640, 2
    images = [bemu.background_image(375, 500), bemu.background_image(500, 375)]
    pool = BackgroundPool(ctx, images, H, W)
    assert pool.geometry[0] == (375, 500, 1.28, 480, 640) and pool.geometry[1][:2] + pool.geometry[1][3:] == (282, 375, 480, 638)
    rng = np.random.default_rng(64)
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    fg = np.zeros((B, H, W), np.uint8)
    fg[0, 100:300, 200:420] = 4
    fg[1, 5:470:3, 7:630:5] = 1
    idx = np.array([1, 0], np.int32)
    got = pool_ingest(ctx, pool, frames, fg, None, idx, MEANS)
    np.testing.assert_array_equal(got, bemu.ingest_pool(frames, fg, None, idx, images, MEANS))


# ---------------------------------------------------------------------------------------------------------- get_pair_image --
@pytest.mark.parametrize("H,W", bemu.GOLDEN_FRAMES)
def test_get_pair_image_against_the_reference_run(ctx, gold, H, W):
    key = "f%dx%d_" % (H, W)
    shapes = [bemu.background_shape(e, H, W) for e in bemu.GOLDEN_BACKGROUNDS]
    images = [bemu.background_image(bh, bw) for bh, bw in shapes]
    B = len(images)
    cfg = default_config()
    cfg.SCALES = [(H, W)]
    cfg.network.PIXEL_MEANS = gold["pixel_means"].copy()
    pool = BackgroundPool(ctx, images, H, W)
    frame, labels = gold[key + "image_observed"], gold[key + "mask_gt_observed"]
    frames = {"image_observed": np.repeat(frame[None], B, 0), "image_rendered": np.repeat(frame[None], B, 0),
              "mask_gt_observed": np.repeat(labels[None], B, 0), "bg_pool": pool, "bg_index": np.arange(B, dtype=np.int32)}
    obs, ren = dimage.get_pair_image(frames, cfg, "train")
    obs, plain = obs.asnumpy(), ren.asnumpy()
    for b, entry in enumerate(bemu.GOLDEN_BACKGROUNDS):
        tag = "f%dx%d_bg%s" % (H, W, entry if entry == "frame" else "%dx%d" % entry)
        ref = gold[tag + "_ref_image_observed_u8"] - gold["pixel_means"][::-1].reshape(1, 3, 1, 1)      # the reference's float64
        assert np.abs(obs[b:b + 1].astype(np.float64) - ref).max() <= 2.0 ** -15, tag
        assert not np.array_equal(obs[b], plain[b])
    # use_bg switches pairs off; the test phase composites nothing; bg_image and bg_pool together are refused
    use = (np.arange(B) % 2).astype(np.int32)
    some = dimage.get_pair_image(dict(frames, use_bg=use), cfg, "train")[0].asnumpy()
    for b in range(B):
        np.testing.assert_array_equal(some[b], obs[b] if use[b] else plain[b])
    np.testing.assert_array_equal(dimage.get_pair_image(frames, cfg, "test")[0].asnumpy(), plain)
    with pytest.raises(ValueError, match="both"):
        dimage.get_pair_image(dict(frames, bg_image=frames["image_observed"]), cfg, "train")
    with pytest.raises(NotImplementedError, match="frame_index"):
        dimage.get_pair_image(dict(frames, frame_index=np.zeros(B, np.int32)), cfg, "train")
    with pytest.raises(ValueError, match="built for"):
        dimage.get_pair_image(dict(frames, bg_pool=BackgroundPool(ctx, images[4:6], H + 1, W)), cfg, "train")


# ------------------------------------------------------------------------------------------------------------------- draws --
def test_draws(ctx):
    seed, P = 2 ** 40 + 17, 64
    ids = np.concatenate([np.arange(300, dtype=np.uint64), np.array([2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5], np.uint64)])
    B = len(ids)
    always = (np.arange(B) % 4 == 0).astype(np.int32)
    for ratio, alw in ((0.3, None), (0.3, always), (0.0, always), (1.0, None), (0.0, None)):
        use, idx = background_draws_device(ctx, B, seed, ids, ratio, P, always=alw)
        assert use.dtype == np.int32 and idx.dtype == np.int32 and use.shape == (B,) and idx.shape == (B,)
        want_use, want_idx, _u = bemu.draws(seed, ids, ratio, P, alw)
        np.testing.assert_array_equal(use.asnumpy(), want_use)
        np.testing.assert_array_equal(idx.asnumpy(), want_idx)
    use, idx = (a.asnumpy() for a in background_draws_device(ctx, B, seed, ids, 0.3, P))
    assert 0 < use.sum() < B and idx.min() >= 0 and idx.max() < P
    # a draw id alone and inside a batch of 7, at any position
    for pos in (0, 3, 6):
        batch = np.array([900, 901, 902, 903, 904, 905, 906], np.uint64)
        batch[pos] = ids[11]
        u7, i7 = (a.asnumpy() for a in background_draws_device(ctx, 7, seed, batch, 0.3, P))
        u1, i1 = (a.asnumpy() for a in background_draws_device(ctx, 1, seed, ids[11:12], 0.3, P))
        assert (u7[pos], i7[pos]) == (u1[0], i1[0]) == (use[11], idx[11])
    # draw_base + b without ids
    u0, i0 = (a.asnumpy() for a in background_draws_device(ctx, 300, seed, None, 0.3, P, draw_base=0))
    np.testing.assert_array_equal(u0, use[:300])
    np.testing.assert_array_equal(i0, idx[:300])
    # stream 3 is not stream 2: the device's mask-dilate draw of the same ids is the emulation's stream 2, whose words differ
    thick = ctx.empty((B, 4), np.int32)
    lib.deepim_sample_mask_dilate(ctx.handle, thick, 10, seed, 0, ctx.array(ids, dtype=np.uint64), B)
    np.testing.assert_array_equal(thick.asnumpy(), pemu.mask_dilate(seed, ids, 10)[0])
    as_stream2 = bemu.draws(seed, ids, 0.3, P, stream=2)
    assert not np.array_equal(as_stream2[1], idx) and not np.array_equal(as_stream2[0], use)
    with pytest.raises(ValueError, match="ratio"):
        background_draws_device(ctx, B, seed, ids, 1.5, P)


# ------------------------------------------------------------------------------------------------------------------ loader --
@pytest.fixture(scope="module")
def loader_pool(ctx, small_images):
    return BackgroundPool(ctx, small_images + [bemu.background_image(tl.H, tl.W)], tl.H, tl.W)


def _bg_config(ratio):
    cfg = tl._config()
    cfg.TRAIN.REPLACE_OBSERVED_BG_RATIO = ratio
    return cfg


def _hand_image_observed(ctx, world, cfg, pool, pairs, ids, ratio, data_syn=None):
    obs = world[2]
    m = np.asarray(pairs) // tl.R
    use, idx = background_draws_device(ctx, len(m), tl.SEED, np.asarray(ids, np.uint64), ratio, len(pool),
                                       always=None if data_syn is None else data_syn[m])
    out = ctx.empty((len(m), 3, tl.H, tl.W))
    lib.deepim_ingest_bgr8_pool(ctx.handle, out, u8(ctx, obs["image_observed"][m]), u8(ctx, obs["mask_gt_observed"][m]), use, idx,
                                pool.pixels, pool.desc, pool.xtab, pool.ytab, len(pool),
                                np.ascontiguousarray(dimage._means_rgb(cfg), np.float32), len(m), tl.H, tl.W)
    return out.asnumpy(), use.asnumpy()


def test_loader_without_backgrounds_is_unchanged(ctx, world):
    cfg = world[0]
    for nb, (data, label) in enumerate(tl._loader(world, backgrounds=None, data_syn=None)):
        pairs = np.arange(nb * tl.BS, (nb + 1) * tl.BS)
        want_data, want_label, _a = tl._hand_batch(ctx, world, cfg, pairs, pairs)
        tl._same(tl._host(data), tl._host(want_data))
        tl._same(tl._host(label), tl._host(want_label))


def test_loader_with_backgrounds(ctx, world, loader_pool):
    cfg = _bg_config(1.0)
    changed = 0
    for nb, ((data, label), (pdata, plabel)) in enumerate(zip(tl._loader(world, cfg=cfg, backgrounds=loader_pool), tl._loader(world))):
        pairs = np.arange(nb * tl.BS, (nb + 1) * tl.BS)
        want, use = _hand_image_observed(ctx, world, cfg, loader_pool, pairs, pairs, 1.0)
        assert use.all()
        data, pdata = tl._host(data), tl._host(pdata)
        np.testing.assert_array_equal(data["image_observed"], want)
        changed += int(np.count_nonzero(data["image_observed"] != pdata["image_observed"]))
        # the object's own pixels and every other tensor are what they were
        m = pairs // tl.R
        on = np.repeat((world[2]["mask_gt_observed"][m] != 0)[:, None], 3, 1)
        np.testing.assert_array_equal(data["image_observed"][on], pdata["image_observed"][on])
        tl._same({k: v for k, v in data.items() if k != "image_observed"}, {k: v for k, v in pdata.items() if k != "image_observed"})
        tl._same(tl._host(label), tl._host(plabel))
    assert changed > 0


def test_loader_backgrounds_depend_on_seed_epoch_and_pair_only(ctx, world, loader_pool):
    cfg = _bg_config(0.5)
    full = tl._loader(world, cfg=cfg, backgrounds=loader_pool, batch_size=1)
    by_pair = [np.concatenate([d["image_observed"].asnumpy() for d, _l in full])]
    full.reset()
    by_pair.append(np.concatenate([d["image_observed"].asnumpy() for d, _l in full]))
    assert not np.array_equal(by_pair[0], by_pair[1])                          # fresh backgrounds every epoch
    shuffled = tl._loader(world, cfg=cfg, backgrounds=loader_pool, shuffle=True)
    for e in range(2):
        order = shuffled.pairs.reshape(-1)
        assert sorted(order.tolist()) != order.tolist()
        got = np.concatenate([d["image_observed"].asnumpy() for d, _l in shuffled])
        np.testing.assert_array_equal(got.view(np.uint32), by_pair[e][order].view(np.uint32))
        shuffled.reset()
    other = tl._loader(world, cfg=cfg, backgrounds=loader_pool, batch_size=1, seed=tl.SEED + 1)
    assert not np.array_equal(np.concatenate([d["image_observed"].asnumpy() for d, _l in other]), by_pair[0])


def test_loader_data_syn_replaces_exactly_the_flagged_frames(ctx, world, loader_pool):
    cfg = _bg_config(0.0)
    syn = np.array([True, False, False, True, False])
    loader = tl._loader(world, cfg=cfg, backgrounds=loader_pool, data_syn=syn)
    for nb, ((data, _l), (pdata, _pl)) in enumerate(zip(loader, tl._loader(world))):
        pairs = np.arange(nb * tl.BS, (nb + 1) * tl.BS)
        want, use = _hand_image_observed(ctx, world, cfg, loader_pool, pairs, pairs, 0.0, syn)
        np.testing.assert_array_equal(use, syn[pairs // tl.R].astype(np.int32))
        got, plain = data["image_observed"].asnumpy(), pdata["image_observed"].asnumpy()
        np.testing.assert_array_equal(got, want)
        for b, p in enumerate(pairs):
            assert np.array_equal(got[b], plain[b]) == (not syn[p // tl.R]), p
    # without flags and at ratio 0 nothing is replaced
    for (data, _l), (pdata, _pl) in zip(tl._loader(world, cfg=cfg, backgrounds=loader_pool), tl._loader(world)):
        np.testing.assert_array_equal(data["image_observed"].asnumpy(), pdata["image_observed"].asnumpy())


def test_loader_reads_nothing_back_with_backgrounds(ctx, world, loader_pool, monkeypatch):
    cfg = tl._config(mask_dilate=True)
    cfg.TRAIN.REPLACE_OBSERVED_BG_RATIO = 0.5
    loader = tl._loader(world, cfg=cfg, backgrounds=loader_pool, data_syn=np.array([1, 0, 0, 0, 1], bool))
    reads = []
    real = DeviceArray.asnumpy
    monkeypatch.setattr(DeviceArray, "asnumpy", lambda self: (reads.append(self.nbytes), real(self))[1])
    n = sum(1 for _ in loader)
    loader.reset()
    n += sum(1 for _ in loader)
    assert n == 6 and reads == []
    assert set(loader.stats()) == {"pairs", "attempts", "exhausted"} and reads == [24]
    monkeypatch.undo()
    assert status(ctx) & BG_RANGE == 0


def test_loader_refuses_a_pool_of_another_size(ctx, world, small_images):
    cfg, rm, observed, points = world
    with pytest.raises(ValueError, match="built for"):
        TrainDataLoader(observed, cfg, rm, points=points, backgrounds=BackgroundPool(ctx, small_images, tl.H, tl.W + 4))
    with pytest.raises(NotImplementedError, match="bg_image"):
        TrainDataLoader(dict(observed, bg_image=observed["image_observed"]), cfg, rm, points=points,
                        backgrounds=BackgroundPool(ctx, small_images, tl.H, tl.W))
