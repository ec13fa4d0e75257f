"""The background path without a GPU: lib/utils/background.py's geometry against what the reference's own get_pair_image asked of
cv2.resize (tests/golden/background_golden.npz, made by tests/golden/make_background_golden.py) and against the independent
restatement (tests/background_emulation.py); the restated crop + resample + paste + composite against the reference's final
tensors; the pool's refusals; the emulated draws; the C ABI of the two entries."""
import ctypes
import os

import numpy as np
import pytest

import background_emulation as bemu
import ingest_emulation as iemu
from mx_deepim_amd.lib.utils import background as dbg
from mx_deepim_amd.runtime import parse_header

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "background_golden.npz")
CASES = [(H, W, entry) for H, W in bemu.GOLDEN_FRAMES for entry in bemu.GOLDEN_BACKGROUNDS]


def tag_of(H, W, entry):
    return "f%dx%d_bg%s" % (H, W, entry if entry == "frame" else "%dx%d" % entry)


def checksum(im):
    return np.int64((im.astype(np.int64).reshape(-1) * (np.arange(im.size, dtype=np.int64) % 251 + 1)).sum())


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def reference_tensor(gold, tag):
    """the reference's float64 image_observed (1,3,H,W): the file holds tensor + mean as uint8, checked at its making to give the
    tensor back bit for bit"""
    return gold[tag + "_ref_image_observed_u8"] - gold["pixel_means"][::-1].reshape(1, 3, 1, 1)


@pytest.mark.parametrize("H,W,entry", CASES)
def test_crop_and_scale_are_what_the_reference_hands_to_cv2(gold, H, W, entry):
    bh, bw = bemu.background_shape(entry, H, W)
    tag = tag_of(H, W, entry)
    want_crop, want_scale = tuple(int(v) for v in gold[tag + "_crop"]), float(gold[tag + "_scale"])
    for mod in (dbg, bemu):
        ch, cw = mod.crop_size(bh, bw, H, W)
        assert (ch, cw) == want_crop
        s, oh, ow = mod.resized_size(ch, cw, H, W)
        assert s == want_scale                                              # the same float64, not a close one
        assert (oh, ow) == bemu.resample(np.zeros((ch, cw, 3), np.uint8), s).shape[:2] and oh <= H and ow <= W


def test_the_golden_cases_reach_every_branch_and_both_kinds_of_strip(gold):
    seen, strips, scales = set(), set(), set()
    for H, W, entry in CASES:
        bh, bw = bemu.background_shape(entry, H, W)
        ch, cw = dbg.crop_size(bh, bw, H, W)
        same = (H / W < 1) == (bh / bw < 1)
        seen.add((same, bh >= bw, (ch, cw) != (bh, bw)))
        s, oh, ow = dbg.resized_size(ch, cw, H, W)
        strips.update({"below"} if oh < H else set(), {"right"} if ow < W else set())
        scales.add("up" if s > 1 else "down" if s < 1 else "one")
    # image.py:122-133 (same orientation: tall or wide, cropped or whole) and :135-141 (the other orientation: always cropped)
    assert {(True, True, True), (True, True, False), (True, False, True), (True, False, False), (False, True, True),
            (False, False, True)} <= seen
    assert strips == {"below", "right"} and scales == {"up", "down", "one"}
    assert dbg.resized_size(*dbg.crop_size(20, 90, 48, 64), 48, 64)[1:] == (47, 64)
    assert dbg.resized_size(*dbg.crop_size(442, 500, 48, 64), 48, 64)[1:] == (48, 54)


@pytest.mark.parametrize("H,W,entry", CASES)
def test_the_restated_background_reproduces_the_reference_run(gold, H, W, entry):
    bh, bw = bemu.background_shape(entry, H, W)
    tag, key = tag_of(H, W, entry), "f%dx%d_" % (H, W)
    bg = bemu.background_image(bh, bw)
    assert checksum(bg) == gold[tag + "_bg_checksum"], "the seeded background is no longer the image the golden file was made of"
    frame, labels = gold[key + "image_observed"][None], gold[key + "mask_gt_observed"][None]
    means_rgb = gold["pixel_means"][::-1]
    got = bemu.ingest_pool(frame, labels, None, [0], [bg], means_rgb)
    ref = reference_tensor(gold, tag)
    assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - ref).max() <= 2.0 ** -15
    # the integers themselves, exactly
    np.testing.assert_array_equal(iemu.composite(frame, bemu.background_frames([bg], [0], H, W), labels)[0][..., ::-1].transpose(2, 0, 1),
                                  gold[tag + "_ref_image_observed_u8"][0])
    assert np.count_nonzero(labels) and not np.array_equal(got, iemu.transform_f32(frame, means_rgb))


def test_resize_table_hand_values():
    assert dbg.resize_table(4, 2, 2.0).tolist() == [[0, 1, 2048, 0], [0, 1, 1536, 512], [0, 1, 512, 1536], [1, 1, 2048, 0]]
    assert bemu.resize_table(4, 2, 2.0) == [(0, 1, 2048, 0), (0, 1, 1536, 512), (0, 1, 512, 1536), (1, 1, 2048, 0)]
    one = dbg.resize_table(9, 9, 1.0)
    assert one[:, 0].tolist() == list(range(9)) and (one[:, 2] == 2048).all() and (one[:, 3] == 0).all()
    rng = np.random.default_rng(3)
    im = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    np.testing.assert_array_equal(bemu.resample(im, 1.0), im)                       # scale 1 is the identity
    assert (bemu.resample(np.full((5, 6, 3), 255, np.uint8), 2.6) == 255).all()     # a constant 255 image stays 255
    assert (bemu.resample(np.full((50, 60, 3), 255, np.uint8), 0.37) == 255).all()


@pytest.mark.parametrize("H,W", bemu.GOLDEN_FRAMES + ((9, 13), (480, 640)))
def test_resize_table_against_the_emulation(H, W):
    sizes = [bemu.background_shape(e, H, W) for e in bemu.GOLDEN_BACKGROUNDS] + [(1, 1), (2, 3), (3, 2), (281, 500), (500, 334)]
    for bh, bw in sizes:
        ch, cw = dbg.crop_size(bh, bw, H, W)
        s, oh, ow = dbg.resized_size(ch, cw, H, W)
        for n_out, n_src in ((ow, cw), (oh, ch)):
            t = dbg.resize_table(n_out, n_src, s)
            assert t.dtype == np.int32 and t.shape == (n_out, 4)
            assert [tuple(r) for r in t.tolist()] == bemu.resize_table(n_out, n_src, s), (bh, bw, n_out, n_src)
            assert (t[:, 2] + t[:, 3] == 2048).all() and (t[:, 2:] >= 0).all()
            assert (t[:, :2] >= 0).all() and (t[:, :2] < n_src).all()                # nothing outside the crop is ever read
            assert ((t[:, 1] == t[:, 0] + 1) | ((t[:, 1] == t[:, 0]) & (t[:, 3] == 0))).all()
            # the packed word the kernel reads gives the four numbers back
            w = dbg.pack_table(t).astype(np.int64)
            assert w.dtype == np.int64 and dbg.pack_table(t).dtype == np.uint32
            back = np.stack([w >> 13, (w >> 13) + ((w >> 12) & 1), 2048 - (w & 0xfff), w & 0xfff], 1)
            np.testing.assert_array_equal(back, t)
    with pytest.raises(ValueError, match="not a resize_table"):
        dbg.pack_table([(0, 2, 2048, 0)])
    with pytest.raises(ValueError, match="not a resize_table"):
        dbg.pack_table([(0, 1, 2047, 0)])


def test_pool_refusals(monkeypatch):
    """every refusal comes before anything is uploaded: no device needed (ctx = None)"""
    with pytest.raises(ValueError, match="no images"):
        dbg.BackgroundPool(None, [], 48, 64)
    with pytest.raises(ValueError, match="uint8"):
        dbg.BackgroundPool(None, [np.zeros((20, 30, 3), np.float32)], 48, 64)
    with pytest.raises(ValueError, match="uint8"):
        dbg.BackgroundPool(None, [np.zeros((20, 30), np.uint8)], 48, 64)
    # the crop rule keeps a crop in the frame's orientation, so no image of the sizes searched reaches the reference's
    # broadcast error; a crop in the other orientation (here forced) does, and is refused
    assert dbg.resized_size(64, 48, 48, 64)[1:] == (64, 48)
    monkeypatch.setattr(dbg, "crop_size", lambda bh, bw, H, W: (min(bh, 64), min(bw, 48)))
    with pytest.raises(ValueError, match="larger than the 48x64 frame"):
        dbg.BackgroundPool(None, [np.zeros((64, 48, 3), np.uint8)], 48, 64)


def test_emulated_draws():
    ids = np.arange(4096, dtype=np.uint64) + np.uint64(1 << 33)
    for P in (1, 3, 64, 1000):
        use, idx, u = bemu.draws(11, ids, 0.25, P)
        assert idx.min() >= 0 and idx.max() < P
        assert P > 64 or set(idx.tolist()) == set(range(P))                   # 4096 draws reach each of up to 64 images
        assert 0.0 < u.min() and u.max() < 1.0
        assert abs(use.mean() - 0.25) < 0.03                                  # 4096 draws: sigma = 0.0068
    assert bemu.draws(11, ids, 0.0, 5)[0].sum() == 0 and bemu.draws(11, ids, 1.0, 5)[0].sum() == len(ids)
    always = (np.arange(len(ids)) % 3 == 0)
    use = bemu.draws(11, ids, 0.0, 5, always)[0]
    np.testing.assert_array_equal(use, always.astype(np.int32))               # data_syn alone decides at ratio 0
    use_q = bemu.draws(11, ids, 0.25, 5, always)[0]
    np.testing.assert_array_equal(use_q, np.maximum(always.astype(np.int32), bemu.draws(11, ids, 0.25, 5)[0]))
    # the index does not depend on ratio or always; another stream, seed or id gives other draws
    np.testing.assert_array_equal(bemu.draws(11, ids, 0.0, 64, always)[1], bemu.draws(11, ids, 1.0, 64)[1])
    base = bemu.draws(11, ids, 0.5, 64)
    for other in (bemu.draws(11, ids, 0.5, 64, stream=2), bemu.draws(12, ids, 0.5, 64), bemu.draws(11, ids + np.uint64(1), 0.5, 64)):
        assert not np.array_equal(other[1], base[1]) and not np.array_equal(other[0], base[0])


def test_prototypes_parse_from_the_header():
    p = parse_header()
    vp, ci, cd, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
    assert p["deepim_ingest_bgr8_pool"] == (ci, [vp] * 10 + [ci, vp] + [ci] * 3,
                                            ["ctx", "out", "frames", "fg_labels", "use_bg", "bg_index", "pool_pixels", "pool_desc",
                                             "xtab", "ytab", "P", "means_rgb", "B", "H", "W"])
    assert p["deepim_sample_backgrounds"] == (ci, [vp] * 4 + [cd, ci, cu, cu, vp, ci],
                                              ["ctx", "use_bg", "bg_index", "always", "ratio", "pool_size", "seed", "draw_base",
                                               "draw_ids", "B"])
