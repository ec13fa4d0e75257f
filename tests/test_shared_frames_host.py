"""Shared-frame batches without a GPU: the restated gather (tests/shared_frames_emulation.py) against the reference-run fixture
tests/golden/ingest_golden.npz, the host range check of frame_index, and the C ABI of the four frame-indexed entries."""
import ctypes
import os

import numpy as np
import pytest

import ingest_emulation as emu
import shared_frames_emulation as semu
from mx_deepim_amd.config import default_config
from mx_deepim_amd.lib.pair_matching import data_pair
from mx_deepim_amd.lib.utils import image as dimage
from mx_deepim_amd.runtime import Context, parse_header

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest_golden.npz")
YAML_MEANS = np.array([123.68, 116.779, 103.939])
FRAME_KEYS = ("image_observed", "image_rendered", "mask_idx", "depth_observed", "depth_gt_observed", "depth_rendered",
              "mask_gt_observed", "mask_observed", "mask_observed_est", "pose_rendered")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def frames_of(gold, tag):
    return {k: gold["%s_%s" % (tag, k)] for k in FRAME_KEYS}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_identity_index_reproduces_the_reference_run(gold, tag):
    """N = B with frame_index = 0 … B-1 is the per-pair batch: the gather through the existing restatements gives the fixture"""
    f = frames_of(gold, tag)
    B = f["mask_idx"].shape[0]
    ident = np.arange(B, dtype=np.int32)
    got = semu.transform_f32(f["image_observed"], ident, YAML_MEANS[::-1])
    assert got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - gold[tag + "_ref_transform"]).max() <= 2.0 ** -15        # bound: tests/test_ingest_host.py
    for key in ("depth_observed", "depth_gt_observed"):
        np.testing.assert_array_equal(semu.depth_f32(f[key], ident), gold["%s_ref_%s" % (tag, key)])
    np.testing.assert_array_equal(semu.depth_f32(f["depth_observed"], ident, 1000, f["mask_gt_observed"], f["mask_idx"]),
                                  gold[tag + "_ref_depth_observed_masked_train"])
    np.testing.assert_array_equal(semu.depth_f32(f["depth_observed"], ident, 1000, f["mask_observed_est"], f["mask_idx"]),
                                  gold[tag + "_ref_depth_observed_masked_test"])
    for init in ("mask_gt_observed", "mask_observed"):
        want = gold["%s_ref_test_%s_mask_observed" % (tag, init)]
        np.testing.assert_array_equal(semu.label_mask(f[init], ident, f["mask_idx"]).astype(np.float64), want.astype(np.float64))
    shared = dict(f, frame_index=ident)
    rep = semu.replicate(shared)
    assert "frame_index" not in rep
    for k in FRAME_KEYS:
        np.testing.assert_array_equal(rep[k], f[k])


def test_gather_follows_a_non_monotonic_index(gold):
    f = frames_of(gold, "a")
    idx = np.array([1, 0, 1, 1, 0], np.int32)
    two = {k: f[k][:2] for k in semu.SHARED_KEYS}
    rep = semu.replicate(dict(two, frame_index=idx, mask_idx=np.array([1, 1, 2, 1, 2], np.int32)))
    for k in semu.SHARED_KEYS:
        assert rep[k].shape[0] == 5
        for b, n in enumerate(idx):
            np.testing.assert_array_equal(rep[k][b], f[k][n])
    lm = semu.label_mask(two["mask_gt_observed"], idx, rep["mask_idx"])
    np.testing.assert_array_equal(lm, emu.label_mask(rep["mask_gt_observed"], rep["mask_idx"]))


def shared_batch(gold, frame_index):
    f = frames_of(gold, "a")
    B = len(frame_index)
    N, H, W = f["depth_observed"][:2].shape
    out = {k: f[k][:2] for k in semu.SHARED_KEYS}
    out.update(frame_index=frame_index, image_rendered=np.zeros((B, H, W, 3), np.uint8), depth_rendered=np.zeros((B, H, W), np.uint16),
               mask_idx=np.ones(B, np.int32), pose_rendered=np.zeros((B, 3, 4), np.float32))
    cfg = default_config()
    cfg.SCALES = [(H, W)]
    return out, cfg


@pytest.mark.parametrize("bad, pair", [([0, 1, -1, 1], 2), ([0, 2, 1, 1], 1), ([5], 0)])
def test_host_range_check_raises_before_a_context_is_needed(gold, monkeypatch, bad, pair):
    def no_device(*a, **k):
        raise AssertionError("the range check must come before any device work")
    monkeypatch.setattr(Context, "default", classmethod(no_device))
    monkeypatch.setattr(Context, "get", classmethod(no_device))
    frames, cfg = shared_batch(gold, np.array(bad, np.int32))
    with pytest.raises(ValueError, match=r"frame_index\[%d\] = %d: pair %d .* 2 shared frames" % (pair, bad[pair], pair)):
        data_pair.get_data_pair_test_batch(frames, cfg)
    with pytest.raises(ValueError, match="pair %d" % pair):
        dimage.check_frame_index(frames)
    frames["frame_index"] = list(bad)                       # a plain list is checked the same way
    with pytest.raises(ValueError, match="pair %d" % pair):
        data_pair.get_data_pair_test_batch(frames, cfg)


def test_host_checks_of_a_well_formed_and_a_malformed_batch(gold):
    frames, cfg = shared_batch(gold, np.array([1, 0, 1, 1, 0], np.int32))
    assert dimage.is_shared(frames) and dimage.check_frame_index(frames) == (5, 2)
    assert not dimage.is_shared({k: v for k, v in frames.items() if k != "frame_index"})
    frames["mask_observed"] = frames["mask_observed"][:1]                       # the shared arrays disagree on N
    with pytest.raises(ValueError, match="disagree"):
        dimage.check_frame_index(frames)
    frames, cfg = shared_batch(gold, np.array([0.0, 1.0]))
    with pytest.raises(TypeError, match="integer"):
        dimage.check_frame_index(frames)
    with pytest.raises(NotImplementedError, match="observed_frames"):
        dimage.get_pair_image(shared_batch(gold, np.array([0, 1], np.int32))[0], cfg, "test")


def test_prototypes_parse_from_the_header():
    p = parse_header()
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    front = ["ctx", "frames_bgr8", "frame_index", "N", "image_rendered", "mask_observed", "mask_rendered", "depth_frames16",
             "depth_labels", "mask_idx", "depth_factor", "depth_rendered", "src_pose", "K_host", "pixel_means_host"]
    front_t = [vp] * 3 + [ci] + [vp] * 6 + [cf] + [vp] * 4
    assert p["deepim_zoom_concat_frames_forward"] == (ci, front_t + [vp] * 2 + [ci] * 3, front + ["net_input", "zoom_factor", "B", "H", "W"])
    assert p["deepim_zoom_concat_frames_forward_h16"] == (ci, front_t + [vp] * 3 + [ci] * 3,
                                                          front + ["main8", "extra2", "zoom_factor", "B", "H", "W"])
    assert p["deepim_ingest_depth16_frames"] == (ci, [vp] * 6 + [cf] + [ci] * 4, ["ctx", "out", "depth", "labels", "frame_index",
                                                                                "mask_idx", "depth_factor", "N", "B", "H", "W"])
    assert p["deepim_ingest_label_mask_frames"] == (ci, [vp] * 5 + [ci] * 4, ["ctx", "out", "labels", "frame_index", "mask_idx", "N",
                                                                              "B", "H", "W"])
