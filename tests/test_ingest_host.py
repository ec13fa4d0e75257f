"""Frame ingest without a GPU: the numpy restatement (tests/ingest_emulation.py) against the outputs of the reference's own files
(tests/golden/ingest_golden.npz, made by tests/golden/make_ingest_golden.py), bit for bit; mask_dilate_draws against the
reference's use of the generator; the C ABI of the four kernels."""
import ctypes
import os

import numpy as np
import pytest

import ingest_emulation as emu
from mx_deepim_amd.lib.utils.mask_dilate import mask_dilate_draws
from mx_deepim_amd.runtime import parse_header

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest_golden.npz")
YAML_MEANS = np.array([123.68, 116.779, 103.939])
NEXT_DRAW_RANGE = 2 ** 31 - 1
TEST_INIT_MASKS = ("mask_gt_observed", "mask_observed", "box_gt_observed", "box_", "box_rendered")
FRAME_KEYS = ("image_observed", "image_rendered", "bg_image", "mask_idx", "use_bg", "depth_observed", "depth_gt_observed",
              "depth_rendered", "mask_gt_observed", "mask_observed", "mask_observed_est", "pose_rendered")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def frames_of(gold, tag):
    return {k: gold["%s_%s" % (tag, k)] for k in FRAME_KEYS}


def same(got, want):
    """bit for bit, the dtype aside (the reference's masks and images are float64 holding float32-exact values where compared)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.astype(np.float64), want.astype(np.float64))


def test_fixture_seeds_cover_every_direction_and_both_thickness_extremes(gold):
    seen, thick = set(), set()
    for s in gold["dilate_seeds"]:
        np.random.seed(int(s))
        seen.add(int(np.random.randint(10)))
        thick.update(mask_dilate_draws(1, rng=np.random.RandomState(int(s))).reshape(-1).tolist())
    assert seen == set(range(10))
    assert {0, 1, 10} <= thick


@pytest.mark.parametrize("m", [0, 1, 2])
def test_draws_and_restated_dilation_reproduce_the_reference(gold, m):
    """per fixture seed: mask_dilate_draws leaves np.random where the reference's call left it, and the restated shifted ORs with
    those draws give the reference's output"""
    mask = gold["dilate_mask%d" % m]
    for i, s in enumerate(gold["dilate_seeds"]):
        np.random.seed(int(s))
        draws = mask_dilate_draws(1)
        assert np.random.randint(NEXT_DRAW_RANGE) == gold["dilate_next%d" % m][i], "seed %d" % s
        assert draws.dtype == np.int32 and draws.shape == (1, 4)
        got = emu.mask_dilate(mask, draws[0])
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, gold["dilate_out%d" % m][i], err_msg="seed %d draws %s" % (s, draws))


def test_draws_for_a_batch_and_a_private_generator():
    """n samples = n successive calls; a RandomState of its own leaves np.random alone"""
    np.random.seed(99)
    one_by_one = np.concatenate([mask_dilate_draws(1) for _ in range(6)])
    after = np.random.randint(NEXT_DRAW_RANGE)
    np.random.seed(99)
    np.testing.assert_array_equal(mask_dilate_draws(6), one_by_one)
    assert np.random.randint(NEXT_DRAW_RANGE) == after
    np.random.seed(99)
    np.testing.assert_array_equal(mask_dilate_draws(6, rng=np.random.RandomState(99)), one_by_one)
    np.testing.assert_array_equal(mask_dilate_draws(6), one_by_one)
    assert mask_dilate_draws(50, max_thickness=3).max() == 3


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_transform_and_composite(gold, tag):
    f = frames_of(gold, tag)
    per_sample = np.concatenate([emu.transform_f64(im, YAML_MEANS) for im in f["image_observed"]])
    same(per_sample, gold[tag + "_ref_transform"])
    same(per_sample, gold[tag + "_ref_image_observed"])
    same(np.concatenate([emu.transform_f64(im, YAML_MEANS) for im in f["image_rendered"]]), gold[tag + "_ref_image_rendered"])
    comp = emu.composite(f["image_observed"], f["bg_image"], f["mask_gt_observed"], f["use_bg"])
    assert not np.array_equal(comp, f["image_observed"])
    same(np.concatenate([emu.transform_f64(im, YAML_MEANS) for im in comp]), gold[tag + "_ref_image_observed_syn"])
    # the fp32 form the kernel computes: within 2^-15 of the float64 result (mean rounded to fp32 <= 2^-18, one fp32 rounding of
    # |x| < 256 <= 2^-17), exact with integer means
    got = emu.transform_f32(f["image_observed"], YAML_MEANS[::-1])
    assert got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - gold[tag + "_ref_transform"]).max() <= 2.0 ** -15
    ints = np.array([104.0, 117.0, 124.0])
    same(emu.transform_f32(f["image_observed"], ints[::-1]),
         np.concatenate([emu.transform_f64(im, ints) for im in f["image_observed"]]))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_depth(gold, tag):
    f = frames_of(gold, tag)
    for key in ("depth_observed", "depth_rendered", "depth_gt_observed"):
        got = emu.depth_f32(f[key])
        assert got.dtype == np.float32 and gold["%s_ref_%s" % (tag, key)].dtype == np.float32
        np.testing.assert_array_equal(got, gold["%s_ref_%s" % (tag, key)])
    np.testing.assert_array_equal(emu.depth_f32(f["depth_observed"], 1000, f["mask_gt_observed"], f["mask_idx"]),
                                  gold[tag + "_ref_depth_observed_masked_train"])
    np.testing.assert_array_equal(emu.depth_f32(f["depth_observed"], 1000, f["mask_observed_est"], f["mask_idx"]),
                                  gold[tag + "_ref_depth_observed_masked_test"])
    assert not np.array_equal(gold[tag + "_ref_depth_observed_masked_test"], gold[tag + "_ref_depth_observed"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_pair_masks(gold, tag):
    f = frames_of(gold, tag)
    B = f["mask_idx"].shape[0]
    for init, dil in (("box_gt", False), ("box_gt", True), ("mask_gt", True)):
        name = "%s_ref_train_%s%s" % (tag, init, "_dilate" if dil else "")
        draws = None
        if dil:
            np.random.seed(int(gold[name + "_seed"]))
            draws = mask_dilate_draws(B)
            assert np.random.randint(NEXT_DRAW_RANGE) == gold[name + "_next"]
        mo, gt, mr = emu.pair_mask_train(f, init, draws)
        same(mo, gold[name + "_mask_observed"])
        same(gt, gold[name + "_mask_gt_observed"])
        same(mr, gold[name + "_mask_rendered"])
    for init in TEST_INIT_MASKS:
        for dil in (False, True):
            name = "%s_ref_test_%s%s" % (tag, init, "_dilate" if dil else "")
            draws = mask_dilate_draws(B, rng=np.random.RandomState(int(gold["test_dilate_seed"]))) if dil else None
            mo, mr = emu.pair_mask_test(f, init, draws)
            same(mo, gold[name + "_mask_observed"])
            same(mr, gold[name + "_mask_rendered"])
        same(gold["%s_ref_testbatch_%s_mask_observed" % (tag, init)], gold["%s_ref_test_%s_mask_observed" % (tag, init)])
    # the dilated fixtures differ from the plain ones: the draws did something
    assert not np.array_equal(gold[tag + "_ref_test_box_rendered_dilate_mask_observed"], gold[tag + "_ref_test_box_rendered_mask_observed"])


def test_prototypes_parse_from_the_header():
    p = parse_header()
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert p["deepim_ingest_bgr8"] == (ci, [vp] * 7 + [ci] * 3, ["ctx", "out", "frames", "bg_frames", "fg_labels", "use_bg",
                                                                 "means_rgb", "B", "H", "W"])
    assert p["deepim_ingest_depth16"] == (ci, [vp] * 5 + [cf] + [ci] * 3, ["ctx", "out", "depth", "labels", "mask_idx",
                                                                          "depth_factor", "B", "H", "W"])
    assert p["deepim_ingest_label_mask"] == (ci, [vp] * 4 + [ci] * 3, ["ctx", "out", "labels", "mask_idx", "B", "H", "W"])
    assert p["deepim_mask_dilate"] == (ci, [vp] * 4 + [ci] * 3, ["ctx", "out", "mask", "thickness", "B", "H", "W"])
