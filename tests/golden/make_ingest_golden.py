#!/usr/bin/env python
"""Golden vectors of the frame-ingest path, produced by running the REFERENCE'S OWN files.

Runs only in the build container (needs /root/reference):  python tests/golden/make_ingest_golden.py
Writes tests/golden/ingest_golden.npz (committed).  TEST INFRASTRUCTURE ONLY.

Imported UNMODIFIED from /root/reference: lib/utils/mask_dilate.py, lib/utils/image.py (with lib/utils/get_min_rect.py) and
lib/pair_matching/data_pair.py. image.py reads its frames with cv2, which is not installed: a stand-in `cv2` module is put
into sys.modules first (tests/golden/fake_mxnet.py is the precedent) whose `imread` hands back in-memory arrays keyed by path
(empty files of those names are created in a temporary directory, for the reference's os.path.exists asserts) and whose `resize`
asserts a scale of 1 and returns its input. Three names NumPy 2 removed are injected before import, as make_golden.py does.

Dilation: mask_dilate(mask) under np.random.seed(s) for the seeds below (all ten directions, thickness 1 and 10) on three
masks; inputs, outputs and the generator's next draw after each call are stored.
Functions, on seeded frames of 6x12 (B = 2) and 7x13 (B = 3): transform, get_pair_image (test phase; train phase with the
data_syn background composite), get_gt_observed_depth, get_pair_depth (with and without network.MASK_INPUTS), get_pair_mask
(train: box_gt, box_gt + MASK_DILATE, mask_gt + MASK_DILATE; test: every TEST.INIT_MASK, with and without TEST.MASK_DILATE)
and get_data_pair_test_batch. Not drivable: get_pair_mask's train "box_rendered" branch (image.py:271-285 assigns
`cur_mask_observed` and appends `mask_observed`, a NameError on the first pair) — tests/ingest_emulation.py restates it.
"""
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from mx_deepim_amd.config import AttrDict  # noqa: E402

DILATE_SEEDS = (0, 1, 2, 4, 5, 6, 7, 12, 13, 17, 41)
YAML_MEANS = np.array([123.68, 116.779, 103.939])     # deepim_flownet_LM_SIXD_v1_ape_RFMx4_8epoch.yaml:44-47
SHAPES = {"a": (2, 6, 12), "b": (3, 7, 13)}
MASK_IDX = {"a": (1, 3), "b": (2, 1, 5)}
DATA_SYN = {"a": (True, False), "b": (True, False, True)}
TRAIN_CASES = (("box_gt", None), ("box_gt", 5), ("mask_gt", 7))           # (TRAIN.INIT_MASK, seed of MASK_DILATE or None)
TEST_INIT_MASKS = ("mask_gt_observed", "mask_observed", "box_gt_observed", "box_", "box_rendered")
TEST_DILATE_SEED = 13
NEXT_DRAW_RANGE = 2 ** 31 - 1

STORE = {}      # path -> array, or a list of arrays handed out one per read


def install_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_COLOR, cv2.IMREAD_UNCHANGED, cv2.INTER_LINEAR, cv2.INTER_NEAREST = 1, -1, 1, 0

    def imread(path, flags=None):
        v = STORE[path]
        if isinstance(v, list):
            return v.pop(0).copy()
        return v.copy()

    def resize(im, dsize, dst=None, fx=None, fy=None, interpolation=None):
        assert dsize is None and fx == 1.0 and fy == 1.0, "stand-in cv2.resize: scale 1 only (%r, %r)" % (fx, fy)
        return im

    cv2.imread, cv2.resize = imread, resize
    sys.modules["cv2"] = cv2


def load_reference():
    np.float = float
    np.int = int
    np.maximum_sctype = lambda t: np.float64
    install_cv2()
    sys.path.insert(0, REF)
    from lib.utils import mask_dilate as MD
    from lib.utils import image as IM
    from lib.pair_matching import data_pair as DP
    return MD, IM, DP


def dilation_masks():
    m0 = np.zeros((40, 56), np.float32)
    m0[12:27, 20:41] = 1
    m0[15:20, 25:30] = 0                      # a hole: interior pixels that a shifted copy can fill
    m0[9:12, 30:34] = 1
    m1 = np.zeros((40, 56), np.float32)
    m1[0:14, 0:23] = 3.0                      # touches the top and left borders; label value 3: the clamp of :46
    m1[30:36, 44:50] = 1.0
    m2 = np.zeros((8, 9), np.float32)         # thickness can exceed the frame
    m2[2:5, 3:6] = 1
    m2[7, 0] = 2.0
    return [m0, m1, m2]


def make_frames(tag, rng):
    B, H, W = SHAPES[tag]
    f = {"image_observed": rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8),
         "image_rendered": rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8),
         "bg_image": rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8),
         "mask_idx": np.array(MASK_IDX[tag], np.int32), "use_bg": np.array(DATA_SYN[tag], np.int32)}
    special = np.array([0, 1, 999, 1000, 65535], np.uint16)
    for key in ("depth_observed", "depth_gt_observed"):
        d = rng.integers(0, 3000, (B, H, W)).astype(np.uint16)
        d.reshape(B, -1)[:, :5] = special
        f[key] = d
    dr = np.zeros((B, H, W), np.uint16)
    gt = np.zeros((B, H, W), np.uint8)
    est = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        y0, x0 = 1 + b % 2, 2 + b
        dr[b, y0:y0 + 3, x0:x0 + 5] = rng.integers(201, 1500, (3, 5))
        dr[b, H - 1, W - 1 - b] = 150          # below 0.2 m: kept by mask_rendered, outside the rectangle's source
        dr[b, y0 + 1, x0 + 1] = 200            # exactly 0.2 m in float32 terms or just off it: `> 0.2` decides
        gt[b, 1:4, 3 + b:8 + b] = MASK_IDX[tag][b]
        gt[b, 4, 5 + b] = MASK_IDX[tag][b]
        est[b, 2:5, 1 + b:6 + b] = MASK_IDX[tag][b]
        est[b, 0:2, 8:11] = MASK_IDX[tag][b] + 1       # another object's label
        est[b, 5, 0] = 255
    f.update(depth_rendered=dr, mask_gt_observed=gt, mask_observed=est, mask_observed_est=est)
    f["pose_rendered"] = rng.standard_normal((B, 3, 4)).astype(np.float32)
    return f


def make_config(tag):
    B, H, W = SHAPES[tag]
    cfg = AttrDict()
    cfg.SCALES = [(H, W)]
    cfg.network = AttrDict(PIXEL_MEANS=YAML_MEANS.copy(), MASK_INPUTS=False, INPUT_DEPTH=True, INPUT_MASK=True)
    cfg.dataset = AttrDict(DEPTH_FACTOR=1000, MASK_GT=False, root_path="", class_name=["ape", "cat"])
    cfg.TRAIN = AttrDict(INIT_MASK="box_gt", MASK_DILATE=False, MASK_SYN=False, REPLACE_OBSERVED_BG_RATIO=0.0)
    cfg.TEST = AttrDict(INIT_MASK="box_rendered", MASK_DILATE=False)
    return cfg


def make_pairdb(tag, frames, tmp, data_syn=False):
    B, H, W = SHAPES[tag]
    pairdb = []
    for b in range(B):
        rec = {"img_flipped": False, "mask_idx": int(frames["mask_idx"][b]), "pose_rendered": frames["pose_rendered"][b],
               "gt_class": "cat", "height": H, "width": W}
        for key in ("image_observed", "image_rendered", "depth_observed", "depth_rendered", "depth_gt_observed",
                    "mask_gt_observed", "mask_observed", "mask_observed_est"):
            path = os.path.join(tmp, "%s_%s_%d.png" % (tag, key, b))
            open(path, "w").close()
            STORE[path] = frames[key][b]
            rec[key] = path
        if data_syn:
            rec["data_syn"] = bool(frames["use_bg"][b])
        pairdb.append(rec)
    return pairdb


def install_voc(tag, frames, tmp):
    """the one-entry background list get_pair_image reads (:101-116); its image is handed out per composited pair"""
    voc = os.path.join(tmp, "VOCdevkit", "VOC2012")
    os.makedirs(os.path.join(voc, "ImageSets", "Main"), exist_ok=True)
    os.makedirs(os.path.join(voc, "JPEGImages"), exist_ok=True)
    with open(os.path.join(voc, "ImageSets", "Main", "diningtable_trainval.txt"), "w") as fh:
        fh.write("bg0  1\nskipped -1\n")
    STORE[os.path.join(voc, "JPEGImages", "bg0.jpg")] = [frames["bg_image"][b] for b in range(SHAPES[tag][0])
                                                         if frames["use_bg"][b]]


def cat(lst):
    return np.concatenate(lst, axis=0)


def main():
    MD, IM, DP = load_reference()
    out = {"dilate_seeds": np.array(DILATE_SEEDS, np.int64)}

    # ---- dilation
    for m, mask in enumerate(dilation_masks()):
        outs, nxt = [], []
        for s in DILATE_SEEDS:
            np.random.seed(s)
            outs.append(MD.mask_dilate(mask))
            nxt.append(np.random.randint(NEXT_DRAW_RANGE))
            assert outs[-1].dtype == np.float32
        out["dilate_mask%d" % m] = mask
        out["dilate_out%d" % m] = np.stack(outs)
        out["dilate_next%d" % m] = np.array(nxt, np.int64)

    # ---- the functions of image.py / data_pair.py
    tmp = tempfile.mkdtemp()
    for tag in sorted(SHAPES):
        B, H, W = SHAPES[tag]
        frames = make_frames(tag, np.random.default_rng(1900 + ord(tag)))
        for k, v in frames.items():
            out["%s_%s" % (tag, k)] = v
        cfg = make_config(tag)
        cfg.dataset.root_path = tmp
        pairdb = make_pairdb(tag, frames, tmp)
        sil = [0] * B

        out[tag + "_ref_transform"] = cat([IM.transform(frames["image_observed"][b], cfg.network.PIXEL_MEANS) for b in range(B)])
        obs, ren, _ = IM.get_pair_image(pairdb, cfg, "test")
        out[tag + "_ref_image_observed"], out[tag + "_ref_image_rendered"] = cat(obs), cat(ren)
        install_voc(tag, frames, tmp)
        obs, _, _ = IM.get_pair_image(make_pairdb(tag, frames, tmp, data_syn=True), cfg, "train")
        out[tag + "_ref_image_observed_syn"] = cat(obs)

        out[tag + "_ref_depth_gt_observed"] = cat(IM.get_gt_observed_depth(pairdb, cfg, sil, "train"))
        dobs, dren = IM.get_pair_depth(pairdb, cfg, sil, "test")
        out[tag + "_ref_depth_observed"], out[tag + "_ref_depth_rendered"] = cat(dobs), cat(dren)
        cfg.network.MASK_INPUTS = True
        out[tag + "_ref_depth_observed_masked_train"] = cat(IM.get_pair_depth(pairdb, cfg, sil, "train", random_k=[1.0] * B)[0])
        out[tag + "_ref_depth_observed_masked_test"] = cat(IM.get_pair_depth(pairdb, cfg, sil, "test")[0])
        cfg.network.MASK_INPUTS = False
        for v in (out[tag + "_ref_depth_observed"], out[tag + "_ref_depth_gt_observed"]):
            assert v.dtype == np.float32

        for init, seed in TRAIN_CASES:
            cfg.TRAIN.INIT_MASK, cfg.TRAIN.MASK_DILATE = init, seed is not None
            name = "%s_ref_train_%s%s" % (tag, init, "" if seed is None else "_dilate")
            if seed is not None:
                np.random.seed(seed)
                out[name + "_seed"] = np.int64(seed)
            mo, gt, mr = IM.get_pair_mask(pairdb, cfg, sil, "train")
            if seed is not None:
                out[name + "_next"] = np.int64(np.random.randint(NEXT_DRAW_RANGE))
            out[name + "_mask_observed"], out[name + "_mask_gt_observed"], out[name + "_mask_rendered"] = cat(mo), cat(gt), cat(mr)
        cfg.TRAIN.INIT_MASK, cfg.TRAIN.MASK_DILATE = "box_gt", False

        out["test_dilate_seed"] = np.int64(TEST_DILATE_SEED)
        for init in TEST_INIT_MASKS:
            for dil in (False, True):
                cfg.TEST.INIT_MASK, cfg.TEST.MASK_DILATE = init, dil
                name = "%s_ref_test_%s%s" % (tag, init, "_dilate" if dil else "")
                if dil:
                    np.random.seed(TEST_DILATE_SEED)
                mo, gt, mr = IM.get_pair_mask(pairdb, cfg, sil, "test")
                assert all(a is b for a, b in zip(mo, gt))        # :387
                out[name + "_mask_observed"], out[name + "_mask_rendered"] = cat(mo), cat(mr)
            # data_pair.py:22-63 (no dilation), every key of :45-58
            cfg.TEST.MASK_DILATE = False
            data, label, im_info = DP.get_data_pair_test_batch(pairdb, cfg)
            assert label == {} and len(data) == B
            keys = ("mask_observed", "mask_rendered")
            if init == TEST_INIT_MASKS[0]:       # the other keys do not depend on INIT_MASK: stored once
                keys += ("image_observed", "image_rendered", "src_pose", "depth_observed", "depth_rendered")
            for key in keys:
                out["%s_ref_testbatch_%s_%s" % (tag, init, key)] = cat([d[key] for d in data])
        cfg.TEST.INIT_MASK = "box_rendered"

    path = os.path.join(HERE, "ingest_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
