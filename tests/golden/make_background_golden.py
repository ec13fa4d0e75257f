#!/usr/bin/env python
"""Golden vectors of the background replacement, produced by running the REFERENCE'S OWN lib/utils/image.py.

Runs only in the build container (needs /root/reference):  python tests/golden/make_background_golden.py
Writes tests/golden/background_golden.npz (committed).  TEST INFRASTRUCTURE ONLY.

As make_ingest_golden.py does, get_pair_image(..., "train") is driven with data_syn=True through a stand-in `cv2`, temporary
files and a one-line VOC list. This time the background is NOT frame-sized: the stand-in `resize` RECORDS the shape it is
handed and fx / fy — what the reference's crop (image.py:111-141) and scale rule (:562-569) come to — and returns
tests/background_emulation.resample of it, cv2 not being installed. So the file pins the reference's crop, scale, paste and
composite; the resample's arithmetic is the emulation's own on both sides.

Per frame size (48x64, 64x48, 30x44) and background (background_emulation.GOLDEN_BACKGROUNDS) it stores the recorded crop shape
and scale, and the reference's final image_observed tensor. That tensor is float64 `pixel - mean` of a uint8 image; it is
stored as the uint8 image (tensor + mean, rounded) after checking that `uint8 - mean` gives the reference's float64 BIT FOR BIT,
an eighth of the bytes. The backgrounds are seeded (background_emulation.background_image); the file stores only a checksum of
each, so that a test notices a generator that no longer makes the same image.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_ingest_golden as mig  # noqa: E402
import background_emulation as bemu  # noqa: E402

CALLS = []


def install_recording_resize():
    cv2 = sys.modules["cv2"]

    def resize(im, dsize, dst=None, fx=None, fy=None, interpolation=None):
        assert dsize is None and interpolation == cv2.INTER_LINEAR
        CALLS.append((im.shape, fx, fy))
        assert fx == fy
        return bemu.resample(im, fx)

    cv2.resize = resize


def tag_of(H, W, entry):
    return "f%dx%d_bg%s" % (H, W, entry if entry == "frame" else "%dx%d" % entry)


def checksum(im):
    return np.int64((im.astype(np.int64).reshape(-1) * (np.arange(im.size, dtype=np.int64) % 251 + 1)).sum())


def main():
    MD, IM, DP = mig.load_reference()
    install_recording_resize()
    tmp = tempfile.mkdtemp()
    voc = os.path.join(tmp, "VOCdevkit", "VOC2012")
    os.makedirs(os.path.join(voc, "ImageSets", "Main"), exist_ok=True)
    os.makedirs(os.path.join(voc, "JPEGImages"), exist_ok=True)
    with open(os.path.join(voc, "ImageSets", "Main", "diningtable_trainval.txt"), "w") as fh:
        fh.write("bg0  1\nskipped -1\n")
    out = {"pixel_means": mig.YAML_MEANS.copy()}
    for H, W in bemu.GOLDEN_FRAMES:
        rng = np.random.default_rng(100 * H + W)
        frame = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        labels = np.zeros((H, W), np.uint8)
        labels[H // 4:H // 2 + 3, W // 3:W // 3 + 9] = 2
        labels[H - 5:H - 2, 1:6] = 7                       # another object's label: image.py:153 tests != 0
        labels[0, 0] = labels[H - 1, W - 1] = 2
        out["f%dx%d_image_observed" % (H, W)], out["f%dx%d_mask_gt_observed" % (H, W)] = frame, labels
        cfg = mig.make_config("a")
        cfg.SCALES = [(min(H, W), max(H, W))]              # (target, max) of image.py:77-78: the frames keep their size
        cfg.dataset.root_path = tmp
        rec = {"img_flipped": False, "mask_idx": 2, "data_syn": True}
        for key, arr in (("image_observed", frame), ("image_rendered", frame), ("mask_gt_observed", labels)):
            rec[key] = os.path.join(tmp, "%dx%d_%s.png" % (H, W, key))
            open(rec[key], "w").close()
            mig.STORE[rec[key]] = arr
        for entry in bemu.GOLDEN_BACKGROUNDS:
            bh, bw = bemu.background_shape(entry, H, W)
            bg = bemu.background_image(bh, bw)
            mig.STORE[os.path.join(voc, "JPEGImages", "bg0.jpg")] = bg
            del CALLS[:]
            obs, _ren, _ = IM.get_pair_image([rec], cfg, "train")
            assert len(CALLS) == 3 and CALLS[0][1] == CALLS[1][1] == 1.0        # the two frames, then the background's crop
            (ch, cw, _c), fx, _fy = CALLS[2]
            ref = obs[0]
            assert ref.dtype == np.float64 and ref.shape == (1, 3, H, W)
            means_rgb = mig.YAML_MEANS[::-1].reshape(1, 3, 1, 1)
            u8 = np.rint(ref + means_rgb).astype(np.uint8)
            assert np.array_equal(u8 - means_rgb, ref) and (u8 - means_rgb).dtype == np.float64
            tag = tag_of(H, W, entry)
            out[tag + "_crop"] = np.array([ch, cw], np.int64)
            out[tag + "_scale"] = np.float64(fx)
            out[tag + "_ref_image_observed_u8"] = u8
            out[tag + "_bg_checksum"] = checksum(bg)
    path = os.path.join(HERE, "background_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
