"""NumPy statement, in this project's own terms, of what the reference's frame-ingest path computes (lib/utils/image.py,
lib/utils/mask_dilate.py, lib/utils/get_min_rect.py; cited by line), on decoded frames instead of file paths.
TEST INFRASTRUCTURE ONLY.

tests/test_ingest_host.py holds it against tests/golden/ingest_golden.npz (outputs of the reference's own files, made by
tests/golden/make_ingest_golden.py); tests/test_gpu_ingest.py holds the kernels against it where the fixture has no case
(the fp32 arithmetic of the kernels, the branch of image.py the reference cannot run: :271-285 assigns `cur_mask_observed` and
appends `mask_observed`).
"""
import numpy as np

f32 = np.float32


# ------------------------------------------------------------------------------------------------ transform / composite --
def transform_f64(im, pixel_means):
    """What image.py:583-594 computes for one (H,W,3) BGR image with pixel_means in BGR order: channels reversed to RGB, each
    less its own mean, in float64, as (1,3,H,W)."""
    rgb = np.asarray(im)[:, :, ::-1].astype(np.float64) - np.asarray(pixel_means, np.float64)[::-1]
    return np.ascontiguousarray(rgb.transpose(2, 0, 1))[np.newaxis]


def transform_f32(frames, means_rgb=None):
    """What deepim_ingest_bgr8 computes: (B,H,W,3) uint8 BGR → (B,3,H,W), float32(pixel) - float32(mean), one fp32 subtraction."""
    means = np.zeros(3, f32) if means_rgb is None else np.asarray(means_rgb, dtype=f32)
    rgb = frames[..., ::-1].astype(f32) - means
    assert rgb.dtype == f32
    return np.ascontiguousarray(rgb.transpose(0, 3, 1, 2))


def composite(frames, bg, fg_labels, use_bg=None):
    """The background replacement of image.py:147-155 for a batch: a pixel keeps the frame where its label is non-zero and
    takes the background elsewhere, for the samples with use_bg != 0 (None: every sample)."""
    on = np.ones(frames.shape[0], bool) if use_bg is None else np.asarray(use_bg) != 0
    take_bg = (fg_labels == 0) & on[:, None, None]
    return np.where(take_bg[..., None], bg, frames)


# ------------------------------------------------------------------------------------------------------- depth / labels --
def depth_f32(depth, depth_factor=1000, labels=None, mask_idx=None):
    """What image.py:203-219 computes: uint16 (B,H,W) → float32 (B,1,H,W) = float32(depth) / float32(factor), one correctly
    rounded division; with labels, zero outside the pair's own label (:211)."""
    d = depth.astype(f32) / f32(depth_factor)
    if labels is not None:
        d = np.where(labels == np.asarray(mask_idx).reshape(-1, 1, 1), d, f32(0))
    assert d.dtype == f32
    return d[:, None]


def label_mask(labels, mask_idx):
    """What image.py:255-260 / :308-312 compute: 1 where the label map holds the pair's mask_idx, else 0 → float32 (B,1,H,W)."""
    return (labels == np.asarray(mask_idx).reshape(-1, 1, 1)).astype(f32)[:, None]


# ------------------------------------------------------------------------------------------------------------- dilation --
def _shifted(a, dy, dx):
    """a moved by (dy, dx) pixels (positive = down / right) inside its frame, zeros moved in; a shift of the frame's size or more
    leaves nothing"""
    H, W = a.shape
    out = np.zeros_like(a)
    if abs(dy) < H and abs(dx) < W:
        out[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = a[max(-dy, 0):H - max(dy, 0), max(-dx, 0):W - max(dx, 0)]
    return out


def mask_dilate(mask_origin, thickness):
    """What lib/utils/mask_dilate.py:19-47 computes once the four draws are known (thickness = down, up, right, left; 0 = side
    off), as the kernel states it: a non-zero pixel keeps its value, clamped to 1; an empty pixel becomes 1 when, for an enabled
    side, the origin pixel exactly that side's thickness away is non-zero."""
    td, tu, tr, tl = (int(t) for t in thickness)
    filled = mask_origin != 0
    hit = np.zeros(mask_origin.shape, bool)
    for t, dy, dx in ((td, 1, 0), (tu, -1, 0), (tr, 0, 1), (tl, 0, -1)):
        if t > 0:
            hit |= _shifted(filled, dy * t, dx * t)
    out = np.where(filled, np.minimum(mask_origin, 1), hit).astype(mask_origin.dtype)
    return out


def mask_dilate_batch(masks, thickness):
    return np.stack([mask_dilate(masks[b, 0], thickness[b])[None] for b in range(masks.shape[0])])


# ------------------------------------------------------------------------------------------------------------ rectangle --
def mask_box(mask):
    """get_min_rect.py:15-23 / image.py:327-336: [y_start:y_end, x_start:x_end] = 1 with end = the LAST index holding a
    non-zero, used as an exclusive bound. An empty mask gives zeros (image.py:343,353)."""
    out = np.zeros(mask.shape, f32)
    ys, xs = np.nonzero(mask)
    if len(ys):
        out[ys.min():ys.max(), xs.min():xs.max()] = 1
    return out


def _boxes(masks):
    return np.stack([mask_box(m[0])[None] for m in masks])


# ----------------------------------------------------------------------------------------------------------- pair masks --
def mask_rendered(depth_rendered, depth_factor=1000):
    """image.py:391-395: depth in metres with every value > 0.2 set to 1 (smaller values kept)."""
    d = depth_f32(depth_rendered, depth_factor)
    return np.where(d > f32(0.2), f32(1), d)


def pair_mask_train(frames, init_mask, thickness=None, depth_factor=1000):
    """image.py:251-295 → (mask_observed, mask_gt_observed, mask_rendered), float32 (B,1,H,W). "mask_gt" hands over the 0 / 1
    mask (the reference copies the raw label map, :265; equal after the dilation's clamp when the map holds 0 and mask_idx
    only). "box_rendered" is what :271-285 means to hand over."""
    gt = label_mask(frames["mask_gt_observed"], frames["mask_idx"])
    if init_mask == "mask_gt":
        mo = gt.copy()
    elif init_mask == "box_gt":
        mo = _boxes(gt)                                                                                                   # :268-270
    elif init_mask == "box_rendered":
        mo = _boxes((depth_f32(frames["depth_rendered"], depth_factor) > 0.2).astype(f32))                                # :276-285
    else:
        raise Exception("Unknown mask type: {}".format(init_mask))
    if thickness is not None:
        mo = mask_dilate_batch(mo, thickness)                                                                             # :289-290
    return mo, gt, mask_rendered(frames["depth_rendered"], depth_factor)


def pair_mask_test(frames, init_mask, thickness=None, depth_factor=1000):
    """image.py:297-399 → (mask_observed, mask_rendered); the `np.sum(depth_rendered) == 0` guard of :301-303 is not restated."""
    if init_mask == "mask_gt_observed":
        mo = label_mask(frames["mask_gt_observed"], frames["mask_idx"])                                                   # :306-312
    elif init_mask == "mask_observed":
        mo = label_mask(frames["mask_observed"], frames["mask_idx"])                                                      # :314-320
    elif init_mask == "box_gt_observed":
        mo = _boxes(label_mask(frames["mask_gt_observed"], frames["mask_idx"]))                                           # :323-336
    elif init_mask == "box_":
        mo = _boxes(label_mask(frames["mask_observed"], frames["mask_idx"]))                                              # :339-352
    elif init_mask == "box_rendered":
        mo = _boxes((depth_f32(frames["depth_rendered"], depth_factor) > 0.2).astype(f32))                                # :359-374
    else:
        raise Exception("Unknown init mask type: {}".format(init_mask))
    if thickness is not None:
        mo = mask_dilate_batch(mo, thickness)                                                                             # :380-381
    return mo, mask_rendered(frames["depth_rendered"], depth_factor)
