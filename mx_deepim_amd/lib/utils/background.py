"""The background replacement of lib/utils/image.py:96-155 on the device: a POOL of decoded background images uploaded once,
per-pair draws from the loader's counter-based generator (csrc/sample.hip, stream 3) and one kernel
(csrc/ingest.hip, deepim_ingest_bgr8_pool) that crops, resamples, pads, composites, subtracts the means and writes the fp32
NCHW tensor. No resized background ever exists in memory.

    pool = BackgroundPool(ctx, images, H, W)          # images: the decoded VOC list, (bh,bw,3) uint8 BGR arrays of any sizes
    use_bg, bg_index = background_draws_device(ctx, B, seed, draw_ids, ratio, len(pool), always=data_syn)
    image_observed = image.transform_batch_pool(ctx, frames_bgr, means, fg_labels, use_bg, bg_index, pool)

A pool image of size (bh, bw) and a frame (H, W) fix everything except the pixels, so all floating-point work happens here,
once per image, and the kernel is integer arithmetic on four taps:

    crop_size       the top-left crop to the frame's aspect ratio (image.py:111-141)
    resized_size    the scale and the size `resize` (image.py:562-569) hands to cv2.resize; smaller than the frame is normal
                    (the rest of the frame stays black, :118,145), larger is an error in the reference and refused here
    resize_table    cv2.resize's generic 8-bit INTER_LINEAR arithmetic: per output index two source indices and two 11-bit
                    weights, (x0, x1, a0, a1) for a column and (y0, y1, b0, b1) for a row; per channel
                        r0 = P[y0][x0] a0 + P[y0][x1] a1        r1 = P[y1][x0] a0 + P[y1][x1] a1
                        v  = clamp((((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2, 0, 255)
    pack_table      a table as the kernel reads it, one 32-bit word per output index

Two deviations from cv2:
1. cv2 is not installed where this was written, so parity with any particular OpenCV build is neither measured nor claimed;
   SIMD and IPP builds differ among themselves by a grey level. The rule above is OpenCV's portable C++ path.
2. cv2 silently switches an exact 2x downscale to INTER_AREA. This rule does not.

File decoding is still the caller's.
"""
import ctypes
import math

import numpy as np

from ...runtime import DeviceArray, lib

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS         # 2048: the two weights of a tap pair sum to it
MAX_SIDE = 1 << 19                # a packed table entry keeps 19 bits of a source index
TAIL_BYTES = 12                   # readable bytes behind the last image: the kernel reads aligned 12-byte windows


def crop_size(bh, bw, H, W):
    """image.py:111-141 → (ch, cw): the top-left crop of a (bh, bw) image that goes into an (H, W) frame."""
    bh, bw, H, W = int(bh), int(bw), int(H), int(W)
    r = float(H) / float(W)
    same = (r < 1 and float(bh) / float(bw) < 1) or (r >= 1 and float(bh) / float(bw) >= 1)
    ch, cw = bh, bw
    if bh >= bw:
        n = int(np.ceil(bw * r))
        if n < bh or not same:
            ch = n
    else:
        n = int(np.ceil(bh / r))
        if n < bw or not same:
            cw = n
    return min(ch, bh), min(cw, bw)           # a numpy slice cannot exceed the image


def resized_size(ch, cw, H, W):
    """`resize` (image.py:562-569) with target min(H,W) and max max(H,W) (:109-110) → (s, oh, ow): the scale and cv2.resize's
    output size, cvRound (round half to even) of each side times s."""
    target, most = min(int(H), int(W)), max(int(H), int(W))
    s = float(target) / float(min(ch, cw))
    if np.round(s * max(ch, cw)) > most:
        s = float(most) / float(max(ch, cw))
    return s, int(round(ch * s)), int(round(cw * s))


def resize_table(n_out, n_src, s):
    """→ int32 (n_out, 4): (i0, i1, w0, w1) of every output index along one axis of a cv2.resize(fx=fy=s, INTER_LINEAR) of 8-bit
    pixels. i1 = min(i0 + 1, n_src - 1): nothing outside the source is read."""
    f32 = np.float32
    d = np.arange(int(n_out), dtype=np.float64)
    f = ((d + 0.5) * (1.0 / float(s)) - 0.5).astype(f32)
    i = np.floor(f).astype(np.int64)
    f = (f - i.astype(f32)).astype(f32)
    low, high = i < 0, i >= n_src - 1
    i = np.where(low, 0, np.where(high, n_src - 1, i))
    f = np.where(low | high, f32(0), f).astype(f32)
    w1 = np.rint((f * f32(COEF_ONE)).astype(f32)).astype(np.int64)
    w0 = np.rint(((f32(1) - f) * f32(COEF_ONE)).astype(f32)).astype(np.int64)
    return np.stack([i, np.minimum(i + 1, n_src - 1), w0, w1], 1).astype(np.int32)


def pack_table(table):
    """resize_table's rows as the kernel reads them → uint32 (n): i0 << 13 | (i1 != i0) << 12 | w1. Nothing is lost: i1 is i0 or
    i0 + 1 and w0 = 2048 - w1."""
    t = np.asarray(table, np.int64)
    if len(t) and (t[:, 0].max() >= MAX_SIDE or ((t[:, 1] != t[:, 0]) & (t[:, 1] != t[:, 0] + 1)).any()
                   or (t[:, 2] + t[:, 3] != COEF_ONE).any() or t[:, 3].min() < 0 or t[:, 3].max() > COEF_ONE):
        raise ValueError("pack_table: not a resize_table")
    return ((t[:, 0] << 13) | ((t[:, 1] != t[:, 0]).astype(np.int64) << 12) | t[:, 3]).astype(np.uint32)


class BackgroundPool(object):
    """P decoded background images on the device, with the tables deepim_ingest_bgr8_pool reads, for (H, W) frames.
    len(pool) = P; pool.nbytes = device bytes; pool.geometry = [(ch, cw, s, oh, ow)] per image, on the host.
    ValueError: an empty pool, an image that is not (bh,bw,3) uint8, an image whose resized crop is larger than the frame
    (the reference's `bg_image_resize[0:h, 0:w] = ...` raises there)."""

    def __init__(self, ctx, images, H, W):
        self.context, self.height, self.width = ctx, int(H), int(W)
        images = list(images)
        if not images:
            raise ValueError("BackgroundPool: no images")
        H, W, P = self.height, self.width, len(images)
        desc = np.zeros((P, 4), np.int64)
        xtab, ytab = np.zeros((P, W), np.uint32), np.zeros((P, H), np.uint32)
        self.geometry, offset = [], 0
        for k, im in enumerate(images):
            im = np.asarray(im)
            if (im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or min(im.shape[:2]) < 1
                    or max(im.shape[:2]) >= MAX_SIDE):
                raise ValueError("BackgroundPool: image %d is %s %s; a decoded (bh,bw,3) uint8 BGR image is expected"
                                 % (k, im.dtype, im.shape))
            bh, bw = im.shape[:2]
            ch, cw = crop_size(bh, bw, H, W)
            s, oh, ow = resized_size(ch, cw, H, W)
            if oh > H or ow > W:
                raise ValueError("BackgroundPool: image %d (%dx%d, crop %dx%d) resizes to %dx%d, larger than the %dx%d frame"
                                 % (k, bh, bw, ch, cw, oh, ow, H, W))
            self.geometry.append((ch, cw, s, oh, ow))
            desc[k] = (offset, bw * 3, oh, ow)
            xtab[k, :ow], ytab[k, :oh] = pack_table(resize_table(ow, cw, s)), pack_table(resize_table(oh, ch, s))
            offset += (bh * bw * 3 + 3) // 4 * 4               # every image starts 4-byte aligned
        pixels = np.zeros(offset + TAIL_BYTES, np.uint8)
        for k, im in enumerate(images):
            pixels[desc[k, 0]:desc[k, 0] + im.size] = np.ascontiguousarray(im).reshape(-1)
        self.pixels = ctx.array(pixels, dtype=np.uint8)
        self.desc = ctx.array(desc, dtype=np.int64)
        self.xtab, self.ytab = ctx.array(xtab, dtype=np.uint32), ctx.array(ytab, dtype=np.uint32)
        self._len = P

    def __len__(self):
        return self._len

    @property
    def nbytes(self):
        return self.pixels.nbytes + self.desc.nbytes + self.xtab.nbytes + self.ytab.nbytes


def background_draws_device(ctx, B, seed, draw_ids, ratio, pool_size, always=None, draw_base=0):
    """The draws of image.py:97-116 from the device's counter-based generator (csrc/sample.hip, stream 3) → device int32
    (use_bg (B), bg_index (B)), never read back: use_bg[b] = always[b] or u < ratio (`always`: the pairs' data_syn flags, host
    or device, None = none; ratio: TRAIN.REPLACE_OBSERVED_BG_RATIO), bg_index[b] uniform in [0, pool_size). Pair b has draw id
    draw_ids[b] (device uint64 (B) or host integers), or draw_base + b: its draw does not depend on where it lands in a batch."""
    B = int(B)
    if draw_ids is not None and not isinstance(draw_ids, DeviceArray):
        draw_ids = ctx.array(np.asarray(draw_ids).reshape(B), dtype=np.uint64)
    if draw_ids is not None and (draw_ids.dtype != np.uint64 or draw_ids.size != B):
        raise TypeError("background_draws_device: draw_ids must be uint64 with %d values" % B)
    if always is not None and not isinstance(always, DeviceArray):
        always = ctx.array(np.asarray(always).reshape(B) != 0, dtype=np.int32)
    if always is not None and (always.dtype != np.int32 or always.size != B):
        raise TypeError("background_draws_device: always must be int32 with %d values" % B)
    if not 0.0 <= float(ratio) <= 1.0 or math.isnan(float(ratio)):
        raise ValueError("background_draws_device: ratio %r is not in [0, 1]" % (ratio,))
    use_bg, bg_index = ctx.empty((B,), np.int32), ctx.empty((B,), np.int32)
    u64 = (1 << 64) - 1
    lib.deepim_sample_backgrounds(ctx.handle, use_bg, bg_index, always, ctypes.c_double(float(ratio)), int(pool_size),
                                  ctypes.c_ulonglong(int(seed) & u64), ctypes.c_ulonglong(int(draw_base) & u64), draw_ids, B)
    return use_bg, bg_index
