"""NumPy statement of the device background path, written from its specification and NOT from lib/utils/background.py (which it
never imports): the crop of lib/utils/image.py:111-141, the size rule of `resize` (:562-569), the 8-bit INTER_LINEAR arithmetic
of cv2.resize's portable path, the paste onto a black frame (:118,145), the composite (:147-155) and the stream-3 draws of
csrc/sample.hip on tests/pose_sampler_emulation.py's Philox.  TEST INFRASTRUCTURE ONLY.

tests/golden/make_background_golden.py hands `resample` to the reference's own get_pair_image as its cv2.resize and records
what the reference asks of it; tests/test_background_host.py holds lib/utils/background.py against this file and against those
records; tests/test_gpu_backgrounds.py holds the kernels against it.
"""
import math

import numpy as np

import ingest_emulation as iemu
import pose_sampler_emulation as pemu

f32 = np.float32

# the backgrounds of the golden file: every branch of image.py:119-141 in landscape and portrait frames, black strips on either
# side, scales below and above 1; "frame" stands for an image of the frame's own size
GOLDEN_BACKGROUNDS = ((375, 500), (500, 375), (333, 500), (500, 500), (20, 90), (90, 20), (24, 32), (37, 53), (7, 5), (442, 500),
                      "frame")
GOLDEN_FRAMES = ((48, 64), (64, 48), (30, 44))
SMALL_BACKGROUNDS = ((20, 90), (90, 20), (24, 32), (37, 53), (7, 5))


def background_shape(entry, H, W):
    return (H, W) if entry == "frame" else entry


def background_image(bh, bw):
    """the seeded (bh,bw,3) uint8 image of that size, the same wherever it is made"""
    return np.random.default_rng(7000 + 1009 * bh + bw).integers(0, 256, (bh, bw, 3), dtype=np.uint8)


def round_half_even(v):
    """cvRound of a non-negative value"""
    lo = math.floor(v)
    d = v - lo
    if d > 0.5 or (d == 0.5 and lo % 2 == 1):
        return int(lo) + 1
    return int(lo)


def crop_size(bh, bw, H, W):
    ratio = float(H) / float(W)
    both = (ratio < 1 and float(bh) / float(bw) < 1) or (ratio >= 1 and float(bh) / float(bw) >= 1)
    if bh >= bw:
        new_h = int(math.ceil(bw * ratio))
        shape = (new_h, bw) if (new_h < bh or not both) else (bh, bw)
    else:
        new_w = int(math.ceil(bh / ratio))
        shape = (bh, new_w) if (new_w < bw or not both) else (bh, bw)
    return min(shape[0], bh), min(shape[1], bw)


def resize_scale(ch, cw, H, W):
    """the im_scale of image.py:562-568 for target min(H,W), max max(H,W)"""
    scale = float(min(H, W)) / float(min(ch, cw))
    if np.round(scale * max(ch, cw)) > max(H, W):
        scale = float(max(H, W)) / float(max(ch, cw))
    return scale


def resized_size(ch, cw, H, W):
    scale = resize_scale(ch, cw, H, W)
    return scale, round_half_even(ch * scale), round_half_even(cw * scale)


def resize_table(n_out, n_src, scale):
    """[(i0, i1, w0, w1)] per output index, one entry at a time in numpy float32 scalars"""
    out = []
    inv = 1.0 / float(scale)
    for d in range(n_out):
        f = f32((d + 0.5) * inv - 0.5)
        i = int(math.floor(f))
        f = f32(f - f32(i))
        if i < 0:
            i, f = 0, f32(0)
        if i >= n_src - 1:
            i, f = n_src - 1, f32(0)
        w1 = round_half_even(float(f32(f * f32(2048))))
        w0 = round_half_even(float(f32((f32(1) - f) * f32(2048))))
        out.append((i, min(i + 1, n_src - 1), w0, w1))
    return out


def resample(im, scale):
    """cv2.resize(im, None, None, fx=scale, fy=scale, INTER_LINEAR) of an (h,w,3) uint8 image by the integer rule"""
    h, w = im.shape[:2]
    oh, ow = round_half_even(h * scale), round_half_even(w * scale)
    xt, yt = np.array(resize_table(ow, w, scale), np.int64), np.array(resize_table(oh, h, scale), np.int64)
    P = im.astype(np.int64)
    a0, a1 = xt[:, 2][None, :, None], xt[:, 3][None, :, None]
    rows = P[:, xt[:, 0]] * a0 + P[:, xt[:, 1]] * a1                     # (h, ow, 3): the horizontal pass
    r0, r1 = rows[yt[:, 0]] >> 4, rows[yt[:, 1]] >> 4
    b0, b1 = yt[:, 2][:, None, None], yt[:, 3][:, None, None]
    v = (((b0 * r0) >> 16) + ((b1 * r1) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def background_frame(im, H, W):
    """image.py:108-145: the image cropped, resized and pasted at the top-left of a black (H,W,3) frame"""
    ch, cw = crop_size(im.shape[0], im.shape[1], H, W)
    small = resample(im[:ch, :cw], resize_scale(ch, cw, H, W))
    out = np.zeros((H, W, 3), np.uint8)
    out[:small.shape[0], :small.shape[1]] = small          # raises where the reference raises: a resized crop beyond the frame
    return out


def background_frames(images, bg_index, H, W):
    """(B,H,W,3): background_frame of images[bg_index[b]]; black for an index outside the pool"""
    out = np.zeros((len(bg_index), H, W, 3), np.uint8)
    for b, k in enumerate(bg_index):
        if 0 <= k < len(images):
            out[b] = background_frame(images[k], H, W)
    return out


def ingest_pool(frames, fg_labels, use_bg, bg_index, images, means_rgb=None):
    """what deepim_ingest_bgr8_pool computes → (B,3,H,W) float32"""
    B, H, W = fg_labels.shape
    bg = background_frames(images, bg_index, H, W)
    return iemu.transform_f32(iemu.composite(frames, bg, fg_labels, use_bg), means_rgb)


def draws(seed, ids, ratio, pool_size, always=None, stream=3):
    """deepim_sample_backgrounds → (use_bg (n) int32, bg_index (n) int32, u (n) float64)"""
    words = pemu.draw(seed, ids, 0, stream)
    u = pemu.uniform(words[:, 0])
    use = u < float(ratio)
    if always is not None:
        use = use | (np.asarray(always).reshape(-1) != 0)
    return use.astype(np.int32), pemu.below(words[:, 1], pool_size).astype(np.int32), u
