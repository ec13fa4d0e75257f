"""Mirror of lib/utils/mask_dilate.py on the device: the random draws stay with the loader (host numpy, the reference's
generator), the shifted ORs run as one kernel over the batch (csrc/ingest.hip, deepim_mask_dilate).

    draws = mask_dilate_draws(B)                     # host int32 (B,4): what B reference calls would have drawn
    out = mask_dilate_batch(mask, ctx.array(draws, dtype=np.int32))

The training loader (core/loader.py) takes its draws from the device's counter-based generator instead, without a host random
number or a read-back: mask_dilate_draws_device (csrc/sample.hip, deepim_sample_mask_dilate).
"""
import ctypes

import numpy as np

from ...runtime import Context, DeviceArray, lib

# mask_dilate.py:22,28,34,40 — the directions for which each of the four blocks is skipped, in the file's order:
# origin shifted down (:24), up (:30), right (:36), left (:42)
_SKIPPED = ((0, 1, 4), (1, 2, 5), (2, 3, 6), (0, 3, 7))


def mask_dilate_draws(n, max_thickness=10, rng=np.random):
    """int32 (n,4) thicknesses of n successive reference calls, 0 where a side is not dilated. Consumes `rng` (np.random or a
    RandomState) exactly as those calls would: per sample one randint(10) for the direction (:19), then one
    randint(max_thickness) + 1 per enabled side, in the file's order."""
    out = np.zeros((int(n), 4), np.int32)
    for i in range(int(n)):
        direction = rng.randint(10)
        for k, skipped in enumerate(_SKIPPED):
            if direction not in skipped:
                out[i, k] = rng.randint(max_thickness) + 1
    return out


def mask_dilate_draws_device(ctx, B, seed, draw_base=0, draw_ids=None, max_thickness=10):
    """The draws of mask_dilate_draws from the device's counter-based generator (csrc/sample.hip, stream 2) → device int32 (B,4),
    never read back. Pair b has draw id draw_ids[b] (device uint64 (B) or host integers), or draw_base + b: its draw does not
    depend on where it lands in a batch. The numbers are the device generator's, not numpy's: the distribution of
    mask_dilate_draws (direction uniform in [0,10), thickness uniform in [1, max_thickness]), not its sequence."""
    B = int(B)
    if draw_ids is not None and not isinstance(draw_ids, DeviceArray):
        draw_ids = ctx.array(np.asarray(draw_ids).reshape(B), dtype=np.uint64)
    if draw_ids is not None and (draw_ids.dtype != np.uint64 or draw_ids.size != B):
        raise TypeError("mask_dilate_draws_device: draw_ids must be uint64 with %d values" % B)
    out = ctx.empty((B, 4), np.int32)
    u64 = (1 << 64) - 1
    lib.deepim_sample_mask_dilate(ctx.handle, out, int(max_thickness), ctypes.c_ulonglong(int(seed) & u64),
                                  ctypes.c_ulonglong(int(draw_base) & u64), draw_ids, B)
    return out


def mask_dilate_batch(mask, thickness, out=None):
    """mask: device fp32 (B,1,H,W) (or (B,H,W)); thickness: int32 (B,4), device or host, from mask_dilate_draws.
    Returns the dilated masks as a new device array of mask's shape (or fills `out`, which must not be `mask`)."""
    ctx = mask.context
    assert mask.dtype == np.float32 and mask.ndim in (3, 4), "mask_dilate_batch: fp32 (B,1,H,W) expected"
    B, H, W = mask.shape[0], mask.shape[-2], mask.shape[-1]
    if not isinstance(thickness, DeviceArray):
        thickness = ctx.array(np.asarray(thickness).reshape(B, 4), dtype=np.int32)
    assert thickness.dtype == np.int32 and thickness.size == B * 4, "mask_dilate_batch: thickness is int32 (B,4)"
    if out is None:
        out = ctx.empty(mask.shape)
    lib.deepim_mask_dilate(ctx.handle, out, mask, thickness, B, H, W)
    return out


def mask_dilate(mask_origin, max_thickness=10):
    """The reference's signature: a 2-D numpy mask in, the dilated mask out (same dtype), drawn from np.random as the
    reference draws, computed on the default device in fp32."""
    mask_origin = np.asarray(mask_origin)
    draws = mask_dilate_draws(1, max_thickness)
    ctx = Context.default()
    m = ctx.array(mask_origin[np.newaxis, np.newaxis], dtype=np.float32)
    return mask_dilate_batch(m, draws).asnumpy()[0, 0].astype(mask_origin.dtype)
