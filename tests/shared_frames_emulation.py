"""NumPy statement of what a shared-frame batch computes (mx_deepim_amd/lib/utils/image.py: N decoded frames for B pairs, pair b
looking at frame frame_index[b]): the gather `frames[frame_index]` handed to the per-pair restatements of
tests/ingest_emulation.py. TEST INFRASTRUCTURE ONLY.

tests/test_shared_frames_host.py holds it against tests/golden/ingest_golden.npz (N = B, identity index: a shared-frame batch
of that kind IS the per-pair batch); tests/test_gpu_shared_frames.py uses `replicate` to build the per-pair batch that the
existing ingest → zoom path is fed as the reference of the frame-indexed kernels.
"""
import numpy as np

import ingest_emulation as emu

SHARED_KEYS = ("image_observed", "depth_observed", "depth_gt_observed", "mask_gt_observed", "mask_observed", "mask_observed_est")


def gather(frames, frame_index):
    """(N,...) shared frames → the (B,...) per-pair array a replicated batch holds"""
    return np.ascontiguousarray(np.asarray(frames)[np.asarray(frame_index).reshape(-1)])


def replicate(frames):
    """A shared-frame `frames` dict → the per-pair dict of the same batch: every shared array gathered, frame_index dropped."""
    out = {k: v for k, v in frames.items() if k != "frame_index"}
    for k in SHARED_KEYS:
        if out.get(k) is not None:
            out[k] = gather(out[k], frames["frame_index"])
    return out


def transform_f32(frames_bgr, frame_index, means_rgb=None):
    return emu.transform_f32(gather(frames_bgr, frame_index), means_rgb)


def depth_f32(depth, frame_index, depth_factor=1000, labels=None, mask_idx=None):
    return emu.depth_f32(gather(depth, frame_index), depth_factor, None if labels is None else gather(labels, frame_index), mask_idx)


def label_mask(labels, frame_index, mask_idx):
    return emu.label_mask(gather(labels, frame_index), mask_idx)
