"""Rendered poses drawn on the device: the rule of toolkit/LM6d_1_gen_rendered_pose.py:80-107 over the counter-based generator
of csrc/sample.hip (deepim_sample_rendered_poses). Where the reference reads poses that the toolkit wrote to disk once, ten per
observed frame, these are drawn when a batch is made: no host random number goes into a pose and nothing is read back.

    pose_rendered, attempts = sample_rendered_poses(pose_observed, K, 640, 480, seed=3, draw_base=first_pair_id)

A pair's pose is a pure function of (seed, draw id, noise, K, frame size, its observed pose): the same wherever the pair lands
in a batch. Differences from the toolkit's loop: a candidate with z <= 0 is rejected (the toolkit divides by z unguarded), at
most `max_attempts` candidates are tried (the toolkit loops for ever), and a pair that exhausts them keeps its observed pose
(attempts == 0, a zero delta).
"""
import ctypes

import numpy as np

from ...runtime import DeviceArray, lib

# toolkit/LM6d_1_gen_rendered_pose.py:54 and :97; max_attempts is where that loop prints its warning (:109)
POSE_NOISE_DEFAULTS = {"angle_std": 15.0, "angle_max": 45.0, "x_std": 0.01, "y_std": 0.01, "z_std": 0.05, "border": 16.0,
                       "max_attempts": 100}
U64 = (1 << 64) - 1


def pose_noise(noise=None):
    """POSE_NOISE_DEFAULTS overridden by `noise` (a dict of some of its keys); unknown keys are refused."""
    out = dict(POSE_NOISE_DEFAULTS)
    if noise:
        unknown = set(noise) - set(out)
        if unknown:
            raise ValueError("pose noise: unknown keys {}".format(sorted(unknown)))
        out.update(noise)
    return out


def noise_array(noise):
    """The five floats the C entries take: angle_std, angle_max (degrees), x_std, y_std, z_std (metres)."""
    return np.array([noise[k] for k in ("angle_std", "angle_max", "x_std", "y_std", "z_std")], dtype=np.float32)


def device_draw_ids(ctx, draw_ids, B):
    """draw_ids (None, a host sequence or a device uint64 array of B ids) as what the C entries take."""
    if draw_ids is None or isinstance(draw_ids, DeviceArray):
        if draw_ids is not None and (draw_ids.dtype != np.uint64 or draw_ids.size != B):
            raise TypeError("draw_ids on the device must be uint64 with %d values" % B)
        return draw_ids
    return ctx.array(np.asarray(draw_ids).reshape(B), dtype=np.uint64)


def sample_rendered_poses(pose_observed, K, width, height, seed, draw_base=0, draw_ids=None, noise=None, with_normals=False):
    """pose_observed: device (B,3,4) float32; K: host 3x3. -> (pose_rendered (B,3,4) float32, attempts (B) int32
    [, normals (B,6) float64: the accepted draw's]), device arrays. Pair b has draw id draw_ids[b] (device uint64 or host
    integers), or draw_base + b without draw_ids. attempts[b] is the number of candidates drawn, 0 where none was accepted
    (pose_rendered[b] is then pose_observed[b])."""
    if not isinstance(pose_observed, DeviceArray) or pose_observed.dtype != np.float32 or pose_observed.shape[1:] != (3, 4):
        raise TypeError("sample_rendered_poses: pose_observed is a device float32 (B,3,4) array")
    ctx = pose_observed.context
    B = pose_observed.shape[0]
    n = pose_noise(noise)
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(3, 3)
    pose, attempts = ctx.empty((B, 3, 4)), ctx.empty((B,), np.int32)
    normals = ctx.empty((B, 6), np.float64) if with_normals else None
    lib.deepim_sample_rendered_poses(ctx.handle, pose, attempts, normals, pose_observed, K, noise_array(n), int(width), int(height),
                                     ctypes.c_float(n["border"]), int(n["max_attempts"]), ctypes.c_ulonglong(int(seed) & U64),
                                     ctypes.c_ulonglong(int(draw_base) & U64), device_draw_ids(ctx, draw_ids, B), B)
    return (pose, attempts, normals) if with_normals else (pose, attempts)
