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


# ---- synthetic observed poses: toolkit/LM6d_ds_0_gen_observed_poses.py ------------------------------------------------------
OBSERVED_TABLE_COLUMNS = 22      # trans_mean[3], trans_std[3], pz_mean[3], angle_max (degrees), fallback pose [12]
BRIGHTNESS_RATIOS = (0.2, 0.25, 0.3, 0.35, 0.4)      # toolkit/LM6d_ds_1_gen_observed.py:86


def _angle(u, v):
    """LM6d_ds_0_gen_observed_poses.py:74-78."""
    c = np.dot(u, v) / (np.linalg.norm(u) * np.linalg.norm(v))
    return np.arccos(np.clip(c, -1, 1)) / np.pi * 180


def observed_pose_stats(poses_by_class):
    """stat_poses() of LM6d_ds_0_gen_observed_poses.py:81-180 in float64 numpy, no device needed. poses_by_class: {class id:
    (n,3,4) training poses} -> {class id: dict(trans_mean (3), trans_std (3) (np.std: population), pz_mean (3) = the mean of
    R e_z, angle_max = the largest angle in degrees of any training pose's R e_z to pz_mean, fallback (3,4) = the training pose
    whose R e_z is closest to pz_mean (what an exhausted draw falls back to; the toolkit loops for ever instead))}."""
    out = {}
    for c, poses in poses_by_class.items():
        poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
        if len(poses) == 0:
            raise ValueError("observed_pose_stats: class {} has no poses".format(c))
        pz = np.dot(poses[:, :, :3], np.array([0.0, 0.0, 1.0]))
        pz_mean = np.mean(pz, 0)
        deg = np.array([_angle(pz_mean, p) for p in pz])
        out[c] = {"trans_mean": np.mean(poses[:, :, 3], 0), "trans_std": np.std(poses[:, :, 3], 0), "pz_mean": pz_mean,
                  "angle_max": float(np.max(deg)), "fallback": poses[int(np.argmin(deg))].copy()}
    return out


def pack_observed_table(stats, n_classes=None):
    """The device table of deepim_sample_observed_poses: (n_classes, 22) float64, row c = stats[c] (trans_mean, trans_std,
    pz_mean, angle_max, fallback rounded to float32). A class without stats gets angle_max = -1 and a zero fallback: every
    candidate is rejected and its pairs come out exhausted, on a zero pose."""
    n = (max(stats) + 1) if n_classes is None else int(n_classes)
    table = np.zeros((n, OBSERVED_TABLE_COLUMNS), np.float64)
    table[:, 9] = -1.0
    for c, s in stats.items():
        if not 0 <= int(c) < n:
            raise ValueError("pack_observed_table: class id {} outside [0, {})".format(c, n))
        if np.any(np.asarray(s["trans_std"], np.float64) < 0):
            raise ValueError("pack_observed_table: trans_std must be >= 0")
        table[int(c)] = np.concatenate([np.asarray(s["trans_mean"], np.float64).reshape(3), np.asarray(s["trans_std"], np.float64).reshape(3),
                                        np.asarray(s["pz_mean"], np.float64).reshape(3), [float(s["angle_max"])],
                                        np.asarray(s["fallback"], np.float32).astype(np.float64).reshape(12)])
    return table


def sample_observed_poses(class_index, table, K, width, height, seed, draw_base=0, draw_ids=None, border=48.0, max_attempts=100,
                          with_normals=False, with_stat=False):
    """class_index: device (B) int32; table: device (n_classes,22) float64 (pack_observed_table); K: host 3x3.
    -> (pose_observed (B,3,4) float32, attempts (B) int32 [, normals (B,7) float64] [, stat (B,4) float64]), device arrays.
    attempts[b]: the candidates drawn; 0 = none accepted (the pose is the class's fallback); -1 = class id outside the table (a
    zero pose, which the render machine draws as an empty frame). deepim_sample_stats_accumulate counts a pair with attempts
    == 0 as exhausted and adds the values as they are, so callers that feed it keep -1 out: core/loader.TrainDataLoader checks
    its synthetic_classes against the table on the host when it is built, and no pair of its batches can carry -1."""
    if not isinstance(class_index, DeviceArray) or class_index.dtype != np.int32:
        raise TypeError("sample_observed_poses: class_index is a device int32 array")
    if not isinstance(table, DeviceArray) or table.dtype != np.float64 or table.ndim != 2 or table.shape[1] != OBSERVED_TABLE_COLUMNS:
        raise TypeError("sample_observed_poses: table is a device float64 (n_classes,22) array")
    ctx, B = class_index.context, class_index.size
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(3, 3)
    pose, attempts = ctx.empty((B, 3, 4)), ctx.empty((B,), np.int32)
    normals = ctx.empty((B, 7), np.float64) if with_normals else None
    stat = ctx.empty((B, 4), np.float64) if with_stat else None
    lib.deepim_sample_observed_poses(ctx.handle, pose, attempts, normals, stat, class_index, table, table.shape[0], K, int(width),
                                     int(height), ctypes.c_float(border), int(max_attempts), ctypes.c_ulonglong(int(seed) & U64),
                                     ctypes.c_ulonglong(int(draw_base) & U64), device_draw_ids(ctx, draw_ids, B), B)
    return (pose, attempts) + ((normals,) if with_normals else ()) + ((stat,) if with_stat else ())


def sample_lights(ctx, B, seed, draw_base=0, draw_ids=None, brightness_ratios=BRIGHTNESS_RATIOS):
    """The light of LM6d_ds_1_gen_observed.py:116-144 for B pairs -> device float32 (light_offset (B,3), light_intensity (B,3),
    brightness_ratio (B)): the offset is 0.5 x row (draw id mod 6) of the file's six positions, the intensity one of its seven
    colour rows times U(0.9, 1.1) per channel, the ratio one of `brightness_ratios` (at most 8)."""
    ratios = np.ascontiguousarray(brightness_ratios, np.float32).reshape(-1)
    offset, intensity, ratio = ctx.empty((B, 3)), ctx.empty((B, 3)), ctx.empty((B,))
    lib.deepim_sample_lights(ctx.handle, offset, intensity, ratio, ratios, len(ratios), ctypes.c_ulonglong(int(seed) & U64),
                             ctypes.c_ulonglong(int(draw_base) & U64), device_draw_ids(ctx, draw_ids, B), B)
    return offset, intensity, ratio


# ---- occluders of a synthetic scene: ours, the reference has no generator for occluded scenes -------------------------------
MAX_SLOTS = 8        # deepim_render_scene_forward: the target and at most seven occluders share a z-buffer plane


def sample_occluders(class_index, pose, occluder_classes, diameters, seed, draw_base=0, draw_ids=None, min_occluders=0,
                     max_occluders=2, lateral=(0.2, 0.9), toward=(0.5, 1.5)):
    """deepim_sample_occluders. class_index: device (B) int32 and pose: device (B,3,4) float32, the targets; occluder_classes:
    device int32 list of class ids; diameters: device float32 (n_classes) in metres, indexed by class id.
    -> device (class (B,S) int32, pose (B,S,3,4) float32, label_value (B,S) int32 = s + 1), S = max_occluders + 1. Slot 0 is the
    target. Stream 7 of the pair's draw id gives the count n in [min_occluders, max_occluders] (attempt 0) and, for slot s = 1..n
    (attempt s), the class out of the list and the translation t_target + d (rho cos phi, rho sin phi, -tau) with rho in
    `lateral`, tau in `toward` (both in diameters d of the target's class) and phi in [0, 2 pi); stream 8, attempt s gives the
    rotation (four normals as a unit quaternion). Slots beyond n, and an occluder behind the camera, are empty: class -1."""
    for a, dt in ((class_index, np.int32), (pose, np.float32), (occluder_classes, np.int32), (diameters, np.float32)):
        if not isinstance(a, DeviceArray) or a.dtype != dt:
            raise TypeError("sample_occluders: class_index / occluder_classes are device int32, pose / diameters device float32 arrays")
    ctx, B, S = class_index.context, class_index.size, int(max_occluders) + 1
    cls, out, label = ctx.empty((B, S), np.int32), ctx.empty((B, S, 3, 4)), ctx.empty((B, S), np.int32)
    cf = ctypes.c_float
    lib.deepim_sample_occluders(ctx.handle, cls, out, label, class_index, pose, occluder_classes, occluder_classes.size, diameters,
                                diameters.size, int(min_occluders), int(max_occluders), cf(lateral[0]), cf(lateral[1]), cf(toward[0]),
                                cf(toward[1]), ctypes.c_ulonglong(int(seed) & U64), ctypes.c_ulonglong(int(draw_base) & U64),
                                device_draw_ids(ctx, draw_ids, B), B)
    return cls, out, label
