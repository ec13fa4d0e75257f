"""Synthetic lit observed frames drawn on the device: what toolkit/LM6d_ds_0_gen_observed_poses.py (poses) and
toolkit/LM6d_ds_1_gen_observed.py over lib/render_glumpy/render_py_light.py (frames) write to disk once, 10 000 PNG triples per
class, made when a batch needs them: the object alone at a sampled pose under a random coloured light, on a black background
that lib/utils/image.py:96-155 always replaces (data_syn), as uint8 BGR / uint16 depth / uint8 label frames in the layout the
ingest kernels read. No PNG and no host round trip: every frame is a pure function of (seed, draw id, class).

    stats = observed_pose_stats({class id: training poses (n,3,4)})
    syn = SyntheticObserved(lit_render_machine, stats, K, seed=3)
    out = syn.frames(class_index, draw_ids)             # device arrays, nothing read back
    observed = syn.to_host(class_index, draw_ids)       # the host `observed` dict core/loader.TrainDataLoader takes

`lit_render_machine`: a render machine whose mesh table carries normals (Render_Py_Light, Render_Py_Light_ModelNet_Multi), one
model per class id. The fragment stage is the lit stage of csrc/render.hip, texture * ((1 - r) + r brightness) * intensity;
render_py_light.py:74 has texture * ((1 - r) + r brightness intensity), which differs where an intensity channel is not 1 (a
colour row with a zero channel leaves (1 - r) of the texture there, not black). KNOWN DIFFERENCE, not restated here.
"""
import ctypes

import numpy as np

from ...runtime import DeviceArray, lib
from ..pair_matching.pose_sampler import (BRIGHTNESS_RATIOS, device_draw_ids, pack_observed_table, sample_lights,
                                          sample_observed_poses)

FRAME_KEYS = (("image_observed", np.uint8, (3,)), ("depth_gt_observed", np.uint16, ()), ("mask_gt_observed", np.uint8, ()))


def runs(rows):
    """[(j0, j1, row0)]: the maximal runs rows[j0:j1] = row0, row0 + 1, ... of a host sequence of destination rows."""
    rows = [int(r) for r in rows]
    out, j0 = [], 0
    for j in range(1, len(rows) + 1):
        if j == len(rows) or rows[j] != rows[j - 1] + 1:
            out.append((j0, j, rows[j0]))
            j0 = j
    return out


class SyntheticObserved(object):
    def __init__(self, lit_render_machine, stats, K, seed, border=48, brightness_ratios=BRIGHTNESS_RATIOS, max_attempts=100,
                 depth_factor=1000):
        rm = lit_render_machine
        self.rm, self.ctx = rm, rm.ctx
        self.table_host = rm.mesh_table()
        if self.table_host.normals is None:
            raise ValueError("SyntheticObserved: the render machine's meshes carry no normals; a lit machine is needed")
        self.n_classes = self.table_host.n_classes
        self.stats = stats
        self.pose_table = self.ctx.array(pack_observed_table(stats, self.n_classes), dtype=np.float64)
        self.K = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        self.seed, self.border, self.max_attempts = int(seed), float(border), int(max_attempts)
        self.brightness_ratios = tuple(float(r) for r in brightness_ratios)
        if not 1 <= len(self.brightness_ratios) <= 8:
            raise ValueError("SyntheticObserved: 1 to 8 brightness ratios")
        self.depth_factor = float(depth_factor)
        self.height, self.width = rm.height, rm.width

    def check_classes(self, classes):
        """Host check of class ids a caller will hand to `frames` on the device: inside the table and with statistics."""
        bad = sorted(set(int(c) for c in classes if not (0 <= int(c) < self.n_classes and int(c) in self.stats)))
        if bad:
            raise KeyError("SyntheticObserved: no model or no pose statistics for class ids {}".format(bad))

    def draw_into(self, image, depth, label, class_index, poses, light_offset, light_intensity, brightness_ratio, rows=None,
                  label_value=None):
        """deepim_render_observed_forward: sample b of the device arrays class_index / poses / lights into row rows[b] (device
        int32, None = b) of image (N,H,W,3) uint8, depth (N,H,W) uint16, label (N,H,W) uint8."""
        t, rm = self.table_host, self.rm
        N, B = image.shape[0], class_index.size
        if image.dtype != np.uint8 or depth.dtype != np.uint16 or label.dtype != np.uint8:
            raise TypeError("draw_into: image / depth / label are uint8 / uint16 / uint8 device arrays")
        if image.shape != (N, self.height, self.width, 3) or depth.shape != (N, self.height, self.width) or label.shape != depth.shape:
            raise ValueError("draw_into: outputs must be (N,%d,%d,3), (N,%d,%d), (N,%d,%d)" % ((self.height, self.width) * 3))
        lib.deepim_render_observed_forward(self.ctx.handle, image, depth, label, rows, N, label_value, ctypes.c_float(self.depth_factor),
                                           class_index, t.mesh_desc, t.n_classes, t.max_V, t.max_F, t.vertices, t.vertex_attr,
                                           t.normals, t.faces, t.textures, poses, self.K, light_offset, light_intensity,
                                           brightness_ratio, B, self.height, self.width, ctypes.c_float(rm.zNear),
                                           ctypes.c_float(rm.zFar))

    def frames(self, class_index, draw_ids, out=None, rows=None, rows_device=None):
        """class_index: device int32 (B) or host ids; draw_ids: device uint64 (B) or host integers. -> dict of device arrays:
        image_observed (N,H,W,3) uint8 BGR, depth_gt_observed (N,H,W) uint16, mask_gt_observed (N,H,W) uint8 (1 on the object),
        pose_observed, attempts (B) int32 (pose_sampler.sample_observed_poses), light_offset, light_intensity (B,3),
        brightness_ratio (B). Two sampler launches and the draw's launch group (project, raster, resolve); nothing is read back.

        `out` + `rows`: out = {"image_observed", "depth_gt_observed", "mask_gt_observed" [, "pose_observed" (N,3,4)]} are a
        batch's own arrays of N >= B rows and sample b goes to row rows[b] (a HOST sequence: the caller planned the batch);
        the other rows are not touched. The frames are written in place by the draw; the poses are placed by one device copy
        per run of consecutive rows. The returned dict holds `out`'s arrays, pose_observed included when it was given (else the
        compact (B,3,4) one). `rows_device`: `rows` as a device int32 (B) array the caller already holds, instead of an upload."""
        ctx = self.ctx
        if not isinstance(class_index, DeviceArray):
            class_index = ctx.array(np.asarray(class_index).reshape(-1), dtype=np.int32)
        B = class_index.size
        draw_ids = device_draw_ids(ctx, draw_ids, B)
        if draw_ids is None:
            raise ValueError("frames: draw_ids are required")
        pose, attempts = sample_observed_poses(class_index, self.pose_table, self.K, self.width, self.height, self.seed,
                                               draw_ids=draw_ids, border=self.border, max_attempts=self.max_attempts)
        off, inten, ratio = sample_lights(ctx, B, self.seed, draw_ids=draw_ids, brightness_ratios=self.brightness_ratios)
        if out is None:
            if rows is not None:
                raise ValueError("frames: rows needs out")
            out = {k: ctx.empty((B, self.height, self.width) + inner, dt) for k, dt, inner in FRAME_KEYS}
            rows_dev = None
        else:
            rows = np.arange(B) if rows is None else np.asarray(rows, np.int64).reshape(B)
            N = out["image_observed"].shape[0]
            if B and (rows.min() < 0 or rows.max() >= N or len(set(rows.tolist())) != B):
                raise ValueError("frames: rows must be distinct and inside [0, %d)" % N)
            rows_dev = ctx.array(rows, dtype=np.int32) if rows_device is None else rows_device
        self.draw_into(out["image_observed"], out["depth_gt_observed"], out["mask_gt_observed"], class_index, pose, off, inten,
                       ratio, rows=rows_dev)
        res = {k: out[k] for k, _dt, _inner in FRAME_KEYS}
        res["pose_observed"] = pose
        if out.get("pose_observed") is not None:
            for j0, j1, r0 in runs(rows):
                out["pose_observed"][r0:r0 + (j1 - j0)].copyfrom(pose[j0:j1])
            res["pose_observed"] = out["pose_observed"]
        res.update(attempts=attempts, light_offset=off, light_intensity=inten, brightness_ratio=ratio, class_index=class_index)
        return res

    def to_host(self, class_index, draw_ids):
        """A fixed synthetic set as the host `observed` dict TrainDataLoader takes: the frames of `frames`, depth_observed a copy
        of the depth, mask_idx 1. Hand the loader data_syn = all True with it, so every frame gets a pool background."""
        cls = np.asarray(class_index).astype(np.int32).reshape(-1)
        self.check_classes(cls)
        f = self.frames(cls, draw_ids)
        depth = f["depth_gt_observed"].asnumpy()
        return {"image_observed": f["image_observed"].asnumpy(), "depth_gt_observed": depth, "depth_observed": depth.copy(),
                "mask_gt_observed": f["mask_gt_observed"].asnumpy(), "mask_idx": np.ones(len(cls), np.int32),
                "pose_observed": f["pose_observed"].asnumpy(), "class_index": cls}
