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

    syn = SyntheticObserved(lit_render_machine, stats, K, seed=3, occluders=OccluderSpec([0, 1], {0: 0.1, 1: 0.12}))

With `occluders` the object is no longer alone: up to max_occluders other objects are drawn into the same frame in front of, beside
and behind it (deepim_sample_occluders, streams 7 and 8 of the draw id; deepim_render_scene_forward, one z-buffer plane for all
slots of a frame). The reference has no generator for such scenes, so the rule is ours; three points of it are the reference's:
    one light per scene, moved to each object's own pose      lib/render_glumpy/render_py_light_multi_program.py:370-396
    a target left with less than min_visible = 0.4 of its pixels falls back to the unoccluded frame      lib/utils/mask_augment.py:91-93
    the label map shows the visible part of the target only (label 1 = mask_idx; occluder slot s carries s + 1), while
    depth_gt_observed stays the target drawn alone, which the flow labels and point clouds are made from      lib/utils/image.py:253-261
"""
import ctypes

import numpy as np

from ...runtime import DeviceArray, lib
from ..pair_matching.pose_sampler import (BRIGHTNESS_RATIOS, MAX_SLOTS, device_draw_ids, pack_observed_table, sample_lights,
                                          sample_observed_poses, sample_occluders)

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


def _range(name, value):
    try:
        lo, hi = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError("OccluderSpec: %s must be a (lo, hi) pair" % name)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError("OccluderSpec: %s must be finite with lo <= hi, got (%r, %r)" % (name, lo, hi))
    return lo, hi


class OccluderSpec(object):
    """What SyntheticObserved draws around its target. Pure host: everything the device cannot report is checked here.

    classes: the class ids an occluder is drawn from (it may be the target's own class); diameters: {class id: metres} (or a
    sequence indexed by class id) with an entry for every class of `classes` and for every class a target may have; the count of
    occluders is uniform in [min_occluders, max_occluders] and max_occluders + 1 slots share a frame (at most 8). An occluder sits
    at t_target + d (rho cos phi, rho sin phi, -tau), d the target's diameter, rho in `lateral`, tau in `toward`, phi in [0, 2 pi).
    A pair whose target keeps less than `min_visible` of its pixels falls back to the unoccluded frame.

    The defaults are design values, not measurements: up to two occluders whose centres lie 0.2 to 0.9 diameters beside the
    target's and 0.5 to 1.5 diameters nearer the camera. min_visible = 0.4 is lib/utils/mask_augment.py:91."""

    def __init__(self, classes, diameters, max_occluders=2, min_occluders=0, lateral=(0.2, 0.9), toward=(0.5, 1.5), min_visible=0.4):
        self.max_occluders, self.min_occluders = int(max_occluders), int(min_occluders)
        if self.max_occluders != max_occluders or self.min_occluders != min_occluders:
            raise ValueError("OccluderSpec: min_occluders and max_occluders are whole numbers")
        if not 0 <= self.min_occluders <= self.max_occluders:
            raise ValueError("OccluderSpec: need 0 <= min_occluders <= max_occluders, got %d, %d" % (self.min_occluders, self.max_occluders))
        if self.max_occluders + 1 > MAX_SLOTS:
            raise ValueError("OccluderSpec: the target and %d occluders are %d slots; a frame has at most %d"
                             % (self.max_occluders, self.max_occluders + 1, MAX_SLOTS))
        self.classes = tuple(int(c) for c in classes)
        if any(c < 0 or c != c0 for c, c0 in zip(self.classes, classes)):
            raise ValueError("OccluderSpec: classes are class ids >= 0")
        if self.max_occluders and not self.classes:
            raise ValueError("OccluderSpec: classes is empty")
        items = diameters.items() if hasattr(diameters, "items") else enumerate(diameters)
        self.diameters = {int(c): float(d) for c, d in items}
        for c, d in self.diameters.items():
            if c < 0 or not (np.isfinite(d) and d > 0):
                raise ValueError("OccluderSpec: the diameter of class %d must be a positive length in metres, got %r" % (c, d))
        missing = sorted(set(self.classes) - set(self.diameters))
        if missing:
            raise KeyError("OccluderSpec: no diameter for class ids {}".format(missing))
        self.lateral, self.toward = _range("lateral", lateral), _range("toward", toward)
        if self.lateral[0] < 0:
            raise ValueError("OccluderSpec: lateral is a distance from the target's axis, >= 0")
        self.min_visible = float(min_visible)
        if not 0.0 <= self.min_visible <= 1.0:
            raise ValueError("OccluderSpec: min_visible must lie in [0, 1], got %r" % (min_visible,))

    @property
    def slots(self):
        """S: the target and max_occluders occluder slots."""
        return self.max_occluders + 1

    def diameter_table(self, n_classes):
        """(n_classes) float32 indexed by class id, 0 where no diameter is known."""
        out = np.zeros(int(n_classes), np.float32)
        for c, d in self.diameters.items():
            if c < n_classes:
                out[c] = d
        return out


class SyntheticObserved(object):
    def __init__(self, lit_render_machine, stats, K, seed, border=48, brightness_ratios=BRIGHTNESS_RATIOS, max_attempts=100,
                 depth_factor=1000, occluders=None):
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
        self.occluders = occluders
        self._alone = None          # the targets drawn alone: B compact rows, grown outside a capture only
        if occluders is not None:
            if not isinstance(occluders, OccluderSpec):
                raise TypeError("SyntheticObserved: occluders is an OccluderSpec")
            bad = sorted(set(c for c in occluders.classes if c >= self.n_classes))
            if bad:
                raise KeyError("SyntheticObserved: no model for occluder class ids {}".format(bad))
            self.occluder_classes = self.ctx.array(np.asarray(occluders.classes, np.int32).reshape(-1), dtype=np.int32)
            self.diameters = self.ctx.array(occluders.diameter_table(self.n_classes))

    def check_classes(self, classes):
        """Host check of class ids a caller will hand to `frames` on the device: inside the table and with statistics; with
        occluders also with a diameter, and the occluder list inside the table."""
        bad = sorted(set(int(c) for c in classes if not (0 <= int(c) < self.n_classes and int(c) in self.stats)))
        if bad:
            raise KeyError("SyntheticObserved: no model or no pose statistics for class ids {}".format(bad))
        if self.occluders is not None:
            bad = sorted(set(int(c) for c in classes if int(c) not in self.occluders.diameters) |
                         set(c for c in self.occluders.classes if c >= self.n_classes))
            if bad:
                raise KeyError("SyntheticObserved: no diameter or no model for class ids {}".format(bad))

    def scene_into(self, image, depth, label, class_index, poses, light_offset, light_intensity, brightness_ratio, slots, rows=None,
                   label_value=None, visible=None):
        """deepim_render_scene_forward: frame f of B = class_index.size / slots, its `slots` slots sharing one z-buffer plane, into
        row rows[f] (device int32, None = f) of image / depth / label; visible: device int32 (B,slots) or None."""
        t, rm = self.table_host, self.rm
        N, B = image.shape[0], class_index.size // int(slots)
        lib.deepim_render_scene_forward(self.ctx.handle, image, depth, label, visible, rows, N, label_value, ctypes.c_float(self.depth_factor),
                                        class_index, t.mesh_desc, t.n_classes, t.max_V, t.max_F, t.vertices, t.vertex_attr, t.normals,
                                        t.faces, t.textures, poses, self.K, light_offset, light_intensity, brightness_ratio, B,
                                        int(slots), self.height, self.width, ctypes.c_float(rm.zNear), ctypes.c_float(rm.zFar))

    def _occluded(self, out, rows_dev, class_index, draw_ids, pose, off, inten, ratio, totals):
        """Steps 2-5 of an occluded batch: the occluder draw, the targets alone (S = 1) into the object's scratch, the scene into
        the batch rows and the gate. -> the extra keys of `frames`."""
        ctx, spec, B = self.ctx, self.occluders, class_index.size
        S = spec.slots
        cls, poses, label_value = sample_occluders(class_index, pose, self.occluder_classes, self.diameters, self.seed, draw_ids=draw_ids,
                                                   min_occluders=spec.min_occluders, max_occluders=spec.max_occluders,
                                                   lateral=spec.lateral, toward=spec.toward)
        if self._alone is None or self._alone[0].shape[0] < B:
            self._alone = [ctx.empty((B, self.height, self.width) + inner, dt) for _k, dt, inner in FRAME_KEYS]
        alone = [a[:B] for a in self._alone]
        full, visible, kept = ctx.empty((B,), np.int32), ctx.empty((B, S), np.int32), ctx.empty((B,), np.int32)
        self.scene_into(alone[0], alone[1], alone[2], class_index, pose, off, inten, ratio, 1, visible=full)
        scene_depth = out.get("depth_observed")
        if scene_depth is None:         # nobody asked for the camera's depth: the scene's goes where the gate puts the target's
            scene_depth = out["depth_gt_observed"]
        self.scene_into(out["image_observed"], scene_depth, out["mask_gt_observed"], cls, poses, off, inten, ratio, S, rows=rows_dev,
                        label_value=label_value, visible=visible)
        lib.deepim_occlusion_gate(ctx.handle, out["image_observed"], out["depth_gt_observed"], out["mask_gt_observed"],
                                  out.get("depth_observed"), kept, totals, rows_dev, out["image_observed"].shape[0], alone[0], alone[1],
                                  alone[2], visible, full, cls, ctypes.c_float(spec.min_visible), B, S, self.height, self.width)
        return dict(depth_observed=out.get("depth_observed"), kept=kept, visible=visible, full=full, occluder_class=cls,
                    occluder_pose=poses)

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

    def frames(self, class_index, draw_ids, out=None, rows=None, rows_device=None, totals=None):
        """class_index: device int32 (B) or host ids; draw_ids: device uint64 (B) or host integers. -> dict of device arrays:
        image_observed (N,H,W,3) uint8 BGR, depth_gt_observed (N,H,W) uint16, mask_gt_observed (N,H,W) uint8 (1 on the object),
        pose_observed, attempts (B) int32 (pose_sampler.sample_observed_poses), light_offset, light_intensity (B,3),
        brightness_ratio (B). Two sampler launches and the draw's launch group (project, raster, resolve); nothing is read back.

        `out` + `rows`: out = {"image_observed", "depth_gt_observed", "mask_gt_observed" [, "pose_observed" (N,3,4)]} are a
        batch's own arrays of N >= B rows and sample b goes to row rows[b] (a HOST sequence: the caller planned the batch);
        the other rows are not touched. The frames are written in place by the draw; the poses are placed by one device copy
        per run of consecutive rows. The returned dict holds `out`'s arrays, pose_observed included when it was given (else the
        compact (B,3,4) one). `rows_device`: `rows` as a device int32 (B) array the caller already holds, instead of an upload.

        With `occluders` the chain is: the pose and light draws as above; the occluder draw (deepim_sample_occluders); the target
        alone through the scene entry with S = 1 into a scratch of B rows the object owns (grown outside a capture only), which
        also counts its pixels; the scene into the batch rows; the gate (deepim_occlusion_gate). More keys come back:
        depth_observed (N,H,W) uint16, the scene's depth, occluders included, as a camera would measure it (out["depth_observed"]
        when `out` carries one, a fresh array without `out`, None when `out` has none: the scene's depth is then not kept);
        kept (B) int32; visible (B,S) int32; full (B) int32; occluder_class (B,S) int32 (slot 0 the target, -1 an empty slot);
        occluder_pose (B,S,3,4). depth_gt_observed stays the target drawn alone; the label map holds 1 on the visible part of the
        target (mask_idx stays 1) and s + 1 on occluder slot s. `totals`: 3 device uint64 the gate adds to (pairs, pairs kept,
        occluder slots drawn), or None."""
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
            if self.occluders is not None:
                out["depth_observed"] = ctx.empty((B, self.height, self.width), np.uint16)
            rows_dev = None
        else:
            rows = np.arange(B) if rows is None else np.asarray(rows, np.int64).reshape(B)
            N = out["image_observed"].shape[0]
            if B and (rows.min() < 0 or rows.max() >= N or len(set(rows.tolist())) != B):
                raise ValueError("frames: rows must be distinct and inside [0, %d)" % N)
            rows_dev = ctx.array(rows, dtype=np.int32) if rows_device is None else rows_device
        extra = {}
        if self.occluders is None:
            self.draw_into(out["image_observed"], out["depth_gt_observed"], out["mask_gt_observed"], class_index, pose, off, inten,
                           ratio, rows=rows_dev)
        elif B:
            extra = self._occluded(out, rows_dev, class_index, draw_ids, pose, off, inten, ratio, totals)
        res = {k: out[k] for k, _dt, _inner in FRAME_KEYS}
        res.update(extra)
        res["pose_observed"] = pose
        if out.get("pose_observed") is not None:
            for j0, j1, r0 in runs(rows):
                out["pose_observed"][r0:r0 + (j1 - j0)].copyfrom(pose[j0:j1])
            res["pose_observed"] = out["pose_observed"]
        res.update(attempts=attempts, light_offset=off, light_intensity=inten, brightness_ratio=ratio, class_index=class_index)
        return res

    def to_host(self, class_index, draw_ids):
        """A fixed synthetic set as the host `observed` dict TrainDataLoader takes: the frames of `frames`, depth_observed a copy
        of the depth (with occluders: the scene's depth), mask_idx 1. Hand the loader data_syn = all True with it, so every frame
        gets a pool background."""
        cls = np.asarray(class_index).astype(np.int32).reshape(-1)
        self.check_classes(cls)
        f = self.frames(cls, draw_ids)
        depth = f["depth_gt_observed"].asnumpy()
        seen = f["depth_observed"].asnumpy() if f.get("depth_observed") is not None else depth.copy()
        return {"image_observed": f["image_observed"].asnumpy(), "depth_gt_observed": depth, "depth_observed": seen,
                "mask_gt_observed": f["mask_gt_observed"].asnumpy(), "mask_idx": np.ones(len(cls), np.int32),
                "pose_observed": f["pose_observed"].asnumpy(), "class_index": cls}
