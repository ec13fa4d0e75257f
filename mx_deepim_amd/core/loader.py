"""The data iterators of deepim/core/loader.py. TestDataLoader (:17-108), which draws every pair's initial pose as decoded
frames on the device, is at the end of this file with its own description; first

The training iterator: TrainDataLoader (deepim/core/loader.py:111-262) over the device's own random draws.

The reference's loader reads, for every observed frame, ten rendered images and poses that toolkit/LM6d_1_gen_rendered_pose.py
and LM6d_2_gen_rendered.py wrote to disk once. This one needs no such dataset: it takes the observed frames and their
ground-truth poses, DRAWS the rendered pose of every pair on the device (lib/pair_matching/pose_sampler.py, csrc/sample.hip),
renders it with the device render machine and makes the labels with lib/pair_matching/data_pair.get_data_pair_train_batch.
Every epoch sees fresh initial poses, no host random number goes into a pose, and nothing is read back inside an epoch.

    loader = TrainDataLoader(observed, config, render_machine, batch_size=4, shuffle=True, seed=3, points=points)
    MutableModule(config, net).fit(loader, ..., updater=batchUpdaterPyMulti(config, H, W, render_machine=render_machine))

`observed`: host numpy arrays for the whole set of M frames, as the decoder left them (lib/utils/image.py):
    image_observed (M,H,W,3) uint8 BGR     depth_gt_observed (M,H,W) uint16     mask_gt_observed (M,H,W) uint8 label maps
    mask_idx (M)     pose_observed (M,3,4) float32     class_index (M)     depth_observed (M,H,W) uint16 with network.INPUT_DEPTH
`points`: {class id: ((3,N) model points, (3,N) weights)} for train_iter.SE3_PM_LOSS, the N points already sampled.

An epoch is the M·R pairs p = m·R + r (R = num_rendered_per_observed), in order or, with `shuffle`, in a permutation drawn from
the loader's own RandomState(seed) at every reset(); a trailing partial batch is dropped, as the reference's iter_next does.
Pair p of epoch e has draw id e·M·R + p wherever the shuffle puts it, so its pose (and its mask-dilate draw) depends on
(seed, e, p) alone. The rendered side is the unquantised float render the batch updater produces between iterations, not the
8-bit / 16-bit files of the reference.

`backgrounds`: a lib/utils/background.BackgroundPool built for the frames' (H, W), or None. With it the observed image gets the
background replacement of image.py:96-155 on the device: the frames flagged in `data_syn` ((M) bool, optional) always, the
others with probability TRAIN.REPLACE_OBSERVED_BG_RATIO, on a pool image chosen by the pair's own draw (stream 3 of its draw
id), cropped, resized and composited by one kernel (deepim_ingest_bgr8_pool). Like the pose, the background of pair p in epoch
e depends on (seed, e, p) alone. Without it every batch is what it was before backgrounds existed.

`synthetic`: a lib/utils/synthetic_observed.SyntheticObserved built for the frames' (H, W), or None. With it an epoch is the M·R
real pairs plus `num_synthetic` fresh synthetic ones (LM6D_REFINE_SYN.py: data_syn = True, mask_idx = 1): n = M·R + S pairs,
pair p >= M·R being synthetic pair s = p − M·R of class synthetic_classes[s mod len(synthetic_classes)] (default: the classes of
the observed set, in order). Every pair, real or synthetic, has draw id e·n + p. A synthetic pair's observed pose and light are
drawn (streams 4-6 of that draw id under the generator's own seed) and its frame is rendered on the device straight into the batch's uint8 / uint16 arrays (deepim_render_observed_forward
through `rows`), next to the uploaded real rows; its rendered pose is then drawn around that observed pose like any other pair's
(streams 0/1 of the same draw id). It counts as data_syn: with a pool it always gets a pool background. Its depth_observed is
its own depth and its mask_idx 1. The synthetic classes are checked against the generator's tables here, on the host, so no
pair can come out with attempts = −1 and the observed attempts feed deepim_sample_stats_accumulate as they are. Without
`synthetic` every batch, draw id and byte is what it is without the argument.

A `synthetic` built with occluders (SyntheticObserved(..., occluders=OccluderSpec(...))) puts up to max_occluders other objects
into a synthetic pair's frame (streams 7 and 8 of its draw id). The plan, the draw ids and the real rows do not change. The
pair's label map shows the visible part of the target only (mask_idx stays 1), its depth_gt_observed stays the target drawn
alone, and with network.INPUT_DEPTH its depth_observed is the scene's depth, occluders included. A pair whose target keeps less
than min_visible of its pixels falls back to today's unoccluded frame. stats() then also counts the pairs gated, kept and the
occluder slots drawn.

`observed` = core/resident.ResidentObserved(observed, ctx, spare_rows=batch_size, points=points): the set uploaded once. The
plan, the draw ids, the seeds and every refusal are the same and so is every byte of every batch, but a batch is made from
indices alone: frame_index (B int32), the draw ids (B uint64) and, with synthetic pairs, their positions and class ids go up;
image_observed is read in place by deepim_ingest_bgr8_frames (_pool_frames with `backgrounds`), the depth and label maps by the
deepim_ingest_*_frames entries, and pose_observed, mask_idx, class_index, the data_syn flags and the point clouds are rows
of resident tables gathered by deepim_gather_rows. The synthetic pair at batch position b is drawn into spare row M + b of the
set (resident.batch_rows), which the loader claims when it is built: safe on one stream, since batch k's ingest is queued
before batch k+1's draw and a batch keeps fp32 copies only. A dict holding a DeviceArray is still refused.

Not part of this loader and refused: ready-made backgrounds (bg_image: the pool is the loader's way), TRAIN.MASK_SYN, resizing (a frame that is not config.SCALES[0]),
shared-frame batches (frame_index), more than one target per synthetic frame, and a synthetic set kept across epochs (SyntheticObserved.to_host makes a fixed one for the `observed` argument).
"""
import numpy as np

from ..cameras import camera_table, has_cameras
from ..lib.pair_matching import data_pair
from ..lib.pair_matching.pose_sampler import pose_noise, sample_rendered_poses
from ..lib.utils import image as _image
from ..lib.utils.background import background_draws_device
from ..lib.utils.mask_dilate import mask_dilate_draws_device
from ..lib.utils.synthetic_observed import runs
from ..runtime import DeviceArray, lib
from .resident import ResidentObserved, batch_rows          # noqa: F401 (re-exported: the set both loaders take)

_DTYPES = {"image_observed": np.uint8, "depth_gt_observed": np.uint16, "mask_gt_observed": np.uint8, "depth_observed": np.uint16}


def epoch_plan(M, R, batch_size, shuffle, rng, epoch, num_synthetic=0):
    """The batches of one epoch over M observed frames with R rendered poses each, no device needed →
    (pairs (n_batches, batch_size) int64, draw_ids (n_batches, batch_size) uint64, dropped).
    pairs holds p = m·R + r in epoch order: arange(M·R), or rng.permutation(M·R) with `shuffle` (rng: a RandomState, consumed
    once per call); the trailing M·R mod batch_size pairs are dropped. draw_ids = epoch·M·R + pairs.
    With num_synthetic = S > 0 the epoch has n = M·R + S pairs, p >= M·R being synthetic pair p − M·R, and n stands for M·R
    in the order, the drop and the draw ids."""
    M, R, batch_size, epoch, S = int(M), int(R), int(batch_size), int(epoch), int(num_synthetic)
    if M < 1 or R < 1 or batch_size < 1 or epoch < 0 or S < 0:
        raise ValueError("epoch_plan: M, R, batch_size must be >= 1 and epoch, num_synthetic >= 0")
    n = M * R + S
    order = rng.permutation(n).astype(np.int64) if shuffle else np.arange(n, dtype=np.int64)
    n_batches = n // batch_size
    pairs = order[:n_batches * batch_size].reshape(n_batches, batch_size)
    return pairs, (pairs + epoch * n).astype(np.uint64), n - n_batches * batch_size


class TrainDataLoader(object):
    def __init__(self, observed, config, render_machine, batch_size=1, shuffle=False, seed=0, num_rendered_per_observed=1,
                 points=None, noise=None, backgrounds=None, data_syn=None, synthetic=None, num_synthetic=0, synthetic_classes=None):
        self.config, self.render_machine, self.ctx = config, render_machine, render_machine.ctx
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        self.R = int(num_rendered_per_observed)
        self.noise = pose_noise(noise)
        self.resident = res = observed if isinstance(observed, ResidentObserved) else None
        if res is not None:        # the host side of the set: its small tables; the frames stay on the device
            if res.ctx is not self.ctx:
                raise ValueError("TrainDataLoader: the resident set lives on another context")
            for k in ("pose_observed", "mask_idx", "class_index"):
                if k not in res.host_tables:
                    raise KeyError("TrainDataLoader: the resident set was built without '%s'" % k)
            observed = dict(res.host_tables)
            if data_syn is None:
                data_syn = observed.get("data_syn")
        for k, v in observed.items():
            if isinstance(v, DeviceArray):
                raise TypeError("TrainDataLoader: observed['%s'] is a device array; the dataset is host numpy arrays (a batch is "
                                "gathered on the host and uploaded) or a ResidentObserved" % k)
        if observed.get("bg_image") is not None:
            raise NotImplementedError("TrainDataLoader: ready-made backgrounds (bg_image) are not part of this loader; pass "
                                      "backgrounds=BackgroundPool(...) and they are drawn, cropped and resized on the device")
        if observed.get("frame_index") is not None:
            raise NotImplementedError("TrainDataLoader: shared frames (frame_index) are a test-phase input; the training loader is "
                                      "per pair")
        if config.TRAIN.get("MASK_SYN", False):
            raise NotImplementedError("TrainDataLoader: TRAIN.MASK_SYN (image.py:205-206) is not part of the device path")
        n = config.network
        self.keys = ["image_observed", "depth_gt_observed", "mask_gt_observed"] + (["depth_observed"] if n.INPUT_DEPTH else [])
        self.observed = {}
        for k in self.keys:
            if res is not None:             # dtypes, shapes and equal M were checked when the set was built
                if k not in res.arrays:
                    raise KeyError("TrainDataLoader: the resident set holds no '%s'" % k)
                continue
            if observed.get(k) is None:
                raise KeyError("TrainDataLoader: observed carries no '%s'" % k)
            v = np.asarray(observed[k])
            if v.dtype != np.dtype(_DTYPES[k]):
                raise TypeError("observed['%s'] is %s; the decoded %s frame is expected" % (k, v.dtype, np.dtype(_DTYPES[k])))
            self.observed[k] = v
        if res is not None:
            self.M, H, W = res.M, res.height, res.width
        else:
            img = self.observed["image_observed"]
            if img.ndim != 4 or img.shape[3] != 3:
                raise ValueError("observed['image_observed'] has shape %s; (M,H,W,3) expected" % (img.shape,))
            self.M, H, W = img.shape[0], img.shape[1], img.shape[2]
        _image._check_size(config, H, W)             # the resize of image.py:552-580 is the caller's
        if (render_machine.height, render_machine.width) != (H, W):
            raise ValueError("the render machine draws %dx%d, the frames are %dx%d" % (render_machine.height, render_machine.width, H, W))
        for k in self.keys[1:]:
            if res is None and self.observed[k].shape != (self.M, H, W):
                raise ValueError("observed['%s'] has shape %s; %s expected" % (k, self.observed[k].shape, (self.M, H, W)))
        self.height, self.width = H, W
        if backgrounds is not None and (backgrounds.height, backgrounds.width) != (H, W):
            raise ValueError("the background pool was built for %dx%d frames, the frames are %dx%d"
                             % (backgrounds.height, backgrounds.width, H, W))
        self.backgrounds = backgrounds
        self.bg_ratio = float(config.TRAIN.get("REPLACE_OBSERVED_BG_RATIO", 0.0))
        self.data_syn = None if data_syn is None else np.asarray(data_syn).astype(bool).reshape(self.M)
        self.pose_observed = np.ascontiguousarray(observed["pose_observed"], dtype=np.float32).reshape(self.M, 3, 4)
        self.mask_idx = np.asarray(observed["mask_idx"]).astype(np.int32).reshape(self.M)
        self.class_index = np.asarray(observed["class_index"]).astype(np.int32).reshape(self.M)
        self.synthetic, self.S = synthetic, int(num_synthetic) if synthetic is not None else 0
        if synthetic is None and (num_synthetic or synthetic_classes is not None):
            raise ValueError("TrainDataLoader: num_synthetic / synthetic_classes need synthetic=SyntheticObserved(...)")
        self.synthetic_classes = np.zeros(0, np.int32)
        if synthetic is not None:
            if self.S < 0:
                raise ValueError("TrainDataLoader: num_synthetic must be >= 0")
            if (synthetic.height, synthetic.width) != (H, W):
                raise ValueError("the synthetic generator draws %dx%d, the frames are %dx%d" % (synthetic.height, synthetic.width, H, W))
            if synthetic.ctx is not self.ctx:
                raise ValueError("TrainDataLoader: the synthetic generator lives on another context")
            classes = sorted(set(self.class_index.tolist())) if synthetic_classes is None else synthetic_classes
            self.synthetic_classes = np.asarray(classes).astype(np.int32).reshape(-1)
            if self.S and self.synthetic_classes.size == 0:
                raise ValueError("TrainDataLoader: synthetic_classes is empty")
            synthetic.check_classes(self.synthetic_classes)         # on the host: no pair can draw attempts = -1
        self.points = None
        if config.train_iter.SE3_PM_LOSS:
            if points is None and (res is None or res.point_tables is None):
                raise ValueError("TrainDataLoader: train_iter.SE3_PM_LOSS needs `points` = {class id: (model points, weights)}")
            if res is not None and res.point_tables is None:
                res.set_points(points)           # once: the per-class tables are gathered on the device from then on
            self.points = res.point_classes if res is not None else {
                int(c): (np.ascontiguousarray(p, np.float32), np.ascontiguousarray(w, np.float32)) for c, (p, w) in points.items()}
            missing = sorted((set(self.class_index.tolist()) | (set(self.synthetic_classes.tolist()) if self.S else set())) - set(self.points))
            if missing:
                raise KeyError("TrainDataLoader: no model points for class ids {}".format(missing))
        if self.M * self.R + self.S < self.batch_size:
            raise ValueError("TrainDataLoader: %d pairs do not fill one batch of %d" % (self.M * self.R + self.S, self.batch_size))
        if res is not None:
            if self.S:               # synthetic pair at batch position b is drawn into spare row M + b
                res.claim_spare_rows(self, self.batch_size)
            if self.backgrounds is not None and (self.data_syn is not None or self.S):
                want = np.zeros(self.M, bool) if self.data_syn is None else self.data_syn
                if "data_syn" not in res.tables or not np.array_equal(res.host_tables["data_syn"], want):
                    res.set_data_syn(want)
        self.K = np.ascontiguousarray(config.dataset.INTRINSIC_MATRIX, np.float32).reshape(3, 3)
        self._rng = np.random.RandomState(self.seed)
        # pairs drawn, sum of attempts, exhausted pairs: device-resident; with `synthetic` the same three of the observed-pose draws
        # with occluders three more: pairs gated, pairs kept, occluder slots drawn
        self.occluded = synthetic is not None and getattr(synthetic, "occluders", None) is not None
        self._totals = self.ctx.zeros((3,) if synthetic is None else (9,) if self.occluded else (6,), np.uint64)
        self.epoch = 0
        self._plan()

    def _plan(self):
        self.pairs, self.draw_ids, self.dropped = epoch_plan(self.M, self.R, self.batch_size, self.shuffle, self._rng, self.epoch,
                                                             self.S)

    def __len__(self):
        return len(self.pairs)

    def reset(self):
        """The next epoch: new draw ids (fresh poses for every pair) and, with shuffle, a new order."""
        self.epoch += 1
        self._plan()

    def stats(self):
        """One read-back: {"pairs": pairs drawn, "attempts": candidates drawn for them, "exhausted": pairs for which none of
        max_attempts candidates was accepted (they train on a zero delta)} since construction. With `synthetic`, from the same
        read-back, also {"observed_pairs", "observed_attempts", "observed_exhausted"}: the synthetic pairs drawn, the observed-pose
        candidates drawn for them and the pairs that fell back to their class's fallback pose."""
        t = self._totals.asnumpy()
        out = {"pairs": int(t[0]), "attempts": int(t[1]), "exhausted": int(t[2])}
        if self.synthetic is not None:
            out.update(observed_pairs=int(t[3]), observed_attempts=int(t[4]), observed_exhausted=int(t[5]))
        if self.occluded:
            out.update(occluded_pairs=int(t[6]), occluded_kept=int(t[7]), occluder_slots=int(t[8]))
        return out

    def _image_observed(self, frames, always, ids):
        """image_observed of the batch; with a background pool, on the backgrounds image.py:96-155 gives it: a data_syn frame
        (`always`: the batch's flags, None = none) always, a real one with probability TRAIN.REPLACE_OBSERVED_BG_RATIO, both
        from the pair's own draw (stream 3)."""
        ctx, means = self.ctx, _image._means_rgb(self.config)
        if self.backgrounds is None:
            return _image.transform_batch(ctx, frames["image_observed"], means)
        use_bg, bg_index = background_draws_device(ctx, ids.size, self.seed, ids, self.bg_ratio, len(self.backgrounds), always=always)
        return _image.transform_batch_pool(ctx, frames["image_observed"], means, frames["mask_gt_observed"], use_bg, bg_index,
                                           self.backgrounds)

    def _upload(self, key, m, real):
        """The batch's (B,H,W[,3]) device array of observed[key]: row b is frame m[b] where real[b]; the synthetic rows are left
        for the generator. A batch of real rows is one upload, as without synthetic pairs; else one upload per run of real rows."""
        src = self.observed[key]
        if real.all():
            return self.ctx.array(src[m], dtype=_DTYPES[key])      # 1 or 2 bytes per value cross PCIe
        out = self.ctx.empty((len(m),) + src.shape[1:], _DTYPES[key])
        for j0, j1, r0 in runs(np.nonzero(real)[0]):
            out[r0:r0 + (j1 - j0)].copyfrom(src[m[r0:r0 + (j1 - j0)]])
        return out

    def make_batch(self, pairs, draw_ids):
        """(data, label) of the given pairs (p = m·R + r, or M·R + s for synthetic pair s) with the given draw ids."""
        ctx, cfg = self.ctx, self.config
        pairs = np.asarray(pairs, np.int64)
        if self.resident is not None:
            return self._make_batch_resident(pairs, draw_ids)
        real = pairs < self.M * self.R
        m = np.where(real, pairs // self.R, 0)
        B = len(m)
        syn = np.nonzero(~real)[0]
        mask_idx, cls, pose = self.mask_idx[m], self.class_index[m], self.pose_observed[m]
        always = None if self.data_syn is None else self.data_syn[m]
        if syn.size:
            cls_syn = self.synthetic_classes[(pairs[syn] - self.M * self.R) % len(self.synthetic_classes)]
            mask_idx[syn], cls[syn], pose[syn] = 1, cls_syn, 0.0
            always = np.zeros(B, bool) if always is None else always.copy()
            always[syn] = True
        frames = {k: self._upload(k, m, real) for k in self.keys}
        frames["mask_idx"] = ctx.array(mask_idx, dtype=np.int32)
        ids = ctx.array(np.asarray(draw_ids).reshape(B), dtype=np.uint64)
        pose_observed = ctx.array(pose)
        if syn.size:      # the synthetic rows: poses, lights and frames made on the device, straight into the batch's arrays
            drawn = self.synthetic.frames(cls_syn, np.asarray(draw_ids).reshape(B)[syn], rows=syn,
                                          out=dict(frames, pose_observed=pose_observed), **self._gate_totals())
            lib.deepim_sample_stats_accumulate(ctx.handle, self._totals[3:6], drawn["attempts"], int(syn.size))
            if cfg.network.INPUT_DEPTH and not self.occluded:       # their depth_observed is their own depth (occluded: the scene's)
                for j0, j1, r0 in runs(syn):
                    frames["depth_observed"][r0:r0 + (j1 - j0)].copyfrom(frames["depth_gt_observed"][r0:r0 + (j1 - j0)])
        batch = {"image_observed": self._image_observed(frames, always, ids),
                 "depth_gt_observed": _image._depth(ctx, frames, "depth_gt_observed", cfg),
                 "mask_gt_observed": _image.label_mask(ctx, frames, "mask_gt_observed"),
                 "pose_observed": pose_observed,
                 "class_index": ctx.array(cls, dtype=np.int32)}
        if cfg.network.INPUT_DEPTH:       # get_pair_depth, train phase: zeroed outside the pair's label with MASK_INPUTS
            batch["depth_observed"] = _image._depth(ctx, frames, "depth_observed", cfg,
                                                    "mask_gt_observed" if cfg.network.get("MASK_INPUTS", False) else None)
        if self.points is not None:
            batch["point_cloud_model"] = ctx.array(np.stack([self.points[int(c)][0] for c in cls]))
            batch["point_cloud_weights"] = ctx.array(np.stack([self.points[int(c)][1] for c in cls]))
        return self._finish(batch, ids, B)

    def _gate_totals(self):
        """The keyword that hands the generator the occlusion gate's three running totals; nothing without occluders."""
        return {"totals": self._totals[6:9]} if self.occluded else {}

    def _finish(self, batch, ids, B):
        """The rendered side and the labels of a batch whose observed side is made: the same for both kinds of set."""
        ctx, cfg = self.ctx, self.config
        batch["pose_rendered"], attempts = sample_rendered_poses(batch["pose_observed"], self.K, self.width, self.height, self.seed,
                                                                 draw_ids=ids, noise=self.noise)
        lib.deepim_sample_stats_accumulate(ctx.handle, self._totals, attempts, B)
        batch["image_rendered"], batch["depth_rendered"] = self.render_machine.render_batch(batch["class_index"], batch["pose_rendered"])
        if cfg.TRAIN.get("MASK_DILATE", False):
            batch["mask_dilate_thickness"] = mask_dilate_draws_device(ctx, B, self.seed, draw_ids=ids)
        out = data_pair.get_data_pair_train_batch(batch, cfg)
        return out["data"], out["label"]

    def _make_batch_resident(self, pairs, draw_ids):
        """make_batch over a ResidentObserved: frame_index, the draw ids and, with synthetic pairs, their positions and class
        ids go up; every row of the batch is read in place or gathered on the device."""
        ctx, cfg, res = self.ctx, self.config, self.resident
        rows, syn = batch_rows(pairs, self.M, self.R)
        B = len(rows)
        fi = ctx.array(rows, dtype=np.int32)
        ids = ctx.array(np.asarray(draw_ids).reshape(B), dtype=np.uint64)
        if syn.size:       # drawn into spare row M + b; class, pose (and mask_idx = data_syn = 1, set once) land in the tables' row
            cls_syn = ctx.array(self.synthetic_classes[(pairs[syn] - self.M * self.R) % len(self.synthetic_classes)], dtype=np.int32)
            if syn.size == B:
                ids_syn, rows_syn = ids, fi
            else:
                at = ctx.array(syn, dtype=np.int32)
                ids_syn = res.gather(ids.reshape((B, 1)), at, syn.size).reshape((syn.size,))
                rows_syn = res.gather(fi, at, syn.size)
            out = {k: res.arrays[k] for k in self.keys}       # depth_observed only with INPUT_DEPTH, as over a host set
            drawn = self.synthetic.frames(cls_syn, ids_syn, rows=rows[syn], rows_device=rows_syn,
                                          out=dict(out, pose_observed=res.tables["pose_observed"]), **self._gate_totals())
            lib.deepim_sample_stats_accumulate(ctx.handle, self._totals[3:6], drawn["attempts"], int(syn.size))
            for j0, j1, r0 in runs(rows[syn]):
                res.tables["class_index"][r0:r0 + (j1 - j0)].copyfrom(cls_syn[j0:j1])
                if cfg.network.INPUT_DEPTH and not self.occluded:       # their depth_observed is their own depth (occluded: the scene's)
                    res.arrays["depth_observed"][r0:r0 + (j1 - j0)].copyfrom(res.arrays["depth_gt_observed"][r0:r0 + (j1 - j0)])
        frames = {k: res.arrays[k] for k in self.keys}
        frames["frame_index"] = fi
        frames["mask_idx"] = res.gather(res.tables["mask_idx"], fi, B)
        means = _image._means_rgb(cfg)
        if self.backgrounds is None:
            image = _image.transform_batch_frames(ctx, frames["image_observed"], fi, means)
        else:
            always = res.gather(res.tables["data_syn"], fi, B) if (self.data_syn is not None or self.S) else None
            use_bg, bg_index = background_draws_device(ctx, B, self.seed, ids, self.bg_ratio, len(self.backgrounds), always=always)
            image = _image.transform_batch_frames(ctx, frames["image_observed"], fi, means, frames["mask_gt_observed"], use_bg,
                                                  bg_index, self.backgrounds)
        batch = {"image_observed": image,
                 "depth_gt_observed": _image._depth(ctx, frames, "depth_gt_observed", cfg),
                 "mask_gt_observed": _image.label_mask(ctx, frames, "mask_gt_observed"),
                 "pose_observed": res.gather(res.tables["pose_observed"], fi, B),
                 "class_index": res.gather(res.tables["class_index"], fi, B)}
        if cfg.network.INPUT_DEPTH:
            batch["depth_observed"] = _image._depth(ctx, frames, "depth_observed", cfg,
                                                    "mask_gt_observed" if cfg.network.get("MASK_INPUTS", False) else None)
        if self.points is not None:
            batch["point_cloud_model"] = res.gather(res.point_tables[0], batch["class_index"], B)
            batch["point_cloud_weights"] = res.gather(res.point_tables[1], batch["class_index"], B)
        return self._finish(batch, ids, B)

    def __iter__(self):
        for pairs, ids in zip(self.pairs, self.draw_ids):
            yield self.make_batch(pairs, ids)


# ---------------------------------------------------------------------------------------------------------- the test phase --
_TEST_DTYPES = {"image_observed": np.uint8, "depth_observed": np.uint16, "depth_gt_observed": np.uint16,
                "mask_gt_observed": np.uint8, "mask_observed": np.uint8, "mask_observed_est": np.uint8}
# TEST.INIT_MASK → the label map lib/utils/image.get_pair_mask reads for it (box_rendered reads the rendered depth alone)
_INIT_MASK_SOURCE = {"mask_gt_observed": "mask_gt_observed", "box_gt_observed": "mask_gt_observed", "mask_observed": "mask_observed",
                     "box_": "mask_observed", "box_rendered": None}


def observed_keys_of_test(config, have=()):
    """The observed arrays the test phase of `config` reads, no device needed: image_observed always; depth_observed with
    network.INPUT_DEPTH (and, with MASK_INPUTS, the label map get_pair_depth zeroes it with); the label map of TEST.INIT_MASK with
    network.INPUT_MASK; for the flow EPE (network.PRED_FLOW and not TEST.FAST_TEST) mask_gt_observed and depth_gt_observed — or
    depth_observed when `have` (the keys on offer) holds no depth_gt_observed (tester.py:541-547)."""
    n = config.network
    keys = ["image_observed"]
    if n.INPUT_DEPTH:
        keys.append("depth_observed")
        if n.get("MASK_INPUTS", False):
            keys.append("mask_gt_observed" if config.dataset.get("MASK_GT", False) else "mask_observed_est")
    if n.INPUT_MASK:
        init = config.TEST.INIT_MASK
        if init not in _INIT_MASK_SOURCE:
            raise Exception("Unknown init mask type: {}".format(init))
        if _INIT_MASK_SOURCE[init] is not None:
            keys.append(_INIT_MASK_SOURCE[init])
    if n.PRED_FLOW and not config.TEST.FAST_TEST:
        keys.append("depth_gt_observed" if ("depth_gt_observed" in have or "depth_observed" not in have) else "depth_observed")
        keys.append("mask_gt_observed")
    if config.TEST.get("DEPTH_ICP", False):        # the depth ICP's target is the raw sensor depth (core/tester.py)
        keys.append("depth_observed")
    return list(dict.fromkeys(keys))


def plan_test_batches(P, batch_size, shuffle, rng):
    """The batches of one pass over P pairs, no device needed → (pairs (n_batches, batch_size) int64, pad). The order is
    arange(P), or rng.permutation(P) with `shuffle` (rng: a RandomState, consumed once per call). No pair is dropped: the last
    batch is filled up with `pad` = n_batches·batch_size − P repeats of its last pair."""
    P, batch_size = int(P), int(batch_size)
    if P < 1 or batch_size < 1:
        raise ValueError("plan_test_batches: P and batch_size must be >= 1")
    order = rng.permutation(P).astype(np.int64) if shuffle else np.arange(P, dtype=np.int64)
    n_batches = -(-P // batch_size)
    pad = n_batches * batch_size - P
    order = np.concatenate([order, np.full(pad, order[-1], np.int64)])
    return order.reshape(n_batches, batch_size), pad


def batch_frames(frame_ids):
    """The frames a shared-frame batch uploads, no device needed → (frames (N,) ascending distinct ids, frame_index (B,) int32):
    pair b looks at row frame_index[b] of the N <= B uploaded frames."""
    uniq, inv = np.unique(np.asarray(frame_ids, np.int64).reshape(-1), return_inverse=True)
    return uniq, inv.reshape(-1).astype(np.int32)


class TestDataLoader(object):
    """The test iterator: TestDataLoader (deepim/core/loader.py:17-108) from observed frames and initial poses alone.

        loader = TestDataLoader(observed, pairdb, config, render_machine, batch_size=2)
        pred_eval(config, Predictor(config, net), loader, imdb, logger=logger, render_machine=render_machine)

    The reference reads, for every pair, the render of its initial pose that toolkit/LM6d_3_gen_PoseCNN_pred_rendered.py:149-155
    wrote to disk once. This one DRAWS it: every batch's initial poses are rendered on the device straight into uint8 / uint16
    frames with the bytes those files hold (Render_Py.render_frames_into), next to each pair's count of covered pixels.

    `observed`: host numpy arrays for the F camera frames as the decoder left them (observed_keys_of_test says which the
    configuration reads): image_observed (F,H,W,3) uint8 BGR; depth_observed / depth_gt_observed (F,H,W) uint16;
    mask_gt_observed / mask_observed / mask_observed_est (F,H,W) uint8 label maps. H x W is config.SCALES[0].
    `pairdb`: a list of P dicts with frame (index into the F frames), gt_class, mask_idx, pose_observed (3,4), pose_rendered
    (3,4) — the initial estimate, all −1 where the detector found nothing (tester.py:285-310) — and optionally K (3,3).

    Every batch is (data, frames, pair_records) as core/tester.pred_eval takes it. With `shared_frames` the distinct frames of
    the batch are uploaded once (N <= B rows) and the pairs name them through a frame_index; without, one row per pair. mask_idx,
    the render machine's class ids and the poses are uploaded; when a record has a K, the batch's (B,3,3) camera table too
    (frames["intrinsics"]), and the draw uses it. frames["rendered_covered"] lets get_pair_mask zero mask_observed of a pair whose
    draw is empty (image.py:301-303) on the device. With TEST.MASK_DILATE the thicknesses come from the device generator with
    the pair's index in `pairdb` as its draw id: a pair's draw depends on (seed, pair) alone. Nothing is read back.

    Differences from the reference: one upload per frame, not per pair; batch_size > 1; the last batch is filled up by repeating
    its last pair, and the repeats' records are copies carrying "pad": True, which pred_eval leaves out of everything it counts
    (the reference hands the pad count to DataBatch); the mask-dilate draws are the device generator's; the empty-draw rule is
    applied on the device and not printed. Order: arange(P), or with `shuffle` a permutation from RandomState(seed), drawn anew
    at each reset().

    `observed` = core/resident.ResidentObserved(observed, ctx): the F frames uploaded once. With `shared_frames` a batch's
    frames dict holds the set's own arrays (N = F) and frame_index = frame[pairs]; without, the per-pair rows are gathered on
    the device by deepim_gather_rows (a frame that is not a multiple of 4 bytes is refused). Only ids, poses and cameras go up.

    Refused: a dict holding a device array, a frame that is not config.SCALES[0] or not the render machine's size, a pair whose frame
    is outside [0, F) or whose gt_class the render machine does not know, and shared_frames with network.INPUT_MASK off (the
    library's shared-frame zoom front end has no mask-less variant: pass shared_frames=False)."""
    __test__ = False          # a data iterator named after the reference's, not a pytest class

    def __init__(self, observed, pairdb, config, render_machine, batch_size=1, shuffle=False, seed=0, shared_frames=True):
        self.config, self.render_machine = config, render_machine
        self.batch_size, self.shuffle, self.seed, self.shared_frames = int(batch_size), bool(shuffle), int(seed), bool(shared_frames)
        if self.batch_size < 1:
            raise ValueError("TestDataLoader: batch_size must be >= 1")
        self.resident = res = observed if isinstance(observed, ResidentObserved) else None
        if res is not None:
            if res.ctx is not render_machine.ctx:
                raise ValueError("TestDataLoader: the resident set lives on another context")
            observed = res.arrays           # checked when the set was built; read below for its keys alone
        else:
            for k, v in observed.items():
                if isinstance(v, DeviceArray):
                    raise TypeError("TestDataLoader: observed['%s'] is a device array; the dataset is host numpy arrays (a batch's "
                                    "frames are gathered on the host and uploaded) or a ResidentObserved" % k)
        if self.shared_frames and not config.network.INPUT_MASK:
            raise NotImplementedError("TestDataLoader: shared_frames needs network.INPUT_MASK — the shared-frame zoom front end "
                                      "has no mask-less variant; pass shared_frames=False")
        self.keys = observed_keys_of_test(config, [k for k, v in observed.items() if v is not None])
        self.observed = {}
        for k in self.keys:
            if observed.get(k) is None:
                raise KeyError("TestDataLoader: observed carries no '%s'" % k)
            if res is not None:
                if not self.shared_frames and (res.arrays[k].nbytes // res.rows) % 4:
                    raise ValueError("TestDataLoader: a '%s' frame of %d bytes is not a multiple of 4 bytes; the per-pair rows of "
                                     "a resident set are gathered in 4-byte words" % (k, res.arrays[k].nbytes // res.rows))
                continue
            v = np.asarray(observed[k])
            if v.dtype != np.dtype(_TEST_DTYPES[k]):
                raise TypeError("observed['%s'] is %s; the decoded %s frame is expected" % (k, v.dtype, np.dtype(_TEST_DTYPES[k])))
            self.observed[k] = v
        if res is not None:
            self.F, H, W = res.M, res.height, res.width
        else:
            img = self.observed["image_observed"]
            if img.ndim != 4 or img.shape[3] != 3 or img.shape[0] < 1:
                raise ValueError("observed['image_observed'] has shape %s; (F,H,W,3) expected" % (img.shape,))
            self.F, H, W = img.shape[0], img.shape[1], img.shape[2]
        _image._check_size(config, H, W)
        if (render_machine.height, render_machine.width) != (H, W):
            raise ValueError("the render machine draws %dx%d, the frames are %dx%d" % (render_machine.height, render_machine.width, H, W))
        for k in self.keys[1:]:
            if res is None and self.observed[k].shape != (self.F, H, W):
                raise ValueError("observed['%s'] has shape %s; %s expected" % (k, self.observed[k].shape, (self.F, H, W)))
        self.height, self.width = H, W
        self.pairdb = list(pairdb)
        self.size = len(self.pairdb)
        if self.size < 1:
            raise ValueError("TestDataLoader: the pairdb is empty")
        classes = list(render_machine.classes)
        self.frame, self.mask_idx = np.zeros(self.size, np.int64), np.zeros(self.size, np.int32)
        self.class_index, self.pose_rendered = np.zeros(self.size, np.int32), np.zeros((self.size, 3, 4), np.float32)
        for p, rec in enumerate(self.pairdb):
            for k in ("frame", "gt_class", "mask_idx", "pose_observed", "pose_rendered"):
                if rec.get(k) is None:
                    raise KeyError("TestDataLoader: pair %d carries no '%s'" % (p, k))
            f = int(rec["frame"])
            if not 0 <= f < self.F:
                raise ValueError("TestDataLoader: pair %d looks at frame %d, outside the %d observed frame%s"
                                 % (p, f, self.F, "" if self.F == 1 else "s"))
            if rec["gt_class"] not in classes:
                raise ValueError("TestDataLoader: pair %d is of class %r, which the render machine (%s) does not draw"
                                 % (p, rec["gt_class"], ", ".join(map(str, classes))))
            if np.shape(rec["pose_rendered"]) != (3, 4) or np.shape(rec["pose_observed"]) != (3, 4):
                raise ValueError("TestDataLoader: pair %d: pose_rendered and pose_observed must be (3,4)" % p)
            self.frame[p], self.mask_idx[p], self.class_index[p] = f, int(rec["mask_idx"]), classes.index(rec["gt_class"])
            self.pose_rendered[p] = np.asarray(rec["pose_rendered"], np.float32)
        self.ctx = render_machine.ctx          # touched last: every refusal above needs no device
        self.K = np.ascontiguousarray(config.dataset.INTRINSIC_MATRIX, np.float32).reshape(3, 3)
        self.depth_factor = float(config.dataset.get("DEPTH_FACTOR", 1000))
        self.dilate = bool(config.network.INPUT_MASK and config.TEST.get("MASK_DILATE", False))
        self._rng = np.random.RandomState(self.seed)
        self._plan()

    def _plan(self):
        self.pairs, self.pad = plan_test_batches(self.size, self.batch_size, self.shuffle, self._rng)

    def __len__(self):
        return len(self.pairs)

    def reset(self):
        """The next pass: with shuffle, the next permutation of the loader's RandomState."""
        self._plan()

    def getpad(self):
        """How many repeats of its last pair fill up the last batch of a pass (their records carry "pad": True)."""
        return self.pad

    def make_batch(self, pairs, pad=0):
        """(data, frames, pair_records) of the pairs `pairs` (indices into the pairdb), the last `pad` of them padding."""
        ctx, cfg = self.ctx, self.config
        pairs = np.asarray(pairs, np.int64).reshape(-1)
        B, H, W = len(pairs), self.height, self.width
        records = [self.pairdb[p] if b < B - pad else dict(self.pairdb[p], pad=True) for b, p in enumerate(pairs)]
        frames = {}
        if self.resident is not None:       # the ids go up; the frames are the set's own (shared) or gathered on the device
            index = ctx.array(self.frame[pairs], dtype=np.int32)
            if self.shared_frames:
                frames["frame_index"] = index
            for k in self.keys:
                frames[k] = self.resident.arrays[k] if self.shared_frames else self.resident.gather(self.resident.arrays[k], index, B)
        else:
            if self.shared_frames:
                rows, index = batch_frames(self.frame[pairs])
                frames["frame_index"] = ctx.array(index, dtype=np.int32)
            else:
                rows = self.frame[pairs]
            for k in self.keys:
                frames[k] = ctx.array(self.observed[k][rows], dtype=_TEST_DTYPES[k])       # 1 or 2 bytes per value cross PCIe
        frames["mask_idx"] = ctx.array(self.mask_idx[pairs], dtype=np.int32)
        frames["class_index"] = ctx.array(self.class_index[pairs], dtype=np.int32)
        frames["pose_rendered"] = ctx.array(self.pose_rendered[pairs])
        cams = None
        if has_cameras(records):
            cams = frames["intrinsics"] = ctx.array(camera_table(records, self.K))
        frames["image_rendered"] = ctx.empty((B, H, W, 3), np.uint8)
        frames["depth_rendered"] = ctx.empty((B, H, W), np.uint16)
        frames["rendered_covered"] = ctx.empty((B,), np.int32)
        self.render_machine.render_frames_into(frames["image_rendered"], frames["depth_rendered"], frames["class_index"],
                                               frames["pose_rendered"], K=cams, covered=frames["rendered_covered"],
                                               depth_factor=self.depth_factor)
        if self.dilate:
            frames["mask_dilate_thickness"] = mask_dilate_draws_device(ctx, B, self.seed, draw_ids=pairs.astype(np.uint64))
        return data_pair.get_data_pair_test_batch(frames, cfg), frames, records

    def __iter__(self):
        for i, pairs in enumerate(self.pairs):
            yield self.make_batch(pairs, self.pad if i == len(self.pairs) - 1 else 0)
