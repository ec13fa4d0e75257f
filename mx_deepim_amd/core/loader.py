"""The training iterator: TrainDataLoader (deepim/core/loader.py:111-262) over the device's own random draws.

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

Not part of this loader and refused: ready-made backgrounds (bg_image: the pool is the loader's way), TRAIN.MASK_SYN, resizing (a frame that is not config.SCALES[0]),
shared-frame batches (frame_index), device-resident datasets.
"""
import numpy as np

from ..lib.pair_matching import data_pair
from ..lib.pair_matching.pose_sampler import pose_noise, sample_rendered_poses
from ..lib.utils import image as _image
from ..lib.utils.background import background_draws_device
from ..lib.utils.mask_dilate import mask_dilate_draws_device
from ..runtime import DeviceArray, lib

_DTYPES = {"image_observed": np.uint8, "depth_gt_observed": np.uint16, "mask_gt_observed": np.uint8, "depth_observed": np.uint16}


def epoch_plan(M, R, batch_size, shuffle, rng, epoch):
    """The batches of one epoch over M observed frames with R rendered poses each, no device needed →
    (pairs (n_batches, batch_size) int64, draw_ids (n_batches, batch_size) uint64, dropped).
    pairs holds p = m·R + r in epoch order: arange(M·R), or rng.permutation(M·R) with `shuffle` (rng: a RandomState, consumed
    once per call); the trailing M·R mod batch_size pairs are dropped. draw_ids = epoch·M·R + pairs."""
    M, R, batch_size, epoch = int(M), int(R), int(batch_size), int(epoch)
    if M < 1 or R < 1 or batch_size < 1 or epoch < 0:
        raise ValueError("epoch_plan: M, R, batch_size must be >= 1 and epoch >= 0")
    n = M * R
    order = rng.permutation(n).astype(np.int64) if shuffle else np.arange(n, dtype=np.int64)
    n_batches = n // batch_size
    pairs = order[:n_batches * batch_size].reshape(n_batches, batch_size)
    return pairs, (pairs + epoch * n).astype(np.uint64), n - n_batches * batch_size


class TrainDataLoader(object):
    def __init__(self, observed, config, render_machine, batch_size=1, shuffle=False, seed=0, num_rendered_per_observed=1,
                 points=None, noise=None, backgrounds=None, data_syn=None):
        self.config, self.render_machine, self.ctx = config, render_machine, render_machine.ctx
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        self.R = int(num_rendered_per_observed)
        self.noise = pose_noise(noise)
        for k, v in observed.items():
            if isinstance(v, DeviceArray):
                raise TypeError("TrainDataLoader: observed['%s'] is a device array; the dataset is host numpy arrays, a batch is "
                                "gathered on the host and uploaded" % k)
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
            if observed.get(k) is None:
                raise KeyError("TrainDataLoader: observed carries no '%s'" % k)
            v = np.asarray(observed[k])
            if v.dtype != np.dtype(_DTYPES[k]):
                raise TypeError("observed['%s'] is %s; the decoded %s frame is expected" % (k, v.dtype, np.dtype(_DTYPES[k])))
            self.observed[k] = v
        img = self.observed["image_observed"]
        if img.ndim != 4 or img.shape[3] != 3:
            raise ValueError("observed['image_observed'] has shape %s; (M,H,W,3) expected" % (img.shape,))
        self.M, H, W = img.shape[0], img.shape[1], img.shape[2]
        _image._check_size(config, H, W)             # the resize of image.py:552-580 is the caller's
        if (render_machine.height, render_machine.width) != (H, W):
            raise ValueError("the render machine draws %dx%d, the frames are %dx%d" % (render_machine.height, render_machine.width, H, W))
        for k in self.keys[1:]:
            if self.observed[k].shape != (self.M, H, W):
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
        self.points = None
        if config.train_iter.SE3_PM_LOSS:
            if points is None:
                raise ValueError("TrainDataLoader: train_iter.SE3_PM_LOSS needs `points` = {class id: (model points, weights)}")
            self.points = {int(c): (np.ascontiguousarray(p, np.float32), np.ascontiguousarray(w, np.float32)) for c, (p, w) in points.items()}
            missing = sorted(set(self.class_index.tolist()) - set(self.points))
            if missing:
                raise KeyError("TrainDataLoader: no model points for class ids {}".format(missing))
        if self.M * self.R < self.batch_size:
            raise ValueError("TrainDataLoader: %d pairs do not fill one batch of %d" % (self.M * self.R, self.batch_size))
        self.K = np.ascontiguousarray(config.dataset.INTRINSIC_MATRIX, np.float32).reshape(3, 3)
        self._rng = np.random.RandomState(self.seed)
        self._totals = self.ctx.zeros((3,), np.uint64)      # pairs drawn, sum of attempts, exhausted pairs: device-resident
        self.epoch = 0
        self._plan()

    def _plan(self):
        self.pairs, self.draw_ids, self.dropped = epoch_plan(self.M, self.R, self.batch_size, self.shuffle, self._rng, self.epoch)

    def __len__(self):
        return len(self.pairs)

    def reset(self):
        """The next epoch: new draw ids (fresh poses for every pair) and, with shuffle, a new order."""
        self.epoch += 1
        self._plan()

    def stats(self):
        """One read-back: {"pairs": pairs drawn, "attempts": candidates drawn for them, "exhausted": pairs for which none of
        max_attempts candidates was accepted (they train on a zero delta)} since construction."""
        t = self._totals.asnumpy()
        return {"pairs": int(t[0]), "attempts": int(t[1]), "exhausted": int(t[2])}

    def _image_observed(self, frames, m, ids):
        """image_observed of the batch; with a background pool, on the backgrounds image.py:96-155 gives it: a data_syn frame
        always, a real one with probability TRAIN.REPLACE_OBSERVED_BG_RATIO, both from the pair's own draw (stream 3)."""
        ctx, means = self.ctx, _image._means_rgb(self.config)
        if self.backgrounds is None:
            return _image.transform_batch(ctx, frames["image_observed"], means)
        use_bg, bg_index = background_draws_device(ctx, len(m), self.seed, ids, self.bg_ratio, len(self.backgrounds),
                                                   always=None if self.data_syn is None else self.data_syn[m])
        return _image.transform_batch_pool(ctx, frames["image_observed"], means, frames["mask_gt_observed"], use_bg, bg_index,
                                           self.backgrounds)

    def make_batch(self, pairs, draw_ids):
        """(data, label) of the given pairs (p = m·R + r) with the given draw ids."""
        ctx, cfg = self.ctx, self.config
        m = np.asarray(pairs, np.int64) // self.R
        B = len(m)
        frames = {k: ctx.array(self.observed[k][m], dtype=_DTYPES[k]) for k in self.keys}      # 1 or 2 bytes per value cross PCIe
        frames["mask_idx"] = ctx.array(self.mask_idx[m], dtype=np.int32)
        ids = ctx.array(np.asarray(draw_ids).reshape(B), dtype=np.uint64)
        batch = {"image_observed": self._image_observed(frames, m, ids),
                 "depth_gt_observed": _image._depth(ctx, frames, "depth_gt_observed", cfg),
                 "mask_gt_observed": _image.label_mask(ctx, frames, "mask_gt_observed"),
                 "pose_observed": ctx.array(self.pose_observed[m]),
                 "class_index": ctx.array(self.class_index[m], dtype=np.int32)}
        if cfg.network.INPUT_DEPTH:       # get_pair_depth, train phase: zeroed outside the pair's label with MASK_INPUTS
            batch["depth_observed"] = _image._depth(ctx, frames, "depth_observed", cfg,
                                                    "mask_gt_observed" if cfg.network.get("MASK_INPUTS", False) else None)
        batch["pose_rendered"], attempts = sample_rendered_poses(batch["pose_observed"], self.K, self.width, self.height, self.seed,
                                                                 draw_ids=ids, noise=self.noise)
        lib.deepim_sample_stats_accumulate(ctx.handle, self._totals, attempts, B)
        batch["image_rendered"], batch["depth_rendered"] = self.render_machine.render_batch(batch["class_index"], batch["pose_rendered"])
        if cfg.TRAIN.get("MASK_DILATE", False):
            batch["mask_dilate_thickness"] = mask_dilate_draws_device(ctx, B, self.seed, draw_ids=ids)
        if self.points is not None:
            cls = self.class_index[m]
            batch["point_cloud_model"] = ctx.array(np.stack([self.points[int(c)][0] for c in cls]))
            batch["point_cloud_weights"] = ctx.array(np.stack([self.points[int(c)][1] for c in cls]))
        out = data_pair.get_data_pair_train_batch(batch, cfg)
        return out["data"], out["label"]

    def __iter__(self):
        for pairs, ids in zip(self.pairs, self.draw_ids):
            yield self.make_batch(pairs, ids)
