"""The data iterators of deepim/core/loader.py over an observed set: TrainDataLoader (:111-262) and, at the end of this file with
its own description, TestDataLoader (:17-108). Neither needs a dataset of rendered images: the training loader DRAWS the rendered
pose of every pair on the device and renders it, the test loader draws every pair's initial pose as decoded frames.

    loader = TrainDataLoader(observed, config, render_machine, batch_size=4, shuffle=True, seed=3, points=points)
    MutableModule(config, net).fit(loader, ..., updater=batchUpdaterPyMulti(config, H, W, render_machine=render_machine))

The set. `observed` is the M observed frames and their ground truth, as the decoder left them (lib/utils/image.py): a dict of
host numpy arrays, or a core/resident.ResidentObserved that holds the same arrays on the device.
    image_observed (M,H,W,3) uint8 BGR     depth_gt_observed (M,H,W) uint16     mask_gt_observed (M,H,W) uint8 label maps
    mask_idx (M)     pose_observed (M,3,4) float32     class_index (M)     depth_observed (M,H,W) uint16 with network.INPUT_DEPTH
A dict is checked by resident.check_observed and wrapped in a resident.HostObserved; from there on the loader talks to the set's
interface alone and every batch, draw id and byte is the same over both kinds (core/resident.py says what each uploads).
`points`: {class id: ((3,N) model points, (3,N) weights)} for train_iter.SE3_PM_LOSS, the N points already sampled.
`synthetic`: a lib/utils/synthetic_observed.SyntheticObserved built for the frames' (H, W), or None: S = `num_synthetic` fresh
synthetic pairs per epoch (LM6D_REFINE_SYN.py: data_syn = True, mask_idx = 1), synthetic pair s being of class
synthetic_classes[s mod len(synthetic_classes)] (default: the classes of the observed set, in order).
`backgrounds`: a lib/utils/background.BackgroundPool built for the frames' (H, W), or None. `data_syn`: (M) bool, optional.

An epoch is the n = M·R + S pairs p = m·R + r (R = num_rendered_per_observed), p >= M·R being synthetic pair p − M·R, in order or,
with `shuffle`, in a permutation drawn from the loader's own RandomState(seed) at every reset(); a trailing partial batch is
dropped, as the reference's iter_next does. Pair p of epoch e has draw id e·n + p wherever the shuffle puts it, so everything
drawn for it depends on (seed, e, p) alone: every epoch sees fresh initial poses, no host random number goes into a pose, and
nothing is read back inside an epoch.

A batch holds, for each of its pairs:
  * the observed side: its frame's image minus the pixel means, depth maps in metres and 0 / 1 label mask, made by the ingest
    kernels from the uint8 / uint16 frames, with pose_observed, class_index and the class's point cloud. With `backgrounds` the
    image gets the background replacement of image.py:96-155 on the device: a data_syn frame always, the others with probability
    TRAIN.REPLACE_OBSERVED_BG_RATIO, on a pool image chosen by the pair's own draw (stream 3 of its draw id), cropped, resized and
    composited by one kernel. With network.INPUT_DEPTH depth_observed, zeroed outside the pair's label with MASK_INPUTS;
  * a synthetic pair's observed side: pose and light drawn (streams 4-6 of its draw id under the generator's own seed) and the
    frame rendered on the device straight into the uint8 / uint16 arrays the real rows lie in. It counts as data_syn, its
    mask_idx is 1 and its depth_observed its own depth. A generator built with occluders (OccluderSpec) puts up to max_occluders
    other objects into the frame (streams 7 and 8): the label map shows the visible part of the target only, depth_gt_observed
    stays the target drawn alone, depth_observed is the scene's depth, and a pair whose target keeps less than min_visible of its
    pixels falls back to the unoccluded frame;
  * the rendered side: a pose drawn around pose_observed (lib/pair_matching/pose_sampler.py, streams 0/1 of the draw id) and its
    unquantised float render by the device render machine, not the 8-bit / 16-bit files of the reference;
  * the labels of lib/pair_matching/data_pair.get_data_pair_train_batch, with TRAIN.MASK_DILATE on the pair's own draw.
stats() counts the pairs drawn, their attempts and the exhausted ones, for the synthetic observed poses too, and with occluders
the pairs gated, kept and the occluder slots drawn. The synthetic classes are checked against the generator's tables on the
host, so no pair can come out with attempts = −1.

Refused at construction: a dict holding a DeviceArray, a missing array, a dtype or shape that is not the decoder's
(resident.check_observed); ready-made backgrounds (bg_image: the pool is the loader's way), TRAIN.MASK_SYN, resizing (a frame
that is not config.SCALES[0]), shared-frame batches (frame_index), a render machine, pool or generator of another frame size,
classes without model points, fewer pairs than one batch, and a resident set on another context or with fewer spare rows than a
batch.
Not built: more than one target per synthetic frame, and a synthetic set kept across epochs (SyntheticObserved.to_host makes a
fixed one for the `observed` argument).
"""
import numpy as np

from ..cameras import camera_table, has_cameras
from ..lib.pair_matching import data_pair
from ..lib.pair_matching.pose_sampler import pose_noise, sample_rendered_poses
from ..lib.utils import image as _image
from ..lib.utils.background import background_draws_device
from ..lib.utils.mask_dilate import mask_dilate_draws_device
from ..runtime import lib
from .resident import HostObserved, ResidentObserved, batch_frames, batch_rows          # noqa: F401 (re-exported with the loaders)


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
        n = config.network
        self.keys = ["image_observed", "depth_gt_observed", "mask_gt_observed"] + (["depth_observed"] if n.INPUT_DEPTH else [])
        tables = ("pose_observed", "mask_idx", "class_index")
        self.resident = observed if isinstance(observed, ResidentObserved) else None
        if self.resident is None:       # a host dict: what only a dict can ask for is refused, then it is checked and wrapped
            if observed.get("bg_image") is not None:
                raise NotImplementedError("TrainDataLoader: ready-made backgrounds (bg_image) are not part of this loader; pass "
                                          "backgrounds=BackgroundPool(...) and they are drawn, cropped and resized on the device")
            if observed.get("frame_index") is not None:
                raise NotImplementedError("TrainDataLoader: shared frames (frame_index) are a test-phase input; the training loader "
                                          "is per pair")
        if config.TRAIN.get("MASK_SYN", False):
            raise NotImplementedError("TrainDataLoader: TRAIN.MASK_SYN (image.py:205-206) is not part of the device path")
        self.set = obs = self.resident or HostObserved(observed, self.ctx, self.keys, tables)
        if obs.ctx is not self.ctx:
            raise ValueError("TrainDataLoader: the resident set lives on another context")
        missing = [k for k in self.keys if k not in obs.arrays] + [k for k in tables if k not in obs.host_tables]
        if missing:
            raise KeyError("TrainDataLoader: the observed set carries no '%s'" % "', '".join(missing))
        self.M, H, W = obs.M, obs.height, obs.width
        _image._check_size(config, H, W)             # the resize of image.py:552-580 is the caller's
        if (render_machine.height, render_machine.width) != (H, W):
            raise ValueError("the render machine draws %dx%d, the frames are %dx%d" % (render_machine.height, render_machine.width, H, W))
        self.height, self.width = H, W
        if backgrounds is not None and (backgrounds.height, backgrounds.width) != (H, W):
            raise ValueError("the background pool was built for %dx%d frames, the frames are %dx%d"
                             % (backgrounds.height, backgrounds.width, H, W))
        self.backgrounds = backgrounds
        self.bg_ratio = float(config.TRAIN.get("REPLACE_OBSERVED_BG_RATIO", 0.0))
        if data_syn is None:
            data_syn = obs.host_tables.get("data_syn")
        self.data_syn = None if data_syn is None else np.asarray(data_syn).astype(bool).reshape(self.M)
        self.class_index = obs.host_tables["class_index"]
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
            if points is None and obs.point_classes is None:
                raise ValueError("TrainDataLoader: train_iter.SE3_PM_LOSS needs `points` = {class id: (model points, weights)}")
            if obs.point_classes is None:
                obs.set_points(points)           # once: a resident set gathers its per-class tables on the device from then on
            self.points = obs.point_classes
            missing = sorted((set(self.class_index.tolist()) | (set(self.synthetic_classes.tolist()) if self.S else set())) - set(self.points))
            if missing:
                raise KeyError("TrainDataLoader: no model points for class ids {}".format(missing))
        if self.M * self.R + self.S < self.batch_size:
            raise ValueError("TrainDataLoader: %d pairs do not fill one batch of %d" % (self.M * self.R + self.S, self.batch_size))
        if self.S:               # a resident set draws the synthetic pair at batch position b into its spare row M + b
            obs.claim_spare_rows(self, self.batch_size)
        if self.backgrounds is not None and (self.data_syn is not None or self.S):
            want = np.zeros(self.M, bool) if self.data_syn is None else self.data_syn
            if not np.array_equal(obs.host_tables.get("data_syn"), want):
                obs.set_data_syn(self.data_syn)
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

    def _draw_synthetic(self, **target):
        """Poses, lights and frames of a batch's synthetic pairs, made on the device where the set wants them (`target`)."""
        totals = {"totals": self._totals[6:9]} if self.occluded else {}      # the occlusion gate's three running totals
        drawn = self.synthetic.frames(**target, **totals)
        lib.deepim_sample_stats_accumulate(self.ctx.handle, self._totals[3:6], drawn["attempts"], len(target["rows"]))

    def make_batch(self, pairs, draw_ids):
        """(data, label) of the given pairs (p = m·R + r, or M·R + s for synthetic pair s) with the given draw ids."""
        ctx, cfg = self.ctx, self.config
        pairs = np.asarray(pairs, np.int64)
        B, n = len(pairs), self.M * self.R
        cls_syn = self.synthetic_classes[(pairs[pairs >= n] - n) % len(self.synthetic_classes)] if (pairs >= n).any() else None
        # a synthetic pair's depth_observed is its own depth (occluded: the scene's, which the generator wrote)
        frames, ids, table, points = self.set.train_batch(pairs, np.asarray(draw_ids).reshape(B), self.R, self.keys, cls_syn,
                                                          self._draw_synthetic, cfg.network.INPUT_DEPTH and not self.occluded)
        use_bg = bg_index = None
        if self.backgrounds is not None:       # image.py:96-155: a data_syn frame always, a real one with probability bg_ratio
            use_bg, bg_index = background_draws_device(ctx, B, self.seed, ids, self.bg_ratio, len(self.backgrounds),
                                                       always=table("data_syn"))
        batch = {"image_observed": _image.image_observed(ctx, frames, cfg, use_bg, bg_index, self.backgrounds),
                 "depth_gt_observed": _image._depth(ctx, frames, "depth_gt_observed", cfg),
                 "mask_gt_observed": _image.label_mask(ctx, frames, "mask_gt_observed"),
                 "pose_observed": table("pose_observed"),
                 "class_index": table("class_index")}
        if cfg.network.INPUT_DEPTH:       # get_pair_depth, train phase: zeroed outside the pair's label with MASK_INPUTS
            batch["depth_observed"] = _image._depth(ctx, frames, "depth_observed", cfg,
                                                    "mask_gt_observed" if cfg.network.get("MASK_INPUTS", False) else None)
        if self.points is not None:
            batch["point_cloud_model"], batch["point_cloud_weights"] = points(batch["class_index"])
        batch["pose_rendered"], attempts = sample_rendered_poses(batch["pose_observed"], self.K, self.width, self.height, self.seed,
                                                                 draw_ids=ids, noise=self.noise)
        lib.deepim_sample_stats_accumulate(ctx.handle, self._totals, attempts, B)
        batch["image_rendered"], batch["depth_rendered"] = self.render_machine.render_batch(batch["class_index"], batch["pose_rendered"])
        if cfg.TRAIN.get("MASK_DILATE", False):
            batch["mask_dilate_thickness"] = mask_dilate_draws_device(ctx, B, self.seed, draw_ids=ids)
        out = data_pair.get_data_pair_train_batch(batch, cfg)
        return out["data"], out["label"]

    def __iter__(self):
        for pairs, ids in zip(self.pairs, self.draw_ids):
            yield self.make_batch(pairs, ids)


# ---------------------------------------------------------------------------------------------------------- the test phase --
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


class TestDataLoader(object):
    """The test iterator: TestDataLoader (deepim/core/loader.py:17-108) from observed frames and initial poses alone.

        loader = TestDataLoader(observed, pairdb, config, render_machine, batch_size=2)
        pred_eval(config, Predictor(config, net), loader, imdb, logger=logger, render_machine=render_machine)

    The reference reads, for every pair, the render of its initial pose that toolkit/LM6d_3_gen_PoseCNN_pred_rendered.py:149-155
    wrote to disk once. This one DRAWS it: every batch's initial poses are rendered on the device straight into uint8 / uint16
    frames with the bytes those files hold (Render_Py.render_frames_into), next to each pair's count of covered pixels.

    `observed`: the F camera frames as the decoder left them, a dict of host numpy arrays or a core/resident.ResidentObserved
    (observed_keys_of_test says which the configuration reads): image_observed (F,H,W,3) uint8 BGR; depth_observed /
    depth_gt_observed (F,H,W) uint16; mask_gt_observed / mask_observed / mask_observed_est (F,H,W) uint8 label maps. H x W is
    config.SCALES[0].
    `pairdb`: a list of P dicts with frame (index into the F frames), gt_class, mask_idx, pose_observed (3,4), pose_rendered
    (3,4) — the initial estimate, all −1 where the detector found nothing (tester.py:285-310) — and optionally K (3,3).

    Every batch is (data, frames, pair_records) as core/tester.pred_eval takes it. With `shared_frames` the batch holds N frames
    once and the pairs name them through a frame_index; without, one row per pair (the set's test_frames, core/resident.py). mask_idx,
    the render machine's class ids and the poses are uploaded; when a record has a K, the batch's (B,3,3) camera table too
    (frames["intrinsics"]), and the draw uses it. frames["rendered_covered"] lets get_pair_mask zero mask_observed of a pair whose
    draw is empty (image.py:301-303) on the device. With TEST.MASK_DILATE the thicknesses come from the device generator with
    the pair's index in `pairdb` as its draw id: a pair's draw depends on (seed, pair) alone. Nothing is read back.

    Differences from the reference: a frame goes up once, not per pair; batch_size > 1; the last batch is filled up by repeating
    its last pair, and the repeats' records are copies carrying "pad": True, which pred_eval leaves out of everything it counts
    (the reference hands the pad count to DataBatch); the mask-dilate draws are the device generator's; the empty-draw rule is
    applied on the device and not printed. Order: arange(P), or with `shuffle` a permutation from RandomState(seed), drawn anew
    at each reset().

    Refused: what resident.check_observed refuses in a dict, a frame that is not config.SCALES[0] or not the render machine's
    size, a pair whose frame is outside [0, F) or whose gt_class the render machine does not know, per-pair rows of a resident set
    whose frames are no multiple of 4 bytes, and shared_frames with network.INPUT_MASK off (the library's shared-frame zoom front
    end has no mask-less variant: pass shared_frames=False)."""
    __test__ = False          # a data iterator named after the reference's, not a pytest class

    def __init__(self, observed, pairdb, config, render_machine, batch_size=1, shuffle=False, seed=0, shared_frames=True):
        self.config, self.render_machine = config, render_machine
        self.batch_size, self.shuffle, self.seed, self.shared_frames = int(batch_size), bool(shuffle), int(seed), bool(shared_frames)
        if self.batch_size < 1:
            raise ValueError("TestDataLoader: batch_size must be >= 1")
        if self.shared_frames and not config.network.INPUT_MASK:
            raise NotImplementedError("TestDataLoader: shared_frames needs network.INPUT_MASK — the shared-frame zoom front end "
                                      "has no mask-less variant; pass shared_frames=False")
        self.resident = observed if isinstance(observed, ResidentObserved) else None
        have = observed if self.resident is None else observed.arrays
        self.keys = observed_keys_of_test(config, [k for k, v in have.items() if v is not None])
        self.set = obs = self.resident or HostObserved(observed, render_machine.ctx, self.keys)      # a dict: checked and wrapped
        if obs.ctx is not render_machine.ctx:
            raise ValueError("TestDataLoader: the resident set lives on another context")
        for k in self.keys:
            if k not in obs.arrays:
                raise KeyError("TestDataLoader: the observed set carries no '%s'" % k)
        if not self.shared_frames:
            obs.check_per_pair(self.keys)
        self.observed = obs.arrays           # numpy arrays over a host dict
        self.F, H, W = obs.M, obs.height, obs.width
        _image._check_size(config, H, W)
        if (render_machine.height, render_machine.width) != (H, W):
            raise ValueError("the render machine draws %dx%d, the frames are %dx%d" % (render_machine.height, render_machine.width, H, W))
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
        frames = self.set.test_frames(self.frame[pairs], self.keys, self.shared_frames)
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
