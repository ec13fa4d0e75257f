"""The observed set both loaders (core/loader.py) read, in its two forms with one interface.

    loader = TrainDataLoader(observed, config, render_machine, ...)       # a host dict: the loader wraps it in a HostObserved
    res = ResidentObserved(observed, ctx, spare_rows=batch_size, points=points)
    loader = TrainDataLoader(res, config, render_machine, batch_size=..., ...)       # or TestDataLoader(res, pairdb, ...)

`observed` is a dict of host numpy arrays for M frames as the decoder left them: the frame arrays of FRAME_DTYPES, which
`check_observed` validates for everyone, and the small per-frame tables of TABLES. A set has M, height, width, ctx, `arrays`
(the checked frame arrays), `host_tables` (the per-frame tables on the host) and `point_classes`, and makes the observed side of
a batch: `train_batch` for the training loader, `test_frames` for the test loader. The loaders never ask which kind they hold.
"""
import weakref

import numpy as np

from ..lib.utils.synthetic_observed import runs
from ..runtime import DeviceArray, lib

FRAME_DTYPES = {"image_observed": np.uint8, "depth_observed": np.uint16, "depth_gt_observed": np.uint16,
                "mask_gt_observed": np.uint8, "mask_observed": np.uint8, "mask_observed_est": np.uint8}
TABLES = (("pose_observed", np.float32, (3, 4)), ("mask_idx", np.int32, ()), ("class_index", np.int32, ()), ("data_syn", bool, ()))
COPY_BYTES = 256 << 20          # the most one host-to-device copy of the constructor moves


def batch_rows(pairs, M, R):
    """The rows of a resident set a training batch reads, no device needed → (frame_index (B,) int32, the synthetic positions).
    Pair p < M·R is observed frame p // R; pair p >= M·R is synthetic and, at batch position b, lives in spare row M + b."""
    pairs = np.asarray(pairs, np.int64).reshape(-1)
    real = pairs < int(M) * int(R)
    rows = np.where(real, pairs // int(R), int(M) + np.arange(len(pairs), dtype=np.int64))
    return rows.astype(np.int32), np.nonzero(~real)[0]


def batch_frames(frame_ids):
    """The frames a shared-frame batch uploads, no device needed → (frames (N,) ascending distinct ids, frame_index (B,) int32):
    pair b looks at row frame_index[b] of the N <= B uploaded frames."""
    uniq, inv = np.unique(np.asarray(frame_ids, np.int64).reshape(-1), return_inverse=True)
    return uniq, inv.reshape(-1).astype(np.int32)


def check_observed(observed, keys=None):
    """The one check of an observed dict, no device needed → ({key: numpy array}, M, H, W) for the frame arrays `keys` (None:
    every frame array the dict carries). Refused: a device array anywhere in the dict (TypeError), a key that is missing or no
    frame array (KeyError), a dtype that is not the decoder's (TypeError), a shape that is not (M,H,W,3) / (M,H,W) with one
    M >= 1 (ValueError). An array that is not among `keys` is not looked at."""
    for k, v in observed.items():
        if isinstance(v, DeviceArray):
            raise TypeError("observed['%s'] is a device array; an observed set is built from host numpy arrays (a "
                            "ResidentObserved keeps them on the device)" % k)
    if keys is None:
        keys = [k for k in FRAME_DTYPES if observed.get(k) is not None]
    keys = list(keys)
    if "image_observed" not in keys:
        raise KeyError("an observed set holds at least 'image_observed'")
    keys.sort(key=lambda k: k != "image_observed")
    arrays = {}
    for k in keys:
        if k not in FRAME_DTYPES:
            raise KeyError("'%s' is not a frame array (%s)" % (k, ", ".join(FRAME_DTYPES)))
        if observed.get(k) is None:
            raise KeyError("observed carries no '%s'" % k)
        v = np.asarray(observed[k])
        if v.dtype != np.dtype(FRAME_DTYPES[k]):
            raise TypeError("observed['%s'] is %s; the decoded %s frame is expected" % (k, v.dtype, np.dtype(FRAME_DTYPES[k])))
        arrays[k] = v
    img = arrays["image_observed"]
    if img.ndim != 4 or img.shape[3] != 3 or img.shape[0] < 1:
        raise ValueError("observed['image_observed'] has shape %s; (M,H,W,3) expected" % (img.shape,))
    M, H, W = img.shape[:3]
    for k in keys[1:]:
        if arrays[k].shape != (M, H, W):
            raise ValueError("observed['%s'] has shape %s; %s expected" % (k, arrays[k].shape, (M, H, W)))
    return arrays, M, H, W


def _host_tables(observed, M, names):
    """The per-frame tables `names` the dict carries, in the dtypes and shapes of TABLES."""
    out = {}
    for k, dt, inner in TABLES:
        if k in names and observed.get(k) is not None:
            v = np.asarray(observed[k])
            if v.size != M * int(np.prod(inner, dtype=np.int64)):
                raise ValueError("observed['%s'] has %d values; %s expected" % (k, v.size, (M,) + inner))
            out[k] = np.ascontiguousarray(v.astype(dt).reshape((M,) + inner))
    return out


def _point_clouds(points):
    return {int(c): (np.ascontiguousarray(p, np.float32), np.ascontiguousarray(w, np.float32)) for c, (p, w) in points.items()}


class HostObserved(object):
    """The set as host numpy arrays: what a loader makes of a plain dict. `tables`: the per-frame tables it reads. A batch is
    gathered on the host and uploaded, 1 or 2 bytes per value; nothing is uploaded before the first batch."""

    def __init__(self, observed, ctx, keys, tables=()):
        self.arrays, self.M, self.height, self.width = check_observed(observed, keys)
        self.host_tables = _host_tables(observed, self.M, tables)
        self.ctx, self.point_classes = ctx, None

    def set_points(self, points):
        """`points` = {class id: ((3,N) model points, (3,N) weights)}: stacked and uploaded per batch."""
        self.point_classes = _point_clouds(points)

    def set_data_syn(self, data_syn):
        """The data_syn flags of the M frames; None: no frame is flagged and a batch without synthetic pairs hands none over."""
        if data_syn is not None:
            self.host_tables["data_syn"] = np.asarray(data_syn).astype(bool).reshape(self.M)

    def claim_spare_rows(self, owner, rows):
        """Nothing to claim: a synthetic pair is drawn into the batch's own arrays."""

    def check_per_pair(self, keys):
        """Nothing to refuse: the per-pair rows of a test batch are indexed on the host, whatever a frame's size."""

    def _upload(self, key, m, real):
        """The batch's device array of arrays[key]: row b is frame m[b] where real[b]; the other rows are left for the generator.
        A batch of real rows is one upload, else one upload per run of real rows."""
        src = self.arrays[key]
        if real.all():
            return self.ctx.array(src[m], dtype=FRAME_DTYPES[key])      # 1 or 2 bytes per value cross PCIe
        out = self.ctx.empty((len(m),) + src.shape[1:], FRAME_DTYPES[key])
        for j0, j1, r0 in runs(np.nonzero(real)[0]):
            out[r0:r0 + (j1 - j0)].copyfrom(src[m[r0:r0 + (j1 - j0)]])
        return out

    def train_batch(self, pairs, draw_ids, R, keys, cls_syn, draw, own_depth):
        """The observed side of a training batch → (frames, ids, table, points): the `frames` dict lib/utils/image.py reads, the
        draw ids on the device, table(name) → the batch's rows of a per-frame table, points(class_index) → its point clouds.
        Row b is frame pairs[b] // R, indexed on the host and uploaded. The synthetic pairs (pairs >= M·R, of classes `cls_syn`)
        are drawn by `draw` (the keywords of SyntheticObserved.frames) into the batch's own arrays at their batch positions, and
        their table rows are patched on the host: mask_idx 1, the class, a zero pose, data_syn true. own_depth: depth_observed
        of a synthetic row is its depth_gt_observed."""
        ctx, t, real = self.ctx, self.host_tables, pairs < self.M * R
        m, syn = np.where(real, pairs // R, 0), np.nonzero(~real)[0]
        mask_idx, cls, pose = t["mask_idx"][m], t["class_index"][m], t["pose_observed"][m]
        if syn.size:
            mask_idx[syn], cls[syn], pose[syn] = 1, cls_syn, 0.0
        frames = {k: self._upload(k, m, real) for k in keys}
        frames["mask_idx"] = ctx.array(mask_idx, dtype=np.int32)
        ids, pose = ctx.array(draw_ids, dtype=np.uint64), ctx.array(pose)
        if syn.size:
            draw(class_index=cls_syn, draw_ids=draw_ids[syn], rows=syn, out=dict(frames, pose_observed=pose))
            if own_depth:
                for j0, j1, r0 in runs(syn):
                    frames["depth_observed"][r0:r0 + (j1 - j0)].copyfrom(frames["depth_gt_observed"][r0:r0 + (j1 - j0)])

        def table(name):
            if name != "data_syn":
                return pose if name == "pose_observed" else ctx.array(cls, dtype=np.int32)
            always = t["data_syn"][m] if "data_syn" in t else None       # host flags: background_draws_device uploads them
            if syn.size:
                always = np.zeros(len(m), bool) if always is None else always
                always[syn] = True
            return always

        def points(_class_index):
            return tuple(ctx.array(np.stack([self.point_classes[int(c)][i] for c in cls])) for i in (0, 1))
        return frames, ids, table, points

    def test_frames(self, frame_ids, keys, shared):
        """The observed frames of a test batch: with `shared` its distinct frames, uploaded once, and the frame_index that names
        them; else one uploaded row per pair."""
        frames, rows = {}, frame_ids
        if shared:
            rows, index = batch_frames(frame_ids)
            frames["frame_index"] = self.ctx.array(index, dtype=np.int32)
        for k in keys:
            frames[k] = self.ctx.array(self.arrays[k][rows], dtype=FRAME_DTYPES[k])       # 1 or 2 bytes per value cross PCIe
        return frames


def _spare(spare_rows):
    if int(spare_rows) < 0:
        raise ValueError("ResidentObserved: spare_rows must be >= 0")
    return int(spare_rows)


class ResidentObserved(object):
    """The set on the device: the frames of a whole dataset uploaded ONCE, and the loaders' batches made from indices.

    Every uint8 / uint16 frame array of the dict (or those named in `keys`) becomes one device array of M + spare_rows rows; the
    per-frame tables — pose_observed (M+spare,3,4) float32, mask_idx, class_index and data_syn (M+spare) int32, each when the
    dict carries it — and, with `points` = {class id: ((3,N) model points, (3,N) weights)}, two (n_classes,3,N) float32 tables
    with rows indexed by class id go up next to them. A whole LINEMOD training set is about 1 200 frames x 2.5 MB = 3 GB, about
    1 % of the card's memory. A batch is then a few hundred bytes of ids: frame_index (B int32), the draw ids (B uint64) and,
    with synthetic pairs, their positions and class ids. The BGR frames are read in place through deepim_ingest_bgr8_frames /
    _pool_frames, the depth and label maps through the deepim_ingest_*_frames entries, and the table rows through
    deepim_gather_rows; no frame crosses PCIe again and no host gather takes place.

    The spare rows are a training loader's scratch for synthetic pairs: the pair at batch position b is drawn into row M + b
    (`batch_rows`). In those rows mask_idx and data_syn are 1, as the synthetic pairs have them. One loader owns them at a time,
    which is safe on one stream: batch k's ingest is queued before batch k+1's draw and a batch keeps fp32 copies only.

    Every refusal comes before the device is touched. A set larger than the card is not handled: the constructor raises what
    the allocator raises."""

    def __init__(self, observed, ctx, keys=None, spare_rows=0, points=None):
        spare = _spare(spare_rows)
        host, self.M, self.height, self.width = check_observed(observed, keys)
        M = self.M
        self.host_tables = _host_tables(observed, M, [k for k, _dt, _inner in TABLES])
        point_tables = None if points is None else _point_tables(points)
        if ctx is None:
            raise ValueError("ResidentObserved: a device context is needed")
        self.ctx, self.spare_rows, self.rows = ctx, spare, M + spare
        self.keys = list(host)
        self.arrays = {}
        for k, v in host.items():
            dev = ctx.empty((self.rows,) + v.shape[1:], FRAME_DTYPES[k])
            step = max(1, COPY_BYTES // max(1, v[0].nbytes))
            for r0 in range(0, M, step):          # bounded slices: no second host copy of the set
                dev[r0:min(M, r0 + step)].copyfrom(v[r0:min(M, r0 + step)])
            if spare:
                tail = dev[M:self.rows]
                lib.deepim_memset(ctx.handle, tail, 0, tail.nbytes)
            self.arrays[k] = dev
        self.tables = {}
        for k, v in self.host_tables.items():
            self._upload_table(k, v)
        self.point_tables = self.point_classes = None
        if point_tables is not None:
            self._upload_points(point_tables)
        self._spare_owner = None

    def _upload_table(self, k, v):
        """A per-frame table with its spare rows as the synthetic pairs have them: mask_idx 1, data_syn 1, the rest 0."""
        fill = 1 if k in ("mask_idx", "data_syn") else 0
        full = np.full((self.rows,) + v.shape[1:], fill, np.float32 if k == "pose_observed" else np.int32)
        full[:self.M] = v
        self.tables[k] = self.ctx.array(full, dtype=full.dtype)

    def _upload_points(self, point_tables):
        model, weights, classes = point_tables
        self.point_tables = (self.ctx.array(model), self.ctx.array(weights))
        self.point_classes = classes

    def set_points(self, points):
        """Upload the per-class point tables after construction (a loader given `points` for a set built without them)."""
        self._upload_points(_point_tables(points))

    def set_data_syn(self, data_syn):
        """The data_syn flags of the M frames (None: all False) as the device table, spare rows 1."""
        v = np.zeros(self.M, bool) if data_syn is None else np.asarray(data_syn).astype(bool).reshape(self.M)
        self.host_tables["data_syn"] = v
        self._upload_table("data_syn", v)

    def claim_spare_rows(self, owner, rows):
        """`owner` (a loader) takes the spare rows as its scratch; they stay its own for as long as it lives."""
        if rows > self.spare_rows:
            raise ValueError("ResidentObserved: %d spare rows are needed (spare_rows >= batch_size), the set has %d"
                             % (rows, self.spare_rows))
        held = self._spare_owner() if self._spare_owner is not None else None
        if held is not None and held is not owner:
            raise ValueError("ResidentObserved: the spare rows of this set are already claimed by another loader")
        self._spare_owner = weakref.ref(owner)

    def check_per_pair(self, keys):
        """The per-pair rows of a test batch are gathered on the device in 4-byte words."""
        for k in keys:
            if (self.arrays[k].nbytes // self.rows) % 4:
                raise ValueError("a '%s' frame of %d bytes is not a multiple of 4 bytes; the per-pair rows of a resident set are "
                                 "gathered in 4-byte words" % (k, self.arrays[k].nbytes // self.rows))

    def gather(self, table, index, B):
        """out[b] = table[index[b]] on the device (deepim_gather_rows): table a DeviceArray of rows that are a multiple of
        4 bytes, index device int32 (B) → a DeviceArray of B rows, same dtype."""
        row_bytes = table.nbytes // table.shape[0]
        if row_bytes % 4:
            raise ValueError("gather: a row of %d bytes is not a multiple of 4 bytes" % row_bytes)
        out = self.ctx.empty((B,) + table.shape[1:], table.dtype)
        lib.deepim_gather_rows(self.ctx.handle, out, table, index, table.shape[0], row_bytes // 4, B)
        return out

    def train_batch(self, pairs, draw_ids, R, keys, cls_syn, draw, own_depth):
        """HostObserved.train_batch from indices: frame_index and the draw ids go up, every frame is read in place through
        frame_index and every table row is gathered on the device. The synthetic pair at batch position b is drawn into spare
        row M + b of the set's own arrays and pose table; its class lands in the table's row next to the mask_idx = data_syn = 1
        set once, so only the positions and the class ids go up with it."""
        ctx = self.ctx
        rows, syn = batch_rows(pairs, self.M, R)
        B = len(rows)
        fi, ids = ctx.array(rows, dtype=np.int32), ctx.array(draw_ids, dtype=np.uint64)
        if syn.size:
            cls_syn = ctx.array(cls_syn, dtype=np.int32)
            if syn.size == B:
                ids_syn, rows_syn = ids, fi
            else:
                at = ctx.array(syn, dtype=np.int32)
                ids_syn = self.gather(ids.reshape((B, 1)), at, syn.size).reshape((syn.size,))
                rows_syn = self.gather(fi, at, syn.size)
            out = {k: self.arrays[k] for k in keys}       # depth_observed only with INPUT_DEPTH, as over a host set
            draw(class_index=cls_syn, draw_ids=ids_syn, rows=rows[syn], rows_device=rows_syn,
                 out=dict(out, pose_observed=self.tables["pose_observed"]))
            for j0, j1, r0 in runs(rows[syn]):
                self.tables["class_index"][r0:r0 + (j1 - j0)].copyfrom(cls_syn[j0:j1])
                if own_depth:
                    self.arrays["depth_observed"][r0:r0 + (j1 - j0)].copyfrom(self.arrays["depth_gt_observed"][r0:r0 + (j1 - j0)])

        def table(name):
            return self.gather(self.tables[name], fi, B) if name in self.tables else None

        def points(class_index):
            return self.gather(self.point_tables[0], class_index, B), self.gather(self.point_tables[1], class_index, B)
        frames = dict({k: self.arrays[k] for k in keys}, frame_index=fi, mask_idx=table("mask_idx"))
        return frames, ids, table, points

    def test_frames(self, frame_ids, keys, shared):
        """The observed frames of a test batch: the ids go up; with `shared` the frames are the set's own arrays (N = M) under
        frame_index = frame_ids, else the per-pair rows are gathered on the device."""
        index = self.ctx.array(frame_ids, dtype=np.int32)
        frames = {"frame_index": index} if shared else {}
        for k in keys:
            frames[k] = self.arrays[k] if shared else self.gather(self.arrays[k], index, len(frame_ids))
        return frames

    @property
    def nbytes(self):
        """device bytes of the frame arrays"""
        return sum(a.nbytes for a in self.arrays.values())

    @staticmethod
    def nbytes_of(observed, keys=None, spare_rows=0):
        """The device bytes the frame arrays of a set built from `observed` would take, no device needed."""
        spare = _spare(spare_rows)
        host, M, _H, _W = check_observed(observed, keys)
        return sum((M + spare) * v[0].nbytes for v in host.values())


def _point_tables(points):
    """{class id: ((3,N) points, (3,N) weights)} → ((n_classes,3,N) float32 model table, weights table, the class ids), on the
    host; a class id without points is a zero row."""
    pts = _point_clouds(points)
    if not pts or min(pts) < 0:
        raise ValueError("ResidentObserved: points needs class ids >= 0")
    shape = next(iter(pts.values()))[0].shape
    if len(shape) != 2 or shape[0] != 3 or any(p.shape != shape or w.shape != shape for p, w in pts.values()):
        raise ValueError("ResidentObserved: every class's model points and weights must be (3,N) with one N")
    model, weights = np.zeros((max(pts) + 1,) + shape, np.float32), np.zeros((max(pts) + 1,) + shape, np.float32)
    for c, (p, w) in pts.items():
        model[c], weights[c] = p, w
    return model, weights, set(pts)
