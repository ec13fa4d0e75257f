"""A device-resident observed set: the frames of a whole dataset uploaded ONCE, and the loaders' batches made from indices.

    res = ResidentObserved(observed, ctx, spare_rows=batch_size, points=points)
    loader = TrainDataLoader(res, config, render_machine, batch_size=..., ...)       # or TestDataLoader(res, pairdb, ...)

`observed` is the host dict the loaders take (core/loader.py). Every uint8 / uint16 frame array in it (or those named in `keys`)
becomes one device array of M + spare_rows rows; the small per-frame tables — pose_observed (M+spare,3,4) float32, mask_idx,
class_index and data_syn (M+spare) int32, each when the dict carries it — and, with `points` = {class id: ((3,N) model points,
(3,N) weights)}, two (n_classes,3,N) float32 tables with rows indexed by class id go up next to them. A whole LINEMOD training
set is about 1 200 frames x 2.5 MB = 3 GB, about 1 % of the card's memory. A batch is then a few hundred bytes of ids: the
BGR frames are read in place through deepim_ingest_bgr8_frames / _pool_frames, the depth and label maps through the
deepim_ingest_*_frames entries, and the table rows through deepim_gather_rows; no frame crosses PCIe again and no host gather
takes place.

The spare rows are a training loader's scratch for synthetic pairs: the pair at batch position b is drawn into row M + b
(`batch_rows`). In those rows mask_idx and data_syn are 1, as the synthetic pairs have them. One loader owns them at a time.

A set larger than the card is not handled: the constructor raises what the allocator raises.
"""
import weakref

import numpy as np

from ..runtime import DeviceArray, lib

FRAME_DTYPES = {"image_observed": np.uint8, "depth_observed": np.uint16, "depth_gt_observed": np.uint16,
                "mask_gt_observed": np.uint8, "mask_observed": np.uint8, "mask_observed_est": np.uint8}
COPY_BYTES = 256 << 20          # the most one host-to-device copy of the constructor moves


def batch_rows(pairs, M, R):
    """The rows of a resident set a training batch reads, no device needed → (frame_index (B,) int32, the synthetic positions).
    Pair p < M·R is observed frame p // R; pair p >= M·R is synthetic and, at batch position b, lives in spare row M + b."""
    pairs = np.asarray(pairs, np.int64).reshape(-1)
    real = pairs < int(M) * int(R)
    rows = np.where(real, pairs // int(R), int(M) + np.arange(len(pairs), dtype=np.int64))
    return rows.astype(np.int32), np.nonzero(~real)[0]


def _checked(observed, keys):
    """The host checks of both loaders on the frame arrays, no device needed → ({key: numpy array}, M, H, W)."""
    for k, v in observed.items():
        if isinstance(v, DeviceArray):
            raise TypeError("ResidentObserved: observed['%s'] is a device array; the set is built from host numpy arrays" % k)
    if keys is None:
        keys = [k for k in FRAME_DTYPES if observed.get(k) is not None]
    keys = list(keys)
    if "image_observed" not in keys:
        raise KeyError("ResidentObserved: the set holds at least 'image_observed'")
    keys.sort(key=lambda k: k != "image_observed")
    arrays = {}
    for k in keys:
        if k not in FRAME_DTYPES:
            raise KeyError("ResidentObserved: '%s' is not a frame array (%s)" % (k, ", ".join(FRAME_DTYPES)))
        if observed.get(k) is None:
            raise KeyError("ResidentObserved: observed carries no '%s'" % k)
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


def _spare(spare_rows):
    if int(spare_rows) < 0:
        raise ValueError("ResidentObserved: spare_rows must be >= 0")
    return int(spare_rows)


class ResidentObserved(object):
    def __init__(self, observed, ctx, keys=None, spare_rows=0, points=None):
        # every refusal comes before the device is touched
        spare = _spare(spare_rows)
        host, self.M, self.height, self.width = _checked(observed, keys)
        M = self.M
        self.host_tables = {}
        for k, dt, inner in (("pose_observed", np.float32, (3, 4)), ("mask_idx", np.int32, ()), ("class_index", np.int32, ()),
                             ("data_syn", bool, ())):
            if observed.get(k) is not None:
                v = np.asarray(observed[k])
                if v.size != M * int(np.prod(inner, dtype=np.int64)):
                    raise ValueError("observed['%s'] has %d values; %s expected" % (k, v.size, (M,) + inner))
                self.host_tables[k] = np.ascontiguousarray(v.astype(dt).reshape((M,) + inner))
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

    def gather(self, table, index, B):
        """out[b] = table[index[b]] on the device (deepim_gather_rows): table a DeviceArray of rows that are a multiple of
        4 bytes, index device int32 (B) → a DeviceArray of B rows, same dtype."""
        row_bytes = table.nbytes // table.shape[0]
        if row_bytes % 4:
            raise ValueError("gather: a row of %d bytes is not a multiple of 4 bytes" % row_bytes)
        out = self.ctx.empty((B,) + table.shape[1:], table.dtype)
        lib.deepim_gather_rows(self.ctx.handle, out, table, index, table.shape[0], row_bytes // 4, B)
        return out

    @property
    def nbytes(self):
        """device bytes of the frame arrays"""
        return sum(a.nbytes for a in self.arrays.values())

    @staticmethod
    def nbytes_of(observed, keys=None, spare_rows=0):
        """The device bytes the frame arrays of a set built from `observed` would take, no device needed."""
        spare = _spare(spare_rows)
        host, M, _H, _W = _checked(observed, keys)
        return sum((M + spare) * v[0].nbytes for v in host.values())


def _point_tables(points):
    """{class id: ((3,N) points, (3,N) weights)} → ((n_classes,3,N) float32 model table, weights table, the class ids), on the
    host; a class id without points is a zero row."""
    pts = {int(c): (np.ascontiguousarray(p, np.float32), np.ascontiguousarray(w, np.float32)) for c, (p, w) in points.items()}
    if not pts or min(pts) < 0:
        raise ValueError("ResidentObserved: points needs class ids >= 0")
    shape = next(iter(pts.values()))[0].shape
    if len(shape) != 2 or shape[0] != 3 or any(p.shape != shape or w.shape != shape for p, w in pts.values()):
        raise ValueError("ResidentObserved: every class's model points and weights must be (3,N) with one N")
    model, weights = np.zeros((max(pts) + 1,) + shape, np.float32), np.zeros((max(pts) + 1,) + shape, np.float32)
    for c, (p, w) in pts.items():
        model[c], weights[c] = p, w
    return model, weights, set(pts)
