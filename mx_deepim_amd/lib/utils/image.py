"""Mirror of the tensor-making half of lib/utils/image.py on the device: `transform` (:583-594), `get_pair_image` (:58-163),
`get_gt_observed_depth` (:166-187), `get_pair_depth` (:190-227) and `get_pair_mask` (:230-399), computed by the ingest kernels
(csrc/ingest.hip) from frames as the decoder left them — uint8 BGR images, uint16 depth maps, uint8 label maps — so 1 or 2
bytes per value cross PCIe and no host arithmetic stands between a camera and the graph.

Where the reference takes a `pairdb` of file paths, these take `frames`: a dict of DECODED arrays, each a device array or a
numpy array (uploaded as it is, never converted on the host), for a batch of B pairs:

    image_observed, image_rendered        (B,H,W,3) uint8, BGR (cv2.imread)
    bg_image                              (B,H,W,3) uint8, optional: the background already cropped and resized to the frame
                                          (image.py:108-145 is cv2 work); composited under mask_gt_observed != 0 (:147-155),
                                          for the samples with use_bg != 0 (int32 (B), optional: every sample)
    depth_observed, depth_rendered, depth_gt_observed     (B,H,W) uint16
    mask_gt_observed, mask_observed, mask_observed_est    (B,H,W) uint8 label maps
    mask_idx                              (B) int32: the pair's label value (pair_rec["mask_idx"])
    bg_pool, bg_index                     instead of bg_image: a lib/utils/background.BackgroundPool of decoded images of any
                                          sizes, uploaded once, and (B) int32, the image each pair composites (with use_bg
                                          as above). The crop, the resize and the padding of image.py:108-145 happen inside the
                                          composite (deepim_ingest_bgr8_pool): no resized background exists in memory
    mask_dilate_thickness                 (B,4) int32 from lib/utils/mask_dilate.mask_dilate_draws, for MASK_DILATE

A dict that carries `frame_index` is a SHARED-FRAME batch: several objects in one camera frame (Occluded LINEMOD, YCB-style
scenes, a detector front end). The observed side then holds N <= B frames once, as the decoder left them, and pair b looks at
frame frame_index[b]:

    frame_index                           (B) int32, numpy or device
    image_observed                        (N,H,W,3) uint8, BGR
    depth_observed, depth_gt_observed     (N,H,W) uint16
    mask_gt_observed, mask_observed, mask_observed_est    (N,H,W) uint8 label maps
    image_rendered, depth_rendered, pose_rendered, mask_idx, mask_dilate_thickness     per pair, (B,...) as above

No fp32 copy of an observed image or depth map is made for the network: `observed_frames` hands the frames themselves to the
zoom front end (deepim_zoom_concat_frames_forward), which gathers its taps from them in every iteration. The per-pair masks and
the flow ground truth's depth are still (B,1,H,W) tensors (deepim_ingest_label_mask_frames / deepim_ingest_depth16_frames). A
numpy frame_index is range-checked on the host before anything is launched (ValueError naming the pair); a device one cannot
be: a pair whose id is outside [0, N) sees an empty frame and sets bit 4 of the status word. Shared frames are test-phase only:
`get_pair_image` (which would have to make the fp32 copies), bg_image and the training loader refuse them.

File decoding and the cv2 resize (:552-580) of the observed and rendered frames are the caller's: a frame whose size is not
config.SCALES[0] is refused. A background is cropped and resized on the device from a bg_pool (lib/utils/background.py, which
also draws use_bg and bg_index for the training loader); a bg_image is taken as the caller made it. A bg_index is never read
by the host: one outside the pool gives that pair a black background and sets bit 5 of the status word. The test phase's `np.sum(depth_rendered) == 0` guard (:301-303) is a host decision per pair and is
the caller's too — unless the frames carry "rendered_covered" (device int32 (B): each pair's count of non-zero depth_rendered
pixels, which Render_Py.render_frames_into writes next to the frames it draws; core/loader.TestDataLoader hands it over): then
`get_pair_mask` zeroes mask_observed of the pairs with a count of 0 on the device (deepim_mask_gate), before TEST.MASK_DILATE.
An empty rectangle source gives zeros and sets bit 2 of the status word (deepim_zoom_status).

The kernels are asynchronous on the context's stream. These wrappers stay asynchronous when frames, ids and draws are device
arrays; a numpy input is uploaded with a synchronous copy into a temporary whose release synchronises the stream again.
"""
import ctypes

import numpy as np

from ...runtime import Context, DeviceArray, lib
from .mask_dilate import mask_dilate_batch


def _context(frames):
    for v in frames.values():
        if isinstance(v, DeviceArray):
            return v.context
    return Context.default()


def _frame(ctx, frames, key, dtype, inner=()):
    """frames[key] as a device array of `dtype`, shape (B,H,W)+inner; numpy input is uploaded in its own dtype."""
    if key not in frames or frames[key] is None:
        raise KeyError("frames carry no '%s'" % key)
    v = frames[key]
    if not isinstance(v, DeviceArray):
        v = np.asarray(v)
        if v.dtype != np.dtype(dtype):
            raise TypeError("frames['%s'] is %s; the decoded %s frame is expected" % (key, v.dtype, np.dtype(dtype)))
        v = ctx.array(v, dtype=dtype)
    if v.dtype != np.dtype(dtype):
        raise TypeError("frames['%s'] is %s; the decoded %s frame is expected" % (key, v.dtype, np.dtype(dtype)))
    if v.ndim != 3 + len(inner) or v.shape[3:] != tuple(inner):
        raise ValueError("frames['%s'] has shape %s; (B,H,W%s) expected" % (key, v.shape, "".join(",%d" % i for i in inner)))
    return v


def _ids(ctx, frames, key, B, cols=None):
    """frames[key] as a device int32 array of B rows (never read back)."""
    if key not in frames or frames[key] is None:
        raise KeyError("frames carry no '%s'" % key)
    v = frames[key]
    if not isinstance(v, DeviceArray):
        v = ctx.array(np.asarray(v).reshape((B,) if cols is None else (B, cols)), dtype=np.int32)
    if v.dtype != np.int32 or v.size != B * (cols or 1):
        raise TypeError("frames['%s'] must be int32 with %d values" % (key, B * (cols or 1)))
    return v


SHARED_KEYS = ("image_observed", "depth_observed", "depth_gt_observed", "mask_gt_observed", "mask_observed", "mask_observed_est")


def is_shared(frames):
    """Whether `frames` is a shared-frame batch (module docstring): it carries a frame_index."""
    return frames.get("frame_index") is not None


def check_frame_index(frames):
    """The host half of a shared-frame batch, no device needed → (B, N). The shared arrays must agree on N; a numpy frame_index
    must lie in [0, N) — ValueError naming the first offending pair. A device frame_index is never read: the kernels guard it."""
    counts = {k: int(frames[k].shape[0] if isinstance(frames[k], DeviceArray) else np.shape(frames[k])[0])
              for k in SHARED_KEYS if frames.get(k) is not None}
    if not counts:
        raise KeyError("a shared-frame batch carries at least one of %s" % ", ".join(SHARED_KEYS))
    N = max(counts.values())
    if min(counts.values()) != N or N < 1:
        raise ValueError("the shared arrays of the batch disagree on the number of frames (or have none): %s" % counts)
    fi = frames["frame_index"]
    if isinstance(fi, DeviceArray):
        if fi.dtype != np.int32:
            raise TypeError("frames['frame_index'] on the device must be int32")
        return int(fi.size), N
    fi = np.asarray(fi)
    if fi.dtype.kind not in "iu":
        raise TypeError("frames['frame_index'] is %s; integer frame numbers are expected" % fi.dtype)
    fi = fi.reshape(-1)
    bad = np.nonzero((fi < 0) | (fi >= N))[0]
    if bad.size:
        raise ValueError("frame_index[%d] = %d: pair %d looks at a frame outside the batch's %d shared frame%s"
                         % (bad[0], fi[bad[0]], bad[0], N, "" if N == 1 else "s"))
    return int(fi.size), N


def _frame_index(ctx, frames):
    """→ (device int32 (B) frame_index, B, N) of a shared-frame batch, after the host checks."""
    B, N = check_frame_index(frames)
    fi = frames["frame_index"]
    if not isinstance(fi, DeviceArray):
        fi = ctx.array(np.asarray(fi).reshape(B), dtype=np.int32)
    return fi, B, N


class ObservedFrames(object):
    """The observed side of a shared-frame batch as the zoom front end reads it (data["observed_frames"]), all on the device:
    image (N,H,W,3) uint8 BGR and frame_index (B) int32; with network.INPUT_DEPTH depth (N,H,W) uint16 and depth_factor, and
    with network.MASK_INPUTS labels (N,H,W) uint8 + mask_idx (B) int32, outside of which the depth is zero."""

    def __init__(self, image, frame_index, depth=None, labels=None, mask_idx=None, depth_factor=1000.0):
        self.image, self.frame_index, self.depth, self.labels, self.mask_idx = image, frame_index, depth, labels, mask_idx
        self.depth_factor = float(depth_factor)
        self.context = image.context

    @property
    def n_frames(self):
        return self.image.shape[0]

    @property
    def n_pairs(self):
        return self.frame_index.size

    def nbytes(self):
        """device bytes the observed side of the batch occupies"""
        return sum(a.nbytes for a in (self.image, self.frame_index, self.depth, self.labels, self.mask_idx) if a is not None)


def observed_frames(frames, config, phase="test"):
    """The observed half of `get_pair_image` / `get_pair_depth` for a shared-frame batch → ObservedFrames: the uint8 / uint16
    frames go to the device as they are (or stay there) and nothing is converted."""
    if phase != "test":
        raise NotImplementedError("shared frames (frames['frame_index']) are a test-phase input: the training loader is per pair")
    ctx = _context(frames)
    fi, B, N = _frame_index(ctx, frames)
    obs = _frame(ctx, frames, "image_observed", np.uint8, (3,))
    _check_size(config, obs.shape[1], obs.shape[2])
    depth = labels = idx = None
    if config.network.INPUT_DEPTH:
        depth = _frame(ctx, frames, "depth_observed", np.uint16)
        if depth.shape != obs.shape[:3]:
            raise ValueError("depth_observed %s and image_observed %s differ in shape" % (depth.shape, obs.shape))
        if config.network.get("MASK_INPUTS", False):
            key = "mask_gt_observed" if config.dataset.get("MASK_GT", False) else "mask_observed_est"      # get_pair_depth
            labels = _frame(ctx, frames, key, np.uint8)
            if labels.shape != depth.shape:
                raise ValueError("frames['%s'] and frames['depth_observed'] differ in shape" % key)
            idx = _ids(ctx, frames, "mask_idx", B)
    return ObservedFrames(obs, fi, depth, labels, idx, _depth_factor(config).value)


def _check_size(config, H, W):
    if (H, W) != tuple(int(s) for s in config.SCALES[0]):
        raise ValueError("frame size %dx%d is not config.SCALES[0] = %s: the resize of image.py:552-580 is not part of the "
                         "device path — resize before handing the frames over" % (H, W, tuple(config.SCALES[0])))


def _depth_factor(config):
    return ctypes.c_float(float(config.dataset.get("DEPTH_FACTOR", 1000)))


def _ingest_bgr8(ctx, frames_bgr, means_rgb, frame_index=None, bg=None, fg=None, use_bg=None, bg_index=None, pool=None):
    """The four BGR entries behind one body → (B,3,H,W) fp32. frame_index (device int32 (B), never read by the host): pair b
    reads frame frame_index[b] of frames_bgr (N,H,W,3) and fg (N,H,W), which stay where they are; None: B = N and its own.
    pool: a BackgroundPool, composited by the pair's bg_index; else bg, the ready-made (B,H,W,3) backgrounds, or none."""
    N, H, W, _ = frames_bgr.shape
    B = N if frame_index is None else frame_index.size
    if frame_index is not None and frame_index.dtype != np.int32:
        raise TypeError("frame_index on the device must be int32")
    means = None if means_rgb is None else np.ascontiguousarray(means_rgb, dtype=np.float32).reshape(3)
    if pool is not None:
        if (pool.height, pool.width) != (H, W):
            raise ValueError("the background pool was built for %dx%d frames, these are %dx%d" % (pool.height, pool.width, H, W))
        if frame_index is not None and (fg is None or fg.shape != (N, H, W)):
            raise ValueError("the pool composite of shared frames needs fg labels of shape %s" % ((N, H, W),))
        tail = (use_bg, bg_index, pool.pixels, pool.desc, pool.xtab, pool.ytab, len(pool), means, B, H, W)
    out = ctx.empty((B, 3, H, W))
    if pool is None and frame_index is None:
        lib.deepim_ingest_bgr8(ctx.handle, out, frames_bgr, bg, fg, use_bg, means, B, H, W)
    elif pool is None:
        lib.deepim_ingest_bgr8_frames(ctx.handle, out, frames_bgr, frame_index, N, means, B, H, W)
    elif frame_index is None:
        lib.deepim_ingest_bgr8_pool(ctx.handle, out, frames_bgr, fg, *tail)
    else:
        lib.deepim_ingest_bgr8_pool_frames(ctx.handle, out, frames_bgr, fg, frame_index, N, *tail)
    return out


def transform_batch(ctx, frames_bgr, means_rgb=None, bg=None, fg=None, use_bg=None):
    """(B,H,W,3) uint8 BGR device frames → (B,3,H,W) fp32, channel i = image channel 2-i minus means_rgb[i]."""
    return _ingest_bgr8(ctx, frames_bgr, means_rgb, bg=bg, fg=fg, use_bg=use_bg)


def transform_batch_pool(ctx, frames_bgr, means_rgb, fg, use_bg, bg_index, pool):
    """transform_batch with the background of image.py:108-155 from a BackgroundPool: where fg (B,H,W) uint8 is 0, in the pairs
    with use_bg != 0 (device int32 (B), None: every pair), the pixel is image bg_index[b] (device int32 (B)) of the pool,
    cropped, resized and padded to the frame inside the kernel."""
    return _ingest_bgr8(ctx, frames_bgr, means_rgb, fg=fg, use_bg=use_bg, bg_index=bg_index, pool=pool)


def image_observed(ctx, frames, config, use_bg=None, bg_index=None, pool=None):
    """frames["image_observed"] → device (B,3,H,W), RGB minus the pixel means; with `pool` on the pool's backgrounds outside
    mask_gt_observed, as transform_batch_pool. In a shared-frame batch the frames are (N,H,W,3) and pair b reads frame
    frame_index[b] without a gather (deepim_ingest_bgr8_frames / _pool_frames); use_bg and bg_index stay per pair."""
    obs = _frame(ctx, frames, "image_observed", np.uint8, (3,))
    fi = _frame_index(ctx, frames)[0] if is_shared(frames) else None
    fg = None if pool is None else _frame(ctx, frames, "mask_gt_observed", np.uint8)
    return _ingest_bgr8(ctx, obs, _means_rgb(config), fi, fg=fg, use_bg=use_bg, bg_index=bg_index, pool=pool)


def transform(im, pixel_means):
    """image.py:583-594: im [height, width, channel] uint8 in BGR, pixel_means in the image's BGR order → numpy
    [1, channel, height, width] in RGB order, computed on the default device in fp32 (the reference computes in float64)."""
    ctx = Context.default()
    im = np.ascontiguousarray(im)
    if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
        raise TypeError("transform: a (height, width, 3) uint8 image is expected")
    means = np.asarray(pixel_means, dtype=np.float64).reshape(-1)[[2, 1, 0]]     # batch_updater_py_multi.py:24
    return transform_batch(ctx, ctx.array(im[np.newaxis], dtype=np.uint8), means).asnumpy()


def _means_rgb(config):
    return np.asarray(config.network.PIXEL_MEANS, dtype=np.float64).reshape(-1)[[2, 1, 0]]


def get_pair_image(frames, config, phase="train"):
    """image.py:58-163 → (image_observed, image_rendered), device (B,3,H,W). In the train phase, frames with a "bg_image" get the
    observed background replaced where mask_gt_observed == 0 (:147-155); frames with a "bg_pool" and a "bg_index" get it from the
    pool's image bg_index[b], cropped and resized as :108-145 do (transform_batch_pool)."""
    if is_shared(frames):
        raise NotImplementedError("get_pair_image would make B fp32 copies of the shared frames (frames['frame_index']): use "
                                  "observed_frames for the observed side and get_rendered_image for image_rendered")
    ctx = _context(frames)
    obs = _frame(ctx, frames, "image_observed", np.uint8, (3,))
    ren = _frame(ctx, frames, "image_rendered", np.uint8, (3,))
    B, H, W, _ = obs.shape
    _check_size(config, H, W)
    if ren.shape != obs.shape:
        raise ValueError("image_rendered %s and image_observed %s differ in shape" % (ren.shape, obs.shape))
    means = _means_rgb(config)
    bg = fg = use_bg = None
    if frames.get("bg_pool") is not None:
        if frames.get("bg_image") is not None:
            raise ValueError("frames carry both a bg_image and a bg_pool: one background per pair")
        if phase == "train":
            fg = _frame(ctx, frames, "mask_gt_observed", np.uint8)
            if fg.shape != obs.shape[:3]:
                raise ValueError("mask_gt_observed does not match image_observed's shape")
            if frames.get("use_bg") is not None:
                use_bg = _ids(ctx, frames, "use_bg", B)
            observed = transform_batch_pool(ctx, obs, means, fg, use_bg, _ids(ctx, frames, "bg_index", B), frames["bg_pool"])
            return observed, transform_batch(ctx, ren, means)
    if phase == "train" and frames.get("bg_image") is not None:
        bg = _frame(ctx, frames, "bg_image", np.uint8, (3,))
        fg = _frame(ctx, frames, "mask_gt_observed", np.uint8)
        if bg.shape != obs.shape or fg.shape != obs.shape[:3]:
            raise ValueError("bg_image / mask_gt_observed do not match image_observed's shape")
        if frames.get("use_bg") is not None:
            use_bg = _ids(ctx, frames, "use_bg", B)
    return transform_batch(ctx, obs, means, bg, fg, use_bg), transform_batch(ctx, ren, means)


def get_rendered_image(frames, config):
    """The rendered half of `get_pair_image` → image_rendered, device (B,3,H,W): per pair in every kind of batch."""
    ctx = _context(frames)
    ren = _frame(ctx, frames, "image_rendered", np.uint8, (3,))
    _check_size(config, ren.shape[1], ren.shape[2])
    return transform_batch(ctx, ren, _means_rgb(config))


def _depth(ctx, frames, key, config, label_key=None):
    """frames[key] / DEPTH_FACTOR → device (B,1,H,W), zeroed outside the pair's label of frames[label_key]. In a shared-frame
    batch the observed maps are (N,H,W) and pair b reads frame frame_index[b] (deepim_ingest_depth16_frames)."""
    d = _frame(ctx, frames, key, np.uint16)
    B, H, W = d.shape
    _check_size(config, H, W)
    shared = is_shared(frames) and key in SHARED_KEYS
    if shared:
        fi, B, N = _frame_index(ctx, frames)
    labels = idx = None
    if label_key is not None:
        labels = _frame(ctx, frames, label_key, np.uint8)
        if labels.shape != d.shape:
            raise ValueError("frames['%s'] and frames['%s'] differ in shape" % (label_key, key))
        idx = _ids(ctx, frames, "mask_idx", B)
    out = ctx.empty((B, 1, H, W))
    if shared:
        lib.deepim_ingest_depth16_frames(ctx.handle, out, d, labels, fi, idx, _depth_factor(config), N, B, H, W)
    else:
        lib.deepim_ingest_depth16(ctx.handle, out, d, labels, idx, _depth_factor(config), B, H, W)
    return out


def get_gt_observed_depth(frames, config, phase="train"):
    """image.py:166-187 → depth_gt_observed, device (B,1,H,W) in metres."""
    return _depth(_context(frames), frames, "depth_gt_observed", config)


def get_pair_depth(frames, config, phase="train"):
    """image.py:190-227 → (depth_observed, depth_rendered). With network.MASK_INPUTS the observed depth is zeroed outside the
    pair's label (:204-211): mask_gt_observed in the train phase or with dataset.MASK_GT, else mask_observed_est."""
    ctx = _context(frames)
    label_key = None
    if config.network.get("MASK_INPUTS", False):
        if config.TRAIN.get("MASK_SYN", False) and phase == "train":
            raise NotImplementedError("TRAIN.MASK_SYN (image.py:205-206) is not part of the device path")
        label_key = "mask_gt_observed" if (config.dataset.get("MASK_GT", False) or phase == "train") else "mask_observed_est"
    return _depth(ctx, frames, "depth_observed", config, label_key), _depth(ctx, frames, "depth_rendered", config)


def label_mask(ctx, frames, key):
    """`label == mask_idx` (image.py:255-260, :308-312) → device (B,1,H,W) of 0 / 1. In a shared-frame batch the label maps
    are (N,H,W) and pair b reads frame frame_index[b] (deepim_ingest_label_mask_frames)."""
    labels = _frame(ctx, frames, key, np.uint8)
    B, H, W = labels.shape
    if is_shared(frames):
        fi, B, N = _frame_index(ctx, frames)
        out = ctx.empty((B, 1, H, W))
        lib.deepim_ingest_label_mask_frames(ctx.handle, out, labels, fi, _ids(ctx, frames, "mask_idx", B), N, B, H, W)
        return out
    out = ctx.empty((B, 1, H, W))
    lib.deepim_ingest_label_mask(ctx.handle, out, labels, _ids(ctx, frames, "mask_idx", B), B, H, W)
    return out


def _box(ctx, mask):
    B, _, H, W = mask.shape
    out = ctx.empty(mask.shape)
    lib.deepim_mask_box_forward(ctx.handle, out, mask, B, H, W)
    return out


def get_pair_mask(frames, config, phase="train", depth_rendered=None):
    """image.py:230-399 → (mask_observed, mask_gt_observed, mask_rendered), device (B,1,H,W).
    train: TRAIN.INIT_MASK mask_gt | box_gt | box_rendered, then TRAIN.MASK_DILATE (:289-290); "mask_gt" hands over the 0 / 1
    mask of the pair's label, as lib/pair_matching/data_pair.get_pair_mask does (the reference copies the raw label map there).
    test: TEST.INIT_MASK mask_gt_observed | mask_observed | box_gt_observed | box_ | box_rendered (:305-378), then
    TEST.MASK_DILATE (:380-381); mask_gt_observed is mask_observed, as at :387.
    depth_rendered: the (B,1,H,W) tensor get_pair_depth already made of frames["depth_rendered"], to skip a second ingest."""
    ctx = _context(frames)
    dr = depth_rendered if depth_rendered is not None else _depth(ctx, frames, "depth_rendered", config)
    B, _, H, W = dr.shape
    if phase == "train":
        if is_shared(frames):
            raise NotImplementedError("shared frames (frames['frame_index']) are a test-phase input: the training loader is per pair")
        from ..pair_matching import data_pair
        batch = {"depth_rendered": dr, "mask_gt_observed": label_mask(ctx, frames, "mask_gt_observed")}
        if frames.get("mask_dilate_thickness") is not None:
            batch["mask_dilate_thickness"] = _ids(ctx, frames, "mask_dilate_thickness", B, 4)
        return data_pair.get_pair_mask(batch, config)
    n = B * H * W
    mask_rendered = ctx.empty((B, 1, H, W))
    lib.deepim_depth_clip_mask(ctx.handle, mask_rendered, dr, ctypes.c_float(0.2), n)
    init = config.TEST.INIT_MASK
    if init == "mask_gt_observed":
        mask_observed = label_mask(ctx, frames, "mask_gt_observed")
    elif init == "mask_observed":
        mask_observed = label_mask(ctx, frames, "mask_observed")
    elif init == "box_gt_observed":
        # [y_start:y_end, x_start:x_end] with end = the LAST index holding a non-zero (:327-336): deepim_mask_box_forward's rectangle
        mask_observed = _box(ctx, label_mask(ctx, frames, "mask_gt_observed"))
    elif init == "box_":
        mask_observed = _box(ctx, label_mask(ctx, frames, "mask_observed"))
    elif init == "box_rendered":
        fg = ctx.empty((B, 1, H, W))
        lib.deepim_depth_to_mask(ctx.handle, fg, dr, ctypes.c_float(0.2), n)
        mask_observed = _box(ctx, fg)
    else:
        raise Exception("Unknown init mask type: {}".format(init))
    if frames.get("rendered_covered") is not None:
        # :301-303: `np.sum(depth_rendered) == 0` gives a zero mask_observed whatever INIT_MASK says — decided on the device from
        # the draw's own per-pair count of covered pixels (deepim_render_frames_forward), never read back and not printed
        covered = frames["rendered_covered"]
        if not isinstance(covered, DeviceArray) or covered.dtype != np.int32 or covered.size != B:
            raise TypeError("frames['rendered_covered'] must be a device int32 array of %d values" % B)
        lib.deepim_mask_gate(ctx.handle, mask_observed, covered, B, H, W)
    if config.TEST.get("MASK_DILATE", False):
        if frames.get("mask_dilate_thickness") is None:
            raise NotImplementedError("TEST.MASK_DILATE: the frames carry no 'mask_dilate_thickness' — the random draws are the "
                                      "loader's (lib/utils/mask_dilate.mask_dilate_draws); the device path has no generator")
        mask_observed = mask_dilate_batch(mask_observed, _ids(ctx, frames, "mask_dilate_thickness", B, 4))
    return mask_observed, mask_observed, mask_rendered
