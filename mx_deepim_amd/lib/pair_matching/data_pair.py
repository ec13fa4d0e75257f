"""Loader-side label generation on the device — mirror of the label half of
lib/pair_matching/data_pair.py:133-248 (`get_data_pair_train_batch`) and of the helpers it calls in
lib/utils/image.py (`get_pair_mask` :229-390, `get_pair_flow` :402-450) and data_pair.py
(`get_point_cloud_observed`).  File decoding / resizing / augmentation (cv2) stay with the caller: this takes the decoded
per-pair tensors already resident in HBM and produces every label tensor the training graph consumes, with no host
round trip:

    rot, trans              calc_RT_delta(pose_rendered, pose_observed, ROT_COORD, ROT_TYPE)     deepim_calc_rt_delta_ex
    flow, flow_weights      calc_flow → (B,2,H,W), weights by TRAIN.FLOW_WEIGHT_TYPE             deepim_pair_flow_labels
    mask_rendered           depth_rendered with values > 0.2 set to 1                            deepim_depth_clip_mask
    mask_observed           TRAIN.INIT_MASK: mask_gt | box_gt | box_rendered                     deepim_mask_box_forward
                            then TRAIN.MASK_DILATE with the loader's draws (image.py:289-290)    deepim_mask_dilate
    point_cloud_observed    R·X + T of the sampled model points                                  deepim_points_transform

`get_data_pair_test_batch` mirrors data_pair.py:22-63 from decoded uint8 / uint16 frames (lib/utils/image.py).
"""
import ctypes

import numpy as np

from ...cameras import validate_cameras
from ...runtime import DeviceArray, lib
from ..utils import image as _image
from ..utils.mask_dilate import mask_dilate_batch
from .RT_transform import calc_RT_delta_batch

FLOW_WEIGHT_TYPE_CODE = {"all": 0, "viz": 1, "valid": 2}


def get_point_cloud_observed(config, points_model, pose_observed):
    """data_pair.py `get_point_cloud_observed`, batched: points_model (B,3,N), pose_observed (B,3,4) device → (B,3,N)."""
    ctx = pose_observed.context
    B, _, N = points_model.shape
    out = ctx.empty((B, 3, N))
    lib.deepim_points_transform(ctx.handle, out, points_model, pose_observed, B, N)
    return out


def get_pair_flow(batch, config):
    """image.py:402-450 on resident depths/poses → (flow (B,2,H,W), flow_weights (B,2,H,W))."""
    wtype = config.TRAIN.FLOW_WEIGHT_TYPE
    if wtype not in FLOW_WEIGHT_TYPE_CODE:
        raise Exception("Unknown FLOW_WEIGHT_TYPE: {}".format(wtype))
    dr = batch["depth_rendered"]
    ctx = dr.context
    B, _, H, W = dr.shape
    flow, wts = ctx.empty((B, 2, H, W)), ctx.empty((B, 2, H, W))
    K = np.ascontiguousarray(config.dataset.INTRINSIC_MATRIX, np.float32).reshape(3, 3)
    lib.deepim_pair_flow_labels(ctx.handle, flow, wts, dr, batch["depth_gt_observed"], batch["pose_rendered"],
                                batch["pose_observed"], K, ctypes.c_float(3e-3),
                                1 if config.network.get("STANDARD_FLOW_REP", False) else 0, FLOW_WEIGHT_TYPE_CODE[wtype], B, H, W)
    return flow, wts


def get_pair_mask(batch, config):
    """image.py:229-390, train phase, on resident tensors → (mask_observed, mask_gt_observed, mask_rendered).
    With TRAIN.MASK_DILATE the batch carries "mask_dilate_thickness": a device int32 (B,4) array of the loader's draws
    (lib/utils/mask_dilate.mask_dilate_draws) — the random numbers are the loader's, the device path has no generator."""
    dr, gt = batch["depth_rendered"], batch["mask_gt_observed"]
    ctx = dr.context
    B, _, H, W = dr.shape
    n = B * H * W
    mask_rendered = ctx.empty((B, 1, H, W))
    lib.deepim_depth_clip_mask(ctx.handle, mask_rendered, dr, ctypes.c_float(0.2), n)
    init = config.TRAIN.INIT_MASK
    if init == "mask_gt":
        mask_observed = gt.copy()
    elif init == "box_gt":
        mask_observed = ctx.empty((B, 1, H, W))
        lib.deepim_mask_box_forward(ctx.handle, mask_observed, gt, B, H, W)
    elif init == "box_rendered":
        # the rectangle of depth_rendered > 0.2 (image.py:270-285; that branch assigns `cur_mask_observed` but appends
        # `mask_observed` — the rectangle is what the code means to hand over)
        fg = ctx.empty((B, 1, H, W))
        lib.deepim_depth_to_mask(ctx.handle, fg, dr, ctypes.c_float(0.2), n)
        mask_observed = ctx.empty((B, 1, H, W))
        lib.deepim_mask_box_forward(ctx.handle, mask_observed, fg, B, H, W)
    else:
        raise Exception("Unknown mask type: {}".format(init))
    if config.TRAIN.get("MASK_DILATE", False):
        thickness = batch.get("mask_dilate_thickness")
        if thickness is None:
            raise NotImplementedError("TRAIN.MASK_DILATE: the batch carries no 'mask_dilate_thickness' — the random draws of "
                                      "image.py:289-290 are the loader's (lib/utils/mask_dilate.mask_dilate_draws); the "
                                      "device path has no generator of its own")
        mask_observed = mask_dilate_batch(mask_observed, thickness)
    return mask_observed, gt, mask_rendered


def get_data_pair_test_batch(frames, config):
    """data_pair.py:22-63 from decoded frames (see lib/utils/image.py for the dict): the reference's `data` keys (:43-60) as
    device tensors for the whole batch — image_observed, image_rendered (B,3,H,W), src_pose (B,3,4) from frames["pose_rendered"],
    class_index handed over as given [, depth_observed, depth_rendered with INPUT_DEPTH][, mask_observed, mask_rendered with
    INPUT_MASK].
    A shared-frame batch (frames["frame_index"], lib/utils/image.py: N frames for B pairs) gives the same keys except that
    image_observed [and depth_observed] are replaced by ONE entry, data["observed_frames"] (lib/utils/image.ObservedFrames): the
    uint8 / uint16 frames on the device with the device frame_index [, the label maps, mask_idx and DEPTH_FACTOR of the observed
    depth], which the network's zoom front end reads in place. A numpy frame_index outside [0, N) raises ValueError before
    anything is uploaded or launched.
    frames["intrinsics"] — per-pair cameras, a (B,3,3) numpy array (validated and uploaded once) or a DeviceArray — is passed
    through as data["intrinsics"]: the zoom front end and the re-render then take pair b's camera from row b."""
    data = {}
    shared = _image.is_shared(frames)
    if shared:
        _image.check_frame_index(frames)
        frames = dict(frames)
        data["observed_frames"] = _image.observed_frames(frames, config, "test")
        frames["frame_index"] = data["observed_frames"].frame_index     # uploaded once for the calls below
        data["image_rendered"] = _image.get_rendered_image(frames, config)
    else:
        data["image_observed"], data["image_rendered"] = _image.get_pair_image(frames, config, "test")
    ctx = data["image_rendered"].context
    B = data["image_rendered"].shape[0]
    if shared and data["observed_frames"].n_pairs != B:
        raise ValueError("frame_index names %d pairs, image_rendered holds %d" % (data["observed_frames"].n_pairs, B))
    pose = frames["pose_rendered"]
    if not isinstance(pose, DeviceArray):
        pose = ctx.array(np.asarray(pose, dtype=np.float32).reshape(B, 3, 4))
    data["src_pose"] = pose
    data["class_index"] = frames.get("class_index")
    cams = frames.get("intrinsics")
    if cams is not None:
        if not isinstance(cams, DeviceArray):
            cams = ctx.array(validate_cameras(cams))
        if cams.shape != (B, 3, 3):
            raise ValueError("frames['intrinsics'] must be (%d,3,3), got %s" % (B, cams.shape))
        data["intrinsics"] = cams
    if config.network.INPUT_DEPTH and shared:
        data["depth_rendered"] = _image._depth(ctx, frames, "depth_rendered", config)
    elif config.network.INPUT_DEPTH:
        data["depth_observed"], data["depth_rendered"] = _image.get_pair_depth(frames, config, "test")
    if config.network.INPUT_MASK:
        data["mask_observed"], _, data["mask_rendered"] = _image.get_pair_mask(frames, config, "test",
                                                                               depth_rendered=data.get("depth_rendered"))
    return data


def get_data_pair_train_batch(batch, config):
    """Device composition of data_pair.py:133-248 given decoded tensors (DeviceArrays):
        image_observed, image_rendered (B,3,H,W); depth_gt_observed, depth_rendered (B,1,H,W) in metres;
        pose_rendered, pose_observed (B,3,4); mask_gt_observed (B,1,H,W) [INPUT_MASK / PRED_MASK];
        depth_observed (B,1,H,W) [INPUT_DEPTH]; point_cloud_model, point_cloud_weights (B,3,N) [SE3_PM_LOSS];
        mask_dilate_thickness: device int32 (B,4) [TRAIN.MASK_DILATE], see get_pair_mask;
        class_index: handed over as given — host ids, or a device int32 array (B) that the render machine draws in one launch
        group without reading it back.
    Returns {"data": {...}, "label": {...}} with the reference's keys."""
    n, c = config.network, config
    data = {"image_observed": batch["image_observed"], "image_rendered": batch["image_rendered"],
            "depth_gt_observed": batch["depth_gt_observed"], "class_index": batch.get("class_index"),
            "src_pose": batch["pose_rendered"], "tgt_pose": batch["pose_observed"]}
    if n.INPUT_DEPTH:
        data["depth_observed"], data["depth_rendered"] = batch["depth_observed"], batch["depth_rendered"]
    rot, trans = calc_RT_delta_batch(batch["pose_rendered"], batch["pose_observed"], c.dataset.trans_means,
                                     c.dataset.trans_stds, n.ROT_COORD, n.ROT_TYPE)
    label = {"rot": rot, "trans": trans}
    if n.INPUT_MASK or n.PRED_MASK:
        mask_observed, mask_gt_observed, mask_rendered = get_pair_mask(batch, config)
        label["mask_gt_observed"] = mask_gt_observed
        if n.INPUT_MASK:
            data["mask_observed"], data["mask_rendered"] = mask_observed, mask_rendered
    if n.PRED_FLOW:
        label["flow"], label["flow_weights"] = get_pair_flow(batch, config)
    if c.train_iter.SE3_PM_LOSS:
        label["point_cloud_model"] = batch["point_cloud_model"]
        label["point_cloud_weights"] = batch["point_cloud_weights"]
        label["point_cloud_observed"] = get_point_cloud_observed(config, batch["point_cloud_model"], batch["pose_observed"])
    return {"data": data, "label": label}
