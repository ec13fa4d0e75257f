"""The test loop — mirror of deepim/core/tester.py: `Predictor` (:27-47), `pred_eval` (:50-527), `par_generate_gt` (:530-569)
and `calc_EPE_one_pair` (:572-589), same names, argument order and log lines, with every tensor resident on the device.

Per batch the loop is the reference's (:340-485): forward → [flow EPE of the first forward, with network.PRED_FLOW and not
TEST.FAST_TEST] → per iteration RT_transform → rotation / translation error → re-render + mask update (update_test_batch, device
class ids) → forward. The refined poses and the errors of all iterations go to one device staging buffer that is read back ONCE
per batch; the flow EPE (deepim_flow_epe) adds into six device doubles that are read once after the last batch.

Differences from the reference:
  * `test_data` is an iterable of (data, frames, pair_records): `data` from lib/pair_matching/data_pair.get_data_pair_test_batch,
    `frames` the decoded frames it was made of (lib/utils/image.py), `pair_records` a list of B dicts with pose_rendered,
    pose_observed, gt_class — the pairdb entries of the batch. B may exceed 1 (the reference asserts BATCH_PAIRS == 1 per
    device, :83): pair b of a batch is treated as that reference's pair. `pairdb` only gives the pair count of the progress line.
  * the render machine is an argument (the reference builds an OpenGL one, :112-143); needed from test_iter = 2 on.
  * a pair whose pose_rendered sums to -12 (:285-310, "no point valid in init pose") stays in its batch: its results are the
    reference's (the initial pose and errors of 1000 in every iteration, no EPE contribution — `skip` of deepim_flow_epe), and
    the batch row it occupies is fed pose_observed instead, so that the network and the renderer see a sane pose there.
  * TEST.VISUALIZE, TEST.PRECOMPUTED_ICP and TEST.BEFORE_ICP read files and draw figures: NotImplementedError.
  * the data / net / calc_gt times of the progress line are host times of asynchronous launches (only the per-batch read-back
    waits for the device).
  * pred_eval returns what it computed (the reference returns None).
  * per-pair cameras: a pair record may carry "K" (3,3). tester.py:424-426 loads a pair's `-K.txt` only for the re-render and
    then leaves that K in the loop variable for every later pair that has no file. Here a pair's K is that pair's camera
    everywhere — zoom centre, re-render, flow ground truth and arp_2d — and it does not leak to other pairs: a record without a
    K gets config.dataset.INTRINSIC_MATRIX. When any record of a batch has one, the batch's (B,3,3) table (cameras.camera_table)
    is uploaded once, set as data["intrinsics"] and bound as the context's camera table (Context.bind_cameras); the K of every
    stored pose is collected in `all_K[cls]`, parallel to all_poses_gt[cls][0], handed to the evaluation and cached in the
    sidecar `<name>_pose_iter<N>_K.pkl` next to the reference's four containers (written only when cameras were used). The
    caller decodes the `-K.txt` files, as it decodes the frames.
  * `test_data` may be a core/loader.TestDataLoader, which makes the batches from observed frames and initial poses alone and
    fills up its last batch by repeating the last pair. Such a record carries "pad": True (the reference's DataBatch.pad): it
    rides through the network like its original and enters no container, no num_inst, no sum, no EPE total and no pair count.
  * TEST.DEPTH_ICP (not a reference key, default off): the device counterpart of the PRECOMPUTED_ICP row. The final poses of each
    batch go through lib/pair_matching/depth_icp.DepthICP.refine against frames["depth_observed"] — the raw sensor depth in
    metres, unmasked: the ICP's distance gate drops the background — with the no_point and pad rows skipped. Their errors
    (deepim_pose_error) and the solver's status ride in the batch's one read-back: the staging buffer grows by one slot. The
    result gains "icp": all_rot_err / all_trans_err / all_poses_est / all_poses_gt (num_cls x 1) and "status" (num_cls lists; 0
    solved, 1 too few pairs, 2 rank-deficient, -1 for a no_point pair, which stores its rendered pose and errors of 1000 as in
    the network rows), and tables["icp"] the three evaluations with their plots under add_plots_depth_ICP and
    arp_2d_plots_depth_ICP. The containers are cached in the sidecar `<name>_pose_iter<N>_icp.pkl`, written only with the key on
    and removed when a run with the key off rewrites the cache; with the key on a cache without that sidecar is not a hit.
    With the key off the loop issues the launches, allocations and read-backs it always did.
"""
from __future__ import print_function, division, absolute_import

import ctypes
import os
import pickle
import time

import numpy as np

from ..cameras import camera_table, has_cameras
from ..lib.pair_matching.batch_updater_py_multi import update_test_batch
from ..lib.pair_matching.depth_icp import DepthICP
from ..lib.utils import image as _image
from ..runtime import DeviceArray, lib
from .loader import TestDataLoader

EPE_KEYS = ("epe_all", "num_all", "epe_viz", "num_viz", "epe_vizbg", "num_vizbg")     # tester.py:581-588
FLOW_THRESH = 3e-3                                                                   # calc_flow's default, flow.py:12


class Predictor(object):
    """tester.py:27-47 over a bound deepIM_flownet (symbols/deepIM_flownet.py) instead of an MXNet module."""

    def __init__(self, config, net):
        self.config = config
        self._mod = self.net = net

    def predict(self, data_batch):
        """net.forward → [the one output dict]: the reference's output names, aliased to the network's device arrays."""
        out = self.net.forward(data_batch)
        res = {"se3_output": out["se3"]}
        if "flow_est_crop" in out:
            res["flow_est_crop_output"] = out["flow_est_crop"]
        if "mask_observed_pred" in out:
            res["mask_observed_pred_output"] = out["mask_observed_pred"]
        return [res]


def par_generate_gt(config, frames):
    """tester.py:530-557 from decoded frames: {"depth_rendered", "depth_observed"}, device (B,1,H,W) in metres — what calc_flow
    is given at :559-566. depth_rendered / DEPTH_FACTOR; depth_gt_observed (or depth_observed when the frames carry none,
    :541-547) / DEPTH_FACTOR, zeroed where mask_gt_observed != mask_idx (:551-556). Two deepim_ingest_depth16 launches."""
    ctx = _image._context(frames)
    key = "depth_gt_observed" if frames.get("depth_gt_observed") is not None else "depth_observed"
    return {"depth_rendered": _image._depth(ctx, frames, "depth_rendered", config),
            "depth_observed": _image._depth(ctx, frames, key, config, "mask_gt_observed")}


def _poses(ctx, p, B):
    if isinstance(p, DeviceArray):
        return p
    return ctx.array(np.asarray(p, dtype=np.float32).reshape(B, 3, 4))


def calc_EPE_batch(config, flow_est, flow_gt, pose_rendered, pose_observed, skip=None, totals=None, out=None, K=None):
    """tester.py:559-589 for a batch, one deepim_flow_epe call and no host round trip: flow_est (B,2,H,W) device (the graph's
    flow_est_crop), flow_gt from par_generate_gt, poses (B,3,4). Returns the device float64 (B,6) array of EPE_KEYS per pair.
    skip: device int32 (B), pairs to leave out; totals: device float64 (6), running sums the rows are added to.
    K: None (config.dataset.INTRINSIC_MATRIX), a host (3,3), or a DeviceArray (B,3,3) of per-pair cameras (bound as the context's
    camera table; each pair's ground truth then comes from its own K and its inverse)."""
    ctx = flow_est.context
    B, _, H, W = flow_est.shape
    if out is None:
        out = ctx.empty((B, 6), dtype=np.float64)
    if isinstance(K, DeviceArray):
        if K.shape != (B, 3, 3):
            raise ValueError("calc_EPE_batch: a device K must be (%d,3,3), got %s" % (B, K.shape))
        ctx.bind_cameras(K)
        K = None
    else:
        K = np.ascontiguousarray(config.dataset.INTRINSIC_MATRIX if K is None else K, dtype=np.float32).reshape(3, 3)
    lib.deepim_flow_epe(ctx.handle, out, totals, flow_est, flow_gt["depth_rendered"], flow_gt["depth_observed"],
                        _poses(ctx, pose_rendered, B), _poses(ctx, pose_observed, B), K, skip, ctypes.c_float(FLOW_THRESH),
                        1 if config.network.get("STANDARD_FLOW_REP", False) else 0, B, H, W)
    return out


def calc_EPE_one_pair(config, flow_est, flow_gt, pose_rendered, pose_observed):
    """tester.py:572-589 for one pair (B = 1 inputs): the dict of six values, read back from the device."""
    row = calc_EPE_batch(config, flow_est, flow_gt, pose_rendered, pose_observed).asnumpy()
    assert row.shape == (1, 6), "calc_EPE_one_pair takes one pair; calc_EPE_batch takes a batch"
    return dict(zip(EPE_KEYS, row[0].tolist()))


def _mkdir_p(path):
    os.makedirs(path, exist_ok=True)


def _as_array(lists):
    try:
        return np.array(lists)
    except ValueError:                 # classes with different pair counts: the object array older NumPy made silently
        return np.array(lists, dtype=object)


def _evaluate(config, imdb_test, all_poses_est, all_poses_gt, all_K=None, plots_suffix=""):
    cams = {} if all_K is None else {"all_K": all_K}      # per-pair cameras (module docstring); without them the reference's calls
    res = {"pose": imdb_test.evaluate_pose(config, all_poses_est, all_poses_gt, **cams)}
    pose_add_plots_dir = os.path.join(imdb_test.result_path, "add_plots" + plots_suffix)
    _mkdir_p(pose_add_plots_dir)
    res["add"] = imdb_test.evaluate_pose_add(config, all_poses_est, all_poses_gt, output_dir=pose_add_plots_dir, **cams)
    pose_arp2d_plots_dir = os.path.join(imdb_test.result_path, "arp_2d_plots" + plots_suffix)
    _mkdir_p(pose_arp2d_plots_dir)
    res["arp_2d"] = imdb_test.evaluate_pose_arp_2d(config, all_poses_est, all_poses_gt, output_dir=pose_arp2d_plots_dir, **cams)
    return res


def camera_cache_file(pose_err_file):
    """The sidecar of the result cache that keeps all_K: `<name>_pose_iter<N>_K.pkl` next to `<name>_pose_iter<N>.pkl`."""
    return pose_err_file[:-len(".pkl")] + "_K.pkl"


def icp_cache_file(pose_err_file):
    """The sidecar of the result cache that keeps the depth ICP's containers: `<name>_pose_iter<N>_icp.pkl`."""
    return pose_err_file[:-len(".pkl")] + "_icp.pkl"


def save_result_cache(pose_err_file, containers, all_K=None, icp=None):
    """The reference's four containers to `pose_err_file`; all_K to the sidecar when per-pair cameras were used — and no
    sidecar otherwise: one left by an earlier run is removed, it would give the cached poses another run's cameras. The same
    rule for `icp`, the "icp" dict of a TEST.DEPTH_ICP run, and its sidecar."""
    with open(pose_err_file, "wb") as f:
        pickle.dump(list(containers), f, protocol=2)
    for side, payload in ((camera_cache_file(pose_err_file), all_K), (icp_cache_file(pose_err_file), icp)):
        if payload is not None:
            with open(side, "wb") as f:
                pickle.dump(payload, f, protocol=2)
        elif os.path.exists(side):
            os.remove(side)


def load_result_cache(pose_err_file):
    """-> ([all_rot_err, all_trans_err, all_poses_est, all_poses_gt], all_K or None): the cache and, when it exists, its sidecar."""
    with open(pose_err_file, "rb") as fid:
        containers = pickle.load(fid, encoding="latin1")
    all_K = None
    side = camera_cache_file(pose_err_file)
    if os.path.exists(side):
        with open(side, "rb") as fid:
            all_K = pickle.load(fid, encoding="latin1")
    return containers, all_K


def load_icp_cache(pose_err_file):
    """-> the "icp" dict a TEST.DEPTH_ICP run cached next to `pose_err_file`, or None without that sidecar"""
    side = icp_cache_file(pose_err_file)
    if not os.path.exists(side):
        return None
    with open(side, "rb") as fid:
        return pickle.load(fid, encoding="latin1")


def _evaluate_icp(config, imdb_test, icp, all_K, logger):
    logger.info("evaluate pose after depth ICP:")
    one = type(config)(config)                      # the evaluations take their column count from TEST.test_iter: one here
    one.TEST = type(config.TEST)(config.TEST, test_iter=1)
    return _evaluate(one, imdb_test, icp["all_poses_est"], icp["all_poses_gt"], all_K, plots_suffix="_depth_ICP")


def pred_eval(config, predictor, test_data, imdb_test, vis=False, ignore_cache=None, logger=None, pairdb=None,
              render_machine=None):
    """tester.py:50-527 (see the module docstring for the shape of `test_data`).
    :param predictor: Predictor (may be None when the result cache is loaded)
    :param imdb_test: lib/dataset/LM6D_REFINE with `name` and `result_path`
    :param ignore_cache: ignore the saved cache file
    :param render_machine: lib/render_glumpy Render_Py (or the lit ModelNet machine); needed from test_iter = 2 on
    Returns a dict: the four cached containers, "all_K" (None unless a pair record carried a "K"), sum_PoseErr, num_inst, "epe"
    (the six totals and the three means) and "tables"; with TEST.DEPTH_ICP also "icp" and tables["icp"] (module docstring)."""
    for key, lines in (("VISUALIZE", ":112, :411-421"), ("PRECOMPUTED_ICP", ":193-242"), ("BEFORE_ICP", ":244-279")):
        if config.TEST.get(key, False):
            raise NotImplementedError("TEST.%s (deepim/core/tester.py%s) reads files and draws figures; it is not part of "
                                      "the device test loop" % (key, lines))
    test_iter = config.TEST.test_iter
    do_icp = bool(config.TEST.get("DEPTH_ICP", False))
    logger.info(imdb_test.result_path)
    logger.info("test iter size: {}".format(test_iter))
    pose_err_file = os.path.join(imdb_test.result_path, imdb_test.name + "_pose_iter{}.pkl".format(test_iter))
    if (os.path.exists(pose_err_file) and not ignore_cache and not vis
            and (not do_icp or os.path.exists(icp_cache_file(pose_err_file)))):
        [all_rot_err, all_trans_err, all_poses_est, all_poses_gt], all_K = load_result_cache(pose_err_file)
        tables = _evaluate(config, imdb_test, all_poses_est, all_poses_gt, all_K)
        res = {"all_rot_err": all_rot_err, "all_trans_err": all_trans_err, "all_poses_est": all_poses_est,
               "all_poses_gt": all_poses_gt, "all_K": all_K, "tables": tables, "from_cache": True}
        if do_icp:
            res["icp"] = load_icp_cache(pose_err_file)
            tables["icp"] = _evaluate_icp(config, imdb_test, res["icp"], all_K, logger)
        return res

    if test_iter > 1 and render_machine is None:
        raise ValueError("pred_eval: TEST.test_iter = %d re-renders between the iterations: pass render_machine" % test_iter)
    if do_icp and render_machine is None:
        raise ValueError("pred_eval: TEST.DEPTH_ICP draws the depth of the poses it refines: pass render_machine")
    net = predictor.net
    ctx = net.ctx
    num_cls = len(imdb_test.classes)
    class_name = list(config.dataset.get("class_name", imdb_test.classes))
    do_epe = bool(config.network.PRED_FLOW and not config.TEST.FAST_TEST)
    num_pairs = len(pairdb) if pairdb is not None else (
        test_data.size if isinstance(test_data, TestDataLoader) else
        sum(len(t[2]) for t in test_data) if isinstance(test_data, (list, tuple)) else -1)

    data_time, net_time, post_time = 0.0, 0.0, 0.0
    epe_totals = ctx.zeros((6,), dtype=np.float64)          # sum_EPE_all, num_inst_all, … of :93-98, on the device
    sum_PoseErr = [np.zeros((num_cls + 1, 2)) for _ in range(test_iter)]
    all_rot_err = [[[] for _ in range(test_iter)] for _ in range(num_cls)]      # num_cls x test_iter
    all_trans_err = [[[] for _ in range(test_iter)] for _ in range(num_cls)]
    all_poses_est = [[[] for _ in range(test_iter)] for _ in range(num_cls)]
    all_poses_gt = [[[] for _ in range(test_iter)] for _ in range(num_cls)]
    all_K = [[] for _ in range(num_cls)]        # the camera of every stored pose, parallel to all_poses_gt[cls][0]
    cameras_used = False
    num_inst = np.zeros(num_cls + 1)
    K = np.ascontiguousarray(config.dataset.INTRINSIC_MATRIX, dtype=np.float32).reshape(3, 3)
    one_point = ctx.zeros((3, 1))       # deepim_pose_error's re / te need no model points; its add / adi / arp_2d go unused
    stage = rbuf = None
    pairs_done = 0
    n_slots = test_iter + (1 if do_icp else 0)          # the depth ICP's poses and errors ride in one more slot of the staging buffer
    icp = icp_res = None
    if do_icp:
        icp = DepthICP(render_machine, config)
        icp_res = {k: [[[]] for _ in range(num_cls)] for k in ("all_rot_err", "all_trans_err", "all_poses_est", "all_poses_gt")}
        icp_res["status"] = [[] for _ in range(num_cls)]

    t_start = time.time()
    t = time.time()
    for idx, (data, frames, pair_records) in enumerate(test_data):
        B = len(pair_records)
        if do_icp and frames.get("depth_observed") is None:
            raise ValueError("pred_eval: TEST.DEPTH_ICP refines against the sensor depth: the frames carry no 'depth_observed'")
        pose_rendered = np.stack([np.asarray(r["pose_rendered"], np.float32).reshape(3, 4) for r in pair_records])
        pose_observed = np.stack([np.asarray(r["pose_observed"], np.float32).reshape(3, 4) for r in pair_records])
        no_point = np.array([np.sum(r["pose_rendered"]) == -12 for r in pair_records])      # NO POINT VALID IN INIT POSE
        pad = np.array([bool(r.get("pad", False)) for r in pair_records])                   # a loader's filler: counted nowhere
        class_ids = [imdb_test.classes.index(r["gt_class"]) for r in pair_records]
        cams = None                                 # the batch's (B,3,3) table: host copy here, cams_d on the device
        if has_cameras(pair_records):
            cams = camera_table(pair_records, K)
            cameras_used = True
        elif data.get("intrinsics") is not None:
            raise ValueError("pred_eval: the batch carries data['intrinsics'] but no pair record has a 'K': the evaluation "
                             "would silently use another camera")
        for b in np.nonzero(no_point & ~pad)[0]:
            print(pairs_done + b)
            print("in test: NO POINT_VALID IN rendered")
        if no_point.all():
            poses_host = errs_host = status_host = None
        else:
            data = dict(data)
            cams_d = None
            if cams is not None:
                cams_d = data["intrinsics"] = ctx.array(cams)       # uploaded once per batch
            skip = None
            if (no_point | pad).any():
                skip = ctx.array((no_point | pad).astype(np.int32), dtype=np.int32)
            if no_point.any():
                parked = np.where(no_point[:, None, None], pose_observed, pose_rendered)
                data["src_pose"] = ctx.array(parked)
            pose_rendered_d = ctx.array(pose_rendered)
            pose_observed_d = ctx.array(pose_observed)
            render_ids = ctx.array(np.array([class_name.index(r["gt_class"]) for r in pair_records], np.int32), dtype=np.int32)
            if stage is None or stage.size != n_slots * B * 17 + (B if do_icp else 0):      # + the ICP's B status words
                stage = ctx.empty((n_slots * B * 17 + (B if do_icp else 0),))
                rbuf = {n: ctx.empty((B, 3 if n == "image_rendered" else 1, net.H, net.W))
                        for n in ("image_rendered", "depth_rendered", "mask_rendered", "mask_observed")}
            poses_d = DeviceArray(ctx, (n_slots, B, 3, 4), ptr=stage.ptr, base=stage)
            errs_d = DeviceArray(ctx, (n_slots, B, 5), ptr=stage.ptr + n_slots * B * 48, base=stage)
            data_time += time.time() - t

            t = time.time()
            output_all = predictor.predict(data)
            net_time += time.time() - t

            t = time.time()
            if do_epe:      # evaluate optical flow: once per pair, from the first forward (:366-378)
                flow_gt = par_generate_gt(config, frames)
                calc_EPE_batch(config, output_all[0]["flow_est_crop_output"], flow_gt, pose_rendered_d, pose_observed_d,
                               skip=skip, totals=epe_totals, K=cams_d)
            post_time += time.time() - t

            for pose_iter_idx in range(test_iter):      # iterative refine se3 estimation
                t = time.time()
                cur = poses_d[pose_iter_idx]
                net.pose_update(data["src_pose"], pose_out=cur)                       # RT_transform, :391-398
                if skip is not None:
                    for b in np.nonzero(no_point)[0]:                                 # keep the parked rows parked
                        cur[int(b)].copyfrom(pose_observed_d[int(b)])
                if cams_d is not None:
                    ctx.bind_cameras(cams_d)
                lib.deepim_pose_error(ctx.handle, errs_d[pose_iter_idx], cur, pose_observed_d, one_point, 1,
                                      None if cams_d is not None else K, B, 1)   # :401
                post_time += time.time() - t
                if pose_iter_idx < test_iter - 1:       # if more than one iteration
                    t = time.time()
                    data = update_test_batch(config, data, render_machine, cur, class_index=render_ids, out=rbuf)
                    data_time += time.time() - t
                    t = time.time()
                    output_all = predictor.predict(data)
                    net_time += time.time() - t
            t = time.time()
            if do_icp:      # "DeepIM + ICP": the final poses against the raw sensor depth; no_point and pad rows keep theirs
                depth_sensor = _image._depth(ctx, frames, "depth_observed", config)
                cur = poses_d[test_iter]
                _, icp_status = icp.refine(poses_d[test_iter - 1], render_ids, depth_sensor, K=cams_d if cams_d is not None else K,
                                           skip=skip, out=cur)
                if cams_d is not None:
                    ctx.bind_cameras(cams_d)
                lib.deepim_pose_error(ctx.handle, errs_d[test_iter], cur, pose_observed_d, one_point, 1,
                                      None if cams_d is not None else K, B, 1)
                DeviceArray(ctx, (B,), np.int32, ptr=stage.ptr + n_slots * B * 68, base=stage).copyfrom(icp_status)
            host = stage.asnumpy()                      # the batch's one read-back
            poses_host = host[:n_slots * B * 12].reshape(n_slots, B, 3, 4)
            errs_host = host[n_slots * B * 12:n_slots * B * 17].reshape(n_slots, B, 5)
            if do_icp:
                status_host = host[n_slots * B * 17:].view(np.int32)
            post_time += time.time() - t

        for b, rec in enumerate(pair_records):          # the containers, pair by pair in the reference's order
            if pad[b]:
                continue
            class_id = class_ids[b]
            all_K[class_id].append(K.copy() if cams is None else cams[b].copy())
            if not no_point[b]:
                num_inst[class_id] += 1
                num_inst[-1] += 1
            for pose_iter_idx in range(test_iter):
                if no_point[b]:
                    pose_est, r_dist, t_dist = rec["pose_rendered"], 1000, 1000       # :288-297
                else:
                    pose_est = poses_host[pose_iter_idx, b].copy()
                    r_dist, t_dist = float(errs_host[pose_iter_idx, b, 0]), float(errs_host[pose_iter_idx, b, 1])
                all_poses_est[class_id][pose_iter_idx].append(pose_est)
                all_poses_gt[class_id][pose_iter_idx].append(rec["pose_observed"])
                all_rot_err[class_id][pose_iter_idx].append(r_dist)
                all_trans_err[class_id][pose_iter_idx].append(t_dist)
                sum_PoseErr[pose_iter_idx][class_id, :] += np.array([r_dist, t_dist])
                sum_PoseErr[pose_iter_idx][-1, :] += np.array([r_dist, t_dist])
            if do_icp:
                if no_point[b]:
                    pose_est, r_dist, t_dist, st = rec["pose_rendered"], 1000, 1000, -1
                else:
                    pose_est = poses_host[test_iter, b].copy()
                    r_dist, t_dist, st = float(errs_host[test_iter, b, 0]), float(errs_host[test_iter, b, 1]), int(status_host[b])
                icp_res["all_poses_est"][class_id][0].append(pose_est)
                icp_res["all_poses_gt"][class_id][0].append(rec["pose_observed"])
                icp_res["all_rot_err"][class_id][0].append(r_dist)
                icp_res["all_trans_err"][class_id][0].append(t_dist)
                icp_res["status"][class_id].append(st)
        first_pair = pairs_done + 1
        pairs_done += B - int(pad.sum())

        if idx % 50 == 0:       # post process
            logger.info("testing {}/{} data {:.4f}s net {:.4f}s calc_gt {:.4f}s".format(
                first_pair, num_pairs, data_time / pairs_done, net_time / pairs_done, post_time / pairs_done))
        t = time.time()

    all_rot_err = _as_array(all_rot_err)
    all_trans_err = _as_array(all_trans_err)

    # save inference results
    _mkdir_p(imdb_test.result_path)
    if not cameras_used:
        all_K = None
    logger.info("saving result cache to {}".format(pose_err_file))
    if do_icp:
        icp_res["all_rot_err"], icp_res["all_trans_err"] = _as_array(icp_res["all_rot_err"]), _as_array(icp_res["all_trans_err"])
    save_result_cache(pose_err_file, [all_rot_err, all_trans_err, all_poses_est, all_poses_gt], all_K, icp_res)
    logger.info("done")

    epe = None
    if config.network.PRED_FLOW:
        tot = dict(zip(EPE_KEYS, epe_totals.asnumpy().tolist()))      # the loop's one read of the running totals
        epe = dict(tot, EPE_all=tot["epe_all"] / max(tot["num_all"], 1.0),
                   EPE_ignore_unvisible=tot["epe_vizbg"] / max(tot["num_vizbg"], 1.0),
                   EPE_visible=tot["epe_viz"] / max(tot["num_viz"], 1.0))
        logger.info("evaluate flow:")
        logger.info("EPE all: {}".format(epe["EPE_all"]))
        logger.info("EPE ignore unvisible: {}".format(epe["EPE_ignore_unvisible"]))
        logger.info("EPE visible: {}".format(epe["EPE_visible"]))

    logger.info("evaluate pose:")
    tables = _evaluate(config, imdb_test, all_poses_est, all_poses_gt, all_K)
    if do_icp:
        tables["icp"] = _evaluate_icp(config, imdb_test, icp_res, all_K, logger)
    logger.info("using {} seconds in total".format(time.time() - t_start))
    res = {"all_rot_err": all_rot_err, "all_trans_err": all_trans_err, "all_poses_est": all_poses_est,
           "all_poses_gt": all_poses_gt, "all_K": all_K, "sum_PoseErr": sum_PoseErr, "num_inst": num_inst, "epe": epe, "tables": tables,
           "from_cache": False}
    if do_icp:
        res["icp"] = icp_res
    return res
