"""The test loop (mx_deepim_amd/core/tester.pred_eval) on the GPU: 480x640 (fc6 fixes the frame size), B = 2, test_iter = 2,
seeded weights, synthetic meshes, PRED_FLOW on and FAST_TEST off. The network, the render machine and one run over two batches
are built once per module and shared."""
import os
import pickle
import re

import numpy as np
import pytest

from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import tester
from mx_deepim_amd.lib.dataset.LM6D_REFINE import LM6D_REFINE
from mx_deepim_amd.lib.pair_matching import data_pair
from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import update_test_batch
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
from mx_deepim_amd.symbols import deepIM_flownet

pytestmark = pytest.mark.gpu
H, W, B = 480, 640, 2
CLASSES = ["ape", "cat"]
MEANS_BGR = np.array([104.0, 117.0, 124.0])


class ListLogger(object):
    def __init__(self):
        self.lines = []

    def info(self, msg, *a):
        self.lines.append(str(msg))


def to_bgr8(t):
    """(B,3,H,W) mean-subtracted RGB tensor of synthetic.make_batch → the uint8 BGR frames a decoder would have handed over"""
    rgb = t + synthetic.PIXEL_MEANS[::-1].reshape(1, 3, 1, 1)
    return np.ascontiguousarray(np.clip(np.rint(rgb), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)[..., ::-1])


def make_batch_inputs(d, order, classes):
    """(frames, pair_records) of the pairs `order` of the synthetic batch d"""
    order = list(order)
    dep_o = d["depth_gt_observed"][order][:, 0]
    frames = {"image_observed": to_bgr8(d["image_observed"][order]), "image_rendered": to_bgr8(d["image_rendered"][0][order]),
              "depth_rendered": np.rint(d["depth_rendered"][0][order][:, 0] * 1000).astype(np.uint16),
              "depth_gt_observed": np.rint(dep_o * 1000).astype(np.uint16),
              "mask_gt_observed": ((dep_o > 0) * 3).astype(np.uint8), "mask_idx": np.full(len(order), 3, np.int32),
              "pose_rendered": d["src_pose"][0][order].copy()}
    recs = [{"pose_rendered": d["src_pose"][0][i].copy(), "pose_observed": d["pose_tgt"][i].copy(), "gt_class": c}
            for i, c in zip(order, classes)]
    return frames, recs


class Setup(object):
    pass


@pytest.fixture(scope="module")
def setup(ctx, small_batch, tmp_path_factory):
    s = Setup()
    cfg = default_config()
    cfg.network.PIXEL_MEANS = MEANS_BGR.astype(np.float32)
    cfg.TEST.test_iter, cfg.TEST.FAST_TEST = 2, False
    cfg.dataset.class_name = list(CLASSES)
    net = deepIM_flownet().get_symbol(cfg)
    assert net.with_flow_head
    params = net.init_weights(cfg, seed=20)
    params["trans_weight"] = params["trans_weight"] * np.float32(0.02)     # keep the object in frame (as bench.py does)
    params["trans_bias"] = params["trans_bias"] * np.float32(0.02)
    net.bind(ctx, B, params)
    meshes = {}
    for i, c in enumerate(CLASSES):
        m = synthetic.ellipsoid_mesh(np.array([0.05, 0.04, 0.035]) * (1.0 + 0.2 * i), 12, 24)
        m.pop("uv")
        meshes[c] = m
    s.cfg, s.net, s.ctx = cfg, net, ctx
    s.rm = Render_Py("unused", CLASSES, cfg.dataset.INTRINSIC_MATRIX, W, H, meshes=meshes, ctx=ctx,
                     pixel_means=MEANS_BGR[::-1].astype(np.float32))
    s.points = {c: meshes[c]["vertices"][::7] for c in CLASSES}
    s.diameters = {c: 0.1 + 0.02 * i for i, c in enumerate(CLASSES)}
    s.batches = [make_batch_inputs(small_batch, (0, 1), ("ape", "cat")), make_batch_inputs(small_batch, (1, 0), ("cat", "cat"))]
    s.result_path = str(tmp_path_factory.mktemp("results"))
    s.log = ListLogger()
    s.imdb = LM6D_REFINE(CLASSES, s.points, s.diameters, ctx=ctx, logger=s.log, name="synt_test", result_path=s.result_path)
    s.test_data = lambda: [(data_pair.get_data_pair_test_batch(f, cfg), f, r) for f, r in s.batches]
    s.res = tester.pred_eval(cfg, tester.Predictor(cfg, net), s.test_data(), s.imdb, logger=s.log, render_machine=s.rm)
    s.first_lines = list(s.log.lines)
    return s


def test_poses_equal_the_loop_stepped_by_hand(setup):
    """forward → pose_update → update_test_batch (device class ids) → forward → pose_update with the existing API, bit for bit"""
    s = setup
    got = s.res["all_poses_est"]
    seen = {c: 0 for c in range(len(CLASSES))}
    for frames, recs in s.batches:
        data = data_pair.get_data_pair_test_batch(frames, s.cfg)
        ids = s.ctx.array(np.array([CLASSES.index(r["gt_class"]) for r in recs], np.int32), dtype=np.int32)
        s.net.forward(data)
        pose1 = s.net.pose_update(data["src_pose"]).copy()
        data = update_test_batch(s.cfg, data, s.rm, pose1, class_index=ids)
        s.net.forward(data)
        pose2 = s.net.pose_update(data["src_pose"]).asnumpy()
        pose1 = pose1.asnumpy()
        assert np.isfinite(pose2).all() and not np.array_equal(pose1, pose2)
        for b, r in enumerate(recs):
            c = CLASSES.index(r["gt_class"])
            k = seen[c]
            seen[c] += 1
            np.testing.assert_array_equal(got[c][0][k].view(np.uint32), pose1[b].view(np.uint32))
            np.testing.assert_array_equal(got[c][1][k].view(np.uint32), pose2[b].view(np.uint32))
            np.testing.assert_array_equal(s.res["all_poses_gt"][c][1][k], r["pose_observed"])
    assert seen == {0: 1, 1: 3}
    assert s.res["num_inst"].tolist() == [1, 3, 4]
    for it in range(2):
        for c in range(2):
            np.testing.assert_allclose(s.res["sum_PoseErr"][it][c], [np.sum(s.res["all_rot_err"][c][it]),
                                                                   np.sum(s.res["all_trans_err"][c][it])], rtol=1e-12)
        assert (np.asarray(s.res["all_rot_err"][1][it]) > 0).all() and (np.asarray(s.res["all_rot_err"][1][it]) < 180).all()


def test_epe_totals_equal_the_sum_of_calc_EPE_batch(setup):
    s = setup
    t = np.zeros(6)
    for frames, recs in s.batches:
        data = data_pair.get_data_pair_test_batch(frames, s.cfg)
        out = s.net.forward(data)
        rows = tester.calc_EPE_batch(s.cfg, out["flow_est_crop"], tester.par_generate_gt(s.cfg, frames), data["src_pose"],
                                     np.stack([r["pose_observed"] for r in recs])).asnumpy()
        assert (rows[:, 1] == H * W).all() and (rows[:, 3] > 100).all() and (rows[:, 5] > rows[:, 3]).all()
        for row in rows:
            t = t + row
    epe = s.res["epe"]
    np.testing.assert_array_equal([epe[k] for k in tester.EPE_KEYS], t)
    assert epe["EPE_all"] == t[0] / t[1] and epe["EPE_visible"] == t[2] / t[3] and epe["EPE_ignore_unvisible"] == t[4] / t[5]


def test_log_lines_follow_the_reference(setup):
    s = setup
    lines = s.first_lines
    epe = s.res["epe"]
    assert lines[0] == s.result_path and lines[1] == "test iter size: 2"
    assert re.match(r"^testing 1/4 data \d+\.\d{4}s net \d+\.\d{4}s calc_gt \d+\.\d{4}s$", lines[2])
    i = lines.index("evaluate flow:")
    assert lines[i + 1] == "EPE all: {}".format(epe["EPE_all"])
    assert lines[i + 2] == "EPE ignore unvisible: {}".format(epe["EPE_ignore_unvisible"])
    assert lines[i + 3] == "EPE visible: {}".format(epe["EPE_visible"])
    assert lines[i + 4] == "evaluate pose:" and lines[i + 5] == "evaluating pose"
    assert lines[i + 6] == "------------ ape -----------"
    assert lines[i + 7] == "{:>24}: {:>7}, {:>7}, {:>7}".format("[rot_thresh, trans_thresh", "RotAcc", "TraAcc", "SpcAcc")
    assert lines[i - 2] == "saving result cache to " + os.path.join(s.result_path, "synt_test_pose_iter2.pkl")
    assert lines[i - 1] == "done"
    assert re.match(r"^using \d+\.\d+ seconds in total$", lines[-1])
    assert "evaluating pose add" in lines and "evaluating pose average re-projection 2d error" in lines


def test_cache_file_is_loaded_instead_of_running_and_ignore_cache_runs_again(setup):
    s = setup
    path = os.path.join(s.result_path, "synt_test_pose_iter2.pkl")
    with open(path, "rb") as f:
        head = f.read(2)
        f.seek(0)
        rot, trans, est, gt = pickle.load(f, encoding="latin1")
    assert head == b"\x80\x02"                                              # pickle protocol 2
    np.testing.assert_array_equal(est[1][1][2], s.res["all_poses_est"][1][1][2])
    tables = s.first_lines[s.first_lines.index("evaluating pose"):-1]
    n = len(s.log.lines)
    res = tester.pred_eval(s.cfg, None, None, s.imdb, logger=s.log)        # no predictor, no data: nothing can run
    assert res["from_cache"]
    assert s.log.lines[n + 2:] == tables
    n = len(s.log.lines)
    res = tester.pred_eval(s.cfg, tester.Predictor(s.cfg, s.net), s.test_data(), s.imdb, ignore_cache=True, logger=s.log,
                           render_machine=s.rm)
    assert not res["from_cache"] and "evaluate flow:" in s.log.lines[n:]
    for c in range(2):
        for it in range(2):
            np.testing.assert_array_equal(np.stack(res["all_poses_est"][c][it]), np.stack(s.res["all_poses_est"][c][it]))
    assert res["epe"] == s.res["epe"]


def test_pair_without_a_valid_initial_pose_keeps_it_and_scores_1000(setup, tmp_path):
    """pose_rendered summing to -12 (tester.py:285-310): the initial pose in every iteration, errors of 1000, no EPE
    contribution; the other pair of the batch is untouched by its neighbour"""
    s = setup
    frames, recs = make_batch_inputs_copy(s.batches[0])
    recs[1]["pose_rendered"] = -np.ones((3, 4), np.float32)
    frames["pose_rendered"][1] = -1
    log = ListLogger()
    imdb = LM6D_REFINE(CLASSES, s.points, s.diameters, ctx=s.ctx, logger=log, name="sentinel", result_path=str(tmp_path))
    res = tester.pred_eval(s.cfg, tester.Predictor(s.cfg, s.net), [(data_pair.get_data_pair_test_batch(frames, s.cfg), frames, recs)],
                           imdb, logger=log, render_machine=s.rm)
    for it in range(2):
        np.testing.assert_array_equal(res["all_poses_est"][1][it][0], -np.ones((3, 4), np.float32))
        assert res["all_rot_err"][1][it][0] == 1000 and res["all_trans_err"][1][it][0] == 1000
        np.testing.assert_array_equal(res["all_poses_est"][0][it][0], s.res["all_poses_est"][0][it][0])
        np.testing.assert_array_equal(res["sum_PoseErr"][it][1], [1000, 1000])
    assert res["num_inst"].tolist() == [1, 0, 1]
    assert res["epe"]["num_all"] == H * W
    data = data_pair.get_data_pair_test_batch(s.batches[0][0], s.cfg)
    rows = tester.calc_EPE_batch(s.cfg, s.net.forward(data)["flow_est_crop"], tester.par_generate_gt(s.cfg, s.batches[0][0]),
                                 data["src_pose"], np.stack([r["pose_observed"] for r in s.batches[0][1]])).asnumpy()
    np.testing.assert_array_equal([res["epe"][k] for k in tester.EPE_KEYS], rows[0])


def make_batch_inputs_copy(batch):
    frames, recs = batch
    return {k: v.copy() for k, v in frames.items()}, [dict(r) for r in recs]


def test_refused_options_raise(setup):
    s = setup
    for key, line in (("VISUALIZE", "411"), ("PRECOMPUTED_ICP", "193"), ("BEFORE_ICP", "244")):
        cfg = default_config()
        cfg.TEST[key] = True
        with pytest.raises(NotImplementedError, match=line):
            tester.pred_eval(cfg, None, [], s.imdb, logger=s.log)
    cfg = default_config()
    cfg.TEST.test_iter = 3
    with pytest.raises(ValueError, match="render_machine"):
        tester.pred_eval(cfg, tester.Predictor(cfg, s.net), [], s.imdb, ignore_cache=True, logger=s.log)
