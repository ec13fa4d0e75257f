"""CPU: the mixed-precision training emulation (tests/fp16_train_emulation.py) with the fp16 rounding replaced by the identity and
S = 1 is the oracle's fp32 training iteration exactly — pins the emulation's wiring (where the scale enters, which tensors round).
Also the graph description of network.FP16_CONV training, which needs no GPU, and its refusals."""
import numpy as np
import pytest

import fp16_train_emulation as emu
from oracle import pipeline as opipe
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.symbols import deepIM_flownet

MEANS_REV = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])


def _setup(heads):
    B = 1
    d = synthetic.make_batch(B, seed=917, n_frames=1)
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = heads
    params = deepIM_flownet().get_symbol(cfg, is_train=True).init_weights(cfg, seed=93)
    pco = np.stack([d["pose_tgt"][b][:, :3].astype(np.float64) @ d["point_cloud_model"][b].astype(np.float64) + d["pose_tgt"][b][:, 3:4]
                    for b in range(B)]).astype(np.float32)
    data = {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][0], "mask_observed": d["mask_observed"],
            "mask_rendered": d["mask_rendered"][0], "src_pose": d["src_pose"][0]}
    label = {"mask_gt_observed": (d["depth_gt_observed"] > 0).astype(np.float32), "point_cloud_model": d["point_cloud_model"],
             "point_cloud_weights": np.ones((B, 3, 3000), np.float32), "point_cloud_observed": pco}
    if heads:    # any flow labels do: both sides read the same ones
        rng = np.random.default_rng(5)
        label["flow"] = rng.standard_normal((B, 2, 480, 640)).astype(np.float32) * 5
        label["flow_weights"] = (rng.random((B, 2, 480, 640)) > 0.5).astype(np.float32)
    return d, cfg, params, data, label


@pytest.mark.parametrize("heads", [False, True])
def test_emulation_with_identity_rounding_and_unit_scale_is_the_oracle_training_iteration(heads):
    d, cfg, params, data, label = _setup(heads)
    t = cfg.train_iter
    args = (params, data, label, d["K"], MEANS_REV, cfg.dataset.trans_means, cfg.dataset.trans_stds, cfg.network.ROT_COORD, t.LW_PM,
            t.NUM_3D_SAMPLE, cfg.dataset.NORMALIZE_3D_POINT, t.SE3_PM_LOSS_TYPE, t.SE3_PM_SL1_SCALAR)
    kw = dict(pred_flow=heads, pred_mask=heads, lw_flow=t.LW_FLOW, lw_mask=t.LW_MASK, normalize_flow=cfg.dataset.NORMALIZE_FLOW)
    loss, g, _ = emu.train_iteration(*args, q=emu.identity, S=1.0, **kw)
    ref_loss, g_ref, _ = opipe.train_iteration(*args, **kw)
    assert loss == ref_loss
    assert set(g) == set(g_ref)
    for name in sorted(g_ref):
        np.testing.assert_array_equal(g[name], g_ref[name], err_msg=name)
    # a power-of-two scale with identity rounding only moves the encoder's dz by that factor: the gradients stay (up to the
    # rounding of the larger intermediate sums, which S = 2^k leaves exact)
    _, g2, fwd2 = emu.train_iteration(*args, q=emu.identity, S=256.0, **kw)
    for name in sorted(g_ref):
        np.testing.assert_allclose(g2[name], g_ref[name], rtol=1e-5, atol=1e-6 * max(1e-30, float(np.abs(g_ref[name]).max())),
                                   err_msg=name)
    # and with fp16 rounding the dz are fp16 values
    _, _, fwd3 = emu.train_iteration(*args, q=emu.q16, S=1024.0, **kw)
    for name, _s, _p in emu.ENCODER:
        np.testing.assert_array_equal(fwd3["dz_" + name], emu.q16(fwd3["dz_" + name]))


def test_fp16_training_graph_builds_without_a_gpu():
    cfg = default_config()
    cfg.network.FP16_CONV = True
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = True
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert net.is_train and net.fp16_conv and not net.x3_conv
    assert net.with_decoder and not net.fp16_decoder          # FP16_DECODER governs the test graph only
    assert net.loss_scale_init == cfg.TRAIN.FP16_LOSS_SCALE and net.loss_scale_window == cfg.TRAIN.FP16_SCALE_WINDOW
    shapes = net.arg_shape_dict()
    assert len(shapes) == 46 and shapes["flow_conv1_weight"] == (64, 8, 7, 7)
    params = net.init_weights(cfg, seed=3)
    assert set(params) == set(shapes)
    # the decoder setting does not change the training graph
    cfg.network.FP16_DECODER = False
    assert not deepIM_flownet().get_symbol(cfg, is_train=True).fp16_decoder


def test_x3_training_still_refused():
    cfg = default_config()
    cfg.network.X3_CONV = True
    with pytest.raises(NotImplementedError):
        deepIM_flownet().get_symbol(cfg, is_train=True)
    cfg.network.FP16_CONV = True                               # X3 beside FP16 as well
    with pytest.raises(NotImplementedError):
        deepIM_flownet().get_symbol(cfg, is_train=True)


@pytest.mark.parametrize("scale", [1000.0, 3.0, 0.5, 0.0, -4.0, 2.0 ** 25, float("inf")])
def test_loss_scale_must_be_a_power_of_two(scale):
    cfg = default_config()
    cfg.network.FP16_CONV = True
    cfg.TRAIN.FP16_LOSS_SCALE = scale
    with pytest.raises(ValueError, match="FP16_LOSS_SCALE"):
        deepIM_flownet().get_symbol(cfg, is_train=True)
    cfg.TRAIN.FP16_LOSS_SCALE = 4096
    assert deepIM_flownet().get_symbol(cfg, is_train=True).loss_scale_init == 4096.0
