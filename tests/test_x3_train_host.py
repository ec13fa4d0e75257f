"""§8f-4e — split-fp16 training (TRAIN.X3_CONV), the parts that need no GPU: the config keys and what the training symbol makes of
them, its refusals, the new C entry points in the header, the emulation's wiring (with the split replaced by the identity and S = 1
it is the oracle's fp32 training iteration exactly), and the accuracy window of the gradient scale that the mode rests on: pairs
carry a gradient at fp32 grade while its scaled maximum lies in [1, 3750], and at no better than fp16 grade at 2^-10."""
import numpy as np
import pytest

import x3_train_emulation as emu
from oracle import pipeline as opipe
from mx_deepim_amd import runtime, synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.symbols import deepIM_flownet

MEANS_REV = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])
NEW_ENTRIES = ("deepim_lrelu_bias_backward_x3", "deepim_conv2d_wgrad_x3", "deepim_conv_x3_pack_dgrad", "deepim_conv2d_dgrad_x3",
               "deepim_conv_dgrad_x3_workspace_size", "deepim_x3_status_to_state", "deepim_split16_to_nchw_f32_unscaled",
               "deepim_x3_weight_range_check")


def test_the_key_defaults_to_off_and_the_training_symbol_follows_it():
    cfg = default_config()
    assert cfg.TRAIN.X3_CONV is False
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert net.train_x3 is False and net.x3_conv is False
    cfg = default_config()
    cfg.TRAIN.X3_CONV = True
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = True
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert net.is_train and net.train_x3 is True and net.x3_conv is True and not net.fp16_conv
    assert net.nc8 is False and net.train_winograd is False
    assert net.with_decoder and not net.fp16_decoder                 # the decoder and heads stay fp32
    assert net.loss_scale_init == cfg.TRAIN.X3_GRAD_SCALE and net.loss_scale_window == cfg.TRAIN.X3_SCALE_WINDOW
    scale = net.loss_scale_init
    assert scale >= 1.0 and np.frexp(scale)[0] == 0.5                # the default is a power of two
    cfg.TRAIN.X3_GRAD_SCALE, cfg.TRAIN.X3_SCALE_WINDOW = 64, 7
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert net.loss_scale_init == 64.0 and net.loss_scale_window == 7
    # the inference symbol is not touched by the key
    cfg = default_config()
    cfg.TRAIN.X3_CONV = True
    assert deepIM_flownet().get_symbol(cfg).x3_conv is False


@pytest.mark.parametrize("scale", [1000.0, 3.0, 0.5, 0.0, -4.0, 2.0 ** 25, float("inf")])
def test_the_gradient_scale_must_be_a_power_of_two(scale):
    cfg = default_config()
    cfg.TRAIN.X3_CONV = True
    cfg.TRAIN.X3_GRAD_SCALE = scale
    with pytest.raises(ValueError, match="X3_GRAD_SCALE"):
        deepIM_flownet().get_symbol(cfg, is_train=True)


@pytest.mark.parametrize("window", [0, -3])
def test_the_scale_window_must_be_positive(window):
    cfg = default_config()
    cfg.TRAIN.X3_CONV = True
    cfg.TRAIN.X3_SCALE_WINDOW = window
    with pytest.raises(ValueError, match="X3_SCALE_WINDOW"):
        deepIM_flownet().get_symbol(cfg, is_train=True)


def test_network_x3_conv_in_training_still_raises():
    cfg = default_config()
    cfg.network.X3_CONV = True
    with pytest.raises(NotImplementedError):
        deepIM_flownet().get_symbol(cfg, is_train=True)
    cfg.TRAIN.X3_CONV = True                                   # the TRAIN key does not lift the refusal of the network key
    with pytest.raises(NotImplementedError):
        deepIM_flownet().get_symbol(cfg, is_train=True)


def test_the_key_together_with_winograd_training_raises():
    cfg = default_config()
    cfg.TRAIN.X3_CONV = cfg.TRAIN.WINOGRAD_CONV = True
    with pytest.raises(ValueError, match="WINOGRAD_CONV"):
        deepIM_flownet().get_symbol(cfg, is_train=True)


def test_the_fp16_graph_ignores_the_key():
    cfg = default_config()
    cfg.TRAIN.X3_CONV = True
    cfg.TRAIN.X3_GRAD_SCALE = 3.0                              # not even validated there
    cfg.network.FP16_CONV = True
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert net.fp16_conv and not net.x3_conv and not net.train_x3
    assert net.loss_scale_init == cfg.TRAIN.FP16_LOSS_SCALE and net.loss_scale_window == cfg.TRAIN.FP16_SCALE_WINDOW
    cfg.TRAIN.WINOGRAD_CONV = True                             # both ignored: no exclusion error either
    assert not deepIM_flownet().get_symbol(cfg, is_train=True).train_x3


def test_the_new_entry_points_are_declared():
    protos = runtime.parse_header()
    for name in NEW_ENTRIES:
        assert name in protos, name
    # the walk takes the arguments of the fp16 walk
    assert [a.split("_")[0] for a in protos["deepim_lrelu_bias_backward_x3"][2]] == \
        [a.split("_")[0] for a in protos["deepim_lrelu_bias_backward_f16"][2]]
    assert protos["deepim_lrelu_bias_backward_x3"][1] == protos["deepim_lrelu_bias_backward_f16"][1]
    assert protos["deepim_conv2d_wgrad_x3"][2] == ["ctx", "dw", "x_split16", "dz_split16", "state", "B", "Cin", "H", "W", "Cout", "k",
                                                   "stride", "pad", "layout", "x_scale"]
    assert protos["deepim_conv2d_dgrad_x3"][2] == ["ctx", "dx_split16", "dz_split16", "w_layer", "ws", "state", "B", "Ci_l", "Hd", "Wd",
                                                   "Co_l", "k", "stride", "pad", "w_scale"]
    assert protos["deepim_conv_x3_pack_dgrad"][2] == ["ctx", "packed", "w_layer", "state", "Co_l", "Ci_l", "k", "ky0", "kx0", "st", "nky",
                                                      "nkx", "w_scale"]
    assert protos["deepim_conv_dgrad_x3_workspace_size"][2] == protos["deepim_conv_dgrad_f16_workspace_size"][2]


def _setup(heads):
    B = 1
    d = synthetic.make_batch(B, seed=917, n_frames=1)
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = heads
    cfg.TRAIN.X3_CONV = True
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
def test_emulation_with_identity_split_and_unit_scale_is_the_oracle_training_iteration(heads):
    d, cfg, params, data, label = _setup(heads)
    t = cfg.train_iter
    args = (params, data, label, d["K"], MEANS_REV, cfg.dataset.trans_means, cfg.dataset.trans_stds, cfg.network.ROT_COORD, t.LW_PM,
            t.NUM_3D_SAMPLE, cfg.dataset.NORMALIZE_3D_POINT, t.SE3_PM_LOSS_TYPE, t.SE3_PM_SL1_SCALAR)
    kw = dict(pred_flow=heads, pred_mask=heads, lw_flow=t.LW_FLOW, lw_mask=t.LW_MASK, normalize_flow=cfg.dataset.NORMALIZE_FLOW)
    loss, g, fwd = emu.train_iteration(*args, split_value=emu.identity, S=1.0, **kw)
    ref_loss, g_ref, _ = opipe.train_iteration(*args, **kw)
    assert loss == ref_loss
    assert set(g) == set(g_ref)
    for name in sorted(g_ref):
        np.testing.assert_array_equal(g[name], g_ref[name], err_msg=name)
    assert not fwd["overflow"]


def test_split_is_the_x3_rule():
    v = np.array([0.0, 1.0, -1.0, 1.0 / 3.0, 1e-3, 3000.0, -1e9, 1e9], np.float32)
    hi, lo = emu.split(v, 16.0)
    x = np.clip(v.astype(np.float64) * 16.0, -60000.0, 60000.0)
    np.testing.assert_array_equal(hi, x.astype(np.float32).astype(np.float16).astype(np.float32))
    assert np.all(np.abs(hi.astype(np.float64) + lo - x) <= np.maximum(np.abs(x) * 2.0 ** -21, 2.0 ** -24))
    assert hi[-1] == 60000.0 and hi[-2] == -60000.0 and lo[-1] == 0.0       # the clamp, not inf
    assert emu.clamps(v, 16.0) and not emu.clamps(v[:5], 16.0) and emu.clamps(np.array([np.nan], np.float32), 1.0)
    np.testing.assert_allclose(emu.pair_value(v[:6], 16.0), v[:6], rtol=2.0 ** -20, atol=2.0 ** -28)


def _conv3_1_problem():
    """conv3_1's geometry on one sample: 256 → 256 channels, 3x3 stride 1 pad 1 over 60 x 80 (K = 4800 pixels in the weight
    gradient). Activations like LeakyReLU outputs, He weights, and a gradient-like dz with 8 octaves of dynamic range and maximum 1."""
    rng = np.random.default_rng(31)
    C, H, W = 256, 60, 80
    x = rng.standard_normal((C, H, W)).astype(np.float32)
    x = np.where(x > 0, x, 0.1 * x).astype(np.float32)
    w = (rng.standard_normal((C, C, 3, 3)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    dz = (rng.choice([-1.0, 1.0], (C, H, W)) * 2.0 ** -rng.uniform(0.0, 8.0, (C, H, W))).astype(np.float32)
    dz.flat[0] = 1.0
    return x, w, dz


@pytest.fixture(scope="module")
def conv3_1():
    x, w, dz = _conv3_1_problem()
    xc = emu.im2col3x3(x)                                              # (4800, 2304)
    dzm = np.ascontiguousarray(dz.reshape(256, -1))                    # (256, 4800)
    # data gradient: dx[pix, ci] = Σ_{tap, co} dz[pix + tap − 1, co] · w[co, ci, 2 − ky, 2 − kx]
    dzc = emu.im2col3x3(dz)                                            # (4800, 9·256), (ky, kx, co)
    wt = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(2, 3, 0, 1).reshape(9 * 256, 256))
    ref_w = dzm.astype(np.float64) @ xc.astype(np.float64)
    ref_d = dzc.astype(np.float64) @ wt.astype(np.float64)
    return xc, dzm, dzc, wt, ref_w, ref_d


def _window_errors(conv3_1, m):
    """Errors ÷ tensor maximum of the emulated weight and data gradient against float64 with the gradient's scaled maximum at m."""
    xc, dzm, dzc, wt, ref_w, ref_d = conv3_1
    m = np.float32(m)
    got_w = emu.matmul3(dzm * m, xc, 1.0, emu.ACT_SCALE).astype(np.float64) / float(m)
    got_d = emu.matmul3(dzc * m, wt, 1.0, emu.weight_scale(wt)).astype(np.float64)
    assert not emu.clamps(got_d, 1.0)                                  # d itself fits its split at scale 1
    got_d = emu.pair_value(got_d.astype(np.float32), 1.0).astype(np.float64) / float(m)
    return (float(np.abs(got_w - ref_w).max() / np.abs(ref_w).max()), float(np.abs(got_d - ref_d).max() / np.abs(ref_d).max()))


@pytest.mark.parametrize("scaled_max", [1.0, 64.0, 3750.0])
def test_pairs_carry_gradients_at_fp32_grade_inside_the_window(conv3_1, scaled_max):
    ew, ed = _window_errors(conv3_1, scaled_max)
    print("scaled max %g: wgrad %.3g, dgrad %.3g of the tensor maximum" % (scaled_max, ew, ed))
    assert ew <= 1e-5 and ed <= 1e-5, (ew, ed)


def test_pairs_are_no_better_than_fp16_below_the_window(conv3_1):
    ew, ed = _window_errors(conv3_1, 2.0 ** -10)
    print("scaled max 2^-10: wgrad %.3g, dgrad %.3g of the tensor maximum" % (ew, ed))
    assert ew > 1e-5 and ed > 1e-5, (ew, ed)
