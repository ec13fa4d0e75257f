"""fp16 FlowNetS decoder and flow / mask heads (network.FP16_CONV with the decoder in the graph, csrc/decoder_f16.hip) against the
fp16 emulation of tests/fp16_decoder_emulation.py, fed the GPU's OWN encoder outputs so that the encoder's fp16 differences (up to
~2e-3 of range after ten layers) neither hide nor excuse decoder errors; the FP16_DECODER = False fallback against the oracle's
fp32 decoder; the kernels alone; graph capture. ulp16(v) = one fp16 ulp at |v|."""
import ctypes

import numpy as np
import pytest

import fp16_decoder_emulation as emu
from oracle import net as onet
from oracle import pipeline as opipe
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import DeviceArray, lib
from mx_deepim_amd.symbols import deepIM_flownet

pytestmark = pytest.mark.gpu
MEANS_REV = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])
H, W = 480, 640
SLOPE = 0.1


def ulp16(v):
    return np.spacing(np.abs(np.asarray(v, np.float32)).astype(np.float16)).astype(np.float32)


def assert_ulp(got, want, what):
    """|got − want| <= ulp16(want) + 1e-5·max|want| everywhere."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bound = ulp16(want) + 1e-5 * np.abs(want).max()
    bad = np.abs(got - want) > bound
    assert not bad.any(), "%s: %d of %d beyond ulp16 + 1e-5 max (worst %.3g)" % (what, bad.sum(), bad.size, np.abs(got - want).max())


def rng_rel(got, want):
    """max |got − want| over the range (max |want|)"""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(1e-30, np.abs(want).max()))


def _bind(ctx, B, seed, fp16_decoder=True, fast_test=False, update_mask=None, pred_mask=True, pred_flow=True, params=None):
    cfg = default_config()
    cfg.network.FP16_CONV = True
    cfg.network.FP16_DECODER = fp16_decoder
    cfg.network.PRED_MASK = pred_mask
    cfg.network.PRED_FLOW = pred_flow
    cfg.TEST.FAST_TEST = fast_test
    if update_mask is not None:
        cfg.TEST.UPDATE_MASK = update_mask
    net = deepIM_flownet().get_symbol(cfg)
    if params is None:
        params = net.init_weights(cfg, seed=seed)
    net.bind(ctx, B, params)
    return cfg, net, params


def _batch(B, seed, occlude=True):
    d = synthetic.make_batch(B, seed=seed, n_frames=1, occlude=occlude)
    npd = {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][0], "mask_observed": d["mask_observed"],
           "mask_rendered": d["mask_rendered"][0], "src_pose": d["src_pose"][0]}
    return d, npd


def _gpu_acts(net):
    return {n: emu.nhwc_to_nchw(net.act[n + "_h"].asnumpy()) for n in ("conv4_1", "conv5_1", "conv6_1")}


def test_fp16_decoder_iteration_matches_emulation_on_own_encoder_outputs(ctx):
    B = 2
    d, npd = _batch(B, 404)
    cfg, net, params = _bind(ctx, B, 44)
    assert net.fp16_decoder and net.with_mask_head and net.with_flow_head
    out = net.forward({k: ctx.array(v) for k, v in npd.items()})
    pose = net.pose_update(ctx.array(npd["src_pose"])).asnumpy()
    acts = _gpu_acts(net)
    zf = net.act["zoom_factor"].asnumpy()
    c2h, c3h = net.act["Concat2_h"].asnumpy(), net.act["Concat3_h"].asnumpy()
    # skip channels bit-exact, pad channels still zero
    np.testing.assert_array_equal(c2h[..., :512].view(np.uint16), net.act["conv5_1_h"].asnumpy().view(np.uint16))
    np.testing.assert_array_equal(c3h[..., :512].view(np.uint16), net.act["conv4_1_h"].asnumpy().view(np.uint16))
    assert not c2h[..., 1026:].view(np.uint16).any() and not c3h[..., 770:].view(np.uint16).any()
    c2, c3 = emu.nhwc_to_nchw(c2h)[:, :1026], emu.nhwc_to_nchw(c3h)[:, :770]
    # layer by layer, each fed the GPU's own input of that layer
    flow6 = net.act["flow6"].asnumpy()
    assert rng_rel(flow6, emu.predictor(params, "Convolution1", acts["conv6_1"])) <= 1e-5
    assert_ulp(c2[:, 512:1024], emu.deconv(params, "deconv5", acts["conv6_1"], 15, 20, SLOPE), "deconv5")
    assert_ulp(c2[:, 1024:1026], emu.upsample_flow(params, "upsample_flow6to5", flow6, 15, 20), "upsample_flow6to5")
    flow5 = net.act["flow5"].asnumpy()
    assert rng_rel(flow5, emu.predictor(params, "Convolution2", c2)) <= 1e-5
    assert_ulp(c3[:, 512:768], emu.deconv(params, "deconv4", c2, 30, 40, SLOPE), "deconv4")
    assert_ulp(c3[:, 768:770], emu.upsample_flow(params, "upsample_flow5to4", flow5, 30, 40), "upsample_flow5to4")
    assert rng_rel(net.act["mask_lowres"].asnumpy(), emu.predictor(params, "mask_conv3", c3)) <= 1e-5
    assert rng_rel(net.act["flow_lowres"].asnumpy(), emu.predictor(params, "Convolution3", c3)) <= 1e-5
    # the whole chain from the GPU's encoder outputs
    dec = emu.decoder(params, acts)
    hd = emu.heads(params, dec["Concat3"], zf, H, W, cfg.dataset.NORMALIZE_FLOW)
    flow = out["flow_est_crop"].asnumpy()
    ef = rng_rel(flow, hd["flow_est"])
    flips = float(np.mean(out["mask_observed_pred"].asnumpy() != hd["mask_observed_pred"]))
    print("flow_est %.3g of range, mask flips %.3g (chained emulation on the GPU's encoder outputs)" % (ef, flips))
    assert ef <= 2e-3 and flips <= 1e-3, (ef, flips)
    # against the full emulation (its own fp16 encoder): a wiring check only
    ref = opipe.refine_iteration(params, npd, d["K"], MEANS_REV, cfg.dataset.trans_means, cfg.dataset.trans_stds,
                                 cfg.network.ROT_COORD, fp16_conv=True)
    full = emu.heads(params, emu.decoder(params, ref)["Concat3"], ref["zoom_factor"], H, W, cfg.dataset.NORMALIZE_FLOW)
    ff = rng_rel(flow, full["flow_est"])
    print("flow_est %.3g of range against the full fp16 emulation" % ff)
    assert ff <= 0.05
    # the pose branch does not see the decoder: bit-identical to a FAST_TEST bind of the same parameters and batch
    _, fast, _ = _bind(ctx, B, 44, fast_test=True, params=params)
    assert not fast.with_decoder
    fast.forward({k: ctx.array(v) for k, v in npd.items()})
    np.testing.assert_array_equal(out["se3"].asnumpy(), fast.act["se3"].asnumpy())
    np.testing.assert_array_equal(pose, fast.pose_update(ctx.array(npd["src_pose"])).asnumpy())


@pytest.mark.parametrize("which", ["mask_only", "flow_only"])
def test_fp16_decoder_with_one_head(ctx, which):
    B = 2
    d, npd = _batch(B, 405)
    if which == "mask_only":     # FAST_TEST with the observed-box mask update (data_pair.py:106 of the reference)
        cfg, net, params = _bind(ctx, B, 45, fast_test=True, update_mask="box_observed")
        assert net.with_mask_head and not net.with_flow_head
    else:
        cfg, net, params = _bind(ctx, B, 45, pred_mask=False)
        assert net.with_flow_head and not net.with_mask_head
    assert net.fp16_decoder
    out = net.forward({k: ctx.array(v) for k, v in npd.items()})
    zf = net.act["zoom_factor"].asnumpy()
    c3 = emu.nhwc_to_nchw(net.act["Concat3_h"].asnumpy())[:, :770]
    dec = emu.decoder(params, _gpu_acts(net))
    hd = emu.heads(params, dec["Concat3"], zf, H, W, cfg.dataset.NORMALIZE_FLOW, mask=net.with_mask_head, flow=net.with_flow_head)
    if net.with_mask_head:
        assert "flow_est_crop" not in out
        assert rng_rel(net.act["mask_lowres"].asnumpy(), emu.predictor(params, "mask_conv3", c3)) <= 1e-5
        flips = float(np.mean(out["mask_observed_pred"].asnumpy() != hd["mask_observed_pred"]))
        assert flips <= 1e-3, flips
    else:
        assert "mask_observed_pred" not in out
        assert rng_rel(net.act["flow_lowres"].asnumpy(), emu.predictor(params, "Convolution3", c3)) <= 1e-5
        assert rng_rel(out["flow_est_crop"].asnumpy(), hd["flow_est"]) <= 2e-3


def test_fp32_decoder_fallback_matches_oracle_on_own_encoder_outputs(ctx):
    """network.FP16_DECODER = False: the fp32 decoder and heads, fed the fp16 encoder's activations converted to fp32."""
    B = 2
    d, npd = _batch(B, 404)
    cfg, net, params = _bind(ctx, B, 44, fp16_decoder=False)
    assert not net.fp16_decoder and net.with_decoder
    out = net.forward({k: ctx.array(v) for k, v in npd.items()})
    acts = _gpu_acts(net)
    zf = net.act["zoom_factor"].asnumpy()
    dec = opipe.decoder(params, acts)
    for name in ("Concat2", "Concat3"):
        assert rng_rel(net.act[name].asnumpy(), dec[name]) <= 1e-4, name
    _, _, mask = opipe.mask_head(params, dec["Concat3"], zf, H, W)
    _, _, flow = opipe.flow_head(params, dec["Concat3"], zf, H, W, cfg.dataset.NORMALIZE_FLOW)
    assert np.abs(out["flow_est_crop"].asnumpy() - flow).max() <= 1e-4 * max(1.0, np.abs(flow).max())
    assert float(np.mean(out["mask_observed_pred"].asnumpy() != mask)) < 1e-4


def _h16(ctx, a):
    return ctx.array(np.ascontiguousarray(a, np.float16), dtype=np.float16)


def _deconv_case(ctx, rng, B, Cin, Cin_pad, in_ct, Hh, Ww, Cout, Ho, Wo, out_ct, coff):
    x = np.zeros((B, Hh, Ww, in_ct), np.float16)
    x[..., :Cin] = rng.standard_normal((B, Hh, Ww, Cin))
    w = (rng.standard_normal((Cin, Cout, 4, 4)) / np.sqrt(4 * Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32) * 0.1
    h = ctx.handle
    pk = DeviceArray(ctx, (lib.load().deepim_deconv_f16_packed_size(Cin_pad, Cout) // 2,), dtype=np.float16)
    lib.deepim_deconv_f16_pack_weights(h, pk, ctx.array(w), Cin, Cin_pad, Cout)
    sentinel = np.full((B, Ho, Wo, out_ct), 1234.0, np.float16)
    out = _h16(ctx, sentinel)
    lib.deepim_deconv4x4s2_crop_f16_forward(h, out, _h16(ctx, x), pk, ctx.array(b), B, Cin_pad, in_ct, Hh, Ww, Cout, Ho, Wo,
                                            ctypes.c_float(SLOPE), out_ct, coff)
    got = out.asnumpy()
    outside = np.ones(out_ct, bool)
    outside[coff:coff + Cout] = False
    np.testing.assert_array_equal(got[..., outside], sentinel[..., outside])
    return x, w, b, emu.nhwc_to_nchw(got[..., coff:coff + Cout])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", [(1024, 1024, 1024, 8, 10, 512, 15, 20, 1032, 512),     # deconv5 → Concat2
                                   (1026, 1032, 1032, 15, 20, 256, 30, 40, 776, 512),     # deconv4 → Concat3
                                   (40, 40, 48, 5, 7, 64, 9, 13, 72, 4)],                 # small, odd output
                         ids=["deconv5", "deconv4", "small_odd"])
def test_deconv_f16_kernel(ctx, B, shape):
    Cin, Cin_pad, in_ct, Hh, Ww, Cout, Ho, Wo, out_ct, coff = shape
    rng = np.random.default_rng(B * 100 + Cin)
    x, w, b, got = _deconv_case(ctx, rng, B, *shape)
    want = emu.q16(onet.deconv4x4s2_crop(emu.nhwc_to_nchw(x[..., :Cin]), emu.q16(w), b, Ho, Wo, (1, 1), SLOPE))
    assert_ulp(got, want, "deconv_f16 %s B=%d" % (shape, B))


def test_deconv_f16_kernel_batch64_against_fp32_kernel(ctx):
    """BASELINE config 5's batch: the fp32 deconvolution kernel on the same fp16 operands (exact products) is the reference."""
    B, Cin, Cin_pad, Hh, Ww, Cout, Ho, Wo = 64, 1026, 1032, 15, 20, 256, 30, 40
    rng = np.random.default_rng(64)
    x, w, b, got = _deconv_case(ctx, rng, B, Cin, Cin_pad, Cin_pad, Hh, Ww, Cout, Ho, Wo, 776, 512)
    h = ctx.handle
    pk = DeviceArray(ctx, (lib.load().deepim_deconv_packed_size(Cin, Cout) // 4,))
    lib.deepim_deconv_pack_weights(h, pk, ctx.array(emu.q16(w)), Cin, Cout)
    ref = ctx.empty((B, Cout, Ho, Wo))
    lib.deepim_deconv4x4s2_crop_forward(h, ref, ctx.array(emu.nhwc_to_nchw(x[..., :Cin])), pk, ctx.array(b), B, Cin, Hh, Ww, Cout,
                                        Ho, Wo, 1, 1, ctypes.c_float(SLOPE), Cout, 0)
    assert_ulp(got, emu.q16(ref.asnumpy()), "deconv_f16 B=64 vs fp32 kernel")


@pytest.mark.parametrize("case", [(770, 776, 30, 40, 1, 2), (1026, 1032, 15, 20, 2, 0), (1024, 1024, 8, 10, 1, 0),
                                  (770, 776, 30, 40, 2, 0)], ids=["mask1+flow2_on_770", "2_on_1026", "1_on_1024", "2_on_770"])
def test_fewout_f16_kernel(ctx, case):
    Cin, Cin_pad, Hh, Ww, n0, n1 = case
    B = 3
    rng = np.random.default_rng(Cin + n0)
    x = np.zeros((B, Hh, Ww, Cin_pad), np.float16)
    x[..., :Cin] = rng.standard_normal((B, Hh, Ww, Cin))
    w0 = (rng.standard_normal((n0, Cin, 3, 3)) / 30).astype(np.float32)
    w1 = (rng.standard_normal((max(n1, 1), Cin, 3, 3)) / 30).astype(np.float32)
    b0, b1 = rng.standard_normal(n0).astype(np.float32), rng.standard_normal(max(n1, 1)).astype(np.float32)
    h = ctx.handle
    pk = DeviceArray(ctx, (lib.load().deepim_fewout_f16_packed_size(Cin_pad) // 2,), dtype=np.float16)
    lib.deepim_fewout_f16_pack_weights(h, pk, ctx.array(w0), n0, ctx.array(w1) if n1 else None, n1, Cin, Cin_pad)
    o0, o1 = ctx.zeros((B, n0, Hh, Ww)), ctx.zeros((B, max(n1, 1), Hh, Ww))
    lib.deepim_conv3x3_fewout_f16_forward(h, o0, n0, o1 if n1 else None, n1, _h16(ctx, x), pk, ctx.array(b0),
                                          ctx.array(b1) if n1 else None, B, Hh, Ww, Cin_pad, Cin_pad)
    xin = emu.nhwc_to_nchw(x[..., :Cin])
    want0 = onet.conv2d(xin, emu.q16(w0), b0, 1, 1, 1.0)
    assert rng_rel(o0.asnumpy(), want0) <= 1e-5
    if n1:
        want1 = onet.conv2d(xin, emu.q16(w1), b1, 1, 1, 1.0)
        assert rng_rel(o1.asnumpy(), want1) <= 1e-5


def test_upsample_flow_f16_and_slice_copy(ctx):
    B = 3
    rng = np.random.default_rng(9)
    flow = (rng.standard_normal((B, 2, 15, 20)) * 3).astype(np.float32)
    w = rng.standard_normal((2, 2, 4, 4)).astype(np.float32)
    b = rng.standard_normal(2).astype(np.float32)
    h = ctx.handle
    sentinel = np.full((B, 30, 40, 776), -77.0, np.float16)
    out = _h16(ctx, sentinel)
    lib.deepim_upsample_flow_f16_forward(h, out, ctx.array(flow), ctx.array(w), ctx.array(b), B, 15, 20, 30, 40, 776, 768)
    got = out.asnumpy()
    want = emu.q16(onet.deconv4x4s2_crop(flow, w, b, 30, 40, (1, 1), 1.0))
    bad = np.abs(emu.nhwc_to_nchw(got[..., 768:770]) - want) > ulp16(want)
    assert not bad.any(), bad.sum()
    np.testing.assert_array_equal(got[..., :768], sentinel[..., :768])
    np.testing.assert_array_equal(got[..., 770:], sentinel[..., 770:])
    # slice copy: bit-exact into [0, 512), the rest untouched
    src = rng.standard_normal((B, 30, 40, 512)).astype(np.float16)
    lib.deepim_copy_channels_nhwc_f16(h, out, 776, 0, _h16(ctx, src), 512, 0, 512, B * 30 * 40)
    got2 = out.asnumpy()
    np.testing.assert_array_equal(got2[..., :512].view(np.uint16), src.view(np.uint16))
    np.testing.assert_array_equal(got2[..., 512:].view(np.uint16), got[..., 512:].view(np.uint16))


def test_fp16_decoder_graph_replay_matches_eager(ctx):
    B = 2
    d, npd = _batch(B, 407)
    cfg, net, params = _bind(ctx, B, 47)
    data = {k: ctx.array(v) for k, v in npd.items()}
    pose_out = ctx.empty((B, 3, 4))
    eager = net.refine_iteration(data, pose_out).asnumpy()
    keys = ("flow_est", "mask_observed_pred", "se3", "Concat3_h")
    want = {k: net.act[k].asnumpy() for k in keys}
    for k in keys:
        net.act[k].copyfrom(np.zeros(net.act[k].shape, net.act[k].dtype))
    gid = net.capture_iteration(data, pose_out)
    net.replay(gid)
    np.testing.assert_array_equal(pose_out.asnumpy(), eager)
    for k in keys:
        np.testing.assert_array_equal(net.act[k].asnumpy(), want[k], err_msg=k)
