"""fp16 Winograd F(2x2,3x3) (csrc/wino_f16.hip, network.FP16_WINOGRAD) on the GPU against the numpy restatement of its arithmetic
contract (tests/fp16_wino_emulation.py, float64 accumulation). Per layer the bar is that of test_conv_f16_matches_emulation, for the
same reason — same operands, another fp32 summation order, one fp16 rounding: max |got - emu| <= 2^-10 max(1, |emu|max) and fewer
than 2 % of the elements differ."""
import ctypes

import numpy as np
import pytest

import fp16_wino_emulation as emu
from oracle import pipeline as opipe
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import DeviceArray, lib
from mx_deepim_amd.symbols import deepIM_flownet
from mx_deepim_amd.symbols.deepIM_flownet import ENCODER

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
MEANS_REV = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])
WINO_LAYERS = ["conv3_1", "conv4_1", "conv5_1", "conv6_1"]

SHAPES = [(1, 32, 2, 2, 128),        # one tile, all halo
          (2, 64, 7, 9, 128),        # odd H and W, a partly filled tile block that spans two images
          (1, 96, 15, 20, 256),      # conv5_1's frame, an odd number of k-steps, channel blocks
          (3, 256, 8, 10, 128),      # conv6_1's frame, a ragged second tile block
          (2, 1024, 8, 10, 256),     # the longest K walk
          (1, 128, 60, 80, 256)]     # conv3_1's frame, many tile blocks


def _inputs(shape):
    B, cin, H, W, cout = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    return x, w, b


def _pack(ctx, w):
    cout, cin = w.shape[:2]
    nb = lib.load().deepim_conv_wino_f16_packed_size(cout, cin)
    assert nb == cout * cin * 32
    pk = DeviceArray(ctx, (nb // 2,), dtype=np.float16)
    lib.deepim_conv_wino_f16_pack_weights(ctx.handle, pk, ctx.array(w), cout, cin)
    return pk


def _wino_f16(ctx, x, w, b, slope=0.1, runs=1):
    """-> `runs` results as NHWC fp16 arrays (fresh output buffer each)"""
    B, cin, H, W = x.shape
    cout = w.shape[0]
    xh = ctx.array(np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(np.float16), dtype=np.float16)
    pk, bd = _pack(ctx, w), ctx.array(b)
    outs = []
    for _ in range(runs):
        oh = ctx.zeros((B, H, W, cout), dtype=np.float16)
        lib.deepim_conv2d_wino_f16_forward(ctx.handle, oh, xh, pk, bd, B, cin, H, W, cout, cf(slope))
        outs.append(oh.asnumpy())
    return outs


def _nchw(h):
    return np.ascontiguousarray(np.asarray(h, np.float32).transpose(0, 3, 1, 2))


def _layer_bar(got, want, what):
    err = np.abs(got - want).max()
    diff = float(np.mean(got != want))
    print("%s: max |got - emu| %.3g (%.3g of the range), %.3f %% of elements differ" %
          (what, err, err / np.abs(want).max(), 100 * diff))
    assert err <= 2.0 ** -10 * max(1.0, np.abs(want).max()), what
    assert diff < 0.02, what


@pytest.mark.parametrize("shape", SHAPES)
def test_wino_f16_matches_emulation(ctx, shape):
    x, w, b = _inputs(shape)
    got = _nchw(_wino_f16(ctx, x, w, b)[0])
    _layer_bar(got, emu.conv_wino(x, w, b, 0.1), str(shape))


def test_packed_weights_decode_to_the_emulations_u(ctx):
    """128 x 64 layer: the packed buffer, read by the layout include/deepim_hip.h documents, is the emulation's U bit for bit."""
    cout, cin = 128, 64
    w = (np.random.default_rng(9).standard_normal((cout, cin, 3, 3)) / 24).astype(np.float32)
    pk = _pack(ctx, w).asnumpy()
    assert pk.dtype == np.float16 and pk.size == cout * cin * 16
    co, ci, p = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(16), indexing="ij")
    lane = co % 32 + 32 * ((ci // 8) % 2)
    idx = ((((co // 32) * (cin // 16) + ci // 16) * 16 + p) * 64 + lane) * 8 + ci % 8
    assert np.unique(idx).size == pk.size
    u = emu.transform_weights(w).reshape(cout, cin, 16).astype(np.float16)
    np.testing.assert_array_equal(pk[idx].view(np.uint16), u.view(np.uint16))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]])
def test_wino_f16_is_deterministic(ctx, shape):
    x, w, b = _inputs(shape)
    outs = _wino_f16(ctx, x, w, b, runs=4)
    for o in outs[1:]:
        np.testing.assert_array_equal(o.view(np.uint16), outs[0].view(np.uint16))


@pytest.mark.parametrize("cin,cout", [(48, 128), (16, 128), (32, 96), (64, 32), (0, 128)])
def test_unsupported_shapes_are_refused(ctx, cin, cout):
    L = lib.load()
    assert L.deepim_conv_wino_f16_supported(cin, cout) == 0
    assert L.deepim_conv_wino_f16_packed_size(cout, cin) == 0
    for ok in ((256, 256), (512, 512), (1024, 1024), (32, 128)):
        assert L.deepim_conv_wino_f16_supported(*ok) == 1
    n = 2 * 4 * 4 * max(cout, 1)
    sentinel = np.full(n, 7.0, np.float16)
    out = ctx.array(sentinel, dtype=np.float16)
    xin = ctx.zeros((2 * 4 * 4 * max(cin, 8),), dtype=np.float16)
    pk = ctx.zeros((max(cout * cin * 16, 64),), dtype=np.float16)
    bias = ctx.zeros((max(cout, 1),))
    with pytest.raises(RuntimeError):
        lib.deepim_conv2d_wino_f16_forward(ctx.handle, out, xin, pk, bias, 2, cin, 4, 4, cout, cf(0.1))
    with pytest.raises(RuntimeError):
        lib.deepim_conv_wino_f16_pack_weights(ctx.handle, pk, ctx.zeros((max(cout * cin * 9, 9),)), cout, cin)
    np.testing.assert_array_equal(out.asnumpy(), sentinel)      # nothing was launched on the output
    assert not pk.asnumpy().any()


def _bind(ctx, B, params=None, wino=False, heads=False):
    cfg = default_config()
    cfg.network.FP16_CONV = True
    cfg.network.FP16_WINOGRAD = wino
    if heads:
        cfg.TEST.FAST_TEST = False
    net = deepIM_flownet().get_symbol(cfg)
    if params is None:
        params = net.init_weights(cfg, seed=7)
    net.bind(ctx, B, params)
    return cfg, net, params


@pytest.fixture(scope="module")
def iteration(ctx, small_batch):
    """One refinement iteration of the same parameters and batch: key off, key on, key off again (same context)."""
    d = small_batch
    B = d["image_observed"].shape[0]
    cfg, off, params = _bind(ctx, B)
    data = {k: ctx.array(d[k]) for k in ("image_observed", "mask_observed")}
    data.update({k: ctx.array(d[k][0]) for k in ("image_rendered", "mask_rendered", "src_pose")})
    pose_off = off.refine_iteration(data).asnumpy().copy()
    _, on, _ = _bind(ctx, B, params, wino=True)
    pose_on = on.refine_iteration(data).asnumpy().copy()
    pose_off_again = off.refine_iteration(data).asnumpy().copy()
    npd = {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][0], "mask_observed": d["mask_observed"],
           "mask_rendered": d["mask_rendered"][0], "src_pose": d["src_pose"][0]}
    args = (params, npd, d["K"], MEANS_REV, cfg.dataset.trans_means, cfg.dataset.trans_stds, cfg.network.ROT_COORD)
    return dict(cfg=cfg, off=off, on=on, params=params, pose_off=pose_off, pose_on=pose_on, pose_off_again=pose_off_again, args=args)


def test_iteration_layers_against_emulation_on_own_inputs(iteration):
    """Every Winograd layer of the keyed network against the emulation fed the GPU's own previous activation."""
    net, params = iteration["on"], iteration["params"]
    assert net.fp16_winograd and net.fp16_wino_layers == WINO_LAYERS
    assert sorted(net.packed_f16_wino) == sorted(WINO_LAYERS)
    names = [e[0] for e in ENCODER]
    for name in WINO_LAYERS:
        x = _nchw(net.act[names[names.index(name) - 1] + "_h"].asnumpy())
        want = emu.conv_wino(x, params[name + "_weight"], params[name + "_bias"], opipe.SLOPE)
        _layer_bar(_nchw(net.act[name + "_h"].asnumpy()), want, name)


def test_iteration_against_emulation_chain_and_fp32(iteration):
    """The whole iteration against the emulation chain at the bars of test_fp16_iteration_vs_emulation_and_fp32, and the pose against
    the fp32 oracle (< 2e-2, that test's bar), printed beside the deviation of the same network bound with the key off."""
    net, args = iteration["on"], iteration["args"]
    ref = emu.refine_iteration(*args, wino_layers=WINO_LAYERS)
    c = net.act["conv6_1"].asnumpy()
    e61 = np.abs(c - ref["conv6_1"]).max() / np.abs(ref["conv6_1"]).max()
    ese3 = np.abs(net.act["se3"].asnumpy() - ref["se3"]).max() / np.abs(ref["se3"]).max()
    epose = np.abs(iteration["pose_on"] - ref["pose_est"]).max() / np.abs(ref["pose_est"]).max()
    print("fp16 Winograd iteration vs its emulation chain: conv6_1 %.3g of range, se3 %.3g, pose %.3g" % (e61, ese3, epose))
    ref32 = opipe.refine_iteration(*args)
    scale = np.abs(ref32["pose_est"]).max()
    dev_on = np.abs(iteration["pose_on"] - ref32["pose_est"]).max() / scale
    dev_off = np.abs(iteration["pose_off"] - ref32["pose_est"]).max() / scale
    print("pose deviation from the fp32 oracle: %.3g with FP16_WINOGRAD, %.3g with the direct fp16 kernels" % (dev_on, dev_off))
    assert e61 <= 2e-3 and ese3 < 1e-3 and epose < 1e-4, (e61, ese3, epose)
    assert dev_on < 2e-2, dev_on


def test_default_network_is_untouched(iteration):
    off = iteration["off"]
    assert off.fp16_winograd is False
    assert not hasattr(off, "packed_f16_wino") and not hasattr(off, "fp16_wino_layers")
    np.testing.assert_array_equal(iteration["pose_off_again"], iteration["pose_off"])
    assert not np.array_equal(iteration["pose_on"], iteration["pose_off"])      # the key does change the arithmetic


def test_heads_read_the_winograd_layers_output(ctx, small_batch):
    """PRED_MASK / PRED_FLOW with the fp16 decoder: one iteration runs, conv4_1 is the Winograd contract's result, and channels 0-511
    of the fp16 Concat3 equal it bit for bit."""
    d = small_batch
    B = d["image_observed"].shape[0]
    _, net, params = _bind(ctx, B, wino=True, heads=True)
    assert net.fp16_decoder and net.with_mask_head and net.with_flow_head and net.fp16_wino_layers == WINO_LAYERS
    data = {k: ctx.array(d[k]) for k in ("image_observed", "mask_observed")}
    data.update({k: ctx.array(d[k][0]) for k in ("image_rendered", "mask_rendered", "src_pose")})
    pose = net.refine_iteration(data).asnumpy()
    assert np.isfinite(pose).all()
    c41 = net.act["conv4_1_h"].asnumpy()
    want = emu.conv_wino(_nchw(net.act["conv4_h"].asnumpy()), params["conv4_1_weight"], params["conv4_1_bias"], opipe.SLOPE)
    _layer_bar(_nchw(c41), want, "conv4_1 (heads graph)")
    np.testing.assert_array_equal(net.act["Concat3_h"].asnumpy()[..., :512].view(np.uint16), c41.view(np.uint16))
    assert np.isfinite(net.act["flow_lowres"].asnumpy()).all() and np.isfinite(net.act["mask_lowres"].asnumpy()).all()
