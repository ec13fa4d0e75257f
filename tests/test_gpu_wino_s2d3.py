"""conv4 / conv5 (3x3, stride 2, pad 1) as fp32 F(2x2,3x3) over the space-to-depth input (csrc/wino.hip, S2D = 2 walk: 25 of the 64
(phase, position) GEMMs) against the C oracle's direct convolution, bar 1e-5 of the layer's range; the bindings of the network and the
heads-mode skip of a space-to-depth activation."""
import ctypes

import numpy as np
import pytest

from oracle import net as onet
from oracle import pipeline as opipe
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import DeviceArray, lib
from mx_deepim_amd.symbols import deepIM_flownet

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
TOL = 1e-5
MEANS_REV = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])


@pytest.fixture(params=[0, 3, 2], ids=["block_64x64", "block_128x32", "block_64x32_two_per_cu"])
def block_shape(ctx, request):
    """Every shared-transform block shape (wino_wide 0 / 3 / 2; 3 falls back to 64 x 64 where Cout % 128 != 0)."""
    lib.deepim_set_option(ctx.handle, b"wino_wide", request.param)
    yield request.param
    for k, v in ((b"wino_wide", 1), (b"wino_streamk", 1), (b"wino_split", 0), (b"wino_s2d_skip", 1), (b"conv_max_split", 0)):
        lib.deepim_set_option(ctx.handle, k, v)


def _from_nc8(y, shape):
    B, C, H, W = shape
    return np.ascontiguousarray(y.reshape(B, C // 8, H, W, 8).transpose(0, 1, 4, 2, 3)).reshape(B, C, H, W)


_REF = {}


def _layer(case):
    """Operands and the oracle's output of a case (B, Cin, H, W, Cout), computed once per module."""
    if case not in _REF:
        B, cin, H, W, cout = case
        rng = np.random.default_rng(sum(case))
        x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
        w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        _REF[case] = (x, w, b, onet.conv2d(x, w, b, 2, 1, 0.1))
    return _REF[case]


def _operands(ctx, case):
    B, cin, H, W, cout = case
    x, w, b, ref = _layer(case)
    xs = ctx.empty((B, 4 * cin, H // 2, W // 2))
    lib.deepim_relayout_nc8_s2d(ctx.handle, xs, ctx.array(x), B, cin, H, W, 1)
    pk = DeviceArray(ctx, (lib.load().deepim_conv_wino_packed_size(cout, 4 * cin) // 4,))
    lib.deepim_conv_wino_pack_weights_s2d3(ctx.handle, pk, ctx.array(w), cout, cin)
    return xs, pk, ctx.array(b), ref


def _run(ctx, case, xs, pk, bias, out_nc8=1):
    B, cin, H, W, cout = case
    Ho, Wo = H // 2, W // 2
    o = ctx.array(np.full((B, cout, Ho, Wo), np.nan, np.float32))        # every output element must be written
    lib.deepim_conv2d_wino_forward_s2d3(ctx.handle, o, xs, pk, bias, B, cin, H, W, cout, cf(0.1), out_nc8, 0, 0)
    if out_nc8 == 1:
        return _from_nc8(o.asnumpy(), (B, cout, Ho, Wo))
    if out_nc8 == 3:
        nchw = ctx.empty((B, cout, Ho, Wo))
        lib.deepim_relayout_nc8_s2d(ctx.handle, nchw, o, B, cout, Ho, Wo, 0)
        return nchw.asnumpy()
    return o.asnumpy()


def _plan(B, cin, H, W, cout, ctx=None):
    plan = (ctypes.c_int * 9)()
    assert lib.load().deepim_conv_wino_plan(ctx.handle if ctx else None, B, 4 * cin, H // 2, W // 2, cout, 1, 2, plan) == 0
    return list(plan)


CASES = [
    (1, 256, 60, 80, 512),     # conv4 at B = 1
    (1, 512, 30, 40, 512),     # conv5 at B = 1 (15 output rows: a half-filled last tile row)
    (2, 16, 12, 16, 64),       # one 8-channel block per phase... of an even pair: one eight-step loop body
    (3, 32, 10, 14, 128),      # ragged tile block, odd plane height and width (5 x 7)
    (2, 64, 6, 10, 64),        # 3 x 5 planes: most patch pixels in the padding
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_stride2_3x3_layer_against_direct_conv(ctx, case, block_shape):
    """The layer within 1e-5 of the direct convolution in every output layout; the full 16-position walk (wino_s2d_skip = 0: the
    dead pairs multiplied as exact zeros, channels in their natural order) agrees to rounding."""
    xs, pk, bias, ref = _operands(ctx, case)
    scale = max(1.0, float(np.abs(ref).max()))
    got = _run(ctx, case, xs, pk, bias)
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= TOL * scale, np.abs(got - ref).max() / scale
    B, cin, H, W, cout = case
    if (H // 2) % 2 == 0 and (W // 2) % 2 == 0:                    # space-to-depth output: the same values at their phase addresses
        np.testing.assert_array_equal(_run(ctx, case, xs, pk, bias, 3), got)
    nchw = _run(ctx, case, xs, pk, bias, 0)
    assert np.abs(nchw - ref).max() <= TOL * scale
    lib.deepim_set_option(ctx.handle, b"wino_s2d_skip", 0)
    try:
        full = _run(ctx, case, xs, pk, bias)
    finally:
        lib.deepim_set_option(ctx.handle, b"wino_s2d_skip", 1)
    assert np.abs(full - ref).max() <= TOL * scale
    assert np.abs(full - got).max() <= 2e-6 * scale


@pytest.mark.parametrize("case", CASES[:2], ids=["conv4", "conv5"])
def test_stride2_3x3_k_split(ctx, case, block_shape):
    """The plan at B = 1 splits K (whole eight-step bodies per slice); one slice (wino_split = 1) gives the same sums to rounding."""
    B, cin, H, W, cout = case
    plan = _plan(B, cin, H, W, cout, ctx)
    assert plan[2] > 1 and plan[3] % 8 == 0, plan
    xs, pk, bias, ref = _operands(ctx, case)
    scale = max(1.0, float(np.abs(ref).max()))
    split = _run(ctx, case, xs, pk, bias)
    lib.deepim_set_option(ctx.handle, b"wino_split", 1)
    try:
        assert _plan(B, cin, H, W, cout, ctx)[2] == 1
        one = _run(ctx, case, xs, pk, bias)
    finally:
        lib.deepim_set_option(ctx.handle, b"wino_split", 0)
    assert np.abs(one - ref).max() <= TOL * scale
    assert np.abs(one - split).max() <= 2e-6 * scale


def test_stride2_3x3_stream_k(ctx, block_shape):
    """Stream-K cuts between eight-step loop bodies (granule = two 8-channel blocks of each input phase)."""
    case = (6, 32, 128, 128, 256)
    B, cin, H, W, cout = case
    xs, pk, bias, ref = _operands(ctx, case)
    scale = max(1.0, float(np.abs(ref).max()))
    outs = []
    for sk in (0, 2):
        lib.deepim_set_option(ctx.handle, b"wino_streamk", sk)
        plan = _plan(B, cin, H, W, cout, ctx)
        if block_shape == 0:
            assert (plan[4] == 2) == (sk > 0), plan            # 16 steps = 2 granules of 8
        outs.append(_run(ctx, case, xs, pk, bias, 3))
    lib.deepim_set_option(ctx.handle, b"wino_streamk", 1)
    assert np.abs(outs[1] - ref).max() <= TOL * scale
    assert np.abs(outs[1] - outs[0]).max() <= 2e-6 * scale


def test_preferred_s2d3(ctx):
    L = lib.load()
    assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 32, 256, 60, 80, 512) == 1          # conv4
    assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 32, 512, 30, 40, 512) == 1          # conv5
    assert L.deepim_conv_wino_preferred_s2d3(None, 32, 512, 30, 40, 512) == 1
    assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 8, 256, 60, 80, 512) == 1           # measured faster from B = 8 on ...
    assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 8, 512, 30, 40, 512) == 1
    assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 4, 256, 60, 80, 512) == 0           # ... not at B = 4
    assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 4, 512, 30, 40, 512) == 0
    assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 32, 512, 15, 20, 1024) == 0         # conv6: odd input, stays direct
    assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 32, 256, 60, 80, 96) == 0           # Cout % 64 != 0
    lib.deepim_set_option(ctx.handle, b"conv_max_split", 1)                                 # the canonical-order configuration
    try:
        assert L.deepim_conv_wino_preferred_s2d3(ctx.handle, 32, 256, 60, 80, 512) == 0
    finally:
        lib.deepim_set_option(ctx.handle, b"conv_max_split", 0)


def _data(ctx, d, f=0):
    return {"image_observed": ctx.array(d["image_observed"]), "image_rendered": ctx.array(d["image_rendered"][f]),
            "mask_observed": ctx.array(d["mask_observed"]), "mask_rendered": ctx.array(d["mask_rendered"][f]),
            "src_pose": ctx.array(d["src_pose"][f])}


def _np_data(d, f=0):
    return {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][f],
            "mask_observed": d["mask_observed"], "mask_rendered": d["mask_rendered"][f], "src_pose": d["src_pose"][f]}


@pytest.fixture(scope="module")
def batch8():
    """8 synthetic 480x640 pairs: the smallest batch at which conv4 / conv5 are bound to the new path."""
    return synthetic.make_batch(8, seed=2334, n_frames=1)


def test_network_binds_conv4_conv5(ctx, batch8):
    """Default bind: conv4 and conv5 on the new path (their producers write space-to-depth), conv6 on the direct kernel; the pose of
    one refinement iteration within 1e-4 of the oracle, conv4 / conv5 within the layer bar. conv_max_split = 1 after bind puts both
    back on the direct kernels (asked per call)."""
    d = batch8
    B = d["image_observed"].shape[0]
    cfg = default_config()
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=7)
    net.bind(ctx, B, params)
    assert sorted(net.wino_s2d3) == ["conv4", "conv5"]
    assert "conv4" not in net.packed_wino and "conv5" not in net.packed_wino
    names = [g[0] for g in net.enc_geom]
    assert [net._enc_out_mode(names.index(n)) for n in ("conv3_1", "conv4_1", "conv5_1")] == [3, 3, 1]
    pose = net.refine_iteration(_data(ctx, d)).asnumpy()
    ref = opipe.refine_iteration(params, _np_data(d), d["K"], MEANS_REV, cfg.dataset.trans_means, cfg.dataset.trans_stds,
                                 cfg.network.ROT_COORD, nc8=True)
    for name in ("conv4", "conv5", "conv6_1"):
        a = net.activation_nchw(name).asnumpy()
        assert np.abs(a - ref[name]).max() <= 1e-5 * np.abs(ref[name]).max(), name
    assert np.abs(pose - ref["pose_est"]).max() / np.abs(ref["pose_est"]).max() < 1e-4
    lib.deepim_set_option(ctx.handle, b"conv_max_split", 1)
    try:
        assert not net._s2d3_live(names.index("conv4")) and net._enc_out_mode(names.index("conv3_1")) == 1
    finally:
        lib.deepim_set_option(ctx.handle, b"conv_max_split", 0)
    net32 = deepIM_flownet().get_symbol(cfg)
    net32.bind(ctx, 32, params)
    assert sorted(net32.wino_s2d3) == ["conv4", "conv5"]
    cfg2 = default_config()
    cfg2.network.WINOGRAD_CONV = False
    net_off = deepIM_flownet().get_symbol(cfg2)
    net_off.bind(ctx, B, params)
    assert not net_off.wino_s2d3 and not net_off.packed_wino


def test_heads_skip_from_space_to_depth_activation(ctx, batch8):
    """Heads mode: conv4_1 is written space-to-depth for conv5 and reaches Concat3 in one pass (deepim_relayout_nc8_s2d_slice) —
    the same bits as its NCHW conversion, and within 1e-5 of the range of the old path's (conv4 / conv5 direct) skip tensors."""
    d = batch8
    B = d["image_observed"].shape[0]
    cfg = default_config()
    cfg.TEST.FAST_TEST = False
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=8)
    net.bind(ctx, B, params)
    assert sorted(net.wino_s2d3) == ["conv4", "conv5"]
    net.forward(_data(ctx, d))
    cat3, cat2 = net.act["Concat3"].asnumpy(), net.act["Concat2"].asnumpy()
    np.testing.assert_array_equal(cat3[:, :512], net.activation_nchw("conv4_1").asnumpy())
    np.testing.assert_array_equal(cat2[:, :512], net.activation_nchw("conv5_1").asnumpy())
    net.wino_s2d3 = {}                                     # the old path: conv4 / conv5 on the direct kernel, NC8 skips
    net.forward(_data(ctx, d))
    old3, old2 = net.act["Concat3"].asnumpy(), net.act["Concat2"].asnumpy()
    for new, old in ((cat3[:, :512], old3[:, :512]), (cat2[:, :512], old2[:, :512])):
        assert np.abs(new - old).max() <= 1e-5 * np.abs(old).max()
