"""conv1 as fp32 Winograd F(2x2,4x4) over its four input phases (csrc/wino_c1.hip) against the C oracle's direct convolution: a
different summation of the same layer, so the bar is 1e-5 of the layer's output range, not bit equality."""
import ctypes

import numpy as np
import pytest

from oracle import net as onet
from mx_deepim_amd.runtime import DeviceArray, lib

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
TOL = 1e-5
SLOPE = 0.1


def _pack(ctx, w):
    pk = DeviceArray(ctx, (lib.load().deepim_conv1_wino_packed_size() // 4,))
    lib.deepim_conv1_wino_pack_weights(ctx.handle, pk, ctx.array(w))
    return pk


def _from_nc8(y, shape):
    B, C, H, W = shape
    return np.ascontiguousarray(y.reshape(B, C // 8, H, W, 8).transpose(0, 1, 4, 2, 3).reshape(B, C, H, W))


def _layer(seed, B, H, W):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, 8, H, W)).astype(np.float32)
    w = (rng.standard_normal((64, 8, 7, 7)) / np.sqrt(8 * 49)).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    return x, w, b


def _run(ctx, x, pk, b, out_mode):
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = ctx.zeros((B, 64, Ho, Wo))
    rc = lib.deepim_conv1_wino_forward(ctx.handle, out, ctx.array(x), pk, ctx.array(b) if b is not None else None, B, H, W,
                                       cf(SLOPE), out_mode)
    assert rc == 0
    if out_mode == 1:
        return _from_nc8(out.asnumpy(), (B, 64, Ho, Wo))
    plain = ctx.zeros((B, 64, Ho, Wo))
    lib.deepim_relayout_nc8_s2d(ctx.handle, plain, out, B, 64, Ho, Wo, 0)
    return plain.asnumpy()


# (B, H, W): the bench geometry at B = 1, reduced images at B = 3 and 32, odd output height / width, a partial last tile block
# (161 tile columns), an input width that is not a multiple of 4, images smaller than one tile block
CASES = [
    (1, 480, 640, 3),
    (3, 96, 128, 3),
    (32, 40, 64, 3),
    (2, 62, 100, 3),      # 31 x 50 output: odd height
    (1, 22, 644, 3),      # 161 tile columns: the last tile block holds one tile
    (2, 37, 41, 1),       # 19 x 21 output, W % 4 != 0: the scalar-load variant
    (1, 5, 7, 1),         # 3 x 4 output: every patch reaches the padding
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_%dx%d_mode%d" % c)
def test_conv1_wino_within_1e5_of_the_direct_convolution(ctx, case):
    B, H, W, mode = case
    if mode == 3 and (((H - 1) // 2 + 1) | ((W - 1) // 2 + 1)) & 1:
        mode = 1
    x, w, b = _layer(hash(case) % (2 ** 31), B, H, W)
    ref = onet.conv2d(x, w, b, 2, 3, SLOPE)
    scale = max(1.0, float(np.abs(ref).max()))
    pk = _pack(ctx, w)
    for m in sorted({1, mode}):
        got = _run(ctx, x, pk, b, m)
        err = np.abs(got - ref).max() / scale
        assert err <= TOL, (m, err)


def test_conv1_wino_bias_and_slope_applied(ctx):
    x, w, b = _layer(5, 2, 30, 40)
    pk = _pack(ctx, w)
    ref_nb = onet.conv2d(x, w, np.zeros_like(b), 2, 3, SLOPE)
    got_nb = _run(ctx, x, pk, None, 1)
    assert np.abs(got_nb - ref_nb).max() <= TOL * max(1.0, np.abs(ref_nb).max())
    got = _run(ctx, x, pk, b, 1)
    assert (got < 0).any() and (got > 0).any()
    assert np.abs(got - onet.conv2d(x, w, b, 2, 3, SLOPE)).max() <= TOL * max(1.0, np.abs(got).max())


def test_conv1_wino_deterministic(ctx):
    x, w, b = _layer(9, 4, 96, 128)
    pk = _pack(ctx, w)
    a = _run(ctx, x, pk, b, 3)
    c = _run(ctx, x, pk, b, 3)
    np.testing.assert_array_equal(a, c)


def test_conv1_wino_routing(ctx):
    h = ctx.handle
    assert lib.load().deepim_conv1_wino_preferred(h, 32, 8, 480, 640, 64) == 1
    assert lib.load().deepim_conv1_wino_preferred(h, 32, 10, 480, 640, 64) == 0    # other input channel counts stay direct
    lib.deepim_set_option(h, b"conv_max_split", 1)
    try:
        assert lib.load().deepim_conv1_wino_preferred(h, 32, 8, 480, 640, 64) == 0  # canonical order: the direct kernel
    finally:
        lib.deepim_set_option(h, b"conv_max_split", 0)


def test_conv1_wino_bound_only_with_winograd_on(ctx):
    from mx_deepim_amd.config import default_config
    from mx_deepim_amd.symbols import deepIM_flownet
    for on in (True, False):
        cfg = default_config()
        cfg.network.WINOGRAD_CONV = on
        net = deepIM_flownet().get_symbol(cfg)
        net.bind(ctx, 1, net.init_weights(cfg, seed=3))
        assert (net.wino_conv1 is not None) == on
        assert "flow_conv1" not in net.packed_wino and "flow_conv1" not in net.wino_s2d
