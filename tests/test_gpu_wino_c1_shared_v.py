"""conv1's shared-transform Winograd kernel (csrc/wino_c1.hip: 64 output channels x 32 tiles per block, V shared through LDS, the
four position roles of a channel half) against the C oracle's direct convolution at 1e-5 of the layer's range, at the shapes that
exercise its branches: the bench batch at full size, small and mid batches, partial last tile blocks, odd output sizes, the
scalar-load variant (W % 4 != 0) and both output modes. Also: two runs are bit-identical, and a sample's output does not depend on
the batch it runs in (the grid size follows the tile count)."""
import ctypes

import numpy as np
import pytest

from oracle import net as onet
from mx_deepim_amd.runtime import DeviceArray, lib

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
TOL = 1e-5
SLOPE = 0.1


def _layer(seed, B, H, W):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, 8, H, W)).astype(np.float32)
    w = (rng.standard_normal((64, 8, 7, 7)) / np.sqrt(8 * 49)).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    return x, w, b


def _pack(ctx, w):
    pk = DeviceArray(ctx, (lib.load().deepim_conv1_wino_packed_size() // 4,))
    lib.deepim_conv1_wino_pack_weights(ctx.handle, pk, ctx.array(w))
    return pk


def _run(ctx, x, pk, b, out_mode):
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = ctx.zeros((B, 64, Ho, Wo))
    rc = lib.deepim_conv1_wino_forward(ctx.handle, out, ctx.array(x), pk, ctx.array(b), B, H, W, cf(SLOPE), out_mode)
    assert rc == 0
    if out_mode == 1:
        y = out.asnumpy()
        return np.ascontiguousarray(y.reshape(B, 8, Ho, Wo, 8).transpose(0, 1, 4, 2, 3).reshape(B, 64, Ho, Wo))
    plain = ctx.zeros((B, 64, Ho, Wo))
    lib.deepim_relayout_nc8_s2d(ctx.handle, plain, out, B, 64, Ho, Wo, 0)
    return plain.asnumpy()


def _check(got, ref):
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max()) / scale
    assert err <= TOL, err


def test_bench_batch_full_size(ctx):
    """B = 32 at 480 x 640 (the bench layer, 19 200 tile blocks over a full grid); three samples checked against the oracle."""
    x, w, b = _layer(31, 32, 480, 640)
    pk = _pack(ctx, w)
    got = _run(ctx, x, pk, b, 3)
    for s in (0, 13, 31):
        _check(got[s], onet.conv2d(x[s:s + 1], w, b, 2, 3, SLOPE)[0])


# (B, H, W, out_mode): B = 4 and 8; one tile block per row (TX = 25 < 32, partial); 161 tile columns (the last block holds one tile);
# odd output height and width; W % 4 != 0 (the scalar-load variant) with a partial block; fewer tile blocks than blocks in the grid
CASES = [
    (4, 96, 128, 3),
    (8, 64, 96, 1),
    (4, 40, 100, 3),
    (1, 18, 644, 1),
    (2, 61, 99, 1),
    (3, 34, 70, 1),
    (2, 28, 43, 3),
    (1, 3, 3, 1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_%dx%d_mode%d" % c)
def test_shapes_within_1e5_of_the_direct_convolution(ctx, case):
    B, H, W, mode = case
    x, w, b = _layer(B * 7919 + H * 31 + W, B, H, W)
    ref = onet.conv2d(x, w, b, 2, 3, SLOPE)
    pk = _pack(ctx, w)
    for m in sorted({1, mode}):
        _check(_run(ctx, x, pk, b, m), ref)


def test_bit_identical_runs_and_independent_of_the_grid(ctx):
    x, w, b = _layer(77, 8, 96, 128)
    pk = _pack(ctx, w)
    a = _run(ctx, x, pk, b, 1)
    np.testing.assert_array_equal(a, _run(ctx, x, pk, b, 1))
    # one sample alone: 48 tile blocks on a grid of 48 blocks instead of 384 on 256; every tile is summed in the same order
    for s in (0, 5):
        np.testing.assert_array_equal(a[s:s + 1], _run(ctx, np.ascontiguousarray(x[s:s + 1]), pk, b, 1))
    # the scalar-load variant (W % 4 != 0) is as deterministic
    xs = np.ascontiguousarray(x[:2, :, :, :127])
    ys = _run(ctx, xs, pk, b, 1)
    np.testing.assert_array_equal(ys, _run(ctx, xs, pk, b, 1))
