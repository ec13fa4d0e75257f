"""The fp32 weight gradient (csrc/backward.hip: few-filter stream kernel, LDS-staged and register-fed MFMA kernels, the scalar and the
four-quarter slice reduce) at its edge shapes — the rows of tests/fp32_backward_cases.py, which tests/test_fp32_backward_cases_host.py
pins to the plans they reach — against int64 / float64 references of the same operands, over the whole tensor:
  a. operands whose every partial sum is an integer below 2^24: deepim_conv2d_wgrad, the tap-major and the channel-blocked entries and
     deepim_conv2d_wgrad_bias equal the int64 sums bit for bit, whatever the chunks, slices and quarters; db too;
  b. random operands: every element within gamma_n * sum|x*dz| + 2^-149 of the float64 sum, n = B*Ho*Wo + 1 (db: n = B*Ho*Wo);
     nothing is normalised by the tensor's maximum;
  c. dw is written whole and only dw: a tail of 64 canary words behind it is untouched and no element keeps the fill pattern;
  d. a second call into a fresh buffer gives the same bits.
The bias-gradient and activation-gradient walks that feed the weight gradient (deepim_bias_grad, deepim_lrelu_bias_backward and its
channel-blocked form) run on exact operands at shapes with a short last slice, a ragged 128-pixel tile and hw % 4 != 0.
Each random test prints the largest ratio of its error to its bound (a figure, not an assertion)."""
import ctypes

import numpy as np
import pytest

import fp32_backward_cases as bc
from mx_deepim_amd.runtime import lib

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
f32, f64, u32 = np.float32, np.float64, np.uint32
FILL, CANARY, TAIL = 0x7FC0BEEF, 0x7FC5A5A5, 64          # two quiet NaNs no sum produces
rows = pytest.mark.parametrize("name", bc.NAMES)


def _plan(name):
    _, (B, cin, H, W, cout, k, s, p), lds, want = bc.BY_NAME[name]
    plan = (ctypes.c_int * 10)()
    assert lib.deepim_conv_wgrad_plan(lds, B, cin, H, W, cout, k, k, s, p, plan) == 0 and tuple(plan) == want


class _Out:
    """A device buffer of n floats pre-filled with FILL, and TAIL canary words behind it"""

    def __init__(self, ctx, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.dev = ctx.array(np.concatenate([np.full(self.n, FILL, u32), np.full(TAIL, CANARY, u32)]), u32)

    def get(self):
        raw = self.dev.asnumpy()
        assert np.all(raw[self.n:] == CANARY), "written past the end"
        assert not np.any(raw[:self.n] == FILL), ("elements never written", np.flatnonzero(raw[:self.n] == FILL)[:8].tolist())
        return raw[:self.n].view(f32).reshape(self.shape)


def _run(ctx, name, kind):
    """Every entry the row applies to, each twice into fresh buffers -> {entry: array}, after checking the two calls bit-equal.
    Keys: "nat", "bias" (dw of deepim_conv2d_wgrad_bias), "db", "tm", "nc8-1", "nc8-3"."""
    _, (B, cin, H, W, cout, k, s, p), lds, _ = bc.BY_NAME[name]
    _plan(name)
    x, dz = bc.operands(name, kind)
    h = ctx.handle
    xd, zd = ctx.array(x), ctx.array(dz)
    nat, tmj = (cout, cin, k, k), (cout, k * k, cin)
    geom = (B, cin, H, W, cout, k, k, s, p)
    out = {}

    def twice(key, shape, call):
        res = []
        for _ in range(2):
            o = _Out(ctx, shape)
            call(o.dev)
            res.append(o.get())
        assert np.array_equal(res[0].view(u32), res[1].view(u32)), key + ": two calls differ"
        out[key] = res[0]

    try:
        lib.deepim_set_option(h, b"wgrad_lds", lds)
        twice("nat", nat, lambda dw: lib.deepim_conv2d_wgrad(h, dw, xd, zd, *geom))
        dbs = []

        def with_bias(dw):
            db = _Out(ctx, (cout,))
            lib.deepim_conv2d_wgrad_bias(h, dw, db.dev, xd, zd, *geom)
            dbs.append(db.get())
        twice("bias", nat, with_bias)
        assert np.array_equal(dbs[0].view(u32), dbs[1].view(u32))
        out["db"] = dbs[0]
        modes = bc.variants(name)
        if modes:
            twice("tm", tmj, lambda dw: lib.deepim_conv2d_wgrad_tm(h, dw, xd, zd, *geom))
        for m in modes:
            x8 = ctx.array(bc.to_nc8(x) if m == 1 else bc.to_nc8_s2d(x))
            twice("nc8-%d" % m, tmj, lambda dw: lib.deepim_conv2d_wgrad_tm_nc8(h, dw, x8, m, zd, *geom))
    finally:
        lib.deepim_set_option(h, b"wgrad_lds", 1)
    return out


def _natural(key, a):
    """A tap-major (Cout, k*k, Cin) result back in the natural order"""
    if key in ("nat", "bias"):
        return a
    cout, kk, cin = a.shape
    k = int(round(kk ** 0.5))
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(cout, cin, k, k)


@rows
def test_exact_operands_give_the_int64_sums_bit_for_bit(ctx, name):
    got = _run(ctx, name, "exact")
    dw, db = bc.reference(name, "exact")
    want = dw.astype(f32)
    for key, a in got.items():
        if key == "db":
            np.testing.assert_array_equal(a.view(u32), db.astype(f32).view(u32), err_msg=key)
        elif key in ("nat", "bias"):
            np.testing.assert_array_equal(a.view(u32), want.view(u32), err_msg=key)
        else:
            np.testing.assert_array_equal(a.view(u32), bc.to_tap_major(want).view(u32), err_msg=key)
    assert set(got) == {"nat", "bias", "db"} | ({"tm"} | {"nc8-%d" % m for m in bc.variants(name)} if bc.variants(name) else set())


@rows
def test_random_operands_within_the_fp32_sum_bound_per_element(ctx, name):
    got = _run(ctx, name, "random")
    S, A, db, Ab = bc.reference(name, "random")
    bound = bc.wgrad_bound(name, A)
    worst = 0.0
    for key, a in got.items():
        if key == "db":
            err, lim = np.abs(a.astype(f64) - db), bc.bias_bound(name, Ab)
        else:
            err, lim = np.abs(_natural(key, a).astype(f64) - S), bound
        bad = ~(err <= lim)
        assert not bad.any(), (key, int(bad.sum()), np.argwhere(bad)[:8].tolist(), float((err / lim).max()))
        if key != "db":
            worst = max(worst, float((err / lim).max()))
    print("\n[wgrad_fp32 family %d %s] largest error / bound = %.4f" % (bc.BY_NAME[name][3][0], name, worst))
    # the layouts are one sum in other places: tap-major, channel-blocked and the bias entry agree with the natural one bit for bit
    for key, a in got.items():
        if key != "db":
            np.testing.assert_array_equal(_natural(key, a).view(u32), got["nat"].view(u32), err_msg=key)
    assert np.count_nonzero(got["nat"]) > 0.9 * got["nat"].size


# ---- the bias-gradient and activation-gradient walks ------------------------------------------------------------------------------
def _walk_entries(shape):
    """(entry, y_mode, with dz_nc8): the plain walk everywhere, the channel-blocked one where C % 8 == 0 (space-to-depth: even H, W)"""
    B, C, H, W = shape
    out = [("plain", 0, False)]
    if C % 8 == 0:
        out += [("nc8", m, z) for m in ((0, 1, 3) if H % 2 == 0 and W % 2 == 0 else (0, 1)) for z in (False, True)]
    return out


WALKS = [(shape, add, e) for shape in bc.WALK_SHAPES for add in (False, True) for e in _walk_entries(shape)]


def _walk(ctx, shape, with_add, entry, slope):
    """In place over dy, as the training graph runs it -> dz, db, dz_nc8 (or None)"""
    B, C, H, W = shape
    kind, y_mode, zout = entry
    dy, add, y = bc.walk_operands(shape, with_add)
    h = ctx.handle
    g = ctx.array(dy)
    addd = ctx.array(add) if with_add else None
    db = _Out(ctx, (C,))
    z8 = _Out(ctx, (B, C // 8, H, W, 8)) if zout else None
    if kind == "plain":
        lib.deepim_lrelu_bias_backward(h, g, db.dev, g, addd, ctx.array(y), cf(slope), B, C, H * W)
    else:
        yd = ctx.array(y if y_mode == 0 else bc.to_nc8(y) if y_mode == 1 else bc.to_nc8_s2d(y))
        lib.deepim_lrelu_bias_backward_nc8(h, g, z8.dev if zout else None, db.dev, g, addd, yd, y_mode, cf(slope), B, C, H, W)
    return g.asnumpy(), db.get(), (z8.get() if zout else None)


@pytest.mark.parametrize("shape,with_add,entry", WALKS, ids=["%dx%dx%dx%d-%s-%s%d%s" % (s + ("add" if a else "noadd", e[0], e[1], "-z8" if e[2] else ""))
                                                              for s, a, e in WALKS])
def test_activation_and_bias_gradient_walks_exact(ctx, shape, with_add, entry):
    dz, db, z8 = _walk(ctx, shape, with_add, entry, bc.SLOPE_EXACT)
    rz, rb = bc.walk_reference(shape, with_add, bc.SLOPE_EXACT)
    np.testing.assert_array_equal(dz.view(u32), rz.astype(f32).view(u32))
    np.testing.assert_array_equal(db.view(u32), rb.astype(f32).view(u32))
    if z8 is not None:
        np.testing.assert_array_equal(z8.view(u32), bc.to_nc8(rz.astype(f32)).view(u32))
    assert np.array_equal(rb, np.rint(rb * 2) / 2) and np.any(rz != np.rint(rz))          # halves occur: the slope side ran


@pytest.mark.parametrize("shape", bc.WALK_SHAPES)
def test_bias_grad_exact(ctx, shape):
    B, C, H, W = shape
    rz, rb = bc.walk_reference(shape, True, bc.SLOPE_EXACT)
    db = _Out(ctx, (C,))
    lib.deepim_bias_grad(ctx.handle, db.dev, ctx.array(rz.astype(f32)), B, C, H * W)
    np.testing.assert_array_equal(db.get().view(u32), rb.astype(f32).view(u32))


@pytest.mark.parametrize("entry", [("plain", 0, False), ("nc8", 3, True)])
def test_activation_gradient_walk_with_the_real_slope(ctx, entry):
    """Slope 0.1 as fp32: dz is the float64 product rounded once, db the exact sum of those values rounded once."""
    shape = bc.WALK_SHAPES[1]
    dz, db, z8 = _walk(ctx, shape, True, entry, bc.SLOPE_REAL)
    rz, rb = bc.walk_reference(shape, True, bc.SLOPE_REAL)
    np.testing.assert_array_equal(dz.view(u32), rz.astype(f32).view(u32))
    np.testing.assert_array_equal(db.view(u32), rb.astype(f32).view(u32))
    if z8 is not None:
        np.testing.assert_array_equal(z8.view(u32), bc.to_nc8(rz.astype(f32)).view(u32))
