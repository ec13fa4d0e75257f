"""The five kernels of csrc/decoder_f16.hip off the network's shapes (the rows of tests/fp16_decoder_cases.py, whose launch plans
tests/test_fp16_decoder_cases_host.py pins) against float64 references of the same fp16 operands, the whole output of every row:
  a. operands whose every partial sum is exact in fp32 under any slicing or order: the deconvolution's slice equals float16(lrelu(S)),
     the few-filter outputs equal float32(S), value for value;
  b. random operands without fp16 subnormals: every element within E = n·u·A / (1 − n·u) of the exact sum, E the a-priori bound of an
     fp32 sum of the element's own n terms (the deconvolution: between the fp16 roundings of lrelu(S) ∓ E, rounding being monotone);
  c. the record around the written slice keeps its sentinel, input channels [Cin_pad, in_ctotal) may hold NaN and [Cin, Cin_pad) any
     finite value, a second call gives the same bits, and sliced rows run after a sliced call that left large sums in the split-K
     scratch;
  d. upsample_flow within one fp16 ulp of the float64 result rounded once (equal on operands exact in fp32), the slice copy bit-exact;
  e. every argument check of the family refuses with nothing written, and an empty batch is a no-op.
Nothing here is measured: the only tolerances are E and the one ulp of upsample_flow."""
import ctypes

import numpy as np
import pytest

import fp16_decoder_cases as dc
from mx_deepim_amd.runtime import DeviceArray, lib

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
deconv_rows = pytest.mark.parametrize("row", dc.DECONV_ROWS, ids=dc.DECONV_IDS)
fewout_rows = pytest.mark.parametrize("row", dc.FEWOUT_ROWS, ids=dc.FEWOUT_IDS)
SENTINEL = 1234.0


def _h16(ctx, a):
    return ctx.array(np.ascontiguousarray(a, np.float16), dtype=np.float16)


def _nchw(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 3, 1, 2))


class _Deconv:
    """One deconvolution case with its operands packed and uploaded once: run(slope) -> the whole output record (B,Ho,Wo,out_ctotal)"""

    def __init__(self, ctx, case, x, w, b):
        B, cin, cpad, in_ct, H, W, cout = case[:7]
        self.ctx, self.case = ctx, case
        self.pk = DeviceArray(ctx, (lib.load().deepim_deconv_f16_packed_size(cpad, cout) // 2,), dtype=np.float16)
        lib.deepim_deconv_f16_pack_weights(ctx.handle, self.pk, ctx.array(w), cin, cpad, cout)
        self.x, self.b = _h16(ctx, dc.nhwc_record(x, cpad, in_ct)), ctx.array(b)

    def run(self, slope):
        B, _, cpad, in_ct, H, W, cout, Ho, Wo, out_ct, coff = self.case
        out = _h16(self.ctx, np.full((B, Ho, Wo, out_ct), SENTINEL, np.float16))
        lib.deepim_deconv4x4s2_crop_f16_forward(self.ctx.handle, out, self.x, self.pk, self.b, B, cpad, in_ct, H, W, cout, Ho, Wo,
                                                cf(slope), out_ct, coff)
        return out.asnumpy()


def _split_record(case, rec):
    """-> the written slice as NCHW float32; asserts the sentinel everywhere else"""
    cout, out_ct, coff = case[6], case[9], case[10]
    outside = np.ones(out_ct, bool)
    outside[coff:coff + cout] = False
    assert (rec[..., outside].view(np.uint16) == np.float16(SENTINEL).view(np.uint16)).all(), "written outside the channel slice"
    return _nchw(rec[..., coff:coff + cout])


def _check_plan_and_dirty_scratch(ctx, rid, case, plan):
    """The library's plan is the pinned one; before a sliced row, a sliced call of another pixel layout leaves sums of about 1e6 in
    all of the split-K scratch the row will use, so a slice entry that is read but never written shows in the output."""
    B, _, cpad, _, H, W, cout, Ho, Wo = case[:9]
    got = (ctypes.c_int * 8)()
    lib.deepim_deconv_f16_plan(B, cpad, H, W, cout, Ho, Wo, got)
    assert tuple(got) == plan
    if plan[6] > 1:
        dirty = dc.dirty_case(rid)
        rec = _Deconv(ctx, dirty, *dc.dirty_operands(dirty)).run(1.0)
        assert np.isinf(rec[0, 2, 2, dirty[10]])      # 1000 · 16 · Cin overflows fp16: the stale sums are that large


@deconv_rows
def test_deconv_exact_sums_value_for_value(ctx, row):
    rid, case, plan = row
    x, w, b = dc.deconv_operands(dc._geometry(case), "exact")
    S, _ = dc.deconv_reference(case, "exact", with_A=False)
    _check_plan_and_dirty_scratch(ctx, rid, case, plan)
    layer = _Deconv(ctx, case, x, w, b)
    rec = layer.run(dc.SLOPE_EXACT)
    np.testing.assert_array_equal(_split_record(case, rec), dc.f16(dc.lrelu(S, dc.SLOPE_EXACT)), err_msg=rid)
    np.testing.assert_array_equal(layer.run(dc.SLOPE_EXACT).view(np.uint16), rec.view(np.uint16), err_msg=rid + ": second call")


@deconv_rows
def test_deconv_random_operands_within_the_fp32_sum_bound(ctx, row):
    rid, case, plan = row
    x, w, b = dc.deconv_operands(dc._geometry(case), "random")
    S, A = dc.deconv_reference(case, "random")
    _check_plan_and_dirty_scratch(ctx, rid, case, plan)
    layer = _Deconv(ctx, case, x, w, b)
    rec = layer.run(0.1)
    got = _split_record(case, rec)
    y, E = dc.lrelu(S, dc.SLOPE_RANDOM), dc.deconv_bound(case, plan, A)
    lo, hi = dc.f16(y - E), dc.f16(y + E)
    bad = (got < lo) | (got > hi) | ~np.isfinite(got)
    print("%s: %d of %d outside the bound, %.3f %% differ from float16(lrelu(S))" % (rid, bad.sum(), bad.size,
                                                                                    100 * np.mean(got != dc.f16(y))))
    assert not bad.any(), (rid, int(bad.sum()), np.argwhere(bad)[:8].tolist())
    np.testing.assert_array_equal(layer.run(0.1).view(np.uint16), rec.view(np.uint16), err_msg=rid + ": second call")


class _Fewout:
    """One few-filter case: run() -> (out0, out1 or None) as float32 NCHW; the outputs start as NaN"""

    def __init__(self, ctx, case, split, x, w, b):
        B, cin, cpad, in_ct, H, W = case
        n0, n1 = split
        self.ctx, self.case, self.split = ctx, case, split
        self.pk = DeviceArray(ctx, (lib.load().deepim_fewout_f16_packed_size(cpad) // 2,), dtype=np.float16)
        w0, w1 = ctx.array(w[:n0]), (ctx.array(w[n0:]) if n1 else None)
        lib.deepim_fewout_f16_pack_weights(ctx.handle, self.pk, w0, n0, w1, n1, cin, cpad)
        self.x = _h16(ctx, dc.nhwc_record(x, cpad, in_ct))
        self.b0, self.b1 = ctx.array(b[:n0]), (ctx.array(b[n0:]) if n1 else None)

    def run(self):
        B, _, cpad, in_ct, H, W = self.case
        n0, n1 = self.split
        o0 = self.ctx.array(np.full((B, n0, H, W), np.nan, np.float32))
        o1 = self.ctx.array(np.full((B, n1, H, W), np.nan, np.float32)) if n1 else None
        lib.deepim_conv3x3_fewout_f16_forward(self.ctx.handle, o0, n0, o1, n1, self.x, self.pk, self.b0, self.b1, B, H, W, in_ct, cpad)
        return np.concatenate([o0.asnumpy()] + ([o1.asnumpy()] if n1 else []), axis=1)


def _check_fewout_plan(case, plan):
    B, _, cpad, _, H, W = case
    got = (ctypes.c_int * 4)()
    lib.deepim_fewout_f16_plan(B, H, W, cpad, got)
    assert tuple(got) == plan


@fewout_rows
def test_fewout_exact_sums_value_for_value(ctx, row):
    rid, case, split, plan = row
    x, w, b = dc.fewout_operands(case, sum(split), "exact")
    S, A = dc.fewout_reference(x, w, b)
    assert A.max() < 2 ** 15
    _check_fewout_plan(case, plan)
    layer = _Fewout(ctx, case, split, x, w, b)
    got = layer.run()
    np.testing.assert_array_equal(got, S.astype(np.float32), err_msg=rid)
    np.testing.assert_array_equal(layer.run().view(np.uint32), got.view(np.uint32), err_msg=rid + ": second call")


@fewout_rows
def test_fewout_random_operands_within_the_fp32_sum_bound(ctx, row):
    rid, case, split, plan = row
    x, w, b = dc.fewout_operands(case, sum(split), "random")
    S, A = dc.fewout_reference(x, w, b)
    _check_fewout_plan(case, plan)
    layer = _Fewout(ctx, case, split, x, w, b)
    got = layer.run()
    E = dc.fewout_bound(case, plan, A)
    bad = ~(np.abs(got.astype(np.float64) - S) <= E)
    print("%s: %d of %d outside the bound, worst error %.3g of its bound" % (rid, bad.sum(), bad.size,
                                                                            np.nanmax(np.abs(got - S) / E)))
    assert not bad.any(), (rid, int(bad.sum()), np.argwhere(bad)[:8].tolist())
    np.testing.assert_array_equal(layer.run().view(np.uint32), got.view(np.uint32), err_msg=rid + ": second call")


@pytest.mark.parametrize("row", dc.UPSAMPLE_ROWS, ids=[str(r) for r in dc.UPSAMPLE_ROWS])
@pytest.mark.parametrize("kind", ["grid", "random"])
def test_upsample_flow_rounds_the_float64_result_once(ctx, row, kind):
    B, H, W, Ho, Wo, out_ct, coff = row
    flow, w, b = dc.upsample_operands(row, kind)
    S, A = dc.upsample_reference(row, flow, w, b)
    sentinel = np.full((B, Ho, Wo, out_ct), -77.0, np.float16)
    out = _h16(ctx, sentinel)
    lib.deepim_upsample_flow_f16_forward(ctx.handle, out, ctx.array(flow), ctx.array(w), ctx.array(b), B, H, W, Ho, Wo, out_ct, coff)
    rec = out.asnumpy()
    got, want = _nchw(rec[..., coff:coff + 2]), dc.f16(S)
    assert kind == "grid" or dc.upsample_margin(S, A).all()
    bad = ~(np.abs(got - want) <= dc.ulp16(want))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist())
    if kind == "grid":       # products and sums exact in fp32: one rounding of the exact value
        np.testing.assert_array_equal(got, want)
    outside = np.ones(out_ct, bool)
    outside[coff:coff + 2] = False
    np.testing.assert_array_equal(rec[..., outside].view(np.uint16), sentinel[..., outside].view(np.uint16))


@pytest.mark.parametrize("row", dc.COPY_ROWS, ids=[str(r) for r in dc.COPY_ROWS])
def test_slice_copy_is_bit_exact_and_touches_nothing_else(ctx, row):
    npix, C, src_ct, src_coff, dst_ct, dst_coff = row
    rng = np.random.default_rng(npix)
    src = rng.integers(0, 1 << 16, (npix, src_ct), dtype=np.uint16)       # every bit pattern, NaNs included
    before = rng.integers(0, 1 << 16, (npix, dst_ct), dtype=np.uint16)
    dst = _h16(ctx, before.view(np.float16))
    lib.deepim_copy_channels_nhwc_f16(ctx.handle, dst, dst_ct, dst_coff, _h16(ctx, src.view(np.float16)), src_ct, src_coff, C, npix)
    want = before.copy()
    want[:, dst_coff:dst_coff + C] = src[:, src_coff:src_coff + C]
    np.testing.assert_array_equal(dst.asnumpy().view(np.uint16), want)


# ---- refusals: RuntimeError, nothing written
def _refused(call, *outs):
    before = [o.asnumpy().tobytes() for o in outs]
    with pytest.raises(RuntimeError):
        call()
    for o, was in zip(outs, before):
        assert o.asnumpy().tobytes() == was


GOOD_DECONV = dict(B=1, Cin_pad=8, in_ctotal=8, H=2, W=2, Cout=64, Ho=3, Wo=3, out_ctotal=72, out_coff=4)
BAD_DECONV = {"Cout = 96": dict(Cout=96, out_ctotal=104), "Cin_pad = 12": dict(Cin_pad=12, in_ctotal=16),
              "in_ctotal < Cin_pad": dict(Cin_pad=16, in_ctotal=8), "slice past the record": dict(out_coff=12),
              "out_coff = 2": dict(out_coff=2), "Ho = 2H + 1": dict(Ho=5), "Wo = 2W + 1": dict(Wo=5), "Ho = 0": dict(Ho=0),
              "2^31 input halves": dict(H=1024, W=1024, in_ctotal=2048, Ho=1, Wo=1)}


@pytest.mark.parametrize("what", list(BAD_DECONV))
def test_deconv_refuses(ctx, what):
    a = dict(GOOD_DECONV, **BAD_DECONV[what])
    assert what != "2^31 input halves" or a["B"] * a["H"] * a["W"] * a["in_ctotal"] == 2 ** 31
    out = _h16(ctx, np.full(4096, SENTINEL))          # small dummy buffers: every check precedes any launch
    x, pk, b = _h16(ctx, np.ones(4096)), _h16(ctx, np.ones(4 * 128 * 4 * 16)), ctx.array(np.ones(128))
    _refused(lambda: lib.deepim_deconv4x4s2_crop_f16_forward(
        ctx.handle, out, x, pk, b, a["B"], a["Cin_pad"], a["in_ctotal"], a["H"], a["W"], a["Cout"], a["Ho"], a["Wo"], cf(0.1),
        a["out_ctotal"], a["out_coff"]), out)


GOOD_FEWOUT = dict(n0=1, n1=1, out1=True, B=1, H=2, W=2, in_ctotal=8, Cin_pad=8)
BAD_FEWOUT = {"n0 = 0": dict(n0=0), "n0 + n1 = 4": dict(n0=2, n1=2), "n1 > 0 with out1 = NULL": dict(out1=False),
              "Cin_pad = 2056": dict(Cin_pad=2056, in_ctotal=2056), "Cin_pad > in_ctotal": dict(Cin_pad=16), "H = 0": dict(H=0),
              "W = 0": dict(W=0), "Cin_pad = 0": dict(Cin_pad=0)}


@pytest.mark.parametrize("what", list(BAD_FEWOUT))
def test_fewout_refuses(ctx, what):
    a = dict(GOOD_FEWOUT, **BAD_FEWOUT[what])
    o0, o1 = ctx.array(np.full(64, SENTINEL, np.float32)), ctx.array(np.full(64, SENTINEL, np.float32))
    x, pk, b = _h16(ctx, np.ones(4096)), _h16(ctx, np.ones(257 * 9 * 3 * 8)), ctx.array(np.ones(4))
    _refused(lambda: lib.deepim_conv3x3_fewout_f16_forward(ctx.handle, o0, a["n0"], o1 if a["out1"] else None, a["n1"], x, pk, b, b,
                                                           a["B"], a["H"], a["W"], a["in_ctotal"], a["Cin_pad"]), o0, o1)


def test_fewout_packer_refuses(ctx):
    pk, w = _h16(ctx, np.full(4096, SENTINEL)), ctx.array(np.ones(4096))
    for n0, n1, w1, cin, cpad in ((1, 0, None, 0, 0), (0, 1, w, 8, 8), (2, 2, w, 8, 8), (1, 1, None, 8, 8), (1, 0, None, 8, 12),
                                  (1, 0, None, 16, 8), (1, 0, None, 8, 2056)):
        _refused(lambda: lib.deepim_fewout_f16_pack_weights(ctx.handle, pk, w, n0, w1, n1, cin, cpad), pk)


def test_upsample_flow_and_slice_copy_refuse(ctx):
    out = _h16(ctx, np.full(4096, SENTINEL))
    flow, w, b = ctx.array(np.ones(64)), ctx.array(np.ones(64)), ctx.array(np.ones(2))
    for B, H, W, Ho, Wo, out_ct, coff in ((1, 2, 2, 3, 3, 8, 3), (1, 2, 2, 5, 3, 8, 2), (1, 2, 2, 3, 5, 8, 2), (1, 2, 2, 3, 3, 8, 8)):
        _refused(lambda: lib.deepim_upsample_flow_f16_forward(ctx.handle, out, flow, w, b, B, H, W, Ho, Wo, out_ct, coff), out)
    src = _h16(ctx, np.ones(4096))
    for dst_ct, dst_coff, src_ct, src_coff, C in ((8, 0, 8, 0, 4), (16, 8, 16, 0, 16), (16, 0, 16, 8, 16), (16, 4, 16, 0, 8)):
        _refused(lambda: lib.deepim_copy_channels_nhwc_f16(ctx.handle, out, dst_ct, dst_coff, src, src_ct, src_coff, C, 4), out)


def test_an_empty_batch_is_a_no_op(ctx):
    out, o32 = _h16(ctx, np.full(4096, SENTINEL)), ctx.array(np.full(64, SENTINEL, np.float32))
    x, f32 = _h16(ctx, np.ones(4096)), ctx.array(np.ones(4096))
    before, before32 = out.asnumpy().tobytes(), o32.asnumpy().tobytes()
    h = ctx.handle
    lib.deepim_deconv4x4s2_crop_f16_forward(h, out, x, x, f32, 0, 8, 8, 2, 2, 64, 3, 3, cf(0.1), 72, 4)
    lib.deepim_conv3x3_fewout_f16_forward(h, o32, 1, o32, 1, x, x, f32, f32, 0, 2, 2, 8, 8)
    lib.deepim_upsample_flow_f16_forward(h, out, f32, f32, f32, 0, 2, 2, 3, 3, 8, 2)
    lib.deepim_copy_channels_nhwc_f16(h, out, 16, 8, x, 8, 0, 8, 0)
    ctx.sync()
    assert out.asnumpy().tobytes() == before and o32.asnumpy().tobytes() == before32
