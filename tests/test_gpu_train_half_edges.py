"""The half-precision encoder backward (csrc/train_half.hip: weight gradient, data gradient, fused activation and bias gradient, in
the fp16 and the split-fp16 "x3" mode) at its edge shapes — the rows of tests/train_half_cases.py, which tests/test_train_half_cases_host.py
pins to the branches they reach — against float64 references of the same stored operands, element by element over the whole tensor:
  a. operands whose every partial sum is exact in fp32 (x3: with non-zero lo halves, reference = the three products the kernels keep):
     the weight gradient equals the reference bit for bit in both layouts; the data gradient, written over a dx pre-filled with 7,
     equals the reference rounded once to the output format; dz of the activation gradient equals its numpy definition and db the
     exact sum; the overflow word stays 0;
  b. random operands: |got − S| <= n·u·A / (1 − n·u) per element (u = 2^-24, n = the summed terms + the slices the plan query reports
     + 2; S the float64 sum, A the sum of the magnitudes), plus what the format costs: train_half_cases.wgrad_bound / dgrad_bound derive
     each term. Nothing is normalised by the tensor's maximum. A second call gives the same bits;
  c. the data gradient stays inside the workspace its size query reports: canary halves behind it are untouched.
Each random test prints the largest ratio of its error to its bound (a figure, not an assertion)."""
import ctypes

import numpy as np
import pytest

import train_half_cases as tc
from mx_deepim_amd.runtime import lib

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
f16, f32, f64 = np.float16, np.float32, np.float64
CANARY = np.arange(1, 257).astype(f16)
wg_cases = pytest.mark.parametrize("rid,mode", tc.WG_CASES, ids=["%s-%s" % c for c in tc.WG_CASES])
dg_cases = pytest.mark.parametrize("rid,mode,ch", tc.DG_CASES, ids=["%s-%s-%dx%d" % ((r, m) + c) for r, m, c in tc.DG_CASES])
lrelu_cases = pytest.mark.parametrize("shape,mode,src", tc.LRELU_CASES, ids=["%s-%s-%dx%dx%dx%d" % ((m, s) + sh) for sh, m, s in tc.LRELU_CASES])


def _state(ctx, scale):
    """A fresh scale state {scale, 1 / scale, 0, 0}; the context's saturation bit is cleared first, into a state nobody reads"""
    st = np.zeros(4, np.uint32)
    st[:2] = np.array([scale, 1.0 / scale], f32).view(np.uint32)
    sink = ctx.array(st, np.uint32)
    lib.deepim_x3_status_to_state(ctx.handle, sink)
    sink.asnumpy()
    return ctx.array(st, np.uint32)


def _wgrad(ctx, rid, mode, kind):
    """-> natural (Cout,Cin,k,k), tap-major (Cout,k*k,Cin), the natural one of a second call, the overflow word"""
    _, _, case, want = tc.WG_BY_ID[rid]
    B, cin, cpad, H, W, cout, k, s, p = case
    plan = (ctypes.c_int * 6)()
    assert lib.deepim_conv_wgrad_half_plan(int(mode == "x3"), B, cpad, H, W, cout, k, s, p, plan) == 0 and tuple(plan) == want
    (xh, xl), (zh, zl) = tc.wgrad_operands(rid, mode, kind)
    h, st = ctx.handle, _state(ctx, tc.WG_SCALE[mode])
    xd, zd = ctx.array(tc.store(mode, xh, xl, cpad), f16), ctx.array(tc.store(mode, zh, zl), f16)
    out = []
    for layout, shape in ((0, (cout, cin, k, k)), (1, (cout, k * k, cin)), (0, (cout, cin, k, k))):
        dw = ctx.array(np.full(shape, 7.0, f32))          # every element is written
        if mode == "x3":
            assert lib.deepim_conv2d_wgrad_x3(h, dw, xd, zd, st, B, cin, H, W, cout, k, s, p, layout, cf(tc.ACT)) == 0
        else:
            assert lib.deepim_conv2d_wgrad_f16(h, dw, xd, zd, st, B, cin, cpad, H, W, cout, k, s, p, layout) == 0
        out.append(dw.asnumpy())
    return out + [int(st.asnumpy()[2])]


@wg_cases
def test_wgrad_exact_sums_bit_for_bit_in_both_layouts(ctx, rid, mode):
    nat, tm, again, flag = _wgrad(ctx, rid, mode, "exact")
    ref = tc.wgrad_reference(rid, mode, "exact").astype(f32)
    np.testing.assert_array_equal(nat, ref)
    np.testing.assert_array_equal(tm, ref.reshape(ref.shape[0], ref.shape[1], -1).transpose(0, 2, 1))
    np.testing.assert_array_equal(again, nat)
    assert flag == 0


@wg_cases
def test_wgrad_random_operands_within_the_fp32_sum_bound_per_element(ctx, rid, mode):
    nat, tm, again, flag = _wgrad(ctx, rid, mode, "random")
    S, A = tc.wgrad_reference(rid, mode, "random")
    bound = tc.wgrad_bound(rid, mode, tc.WG_BY_ID[rid][3], A)
    err = np.abs(nat.astype(f64) - S)
    print("\n[wgrad_%s %s] largest error / bound = %.3f" % (mode, rid, float((err / bound).max())))
    bad = ~(err <= bound)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist())
    np.testing.assert_array_equal(tm, nat.reshape(nat.shape[0], nat.shape[1], -1).transpose(0, 2, 1))
    np.testing.assert_array_equal(again, nat)          # fixed slices, sums in a fixed order
    assert flag == 0 and np.count_nonzero(nat) > 0.9 * nat.size


def _conv_slices(mode, rid, ch):
    """The K slices (uniform split-K or tail split) of each forward convolution the data gradient runs, from the plan query"""
    B, Hd, Wd, k, s, p = tc.DG_BY_ID[rid]
    ho, wo = tc.out_hw(Hd, Wd, k, s, p)
    out = []
    for _, _, nky, nkx, P in tc.dgrad_convs(rid):
        plan = (ctypes.c_int * 8)()
        assert lib.deepim_conv_f16_plan(None, int(mode == "x3"), B, ch[1], ho, wo, ch[0], nky, nkx, 1, P, plan) == 0
        out.append(max(plan[5], plan[6], 1))
    return out


def _dgrad(ctx, rid, mode, ch, kind):
    """-> dx as NCHW (hi, lo), the stored halves of a second call's dx and of this one's, the overflow word"""
    B, Hd, Wd, k, s, p = tc.DG_BY_ID[rid]
    ci, co = ch
    w, sw, _, (zh, zl) = tc.dgrad_operands(rid, mode, ch, kind)
    h, L = ctx.handle, lib.load()
    size = L.deepim_conv_dgrad_x3_workspace_size if mode == "x3" else L.deepim_conv_dgrad_f16_workspace_size
    nb = size(B, ci, Hd, Wd, co, k, s, p)
    half = (nb + 1) // 2
    assert nb > 0
    wd, zd = ctx.array(w), ctx.array(tc.store(mode, zh, zl), f16)
    raw = []
    for _ in range(2):
        st = _state(ctx, 1.0)
        ws = ctx.array(np.concatenate([np.zeros(half, f16), CANARY]), f16)          # the canary lies inside the allocation
        dx = ctx.array(np.full((B, Hd, Wd, (2 if mode == "x3" else 1) * ci), 7.0), f16)
        if mode == "x3":
            assert lib.deepim_conv2d_dgrad_x3(h, dx, zd, wd, ws, st, B, ci, Hd, Wd, co, k, s, p, cf(sw)) == 0
        else:
            assert lib.deepim_conv2d_dgrad_f16(h, dx, zd, wd, ws, B, ci, Hd, Wd, co, k, s, p) == 0
        raw.append(dx.asnumpy())
        np.testing.assert_array_equal(ws.asnumpy()[half:], CANARY)
        flag = int(st.asnumpy()[2])
    return tc.load(mode, raw[0]), raw[1].view(np.uint16), raw[0].view(np.uint16), flag


@dg_cases
def test_dgrad_exact_sums_rounded_once_to_the_output_format(ctx, rid, mode, ch):
    (hi, lo), again, first, flag = _dgrad(ctx, rid, mode, ch, "exact")
    ref = tc.dgrad_reference(rid, mode, ch, "exact")
    rh, rl = tc.round_to_output(mode, ref)
    np.testing.assert_array_equal(hi, rh)          # (a 7.0 left over from the fill fails here: every element is written)
    np.testing.assert_array_equal(lo, rl)
    unreached = ~tc.dgrad_reached(rid, ch)
    assert not np.any(hi[:, :, unreached]) and not np.any(lo[:, :, unreached])
    np.testing.assert_array_equal(again, first)
    assert flag == 0


@dg_cases
def test_dgrad_random_operands_within_the_derived_bound_per_element(ctx, rid, mode, ch):
    (hi, lo), again, first, flag = _dgrad(ctx, rid, mode, ch, "random")
    S, A = tc.dgrad_reference(rid, mode, ch, "random")
    bound = tc.dgrad_bound(rid, mode, ch, _conv_slices(mode, rid, ch), S, A)
    err = np.abs(hi + lo - S)
    print("\n[dgrad_%s %s %s] largest error / bound = %.3f" % (mode, rid, ch, float((err / bound).max())))
    bad = ~(err <= bound)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist())
    np.testing.assert_array_equal(again, first)
    assert flag == 0 and np.count_nonzero(hi) > 0.9 * hi.size


def _lrelu(ctx, shape, mode, src, kind):
    """In place over d, as the training graph runs it -> dz as NCHW (hi, lo), db, the overflow word"""
    B, C, H, W = shape
    y, d, add, slope = tc.lrelu_operands(shape, mode, src, kind)
    h, st = ctx.handle, _state(ctx, tc.LRELU_SCALE)
    yd = ctx.array(tc.store(mode, *y), f16)
    dd = ctx.array(tc.store(mode, *d), f16) if d is not None else None
    dz = dd if dd is not None else ctx.array(np.full((B, H, W, (2 if mode == "x3" else 1) * C), 7.0), f16)
    db = ctx.array(np.full((C,), 7.0, f32))
    fn = lib.deepim_lrelu_bias_backward_x3 if mode == "x3" else lib.deepim_lrelu_bias_backward_f16
    assert fn(h, dz, db, dd, ctx.array(add) if add is not None else None, yd, st, cf(slope), B, C, H, W) == 0
    return tc.load(mode, dz.asnumpy()), db.asnumpy(), int(st.asnumpy()[2])


@lrelu_cases
def test_lrelu_bias_backward_exact_operands(ctx, shape, mode, src):
    (hi, lo), db, flag = _lrelu(ctx, shape, mode, src, "exact")
    (rh, rl), db_ref, _ = tc.lrelu_reference(shape, mode, src, "exact")
    np.testing.assert_array_equal(hi, rh)
    np.testing.assert_array_equal(lo, rl)
    np.testing.assert_array_equal(db, db_ref.astype(f32))          # exact sums: the existing form's 1e-5 of the maximum, and every bit
    assert np.abs(db - db_ref).max() / max(1e-30, np.abs(db_ref).max()) < 1e-5
    assert flag == 0


@lrelu_cases
def test_lrelu_bias_backward_random_operands(ctx, shape, mode, src):
    """dz is its numpy definition bit for bit; db is an fp32 sum of a channel's B·H·W values of dz in some order, then one multiply by
    1 / S: n = B·H·W + 2."""
    (hi, lo), db, flag = _lrelu(ctx, shape, mode, src, "random")
    (rh, rl), db_ref, mag = tc.lrelu_reference(shape, mode, src, "random")
    np.testing.assert_array_equal(hi, rh)
    np.testing.assert_array_equal(lo, rl)
    bound = tc.sum_bound(shape[0] * shape[2] * shape[3] + 2, mag)
    err = np.abs(db.astype(f64) - db_ref)
    print("\n[lrelu_%s %s %s] largest error / bound = %.3f" % (mode, src, shape, float((err / bound).max())))
    assert np.all(err <= bound)
    assert np.abs(db - db_ref).max() / max(1e-30, np.abs(db_ref).max()) < 1e-5
    assert flag == 0
