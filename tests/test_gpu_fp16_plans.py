"""Every launch plan of deepim_conv2d_f16_forward (kernel x tile x K slicing; the rows of tests/fp16_plan_cases.py, pinned on the host by
tests/test_fp16_plan_host.py) against a float64 convolution of the same fp16 operands — the WHOLE output tensor of every row (the
largest reference, 10 GMAC, takes about a second on the CPU), element by element:
  a. operands whose partial sums are exact in fp32 under any order: the output equals float16(lrelu(S)) bit for bit, with the layer's
     bias and slope and — on sliced plans — with no bias and slope 1, the form the data gradient calls;
  b. random operands: every element lies between the fp16 roundings of lrelu(S ∓ e), e the a-priori bound of an fp32 sum of the
     element's own terms in any order (no scaling by the tensor's maximum), and fewer than 2 % of elements differ from float16(lrelu(S));
  c. sliced plans (split-K, tail split) give the same bits on every run: the partial tiles are reduced in a fixed order.
The frame's bottom row and right column (padding taps) lie inside the tail tiles of every tail-split row, and the reference is
non-zero there."""
import contextlib
import ctypes

import numpy as np
import pytest

import fp16_plan_cases as pc
from mx_deepim_amd.runtime import DeviceArray, lib

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
rows = pytest.mark.parametrize("row", pc.ROWS, ids=pc.ROW_IDS)
sliced_rows = pytest.mark.parametrize("row", [r for r in pc.ROWS if pc.sliced(r[3])], ids=[r[0] for r in pc.ROWS if pc.sliced(r[3])])


@contextlib.contextmanager
def _options(ctx, row):
    """The row's context options, and the plan the library reports under them: the one the row is there for."""
    _, case, opts, want = row
    try:
        for name, value in opts.items():
            lib.deepim_set_option(ctx.handle, name.encode(), value)
        B, _, H, W, cout, k, s, p = case
        plan = (ctypes.c_int * 8)()
        lib.deepim_conv_f16_plan(ctx.handle, 0, B, pc.cin_pad(case), H, W, cout, k, k, s, p, plan)
        assert tuple(plan) == want
        yield
    finally:
        lib.deepim_set_option(ctx.handle, b"f16_dev_flags", 0)
        lib.deepim_set_option(ctx.handle, b"conv_max_split", 0)


class _Layer:
    """_conv_f16 of tests/test_gpu_fp16.py with the operands converted and packed once: run(bias or None, slope) -> NCHW float32"""

    def __init__(self, ctx, case, x, w):
        B, cin, H, W, cout, k, _, _ = case
        self.ctx, self.case, self.cpad = ctx, case, pc.cin_pad(case)
        self.xh = ctx.empty((B, H, W, self.cpad), dtype=np.float16)
        lib.deepim_nchw_f32_to_nhwc_f16(ctx.handle, self.xh, ctx.array(x), B, cin, H, W, self.cpad)
        self.pk = DeviceArray(ctx, (lib.load().deepim_conv_f16_packed_size(cout, self.cpad, k, k) // 2,), dtype=np.float16)
        lib.deepim_conv_f16_pack_weights(ctx.handle, self.pk, ctx.array(w), cout, cin, self.cpad, k, k)

    def run(self, b, slope):
        B, _, H, W, cout, k, s, p = self.case
        ctx, (ho, wo) = self.ctx, pc.out_hw(self.case)
        oh = ctx.empty((B, ho, wo, cout), dtype=np.float16)
        lib.deepim_conv2d_f16_forward(ctx.handle, oh, self.xh, self.pk, None if b is None else ctx.array(b), B, self.cpad, H, W, cout,
                                      k, k, s, p, cf(slope))
        out = ctx.empty((B, cout, ho, wo))
        lib.deepim_nhwc_f16_to_nchw_f32(ctx.handle, out, oh, B, cout, ho, wo)
        return out.asnumpy()


def _assert_borders_inside_tail_tiles(case, plan, ref):
    """The tail tiles hold the last pixels of the last sample: its bottom row and the end of its right column, where the window
    hangs over the frame. The reference has values there, so a tail slice that mistreats a padding tap shows."""
    if plan[6] <= 1:
        return
    pix0, co0 = pc.tail_region(case, plan)
    ho, wo = pc.out_hw(case)
    first = pix0 - (case[0] - 1) * ho * wo            # first tail pixel within the last sample
    assert case[7] > 0 and 0 <= first <= (ho - 2) * wo, (first, ho, wo)   # the bottom row and a right-column pixel above it
    tail = ref[-1, co0:].reshape(ref.shape[1] - co0, ho * wo)[:, max(first, 0):]
    bottom = ref[-1, co0:, ho - 1, :]
    right = ref[-1, co0:, -(-first // wo):, wo - 1]
    assert tail.shape[1] == plan[7] * plan[2] - (-pc.npix(case) % plan[2])
    assert right.shape[1] >= 2 and np.count_nonzero(bottom) > 0.9 * bottom.size and np.count_nonzero(right) > 0.9 * right.size


@rows
def test_exact_sums_bit_for_bit(ctx, row):
    rid, case, _, plan = row
    x, w, b = pc.exact_operands(case, pc.ROW_IDS.index(rid))
    S0 = pc.conv64(x, w, case[6], case[7])
    assert np.abs(S0).max() + 8 < 2 ** 15
    forms = [(b, pc.SLOPE_EXACT)] + ([(None, 1.0)] if pc.sliced(plan) else [])
    with _options(ctx, row):
        layer = _Layer(ctx, case, x, w)
        got = [layer.run(b_, slope) for b_, slope in forms]
    for (b_, slope), g in zip(forms, got):
        ref = pc.lrelu16(S0 if b_ is None else S0 + b_.astype(np.float64)[None, :, None, None], slope)
        _assert_borders_inside_tail_tiles(case, plan, ref)
        np.testing.assert_array_equal(g, ref, err_msg="%s bias %s slope %g" % (rid, b_ is not None, slope))


@rows
def test_random_operands_within_the_fp32_sum_bound_per_element(ctx, row):
    rid, case, _, plan = row
    x, w, b = pc.random_operands(case, 100 + pc.ROW_IDS.index(rid))
    with _options(ctx, row):
        got = _Layer(ctx, case, x, w).run(b, 0.1)
    S, A = pc.random_reference(case, x, w, b)
    e = pc.fp32_sum_bound(case, plan, A)
    lo, hi, ref = pc.lrelu16(S - e, pc.SLOPE_RANDOM), pc.lrelu16(S + e, pc.SLOPE_RANDOM), pc.lrelu16(S, pc.SLOPE_RANDOM)
    _assert_borders_inside_tail_tiles(case, plan, ref)
    bad = (got < lo) | (got > hi) | ~np.isfinite(got)
    differ = float(np.mean(got != ref))
    print("%s: %d of %d outside the bound, %.3f %% differ from the float64 rounding" % (rid, bad.sum(), bad.size, 100 * differ))
    assert not bad.any(), (rid, int(bad.sum()), np.argwhere(bad)[:8].tolist())
    assert differ < 0.02


@sliced_rows
def test_sliced_plans_are_deterministic(ctx, row):
    rid, case, _, plan = row
    x, w, b = pc.random_operands(case, 200 + pc.ROW_IDS.index(rid))
    with _options(ctx, row):
        layer = _Layer(ctx, case, x, w)
        first, again = layer.run(b, 0.1), [layer.run(b, 0.1) for _ in range(2)]
    assert np.isfinite(first).all() and first.any()
    for g in again:
        np.testing.assert_array_equal(g, first)
