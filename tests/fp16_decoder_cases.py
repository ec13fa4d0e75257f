"""The shapes at which tests/test_gpu_fp16_decoder_edges.py runs the five kernels of csrc/decoder_f16.hip off the network's geometry,
the launch plans tests/test_fp16_decoder_cases_host.py pins for them, and the float64 references, operands and bounds both share.

Deconvolution row: id, (B, Cin, Cin_pad, in_ctotal, H, W, Cout, Ho, Wo, out_ctotal, out_coff), and the eight ints
deepim_deconv_f16_plan reports: block tiles of all classes, pixels of parity class 0..3, k-steps, ksplit, k-steps per slice.
Few-filter row: id, (B, Cin, Cin_pad, in_ctotal, H, W), (n0, n1), and the four ints of deepim_fewout_f16_plan: threads, seg, nseg, waves.

References are float64 on the CPU (torch) of the fp16-rounded operands; each comes with A, the same operation on the absolute values
plus |bias|, which bounds every partial sum in any order. An fp32 sum of n terms in any order is within n·u·A / (1 − n·u) of the
exact one (u = 2^-24): fp32_sum_bound, with n = the K terms (products exact) + the slices' or waves' adds + the bias add and the
slope multiply."""
import functools

import numpy as np

DECONV_ROWS = [
    # one octet per tap (oc += 2 wraps twice per step), three empty classes, one M block whose wm = 1 waves idle
    ("one-pixel", (1, 5, 8, 8, 1, 1, 64, 1, 1, 64, 0), (1, 1, 0, 0, 0, 2, 1, 2)),
    # one octet per tap again, on a frame where all four taps of the second k-step land inside it (one-pixel's are all outside, so
    # a tap index that advances by one per step instead of two would not show there)
    ("octet", (2, 6, 8, 16, 3, 4, 64, 6, 7, 64, 0), (4, 24, 18, 24, 18, 2, 1, 2)),
    # H = 1, odd Wo, odd noct = 9
    ("row", (2, 70, 72, 80, 1, 6, 64, 2, 11, 72, 4), (4, 12, 10, 12, 10, 18, 1, 18)),
    # Wo = 1: classes 1 and 3 empty
    ("column", (1, 72, 72, 72, 5, 1, 128, 9, 1, 128, 0), (2, 5, 0, 4, 0, 18, 1, 18)),
    # Ho, Wo < 2H − 1
    ("crop", (2, 100, 104, 104, 6, 6, 64, 9, 10, 68, 4), (4, 50, 50, 40, 40, 26, 1, 26)),
    # 50 steps → slices of 17, 17, 16 that start mid-tap (noct 25)
    ("three-ragged", (1, 200, 200, 208, 4, 5, 64, 7, 9, 64, 0), (4, 20, 16, 15, 12, 50, 3, 17)),
    # the tile rule asks for 8 slices, the 16-step floor leaves 2; Cout = 192: a half-empty second M block
    ("floor-trim", (1, 130, 136, 136, 4, 4, 192, 8, 8, 200, 8), (8, 16, 16, 16, 16, 34, 2, 17)),
    # noct 33 is odd: the two lane halves of a step straddle a tap boundary; last slice of 15 steps
    ("four-odd", (1, 260, 264, 264, 3, 5, 192, 6, 9, 192, 0), (8, 15, 12, 15, 12, 66, 4, 17)),
    # eight slices, the last of 11 steps
    ("eight-ragged", (1, 518, 520, 528, 3, 3, 64, 5, 6, 64, 0), (4, 9, 9, 6, 6, 130, 8, 17)),
    # exactly 512 tiles: unsplit by the tile rule although 32 steps would allow 2
    ("tiles-512", (4, 128, 128, 128, 32, 32, 512, 64, 64, 512, 0), (512, 4096, 4096, 4096, 4096, 32, 1, 32)),
    # just below the boundary: the same K is sliced
    ("tiles-504", (4, 128, 128, 128, 32, 32, 512, 63, 64, 512, 0), (504, 4096, 4096, 3968, 3968, 32, 2, 16)),
]
DECONV_IDS = [r[0] for r in DECONV_ROWS]
# what tests/test_gpu_fp16_decoder.py runs (its shape tuples, B in front): the network rows stay there
EXISTING_DECONV_SHAPES = [(1024, 1024, 1024, 8, 10, 512, 15, 20, 1032, 512), (1026, 1032, 1032, 15, 20, 256, 30, 40, 776, 512),
                          (40, 40, 48, 5, 7, 64, 9, 13, 72, 4)]
EXISTING_DECONV_CASES = [(B,) + s for B in (1, 3) for s in EXISTING_DECONV_SHAPES] + \
    [(64, 1026, 1032, 1032, 15, 20, 256, 30, 40, 776, 512)]

FEWOUT_ROWS = [
    ("one-pixel", (1, 5, 8, 8, 1, 1), (1, 0), (64, 1, 1, 1)),             # one octet, 63 idle lanes
    ("clipped", (1, 24, 24, 32, 2, 3), (2, 0), (64, 1, 3, 1)),            # segments clipped by W
    ("four-waves", (1, 1540, 1544, 1552, 3, 5), (3, 0), (256, 2, 3, 4)),  # 63 idle lanes in the last wave, segments 2, 2, 1
    ("wide", (1, 40, 40, 48, 2, 70), (1, 1), (64, 18, 4, 1)),             # W > 64 with few rows: 18, 18, 18, 16
    ("width-only", (1, 8, 8, 8, 2, 300), (1, 2), (64, 60, 5, 1)),         # segment count from the width alone
    ("1024-rows", (16, 16, 16, 16, 64, 20), (2, 1), (64, 20, 1, 1)),      # one segment per row
    ("full-wave", (2, 512, 512, 512, 4, 8), (1, 2), (64, 2, 4, 1)),       # one wave, every lane active
    ("one-lane", (2, 518, 520, 520, 4, 8), (2, 0), (128, 2, 4, 2)),       # one lane in the second wave
    ("largest", (1, 2048, 2048, 2048, 2, 4), (3, 0), (256, 1, 4, 4)),     # the largest input the kernel takes
    # three waves with a ragged last segment (2, 2, 1), H = 1: Convolution2's plan at B = 32, which no other row has
    ("three-waves", (1, 1030, 1032, 1040, 1, 5), (2, 0), (192, 2, 3, 3)),
]
FEWOUT_IDS = [r[0] for r in FEWOUT_ROWS]
EXISTING_FEWOUT_CASES = [(3, 770, 776, 776, 30, 40), (3, 1026, 1032, 1032, 15, 20), (3, 1024, 1024, 1024, 8, 10)]

UPSAMPLE_ROWS = [(1, 1, 1, 1, 1, 2, 0), (2, 3, 5, 5, 9, 8, 6), (1, 4, 6, 6, 10, 4, 2),
                 (3, 9, 11, 18, 22, 16, 8)]           # B, H, W, Ho, Wo, out_ctotal, out_coff; the last: 1188 pixels, no multiple of 256
COPY_ROWS = [(1, 8, 16, 8, 24, 16),                    # npix, C, src_ctotal, src_coff, dst_ctotal, dst_coff: one thread
             (37, 24, 40, 8, 48, 16),                  # 111 pixel x octet pairs: part of one block
             (101, 40, 56, 16, 64, 8)]                 # 505: two blocks, the second ragged

# a sliced call whose split-K scratch covers that of every small sliced row, on another pixel layout; tiles-504's own twin
DIRTY_SMALL = (1, 264, 264, 264, 4, 6, 192, 7, 11, 192, 0)
DIRTY_504 = (4, 128, 128, 128, 32, 32, 512, 64, 63, 512, 0)

SLOPE_EXACT = 0.5
SLOPE_RANDOM = float(np.float32(0.1))   # the slope the kernel multiplies by
U = 2.0 ** -24
F16_MIN_NORMAL = 2.0 ** -14


# ---- what a plan means for the kernel
def noct(case):
    return case[2] // 8


def slice_steps(plan):
    """k-steps of each K slice"""
    nsteps, ksplit, sps = plan[5:8]
    return [min(nsteps, (s + 1) * sps) - s * sps for s in range(ksplit)]


def scratch_floats(case, plan):
    return plan[6] * case[0] * case[7] * case[8] * case[6] if plan[6] > 1 else 0


def dirty_case(rid):
    return DIRTY_504 if rid == "tiles-504" else DIRTY_SMALL


def deconv_combination(case, plan):
    """What decides which code of the deconvolution runs: K sliced (partial stores + second pass) or not, a ragged last slice, a
    slice that starts inside a tap, noct odd (a step's two lane halves can sit in different taps), one octet per tap, an empty
    parity class, a half-empty last M block."""
    sps = plan[7]
    return (plan[6] > 1, len(set(slice_steps(plan))) > 1, any((2 * s * sps) % noct(case) for s in range(1, plan[6])),
            noct(case) % 2 == 1, noct(case) == 1, 0 in plan[1:5], case[6] % 128 != 0)


def fewout_segments(case, plan):
    W, (_, seg, nseg, _) = case[5], plan
    return [min(W, (i + 1) * seg) - i * seg for i in range(nseg)]


def fewout_nseg_rule(case):
    """Which term of the plan sets the segment count: 'width' (ceil(W / 64)), 'rows' (until ~1024 blocks run, at most 4), or
    'clipped' (no more segments than columns)."""
    B, _, _, _, H, W = case
    by_width, by_rows = -(-W // 64), min(4, -(-1024 // (B * H)))
    if max(by_width, by_rows) > W:
        return "clipped"
    return "width" if by_width >= by_rows else "rows"


def fewout_combination(case, plan):
    """What decides which code of the few-filter kernel runs: waves per block (the block reduction's length), idle lanes in the
    last wave, more than one segment per row (a left neighbour column that is real), a ragged last segment."""
    segs = fewout_segments(case, plan)
    return (plan[3], noct(case) % 64 != 0, plan[2] > 1, len(set(segs)) > 1)


# ---- operands
def flush16(a):
    """Round to fp16 and replace every fp16 subnormal by 0: the bounds then hold whatever v_dot2 or the MFMA do with subnormals."""
    h = np.asarray(a).astype(np.float16)
    h[np.abs(h.astype(np.float32)) < F16_MIN_NORMAL] = 0
    return h


def _exact(rng, xshape, wshape, nb):
    x = rng.integers(-4, 5, xshape).astype(np.float32)
    w = (rng.integers(-2, 3, wshape) * 0.5).astype(np.float32)
    b = (rng.integers(-32, 33, nb) * 0.25).astype(np.float32)
    return x, w, b


def _random(rng, xshape, wshape, nb, K):
    x = flush16(rng.standard_normal(xshape)).astype(np.float32)
    w = flush16(rng.standard_normal(wshape) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(nb).astype(np.float32)
    return x, w, b


def _geometry(case):
    """The operands and the uncropped reference depend on (B, Cin, H, W, Cout) alone: tiles-512 and tiles-504 share theirs."""
    return (case[0], case[1], case[4], case[5], case[6])


@functools.lru_cache(maxsize=None)
def deconv_operands(geometry, kind):
    """x (B,Cin,H,W), w (Cin,Cout,4,4), bias (Cout), float32 holding fp16 values (bias: any fp32). kind 'exact': integer x in [-4, 4],
    w in {-1, -0.5, 0, 0.5, 1}, bias a multiple of 0.25 in [-8, 8]: with slope 0.5 every value on the way is a multiple of 0.125 below
    16·Cin + 8 < 2^15, exact in fp32 under any slicing or order. kind 'random': N(0,1), N(0,1)/sqrt(4·Cin), N(0,1), no fp16 subnormal."""
    B, cin, H, W, cout = geometry
    rng = np.random.default_rng([B, cin, H, W, cout, int(kind == "exact")])
    if kind == "exact":
        assert 16 * cin + 8 < 2 ** 15
        out = _exact(rng, (B, cin, H, W), (cin, cout, 4, 4), cout)
    else:
        out = _random(rng, (B, cin, H, W), (cin, cout, 4, 4), cout, 4 * cin)
    for a in out:
        a.setflags(write=False)
    return out


def fewout_operands(case, nout, kind):
    """x (B,Cin,H,W), w (nout,Cin,3,3), bias (nout) as deconv_operands; the exact kind's limit is asserted on A by fewout_reference."""
    B, cin, _, _, H, W = case
    rng = np.random.default_rng([B, cin, H, W, nout, int(kind == "exact")])
    if kind == "exact":
        return _exact(rng, (B, cin, H, W), (nout, cin, 3, 3), nout)
    return _random(rng, (B, cin, H, W), (nout, cin, 3, 3), nout, 9 * cin)


def dirty_operands(case):
    """|x| = 1000, w = 1: every split-K partial sum is a large finite fp32 value"""
    B, cin, _, _, H, W, cout = case[:7]
    return np.full((B, cin, H, W), 1000.0, np.float32), np.ones((cin, cout, 4, 4), np.float32), np.zeros(cout, np.float32)


def nhwc_record(x, cin_pad, ctotal):
    """(B,Cin,H,W) → NHWC fp16 records of ctotal channels: channels [Cin, Cin_pad) finite non-zero (their packed weights are zero),
    channels [Cin_pad, ctotal) NaN (the kernels must not read them)."""
    B, cin, H, W = x.shape
    rec = np.full((B, H, W, ctotal), np.nan, np.float16)
    rec[..., :cin] = x.transpose(0, 2, 3, 1)
    rec[..., cin:cin_pad] = np.float16(-3.5)
    return rec


# ---- float64 references
def _t64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def deconv64(x, w):
    """float64 Deconvolution k4 s2 p0, uncropped (2H+2, 2W+2), no bias"""
    import torch
    return torch.nn.functional.conv_transpose2d(_t64(x), _t64(w), None, 2).numpy()


def conv64(x, w):
    """float64 3x3 stride-1 pad-1 convolution, no bias"""
    import torch
    return torch.nn.functional.conv2d(_t64(x), _t64(w), None, 1, 1).numpy()


@functools.lru_cache(maxsize=None)
def _deconv_full(geometry, kind, absolute):
    x, w, _ = deconv_operands(geometry, kind)
    out = deconv64(np.abs(x), np.abs(w)) if absolute else deconv64(x, w)
    out.setflags(write=False)
    return out


def deconv_reference(case, kind, with_A=True):
    """S = Crop(1,1)(deconv(x, w)) + b at (Ho, Wo), and A = the same of the absolute values (None without with_A)"""
    g, (Ho, Wo) = _geometry(case), case[7:9]
    b = deconv_operands(g, kind)[2].astype(np.float64)[None, :, None, None]
    S = _deconv_full(g, kind, False)[:, :, 1:1 + Ho, 1:1 + Wo] + b
    A = _deconv_full(g, kind, True)[:, :, 1:1 + Ho, 1:1 + Wo] + np.abs(b) if with_A else None
    return S, A


def fewout_reference(x, w, b):
    b64 = b.astype(np.float64)[None, :, None, None]
    return conv64(x, w) + b64, conv64(np.abs(x), np.abs(w)) + np.abs(b64)


def lrelu(s, slope):
    return np.where(s > 0, s, s * slope)


def f16(a):
    """round a float64 array to fp16 once; as float32 values"""
    return np.asarray(a).astype(np.float16).astype(np.float32)


def fp32_sum_bound(n, A):
    return n * U * A / (1.0 - n * U)


def deconv_bound(case, plan, A):
    return fp32_sum_bound(4 * case[2] + plan[6] + 2, A)


def fewout_bound(case, plan, A):
    return fp32_sum_bound(9 * case[2] + plan[3] + 2, A)


# ---- upsample_flow
def ulp16(v):
    return np.spacing(np.abs(np.asarray(v, np.float32)).astype(np.float16)).astype(np.float32)


def upsample_operands(row, kind):
    """flow (B,2,H,W), w (2,2,4,4), bias (2), fp32. 'grid': multiples of 1/8 (flow in [-16, 16], w in [-2, 2], bias in [-4, 4]), so
    that the kernel's fp32 products and sums are exact. 'random': flow 3·N(0,1), w N(0,1), bias ±48 + N(0,1): the outputs stay away
    from zero, where one fp16 ulp is smaller than the fp32 sum's own error (upsample_margin asserts that they do)."""
    B, H, W = row[:3]
    rng = np.random.default_rng([B, H, W, int(kind == "grid")])
    if kind == "grid":
        return ((rng.integers(-128, 129, (B, 2, H, W)) / 8).astype(np.float32), (rng.integers(-16, 17, (2, 2, 4, 4)) / 8).astype(np.float32),
                (rng.integers(-32, 33, 2) / 8).astype(np.float32))
    return ((3 * rng.standard_normal((B, 2, H, W))).astype(np.float32), rng.standard_normal((2, 2, 4, 4)).astype(np.float32),
            (np.array([48.0, -48.0]) + rng.standard_normal(2)).astype(np.float32))


def upsample_reference(row, flow, w, b):
    Ho, Wo = row[3:5]
    b64 = b.astype(np.float64)[None, :, None, None]
    return (deconv64(flow, w)[:, :, 1:1 + Ho, 1:1 + Wo] + b64,
            deconv64(np.abs(flow), np.abs(w))[:, :, 1:1 + Ho, 1:1 + Wo] + np.abs(b64))


def upsample_margin(S, A):
    """True where the one-ulp statement cannot fail a correct kernel: the fp32 evaluation (16 rounded products, 16 adds: within
    32·u·A of S, first order) stays within half an fp16 ulp of S, so its rounding is float16(S) or a neighbour."""
    return fp32_sum_bound(32, A) < 0.5 * ulp16(S)
