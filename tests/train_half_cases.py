"""The edge shapes of the half-precision encoder backward (csrc/train_half.hip, fp16 and split-fp16 "x3" mode) that
tests/test_gpu_train_half_edges.py runs and tests/test_train_half_cases_host.py pins, the operands of both kinds and the float64
references. Every shape of tests/golden/make_train_half_digests.py is a row here, so each recorded digest also has a reference. Nothing
here touches the GPU runtime.

Weight-gradient rows: id, modes, case (B, Cin, Cin_pad, H, W, Cout, k, stride, pad) and the six ints deepim_conv_wgrad_half_plan must
report: m-tiles, n-tiles, k-steps, S, steps_per_split, ragged last k-step. Data-gradient rows: id and (B, Hd, Wd, k, stride, pad); each
runs at every (Ci_l, Co_l) pair of its mode.

Operands are kept as NCHW float64 arrays (hi, lo) of fp16-representable halves; fp16 mode has lo = 0. A stored tensor carries hi + lo
(x3: at the tensor's scale). Two kinds:
  exact    small integers and halves whose every product and partial sum is exact in fp32 under any slicing and order (the maker
           asserts the bit span of the largest possible sum from the shape); x3 operands carry lo = j·2^-11·|hi|, |j| <= 3, and the
           reference is the three-term sum hi·hi + hi·lo + lo·hi, because the kernels drop lo·lo;
  random   standard_normal with the scalings of tests/test_gpu_fp16_train.py and tests/test_gpu_x3_train.py; the reference S is the
           float64 sum over the values the stored operands carry, A the same sum over absolute values."""
import functools
import importlib.util
import os
import zlib

import numpy as np

import fp16_plan_cases as pc
import x3_train_emulation as emu

_spec = importlib.util.spec_from_file_location(
    "make_train_half_digests", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_train_half_digests.py"))
digests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digests)

MODES = digests.MODES
F16_ONLY = ("f16",)
f16, f32, f64 = np.float16, np.float32, np.float64
U = 2.0 ** -24
ACT = 16.0                       # the scale x3 stores activations at
WG_SCALE = {"f16": 256.0, "x3": 4096.0}      # the loss / gradient scale S of the weight-gradient cases (a power of two)
LRELU_SCALE = 1024.0
SLOPE_EXACT, SLOPE_RANDOM = 0.5, float(f32(0.1))

# ---- the tables ----------------------------------------------------------------------------------------------------------------
WG_ROWS = [("digest-%d" % i, r[9], r[:9], plan) for i, (r, plan) in enumerate(zip(digests.WGRAD, [
    (1, 2, 1, 1, 1, 1), (2, 2, 2, 2, 1, 1), (1, 7, 1, 1, 1, 1), (1, 4, 2, 2, 1, 1)]))] + [
    # S > 1, two steps per slice, the last of the 73 slices one step: every digest row has steps_per_split == 1
    ("split-short-last", MODES, (1, 16, 16, 68, 68, 144, 3, 1, 1), (2, 2, 145, 73, 2, 1)),
    # S == 1 with two k-steps: the double-buffered loop runs into the direct store (conv6_1's plan at B = 1 and at B >= 4)
    ("direct-2steps-ragged", MODES, (1, 1024, 1024, 6, 7, 1024, 3, 1, 1), (8, 72, 2, 1, 2, 1)),
    ("direct-2steps-whole", MODES, (1, 1024, 1024, 8, 8, 1024, 3, 1, 1), (8, 72, 2, 1, 2, 0)),
    # fp16 only: the ci >= Cin mask under a 3x3 kernel; a single octet of output channels
    ("cin12-pad16", F16_ONLY, (2, 12, 16, 7, 9, 40, 3, 1, 1), (1, 2, 4, 4, 1, 1)),
    ("cout8", F16_ONLY, (1, 16, 16, 6, 9, 8, 3, 1, 1), (1, 2, 2, 2, 1, 1)),
    # stride 2 over an odd frame with a 5x5 kernel
    ("s2-odd-k5", MODES, (2, 16, 16, 13, 15, 48, 5, 2, 2), (1, 4, 4, 4, 1, 1)),
    # the combinations the encoder takes at 480x640: whole tiles with whole and ragged last k-step (conv3 ... conv6), a partial
    # n-tile with whole m-tile (conv2), partial m- and n-tile with a whole last k-step (flow_conv1)
    ("split-whole-tiles", MODES, (1, 128, 128, 32, 32, 256, 3, 1, 1), (2, 9, 32, 16, 2, 0)),
    ("split-whole-tiles-ragged", MODES, (1, 128, 128, 31, 33, 256, 3, 1, 1), (2, 9, 32, 16, 2, 1)),
    ("split-partial-n", MODES, (1, 64, 64, 40, 40, 128, 5, 1, 2), (1, 13, 50, 25, 2, 0)),
    ("split-partial-mn", MODES, (1, 16, 16, 48, 50, 64, 7, 1, 3), (1, 7, 75, 38, 2, 0)),
]
WG_CASES = [(rid, mode) for rid, modes, _, _ in WG_ROWS for mode in modes]
WG_BY_ID = {r[0]: r for r in WG_ROWS}

DG_ROWS = [("digest-%d" % i, g) for i, g in enumerate(digests.DGRAD)] + \
    [("s2-%dx%d-k%d" % (h, w, k), (2, h, w, k, 2, k // 2)) for h, w in ((7, 9), (8, 9), (7, 10)) for k in (3, 5, 7)
     if (2, h, w, k, 2, k // 2) not in digests.DGRAD] + \
    [("s2-7x9-k5-B1", (1, 7, 9, 5, 2, 2)), ("s1-k3-B1", (1, 5, 9, 3, 1, 1)), ("s1-k1", (2, 6, 7, 1, 1, 0))]
DG_CH = {"f16": [digests.DGRAD_CH["f16"], (136, 72)], "x3": [digests.DGRAD_CH["x3"], (256, 96)]}      # (Ci_l, Co_l)
DG_CASES = [(rid, mode, ch) for rid, _ in DG_ROWS for mode in MODES for ch in DG_CH[mode]]
DG_BY_ID = dict(DG_ROWS)
DG_WSCALE_EXACT = 4.0

LRELU_CASES = [(shape, mode, src) for shape in digests.LRELU for mode in MODES for src in ("d", "add", "both")]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ---- layouts -------------------------------------------------------------------------------------------------------------------
def store(mode, hi, lo, cpad=None):
    """NCHW (hi, lo) -> what the entry points read: NHWC fp16 (channels padded with zeros to cpad), or split16 records (B,H,W,2C)"""
    B, C, H, W = hi.shape
    if mode == "f16":
        assert not np.any(lo)
        out = np.zeros((B, H, W, cpad or C), f16)
        out[..., :C] = hi.transpose(0, 2, 3, 1)
        assert np.array_equal(out[..., :C].astype(f64), hi.transpose(0, 2, 3, 1))
        return out
    rec = np.stack([a.transpose(0, 2, 3, 1).reshape(B, H, W, C // 16, 16) for a in (hi, lo)], axis=4)
    out = np.ascontiguousarray(rec.reshape(B, H, W, 2 * C)).astype(f16)
    assert np.array_equal(out.astype(f64), rec.reshape(B, H, W, 2 * C))        # the halves are stored as they are
    return out


def load(mode, a):
    """What an entry point wrote -> NCHW float64 (hi, lo)"""
    a = np.asarray(a)
    if mode == "f16":
        hi = np.ascontiguousarray(a.astype(f64).transpose(0, 3, 1, 2))
        return hi, np.zeros_like(hi)
    B, H, W, C2 = a.shape
    rec = a.reshape(B, H, W, C2 // 32, 2, 16).astype(f64)
    return tuple(np.ascontiguousarray(rec[..., i, :].reshape(B, H, W, C2 // 2).transpose(0, 3, 1, 2)) for i in (0, 1))


def split1(v):
    """x3_split(v, 1) of fp32-representable values -> (hi, lo) float64"""
    hi, lo = emu.split(np.asarray(v, f32), 1.0)
    return hi.astype(f64), lo.astype(f64)


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _exact_pairs(rng, shape, amp, mode, step=1.0):
    """hi = step · an integer in [-amp, amp]; x3: lo = j·2^-11·|hi|, j in [-3, 3]"""
    hi = rng.integers(-amp, amp + 1, shape).astype(f64) * step
    lo = np.zeros(shape) if mode == "f16" else rng.integers(-3, 4, shape) * 2.0 ** -11 * np.abs(hi)
    return hi, lo


def _random_pairs(rng, shape, scale, mode, store_scale=1.0):
    """standard_normal · scale, as the mode stores it: rounded to fp16, or split at store_scale (the stored halves)"""
    v = (rng.standard_normal(shape) * scale).astype(f32)
    if mode == "f16":
        hi = v.astype(f16).astype(f64)
        return hi, np.zeros_like(hi)
    hi, lo = emu.split(v, store_scale)
    return hi.astype(f64), lo.astype(f64)


def wg_npix(case):
    B, _, _, H, W, _, k, s, p = case
    ho, wo = out_hw(H, W, k, s, p)
    return B * ho * wo


def wgrad_operands(rid, mode, kind):
    """-> x (hi, lo) (B,Cin,H,W), dz (hi, lo) (B,Cout,Ho,Wo): the stored halves"""
    B, cin, _, H, W, cout, k, s, p = WG_BY_ID[rid][2]
    ho, wo = out_hw(H, W, k, s, p)
    rng = _rng("wgrad", rid, mode, kind)
    if kind == "random":
        return (_random_pairs(rng, (B, cin, H, W), 1.0, mode, ACT), _random_pairs(rng, (B, cout, ho, wo), 64.0, mode))
    npix = B * ho * wo
    if mode == "f16":
        # x a multiple of 0.5 in [-4, 4], dz an integer in [-8, 8]: every sum is a multiple of 0.5 below 32·npix
        assert 32 * npix * 2 < 2 ** 24
        return _exact_pairs(rng, (B, cin, H, W), 8, mode, 0.5), _exact_pairs(rng, (B, cout, ho, wo), 8, mode)
    # integers up to ax and az with lo halves: every term is a multiple of 2^-11, a pixel's three terms are at most
    # ax·az·(1 + 6·2^-11), so every sum is a multiple of 2^-11 below npix·ax·az·(1 + 6·2^-11)
    budget = (2 ** 24 - 1) // (npix * (2 ** 11 + 6))
    az = min(8, budget)
    ax = min(4, budget // max(az, 1))
    assert ax >= 1 and az >= 1 and npix * ax * az * (2 ** 11 + 6) < 2 ** 24
    return _exact_pairs(rng, (B, cin, H, W), ax, mode), _exact_pairs(rng, (B, cout, ho, wo), az, mode)


def dgrad_operands(rid, mode, ch, kind):
    """-> w (Co_l,Ci_l,k,k) fp32 as the entry point takes it, its scale (x3; 1 for fp16), w's halves (hi, lo) at that scale as the
    kernel's own split gives them, dz (hi, lo) (B,Co_l,Ho,Wo)"""
    B, Hd, Wd, k, s, p = DG_BY_ID[rid]
    ci, co = ch
    ho, wo = out_hw(Hd, Wd, k, s, p)
    rng = _rng("dgrad", rid, mode, ch, kind)
    n = co * k * k
    if kind == "random":
        if mode == "f16":
            w, sw = (rng.standard_normal((co, ci, k, k)) / np.sqrt(ci * k * k)).astype(f32), 1.0
        else:
            w = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(f32)
            sw = emu.weight_scale(w)
        dz = _random_pairs(rng, (B, co, ho, wo), 1.0 if mode == "f16" else 64.0, mode)
    elif mode == "f16":
        # w in {-1, -0.5, 0, 0.5, 1}, dz an integer in [-4, 4]: sums are multiples of 0.5 below 4·n, inside fp32 and fp16's range
        assert 4 * n * 2 < 2 ** 24 and 4 * n < 65504
        w, sw = (rng.integers(-2, 3, (co, ci, k, k)) * 0.5).astype(f32), 1.0
        dz = _exact_pairs(rng, (B, co, ho, wo), 4, mode)
    else:
        # w·s_w = ±(1 + b·2^-11), b in {0, 1}, or 0: the kernel's split gives hi = ±1, lo = ±b·2^-11 (a tie, to the even mantissa). dz
        # integers up to az with lo = j·2^-11·|hi|: a term's three products are multiples of 2^-11, at most az·(1 + 4·2^-11) together
        az = min(4, (2 ** 24 - 1) // (n * (2 ** 11 + 4)))
        assert az >= 1 and n * az * (2 ** 11 + 4) < 2 ** 24
        sw = DG_WSCALE_EXACT
        sign = rng.choice([-1.0, 0.0, 1.0], (co, ci, k, k), p=[0.4, 0.2, 0.4])
        w = (sign * (1.0 + rng.integers(0, 2, (co, ci, k, k)) * 2.0 ** -11) / sw).astype(f32)
        dz = _exact_pairs(rng, (B, co, ho, wo), az, mode)
    if mode == "f16":
        wh = w.astype(f16).astype(f64)
        wl = np.zeros_like(wh)
    else:
        wh, wl = (a.astype(f64) for a in emu.split(w, sw))
        if kind == "exact":
            assert np.all(np.abs(wh) <= 1.0) and np.array_equal(wh, np.rint(wh)) and np.array_equal((wh + wl) / sw, w.astype(f64))
    return w, sw, (wh, wl), dz


def lrelu_operands(shape, mode, src, kind):
    """-> y (hi, lo) (x3: stored at ACT), d (hi, lo) or None, add (B,C,H,W) fp32 or None, slope"""
    B, C, H, W = shape
    rng = _rng("lrelu", shape, mode, src, kind)
    if kind == "random":
        y = _random_pairs(rng, (B, C, H, W), 1.0, mode, ACT)
        d = _random_pairs(rng, (B, C, H, W), 8.0 if mode == "f16" else 64.0, mode)
        add = (rng.standard_normal((B, C, H, W)) * 1e-3).astype(f32)
        slope = SLOPE_RANDOM
    else:
        # e = d + S·add with S·add a multiple of 0.25; slope 0.5. fp16: |e| <= 10 in multiples of 0.25, so dz is a multiple of 0.125
        # and exact in fp16, and a channel's sum over npix pixels stays below npix·10·8 units. x3: |d| <= 2 + 6·2^-11, |S·add| <= 0.5,
        # so dz is a multiple of 2^-12 below 2.5 + 6·2^-11 (14 bits: an exact pair) and a channel's sum below npix·(2.5·2^12 + 12) units
        npix = B * H * W
        y = _exact_pairs(rng, (B, C, H, W), 2, "f16")                  # zeros included: the slope side of y > 0
        if mode == "f16":
            assert npix * 10 * 8 < 2 ** 24
            d, amax = _exact_pairs(rng, (B, C, H, W), 8, mode), 8
        else:
            assert npix * (10240 + 12) < 2 ** 24
            d, amax = _exact_pairs(rng, (B, C, H, W), 2, mode), 2
        add = (rng.integers(-amax, amax + 1, (B, C, H, W)) * 0.25 / LRELU_SCALE).astype(f32)
        slope = SLOPE_EXACT
    return y, (d if src != "add" else None), (add if src != "d" else None), slope


# ---- float64 references --------------------------------------------------------------------------------------------------------
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, f64))


def wgrad64(x, dz, k, s, p):
    """Σ_pix dz ⊗ im2col(x) in float64 -> (Cout,Cin,k,k)"""
    import torch
    return torch.nn.grad.conv2d_weight(_t(x), (dz.shape[1], x.shape[1], k, k), _t(dz), stride=s, padding=p).numpy()


def dgrad64(w, dz, Hd, Wd, s, p):
    """conv_transpose(dz, w) in float64 -> (B,Ci_l,Hd,Wd)"""
    import torch
    return torch.nn.grad.conv2d_input((dz.shape[0], w.shape[1], Hd, Wd), _t(w), _t(dz), stride=s, padding=p).numpy()


@functools.lru_cache(maxsize=None)
def wgrad_reference(rid, mode, kind):
    """exact: the natural-layout gradient, every element fp32-representable. random: (S, A)."""
    _, _, _, _, _, _, k, s, p = WG_BY_ID[rid][2]
    (xh, xl), (zh, zl) = wgrad_operands(rid, mode, kind)
    unit = WG_SCALE[mode] * (ACT if mode == "x3" else 1.0)
    if kind == "exact":
        ref = (wgrad64(xh + xl, zh, k, s, p) + (wgrad64(xh, zl, k, s, p) if mode == "x3" else 0.0)) / unit
        assert np.array_equal(ref.astype(f32).astype(f64), ref)
        return ref
    return wgrad64(xh + xl, zh + zl, k, s, p) / unit, wgrad64(np.abs(xh) + np.abs(xl), np.abs(zh) + np.abs(zl), k, s, p) / unit


@functools.lru_cache(maxsize=None)
def dgrad_reference(rid, mode, ch, kind):
    """exact: the NCHW data gradient before the one rounding to the output format. random: (S, A)."""
    _, Hd, Wd, _, s, p = DG_BY_ID[rid]
    _, sw, (wh, wl), (zh, zl) = dgrad_operands(rid, mode, ch, kind)
    if kind == "exact":
        ref = (dgrad64(wh + wl, zh, Hd, Wd, s, p) + (dgrad64(wh, zl, Hd, Wd, s, p) if mode == "x3" else 0.0)) / sw
        assert np.array_equal(ref.astype(f32).astype(f64), ref)
        return ref
    return (dgrad64(wh + wl, zh + zl, Hd, Wd, s, p) / sw,
            dgrad64(np.abs(wh) + np.abs(wl), np.abs(zh) + np.abs(zl), Hd, Wd, s, p) / sw)


def dgrad_reached(rid, ch):
    """(Hd, Wd) bool: the pixels of dx some output pixel reaches through some tap"""
    B, Hd, Wd, k, s, p = DG_BY_ID[rid]
    ho, wo = out_hw(Hd, Wd, k, s, p)
    return dgrad64(np.ones((1, 1, k, k)), np.ones((1, 1, ho, wo)), Hd, Wd, s, p)[0, 0] > 0


def round_to_output(mode, ref):
    """The one rounding of the output format -> (hi, lo) float64"""
    if mode == "f16":
        hi = ref.astype(f16).astype(f64)
        return hi, np.zeros_like(hi)
    return split1(ref)


def lrelu_reference(shape, mode, src, kind):
    """The numpy definition -> dz (hi, lo), the per-channel float64 sum of dz / S, the same sum of |dz| / S"""
    (yh, _), d, add, slope = lrelu_operands(shape, mode, src, kind)
    S = f32(LRELU_SCALE)
    e = np.zeros(shape, f32) if d is None else (d[0].astype(f32) + d[1].astype(f32)).astype(f32)
    if add is not None:
        e = (e + (S * add).astype(f32)).astype(f32) if d is not None else (S * add).astype(f32)
    t = np.where(yh > 0, e, (e * f32(slope)).astype(f32)).astype(f32)
    hi, lo = round_to_output(mode, t)
    v = hi + lo
    return (hi, lo), v.sum(axis=(0, 2, 3)) / LRELU_SCALE, np.abs(v).sum(axis=(0, 2, 3)) / LRELU_SCALE


# ---- the parity classes of the stride-2 data gradient, and the bound -------------------------------------------------------------
def s2_classes(k, pad):
    """{(py, px): (nky, nkx, P)}: the sub-kernel each output parity class of a stride-2 layer convolves with, and its padding"""
    out = {}
    for py in (0, 1):
        for px in (0, 1):
            nky, nkx = (k - (py + pad) % 2 + 1) // 2, (k - (px + pad) % 2 + 1) // 2
            out[(py, px)] = (nky, nkx, max(nky, nkx) - 1)
    return out


def dgrad_convs(rid):
    """The forward convolutions a data gradient runs: [(rows slice, cols slice, nky, nkx, P)] over dx"""
    _, _, _, k, s, p = DG_BY_ID[rid]
    if s == 1:
        return [(slice(None), slice(None), k, k, k - 1 - p)]
    return [(slice(py, None, 2), slice(px, None, 2)) + c for (py, px), c in s2_classes(k, p).items()]


def sum_bound(n, A):
    """|an fp32 sum of n roundings in any order − the exact sum| <= n·u·A / (1 − n·u), u = 2^-24 (as fp16_plan_cases.fp32_sum_bound)"""
    nu = n * U
    return nu * A / (1.0 - nu)


def wgrad_bound(rid, mode, plan, A):
    """fp32 is the output format, so the sum is all there is: terms = a product per pixel (x3: three), plus the slices' adds, plus 2
    (the unscale multiply and one spare, as fp16_plan_cases counts). x3 adds the dropped lo·lo products: |lo| <= 2^-11·|hi|, so they
    are at most 2^-22·A together."""
    terms = wg_npix(WG_BY_ID[rid][2]) * (3 if mode == "x3" else 1)
    return sum_bound(terms + plan[3] + 2, A) + (2.0 ** -22 * A if mode == "x3" else 0.0)


def dgrad_bound(rid, mode, ch, slices, S, A):
    """Per element: the fp32 sum of its class's Co_l·nky·nkx products (x3: three each) plus the slices' adds plus 2, e; x3's dropped
    lo·lo products, at most 2^-22·A; and the one rounding of the stored value v = S + δ, |δ| <= e:
      fp16  half a spacing of fp16 at |v| <= |S| + e (np.spacing of the rounded magnitude is that binade's or the next one's);
      x3    hi = f16(v) and r = v − hi are exact, lo = f16(r) errs by at most 2^-11·|r| <= 2^-22·|v|, or 2^-25 where r is subnormal.
    slices: one count per convolution of dgrad_convs(rid), from deepim_conv_f16_plan."""
    e = np.zeros_like(A)
    for (rows, cols, nky, nkx, _), sl in zip(dgrad_convs(rid), slices):
        n = ch[1] * nky * nkx * (3 if mode == "x3" else 1) + sl + 2
        e[:, :, rows, cols] = sum_bound(n, A[:, :, rows, cols])
    if mode == "x3":
        e += 2.0 ** -22 * A
        return e + np.maximum(2.0 ** -22 * (np.abs(S) + e), 2.0 ** -25)
    return e + 0.5 * np.spacing((np.abs(S) + e).astype(f16)).astype(f64)


# ---- the oracle's fp32 accumulation of the same operands (the host test's premises) ------------------------------------------------
def wgrad_fp32_chain(x, dz, k, s, p):
    """The weight gradient as one fp32 fmaf chain per element (oracle.net.conv2d: the frame as the input, the gradient, dilated by
    the stride, as the kernel) -> (Cout,Cin,k,k) float32"""
    from oracle import net as onet
    B, cin, H, W = x.shape
    _, cout, ho, wo = dz.shape
    xp = np.zeros((cin, B, H + 2 * p, W + 2 * p), f32)
    xp[:, :, p:p + H, p:p + W] = x.transpose(1, 0, 2, 3)
    zd = np.zeros((cout, B, (ho - 1) * s + 1, (wo - 1) * s + 1), f32)
    zd[:, :, ::s, ::s] = dz.transpose(1, 0, 2, 3)
    out = onet.conv2d(xp, zd, np.zeros(cout, f32), 1, 0)
    return np.ascontiguousarray(out[:, :, :k, :k].transpose(1, 0, 2, 3))


def dgrad_fp32_chain(w, dz, Hd, Wd, s, p):
    """The data gradient as one fp32 fmaf chain per element (oracle.net.conv2d of the dilated, padded gradient with the transposed,
    flipped weights) -> (B,Ci_l,Hd,Wd) float32"""
    from oracle import net as onet
    B, co, ho, wo = dz.shape
    k, q = w.shape[2], w.shape[2] - 1 - p
    zp = np.zeros((B, co, Hd + k - 1, Wd + k - 1), f32)
    zp[:, :, q:q + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s] = dz
    wt = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]).astype(f32)
    return onet.conv2d(zp, wt, np.zeros(w.shape[1], f32), 1, 0)


assert pc.fp32_sum_bound((1, 8, 1, 1, 1, 1, 1, 0), (0,) * 8, 3.0) == sum_bound(8 + 1 + 2, 3.0)      # one formula, two homes
