"""The launch plans of deepim_conv2d_f16_forward that tests/test_gpu_fp16_plans.py runs and tests/test_fp16_plan_host.py pins, and the
float64 references both share. A row: id, case (B, Cin, H, W, Cout, k, stride, pad), the context options it runs under, and the eight
ints deepim_conv_f16_plan must report for it under those options: kernel (0 register-staged, 1 four-wave LDS-DMA, 2 ping-pong), BM, BN,
tiles, K chunks, ksplit, tail_s, R (tiles of the last, partly filled round; 0 without a tail split)."""
import numpy as np

REG, DMA, PP = 0, 1, 2
NO_PP = {"f16_dev_flags": 16}
NO_SPLIT = {"conv_max_split": 1}

ROWS = [
    # ping-pong kernel with a tail split of the last round (256 resident blocks): whole and ragged last pixel tile, both tile shapes
    ("pp-tail2", (1, 64, 132, 256, 512, 3, 1, 1), {}, (PP, 256, 256, 264, 9, 1, 2, 8)),
    ("pp-tail3-ragged", (1, 128, 131, 255, 512, 3, 1, 1), {}, (PP, 256, 256, 262, 18, 1, 3, 6)),
    ("pp128-tail2-ragged", (1, 64, 259, 515, 128, 3, 1, 1), {}, (PP, 128, 512, 261, 9, 1, 2, 5)),
    ("pp128-tail2", (1, 64, 87, 512, 384, 3, 1, 1), {}, (PP, 128, 512, 261, 9, 1, 2, 5)),
    # ping-pong kernel with uniform split-K
    ("pp-split3", (1, 128, 90, 93, 512, 3, 1, 1), {}, (PP, 256, 256, 66, 18, 3, 0, 0)),
    ("pp-split3-whole", (1, 128, 64, 128, 512, 3, 1, 1), {}, (PP, 256, 256, 64, 18, 3, 0, 0)),
    ("pp128-split3", (1, 64, 131, 255, 128, 5, 1, 2), {}, (PP, 128, 512, 66, 25, 3, 0, 0)),
    # ping-pong kernel, no K slicing: three channel tiles of 128; whole pixel tiles of either shape
    ("pp128-3M", (1, 64, 130, 131, 384, 3, 1, 1), {}, (PP, 128, 512, 102, 9, 1, 0, 0)),
    ("pp128-whole", (1, 64, 128, 256, 128, 3, 1, 1), {}, (PP, 128, 512, 64, 9, 1, 0, 0)),
    ("pp-whole", (1, 64, 64, 128, 512, 3, 1, 1), {}, (PP, 256, 256, 64, 9, 1, 0, 0)),
    # four-wave kernel with a tail split (512 resident blocks): the ping-pong rows' geometry with the ping-pong kernel switched off
    ("dma-tail", (1, 128, 131, 255, 512, 3, 1, 1), NO_PP, (DMA, 256, 128, 522, 18, 1, 4, 10)),
    ("dma128-tail", (1, 64, 259, 515, 128, 3, 1, 1), NO_PP, (DMA, 128, 256, 522, 9, 1, 2, 10)),
    # four-wave kernel, Cout % 128 != 0: guarded partial store under split-K, quad-store epilogue without
    ("dma-raggedM-split2", (1, 64, 30, 33, 192, 3, 1, 1), {}, (DMA, 128, 256, 8, 9, 2, 0, 0)),
    ("dma-raggedM-split4", (1, 128, 30, 33, 320, 3, 1, 1), {}, (DMA, 128, 256, 12, 18, 4, 0, 0)),
    ("dma-raggedM-whole-192", (1, 64, 30, 33, 192, 3, 1, 1), NO_SPLIT, (DMA, 128, 256, 8, 9, 1, 0, 0)),
    ("dma-raggedM-whole-320", (1, 128, 30, 33, 320, 3, 1, 1), NO_SPLIT, (DMA, 128, 256, 12, 18, 1, 0, 0)),
    # four-wave kernel with uniform split-K as the network's small batches take it: 128x256 whole, 256x128 whole and ragged
    ("dma128-split-whole", (1, 64, 16, 16, 128, 3, 1, 1), {}, (DMA, 128, 256, 1, 9, 2, 0, 0)),
    ("dma-split-whole", (1, 64, 16, 16, 256, 3, 1, 1), {}, (DMA, 256, 128, 2, 9, 2, 0, 0)),
    ("dma-split-ragged", (1, 64, 15, 20, 256, 3, 1, 1), {}, (DMA, 256, 128, 3, 9, 2, 0, 0)),
    # register-staged kernel <1,4,2,2,true> (Cout <= 64, Cin % 64 == 0); Cout 32 leaves half the channel tile empty
    ("reg-ut-64", (1, 64, 16, 20, 64, 3, 1, 1), {}, (REG, 64, 256, 2, 9, 2, 0, 0)),
    ("reg-ut-32", (1, 64, 16, 20, 32, 3, 1, 1), {}, (REG, 64, 256, 2, 9, 2, 0, 0)),
    ("reg-ut-deep", (1, 128, 9, 11, 48, 5, 1, 2), {}, (REG, 64, 256, 1, 50, 10, 0, 0)),   # 12 slices asked: 10 of 5 chunks cover 50
    # the three register-staged kernels with a per-octet tap (Cin % 64 != 0) under split-K
    ("reg-split-128", (1, 40, 12, 14, 128, 5, 1, 2), {}, (REG, 128, 256, 1, 16, 4, 0, 0)),
    ("reg-split-256", (1, 40, 12, 14, 256, 5, 1, 2), {}, (REG, 256, 256, 1, 16, 4, 0, 0)),
    ("reg-split-64", (1, 24, 12, 14, 64, 7, 1, 3), {}, (REG, 64, 256, 1, 19, 4, 0, 0)),
]
ROW_IDS = [r[0] for r in ROWS]
X3_TAIL_CASE = (4, 32, 120, 160, 256, 3, 1, 1)   # tests/test_gpu_x3.py::test_conv_x3_is_fp32_grade relies on its tail split

SLOPE_EXACT = 0.5
SLOPE_RANDOM = float(np.float32(0.1))   # the slope the kernel multiplies by


def out_hw(case):
    _, _, H, W, _, k, s, p = case
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def npix(case):
    ho, wo = out_hw(case)
    return case[0] * ho * wo


def cin_pad(case):
    return (case[1] + 7) // 8 * 8


def sliced(plan):
    return plan[5] > 1 or plan[6] > 1


def slices(plan):
    return max(plan[5], plan[6], 1)


def combination(case, plan):
    """What decides which code runs: kernel, tile, uniform split-K or not, tail split or not, ragged last pixel tile or not."""
    return (plan[0], plan[1], plan[2], plan[5] > 1, plan[6] > 1, npix(case) % plan[2] != 0)


def tail_region(case, plan):
    """(first pixel, first channel) of the tail tiles: tiles run pixel tile fastest, so the last R tiles are the last R pixel tiles of
    the last channel tile (every row here has R <= pixel tiles)."""
    gx = -(-npix(case) // plan[2])
    assert 0 < plan[7] <= gx
    return (gx - plan[7]) * plan[2], (plan[3] // gx - 1) * plan[1]


def conv64(x, w, stride, pad):
    """float64 convolution of float64 operands on the CPU, no bias"""
    import torch
    return torch.nn.functional.conv2d(torch.from_numpy(np.ascontiguousarray(x, np.float64)),
                                      torch.from_numpy(np.ascontiguousarray(w, np.float64)), None, stride, pad).numpy()


def lrelu16(s, slope):
    """float16(LeakyReLU(s)) of a float64 array, as float32 values"""
    return np.where(s > 0, s, s * slope).astype(np.float16).astype(np.float32)


def exact_operands(case, seed):
    """Operands whose every partial sum is exact in fp32 under any order, slicing or tiling: integer x in [-4, 4], w in
    {-1, -0.5, 0, 0.5, 1}, bias a multiple of 0.25 in [-8, 8]; with slope 0.5 every value on the way is a multiple of 0.125 below
    4·k·k·Cin + 8 < 2^15."""
    B, cin, H, W, cout, k, _, _ = case
    assert 4 * k * k * cin + 8 < 2 ** 15
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, (B, cin, H, W)).astype(np.float32)
    w = (rng.integers(-2, 3, (cout, cin, k, k)) * 0.5).astype(np.float32)
    b = (rng.integers(-32, 33, cout) * 0.25).astype(np.float32)
    return x, w, b


def random_operands(case, seed):
    B, cin, H, W, cout, k, _, _ = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    return x, w, b


def random_reference(case, x, w, b):
    """S = conv(xq, wq) + b and A = conv(|xq|, |wq|) + |b| in float64 for the fp16-rounded operands"""
    _, _, _, _, _, _, s, p = case
    xq, wq = x.astype(np.float16).astype(np.float64), w.astype(np.float16).astype(np.float64)
    b64 = b.astype(np.float64)[None, :, None, None]
    return conv64(xq, wq, s, p) + b64, conv64(np.abs(xq), np.abs(wq), s, p) + np.abs(b64)


def fp32_sum_bound(case, plan, A):
    """|fp32 sum in any order − exact sum| <= n·u·A / (1 − n·u), u = 2^-24, for n = the K terms + the slices' adds + the bias add and
    the slope multiply"""
    n = case[5] * case[5] * cin_pad(case) + slices(plan) + 2
    nu = n * 2.0 ** -24
    return nu * A / (1.0 - nu)
