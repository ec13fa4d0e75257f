"""The edge shapes of the fp32 weight gradient (csrc/backward.hip: the few-filter stream kernel, the LDS-staged MFMA kernel, the
register-fed MFMA kernel and their slice reduce passes) that tests/test_gpu_fp32_wgrad_edges.py runs and
tests/test_fp32_backward_cases_host.py pins, the operands of both kinds and the float64 / int64 references. Nothing here touches the
GPU runtime.

A row: name, (B, Cin, H, W, Cout, k, stride, pad), the option "wgrad_lds", and the ten ints deepim_conv_wgrad_plan must report:
family (0 few-filter, 1 LDS-staged, 2 register-fed), bm, m-tiles, k-tiles, units (16-pixel chunks of one sample for the LDS-staged
kernel, groups of 8 pixels for the register-fed one), S, units per slice, units of the last slice, reduce pass (0 none, 1 scalar,
2 four quarters), ragged last unit of a sample. Every row keeps Ho*Wo a multiple of 4 (the entries refuse anything else) and stays
below 2 MB of operands.

Operands, seeded from the row's name:
  exact    integers in [-2, 2] as float32: every product and every partial sum in any order is an integer below 2^24, so the result
           must equal the int64 sum bit for bit whatever the chunking and slicing; one dropped, doubled or misplaced term shows;
  random   standard normal float32; per element |got - ref| <= gamma_n * sum|x*dz| + 2^-149 with gamma_n = n*u / (1 - n*u), u = 2^-24
           and n = B*Ho*Wo + 1 terms: the worst case of n rounded products added in fp32 in ANY order, of which the kernels' chunks,
           slices and quarters are one. Nothing is measured into the bound.
References: an explicit im2col of the zero-padded input, times dz, in numpy (int64 for the exact kind, float64 for the random)."""
import functools
import zlib

import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64
U = 2.0 ** -24
FEW, LDS, REG = 0, 1, 2
NONE, SCALAR, QUARTERS = 0, 1, 2

# ---- the tables ----------------------------------------------------------------------------------------------------------------
#          name                   (B, Cin, H, W, Cout, k, s, p)     lds  family bm  mt kt units S  per last reduce    ragged
LDS_ROWS = [
    ("one-chunk",          (1, 8, 2, 2, 8, 1, 1, 0),        1, (LDS, 64, 1, 1, 1, 1, 1, 1, NONE, 1)),
    ("tiny-ragged",        (3, 8, 2, 2, 8, 3, 1, 1),        1, (LDS, 64, 1, 1, 3, 1, 3, 3, NONE, 1)),
    ("direct-ragged12",    (1, 8, 18, 22, 72, 3, 1, 1),     1, (LDS, 128, 1, 1, 25, 1, 25, 25, NONE, 1)),
    ("direct64-ragged12",  (2, 24, 6, 10, 16, 3, 1, 1),     1, (LDS, 64, 1, 2, 8, 1, 8, 8, NONE, 1)),
    ("direct-whole",       (2, 8, 8, 8, 16, 3, 1, 1),       1, (LDS, 64, 1, 1, 8, 1, 8, 8, NONE, 0)),
    ("conv5-like",         (2, 64, 30, 40, 128, 3, 2, 1),   1, (LDS, 128, 1, 5, 38, 2, 19, 19, SCALAR, 1)),
    ("conv1-like",         (3, 8, 30, 40, 64, 7, 2, 3),     1, (LDS, 64, 1, 4, 57, 3, 19, 19, SCALAR, 1)),
    ("ragged-m-k5",        (3, 16, 29, 40, 200, 5, 2, 2),   1, (LDS, 128, 2, 4, 57, 3, 19, 19, SCALAR, 1)),
    ("cout5-whole",        (5, 3, 14, 18, 5, 3, 1, 1),      1, (LDS, 64, 1, 1, 80, 5, 16, 16, SCALAR, 1)),
    ("short-last",         (9, 8, 10, 14, 16, 3, 1, 1),     1, (LDS, 64, 1, 1, 81, 5, 17, 13, SCALAR, 1)),
    ("ragged8",            (5, 8, 12, 14, 16, 3, 1, 1),     1, (LDS, 64, 1, 1, 55, 3, 19, 17, SCALAR, 1)),
    ("s15-scalar",         (5, 6, 26, 30, 5, 3, 1, 1),      1, (LDS, 64, 1, 1, 245, 15, 17, 7, SCALAR, 1)),
    ("s11-scalar-mod4",    (6, 5, 18, 26, 7, 3, 1, 1),      1, (LDS, 64, 1, 1, 180, 11, 17, 10, SCALAR, 1)),
    ("quarters-s9",        (6, 8, 18, 22, 16, 3, 1, 1),     1, (LDS, 64, 1, 1, 150, 9, 17, 14, QUARTERS, 1)),
    ("quarters-s10",       (7, 8, 18, 22, 130, 3, 1, 1),    1, (LDS, 128, 2, 1, 175, 10, 18, 13, QUARTERS, 1)),
    ("quarters-s13",       (11, 8, 30, 40, 64, 3, 2, 1),    1, (LDS, 64, 1, 1, 209, 13, 17, 5, QUARTERS, 1)),
    ("quarters-s18-mod4",  (4, 8, 33, 36, 64, 3, 1, 1),     1, (LDS, 64, 1, 1, 300, 18, 17, 11, QUARTERS, 1)),
    ("quarters-s20-last2", (13, 8, 18, 22, 64, 3, 1, 1),    1, (LDS, 64, 1, 1, 325, 20, 17, 2, QUARTERS, 1)),
    # branch signatures the network's layers take at 480x640 that no row above carries (whole 16-pixel chunks: the maps of conv1 ...
    # conv4_1 and conv6; the signature test of tests/test_fp32_backward_cases_host.py names the layers)
    ("net-64-quarters-whole",    (8, 8, 16, 16, 8, 3, 1, 1),    1, (LDS, 64, 1, 1, 128, 8, 16, 16, QUARTERS, 0)),     # conv1, B = 1 ... 8
    ("net-64-quarters-short",    (11, 8, 12, 16, 16, 3, 1, 1),  1, (LDS, 64, 1, 1, 132, 8, 17, 13, QUARTERS, 0)),    # conv1
    ("net-128-direct-whole",     (1, 8, 8, 8, 130, 3, 1, 1),    1, (LDS, 128, 2, 1, 4, 1, 4, 4, NONE, 0)),           # conv6, conv6_1, deconv5
    ("net-128-s2-whole",         (2, 16, 16, 16, 72, 3, 1, 1),  1, (LDS, 128, 1, 2, 32, 2, 16, 16, SCALAR, 0)),      # conv4_1, conv6
    ("net-128-s3-short",         (13, 8, 8, 8, 72, 3, 1, 1),    1, (LDS, 128, 1, 1, 52, 3, 18, 16, SCALAR, 0)),      # conv4, conv4_1 at B = 1
    ("net-128-s2-short-ragged",  (3, 8, 12, 14, 72, 3, 1, 1),   1, (LDS, 128, 1, 1, 33, 2, 17, 16, SCALAR, 1)),      # conv5, conv5_1, deconv4 at B >= 8
    ("net-128-quarters-whole",   (8, 8, 16, 16, 72, 3, 1, 1),   1, (LDS, 128, 1, 1, 128, 8, 16, 16, QUARTERS, 0)),   # conv3, conv4
    ("net-128-quarters-ragged",  (9, 8, 14, 18, 72, 3, 1, 1),   1, (LDS, 128, 1, 1, 144, 9, 16, 16, QUARTERS, 1)),   # deconv4 at B = 32
    ("net-128-quarters-short",   (7, 8, 16, 24, 72, 3, 1, 1),   1, (LDS, 128, 1, 1, 168, 10, 17, 15, QUARTERS, 0)),  # conv2, conv3_1
]
REG_ROWS = [
    ("reg-one-chunk",         (1, 8, 2, 2, 8, 1, 1, 0),     0, (REG, 128, 1, 1, 1, 1, 1, 1, SCALAR, 1)),
    ("reg-quarters-s9-mod8",  (4, 8, 33, 36, 64, 3, 1, 1),  0, (REG, 128, 1, 1, 596, 9, 67, 60, QUARTERS, 1)),
    ("reg-s6-ktiles2",        (3, 16, 30, 38, 40, 3, 1, 1), 0, (REG, 128, 1, 2, 429, 6, 72, 69, SCALAR, 1)),
    ("reg-whole-groups",      (2, 8, 16, 24, 16, 3, 1, 1),  0, (REG, 128, 1, 1, 96, 1, 96, 96, SCALAR, 0)),
]
_FEW_PLAN = (FEW, 64, 1, 1, 0, 1, 0, 0, NONE, 0)
FEW_ROWS = [(n, g, 1, _FEW_PLAN) for n, g in (
    ("few-co3-k3",      (2, 5, 18, 22, 3, 3, 1, 1)),       # the CO = 4 template with one dead filter; 396 pixels
    ("few-co3-k4-s2",   (3, 3, 16, 22, 3, 4, 2, 1)),       # 8 x 11 = 88 pixels
    ("few-co1-k4-s2",   (2, 2, 32, 42, 1, 4, 2, 0)),       # 15 x 20
    ("few-co4-k4",      (1, 7, 13, 17, 4, 4, 1, 1)),       # 12 x 16
    ("few-co1-k3",      (2, 6, 30, 40, 1, 3, 1, 1)),       # 1200 pixels: five turns of the 256-pixel loop
    ("few-co2-k3-s2",   (1, 9, 10, 16, 2, 3, 2, 1)),       # 5 x 8
    ("few-co2-k4",      (1, 4, 11, 15, 2, 4, 1, 1)),       # 10 x 14
    ("few-co4-k3-s2",   (2, 3, 20, 24, 4, 3, 2, 1)),       # 10 x 12
)]
ROWS = LDS_ROWS + REG_ROWS + FEW_ROWS
BY_NAME = {r[0]: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
NAMES = [r[0] for r in ROWS]
KINDS = ("exact", "random")
# the existing row of tests/test_gpu_backward.py (WG_CASES) that has Ho*Wo % 16 == 0 on the LDS-staged kernel with S > 1
EXISTING_WHOLE_CHUNK_ROW = (2, 8, 32, 40, 64, 7, 2, 3)

# what the entries refuse: Ho*Wo % 4 != 0 (odd maps, 5 x 6), no output pixel, no stride, empty operands
REFUSED = [(1, 9, 10, 12, 2, 3, 2, 1), (1, 8, 5, 5, 8, 3, 1, 1), (2, 8, 7, 6, 16, 3, 1, 1), (1, 8, 2, 2, 8, 5, 1, 0), (1, 8, 8, 8, 8, 3, 0, 1),
           (0, 8, 8, 8, 8, 3, 1, 1), (1, 0, 8, 8, 8, 3, 1, 1), (1, 8, 8, 8, 0, 3, 1, 1), (1, 8, 8, 8, 8, 0, 1, 1), (1, 8, 8, 8, 8, 3, 1, -1)]

# the bias-gradient / activation-gradient walks: (B, C, H, W)
WALK_SHAPES = [(1, 5, 67, 63),      # hw = 4221, not a multiple of 4: the scalar walk; S = 2, 3072 per slice, the last 1149
               (2, 8, 66, 64),      # hw = 4224 = 33 tiles of 128: several slices of whole tiles on the channel-blocked walk
               (1, 16, 15, 20)]     # hw = 300: a ragged 128-pixel tile
SLOPE_EXACT, SLOPE_REAL = 0.5, float(f32(0.1))


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def npix(case):
    B, _, H, W, _, k, s, p = case
    ho, wo = out_hw(H, W, k, s, p)
    return B * ho * wo


def variants(name):
    """The x_mode values deepim_conv2d_wgrad_tm_nc8 also runs a row at ([] = no tap-major variant at all)"""
    _, (B, cin, H, W, cout, k, s, p), lds, plan = BY_NAME[name]
    if not (lds == 1 and plan[0] == LDS and cin % 8 == 0 and cout > 4):
        return []
    return [1, 3] if H % 2 == 0 and W % 2 == 0 else [1]


# ---- operands ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(name, kind):
    """-> x (B,Cin,H,W), dz (B,Cout,Ho,Wo), float32"""
    B, cin, H, W, cout, k, s, p = BY_NAME[name][1]
    ho, wo = out_hw(H, W, k, s, p)
    rng = _rng("fp32-wgrad", name, kind)
    if kind == "exact":
        x, dz = rng.integers(-2, 3, (B, cin, H, W)).astype(f32), rng.integers(-2, 3, (B, cout, ho, wo)).astype(f32)
    else:
        x, dz = rng.standard_normal((B, cin, H, W)).astype(f32), rng.standard_normal((B, cout, ho, wo)).astype(f32)
    x.setflags(write=False)
    dz.setflags(write=False)
    return x, dz


def exact_sum_limit(name):
    """The largest magnitude any partial sum of an exact row can reach: every term is at most 2 * 2"""
    return 4 * npix(BY_NAME[name][1])


def to_nc8(x):
    """NCHW -> channel-blocked (B, C/8, H, W, 8)"""
    B, C, H, W = x.shape
    return np.ascontiguousarray(x.reshape(B, C // 8, 8, H, W).transpose(0, 1, 3, 4, 2))


def to_nc8_s2d(x):
    """NCHW -> the same records in space-to-depth order: pixel (y, x), channel c at channel ((y & 1) * 2 + (x & 1)) * C + c, position
    (y / 2, x / 2) of a (B, 4 C / 8, H / 2, W / 2, 8) tensor"""
    B, C, H, W = x.shape
    planes = np.concatenate([x[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], axis=1)
    return to_nc8(planes)


def to_tap_major(dw):
    """(Cout, Cin, k, k) -> (Cout, k*k, Cin)"""
    return np.ascontiguousarray(dw.reshape(dw.shape[0], dw.shape[1], -1).transpose(0, 2, 1))


# ---- references ----------------------------------------------------------------------------------------------------------------
def im2col(x, k, s, p):
    """x (B,Cin,H,W) -> (B*Ho*Wo, Cin*k*k): row (n, ho, wo), column (ci, ky, kx) = the zero-padded x[n, ci, ho*s + ky - p, wo*s + kx - p]"""
    B, cin, H, W = x.shape
    ho, wo = out_hw(H, W, k, s, p)
    xp = np.zeros((B, cin, H + 2 * p, W + 2 * p), x.dtype)
    xp[:, :, p:p + H, p:p + W] = x
    cols = np.empty((B, ho, wo, cin, k, k), x.dtype)
    for ky in range(k):
        for kx in range(k):
            cols[:, :, :, :, ky, kx] = xp[:, :, ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s].transpose(0, 2, 3, 1)
    return cols.reshape(B * ho * wo, cin * k * k)


def _rows(dz):
    """dz (B,Cout,Ho,Wo) -> (Cout, B*Ho*Wo), pixels in im2col's row order"""
    return np.ascontiguousarray(dz.transpose(1, 0, 2, 3).reshape(dz.shape[1], -1))


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """exact: (dw, db) int64. random: (dw, A, db, Ab) float64: the sums and the sums of the absolute products (db: of |dz|)."""
    B, cin, H, W, cout, k, s, p = BY_NAME[name][1]
    x, dz = operands(name, kind)
    t = i64 if kind == "exact" else f64
    cols, rows = im2col(x.astype(t), k, s, p), _rows(dz.astype(t))
    dw = (rows @ cols).reshape(cout, cin, k, k)
    db = rows.sum(axis=1)
    if kind == "exact":
        return dw, db
    return dw, (np.abs(rows) @ np.abs(cols)).reshape(cout, cin, k, k), db, np.abs(rows).sum(axis=1)


def gamma(n):
    return n * U / (1.0 - n * U)


def wgrad_bound(name, A):
    """Per element: n = B*Ho*Wo + 1 terms"""
    return gamma(npix(BY_NAME[name][1]) + 1) * A + 2.0 ** -149


def bias_bound(name, Ab):
    return gamma(npix(BY_NAME[name][1])) * Ab + 2.0 ** -149


# ---- the bias-gradient and activation-gradient walks ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_operands(shape, with_add):
    """-> dy, add (or None), y: integers in [-2, 2] as float32 (y with zeros: the slope side of y > 0)"""
    rng = _rng("fp32-walk", shape, with_add)
    dy = rng.integers(-2, 3, shape).astype(f32)
    add = rng.integers(-2, 3, shape).astype(f32) if with_add else None
    y = rng.integers(-2, 3, shape).astype(f32)
    for a in (dy, add, y):
        if a is not None:
            a.setflags(write=False)
    return dy, add, y


def walk_reference(shape, with_add, slope):
    """The float64 walk -> dz (float64, every element fp32-representable after ONE rounding), db (float64, exact: every dz is a
    multiple of 2^-27 below 8 and there are fewer than 2^14 of them per channel)"""
    dy, add, y = walk_operands(shape, with_add)
    g = dy.astype(f64) + (add.astype(f64) if add is not None else 0.0)
    dz = np.where(y > 0, g, g * f64(f32(slope))).astype(f32).astype(f64)
    return dz, dz.sum(axis=(0, 2, 3))
