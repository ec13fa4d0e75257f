"""The arithmetic of csrc/wino_c1.hip restated in float64 (no GPU): conv1's 7x7 stride-2 pad-3 layer as Winograd F(2x2,4x4) over the
four input phases equals the direct sum, and the even phases' transformed weights vanish at exactly the positions the kernel skips."""
import numpy as np

# interpolation points 0, 1, -1, 1/2, infinity; rows of B^T scaled to small integers, G scaled to match (csrc/wino_c1.hip)
BT = np.array([[1, -2, -1, 2, 0], [0, -1, 1, 2, 0], [0, -1, 3, -2, 0], [0, 1, 0, -1, 0], [0, 1, -2, -1, 2]], np.float64)
G = np.array([[1, 0, 0, 0], [.5, .5, .5, .5], [1 / 6, -1 / 6, 1 / 6, -1 / 6], [8 / 3, 4 / 3, 2 / 3, 1 / 3], [0, 0, 0, .5]])
AT = np.array([[1, 1, 1, 1, 0], [0, 1, -1, .5, 1]], np.float64)


def _phase_kernel(w, py, px):
    """(Cout, Cin, 4, 4) taps of input phase (py, px): tap (a, b) = w[2a + py - 1][2b + px - 1], zero where an index is -1."""
    g = np.zeros(w.shape[:2] + (4, 4))
    for a in range(4):
        for b in range(4):
            ky, kx = 2 * a + py - 1, 2 * b + px - 1
            if ky >= 0 and kx >= 0:
                g[:, :, a, b] = w[:, :, ky, kx]
    return g


def _direct(x, w):
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.pad(x, ((0, 0), (0, 0), (3, 3 + 1), (3, 3 + 1)))
    out = np.zeros((B, w.shape[0], Ho, Wo))
    for ky in range(7):
        for kx in range(7):
            patch = xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
            out += np.einsum("bchw,oc->bohw", patch, w[:, :, ky, kx])
    return out


def _wino(x, w):
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    TY, TX = (Ho + 1) // 2, (Wo + 1) // 2
    # phase (py, px) at phase index (i, j) = x[2i + py][2j + px]; a tile's patch covers phase indices 2t - 2 .. 2t + 2
    Hp, Wp = 2 * TY + 4, 2 * TX + 4
    M = np.zeros((B, w.shape[0], TY, TX, 5, 5))
    for py in range(2):
        for px in range(2):
            ph = np.zeros((B, C, Hp, Wp))
            sub = x[:, :, py::2, px::2]
            ph[:, :, 2:2 + sub.shape[2], 2:2 + sub.shape[3]] = sub[:, :, :Hp - 2, :Wp - 2]
            U = np.einsum("xa,ocab,yb->ocxy", G, _phase_kernel(w, py, px), G)
            d = np.stack([np.stack([ph[:, :, 2 * ty:2 * ty + 5, 2 * tx:2 * tx + 5] for tx in range(TX)], 2) for ty in range(TY)], 2)
            V = np.einsum("xr,bcijrs,ys->bcijxy", BT, d, BT)
            M += np.einsum("ocxy,bcijxy->boijxy", U, V)
    Y = np.einsum("px,noijxy,qy->noijpq", AT, M, AT)
    out = Y.transpose(0, 1, 2, 4, 3, 5).reshape(B, w.shape[0], 2 * TY, 2 * TX)
    return out[:, :, :Ho, :Wo]


def test_f24_phase_transforms_equal_the_direct_sum():
    rng = np.random.default_rng(0)
    for B, H, W in ((2, 16, 20), (1, 13, 9), (1, 6, 5)):
        x = rng.standard_normal((B, 8, H, W))
        w = rng.standard_normal((5, 8, 7, 7))
        ref = _direct(x, w)
        got = _wino(x, w)
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_81_of_100_phase_positions_are_nonzero():
    rng = np.random.default_rng(1)
    w = rng.standard_normal((4, 8, 7, 7))
    nz = 0
    for py in range(2):
        for px in range(2):
            U = np.einsum("xa,ocab,yb->ocxy", G, _phase_kernel(w, py, px), G)
            mask = np.abs(U).max(axis=(0, 1)) > 0
            want = np.ones((5, 5), bool)
            if py == 0:
                want[0, :] = False
            if px == 0:
                want[:, 0] = False
            np.testing.assert_array_equal(mask, want)
            nz += int(mask.sum())
    assert nz == 81


def test_f24_in_float32_stays_within_1e5_of_range():
    """The same transforms with float32 data and U rounded once to float32 (the kernel packs U in double, rounds once)."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1, 8, 24, 32)).astype(np.float32)
    w = (rng.standard_normal((64, 8, 7, 7)) / np.sqrt(8 * 49)).astype(np.float32)
    ref = _direct(x.astype(np.float64), w.astype(np.float64))
    B, C, H, W = x.shape
    Ho, Wo = ref.shape[2:]
    TY, TX = (Ho + 1) // 2, (Wo + 1) // 2
    Hp, Wp = 2 * TY + 4, 2 * TX + 4
    f = np.float32
    M = np.zeros((B, 64, TY, TX, 5, 5), f)
    for py in range(2):
        for px in range(2):
            ph = np.zeros((B, C, Hp, Wp), f)
            sub = x[:, :, py::2, px::2]
            ph[:, :, 2:2 + sub.shape[2], 2:2 + sub.shape[3]] = sub[:, :, :Hp - 2, :Wp - 2]
            U = np.einsum("xa,ocab,yb->ocxy", G, _phase_kernel(w.astype(np.float64), py, px), G).astype(f)
            d = np.stack([np.stack([ph[:, :, 2 * ty:2 * ty + 5, 2 * tx:2 * tx + 5] for tx in range(TX)], 2) for ty in range(TY)], 2)
            V = np.einsum("xr,bcijrs,ys->bcijxy", BT.astype(f), d, BT.astype(f))
            M += np.einsum("ocxy,bcijxy->boijxy", U, V)
    Y = np.einsum("px,noijxy,qy->noijpq", AT.astype(f), M, AT.astype(f))
    got = Y.transpose(0, 1, 2, 4, 3, 5).reshape(B, 64, 2 * TY, 2 * TX)[:, :, :Ho, :Wo]
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
