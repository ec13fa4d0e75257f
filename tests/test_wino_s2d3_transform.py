"""The 3x3 stride-2 pad-1 layers (conv4 / conv5 / conv6) as F(2x2,3x3) over the space-to-depth input, restated in float64 (no
device): the kernel is taps 1..3 of a 5x5 stride-2 pad-2 kernel, phase (py, px) of the input carries tap (a, b) = w[2a + py - 1][2b + px - 1]
where both indices lie in 0..2, and only 25 of the 64 (phase, position) pairs of U = G g G^T can be non-zero. Plus the launch plans of
conv4 / conv5 under the default options (host arithmetic of deepim_conv_wino_plan with s2d = 2)."""
import ctypes

import numpy as np
import pytest

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def phase_taps(w):
    """(Cout, Cin, 3, 3) stride-2 pad-1 kernel -> (4, Cout, Cin, 3, 3): the 3x3 stride-1 pad-1 kernel of each input phase py*2 + px."""
    g = np.zeros((4,) + w.shape, w.dtype)
    for py in range(2):
        for px in range(2):
            for a in range(3):
                for b in range(3):
                    ky, kx = 2 * a + py - 1, 2 * b + px - 1
                    if 0 <= ky < 3 and 0 <= kx < 3:
                        g[py * 2 + px, :, :, a, b] = w[:, :, ky, kx]
    return g


def live_pairs():
    """(phase, xi, nu) that the kernel's S2D = 2 walk keeps (W8_XLIVE / W8_NLIVE in csrc/wino.hip, restated)."""
    out = set()
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        for xi in range(4):
            for nu in range(4):
                if xi != 3 and nu != 3 and (py or xi != 0) and (px or nu != 0):
                    out.add((ph, xi, nu))
    return out


def conv_s2_direct(x, w):
    B, C, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, C, 2 * Ho + 2, 2 * Wo + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    y = np.zeros((B, w.shape[0], Ho, Wo))
    for ky in range(3):
        for kx in range(3):
            y += np.einsum("bchw,oc->bohw", xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], w[:, :, ky, kx])
    return y


def conv_s2_winograd_s2d(x, w):
    """Space-to-depth (odd planes padded with a zero row / column), U per phase, V = B^T d B over 4x4 patches of every phase plane,
    M = sum over phases and channels of U * V at the live pairs only, Y = A^T M A."""
    B, C, H, W = x.shape
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    xe = np.zeros((B, C, 2 * Hp, 2 * Wp))
    xe[:, :, :H, :W] = x
    planes = [xe[:, :, py::2, px::2] for py in range(2) for px in range(2)]
    U = np.einsum("xa,pocab,nb->pocxn", G, phase_taps(w), G)            # (4, Cout, Cin, 4, 4)
    TY, TX = (Hp + 1) // 2, (Wp + 1) // 2
    y = np.zeros((B, w.shape[0], 2 * TY, 2 * TX))
    live = live_pairs()
    for ph, P in enumerate(planes):
        pad = np.zeros((B, C, 2 * TY + 2, 2 * TX + 2))
        pad[:, :, 1:Hp + 1, 1:Wp + 1] = P
        for ty in range(TY):
            for tx in range(TX):
                d = pad[:, :, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]
                V = np.einsum("xi,bcij,nj->bcxn", BT, d, BT)
                M = np.zeros((B, w.shape[0], 4, 4))
                for (p_, xi, nu) in live:
                    if p_ == ph:
                        M[:, :, xi, nu] = np.einsum("oc,bc->bo", U[ph, :, :, xi, nu], V[:, :, xi, nu])
                y[:, :, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] += np.einsum("ax,boxn,cn->boac", AT, M, AT)
    return y[:, :, :Hp, :Wp]


def test_exactly_25_live_phase_position_pairs():
    rng = np.random.default_rng(0)
    w = rng.standard_normal((5, 3, 3, 3))
    U = np.einsum("xa,pocab,nb->pocxn", G, phase_taps(w), G)
    nz = {(ph, xi, nu) for ph in range(4) for xi in range(4) for nu in range(4) if np.abs(U[ph, :, :, xi, nu]).max() > 0}
    assert nz == live_pairs() and len(nz) == 25
    dead = [(ph, xi, nu) for ph in range(4) for xi in range(4) for nu in range(4) if (ph, xi, nu) not in nz]
    assert len(dead) == 39 and all(np.all(U[ph, :, :, xi, nu] == 0.0) for ph, xi, nu in dead)   # identically zero, not small
    assert sorted(sum(1 for p_, _, _ in nz if p_ == ph) for ph in range(4)) == [4, 6, 6, 9]


@pytest.mark.parametrize("shape", [(2, 3, 8, 12), (1, 2, 7, 9), (2, 2, 15, 20), (1, 3, 6, 5)])
def test_decomposition_matches_direct_stride2_conv(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape)
    w = rng.standard_normal((4, shape[1], 3, 3))
    want = conv_s2_direct(x, w)
    got = conv_s2_winograd_s2d(x, w)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def _plan(B, cin, H, W, cout, out_nc8=1, s2d=2):
    from mx_deepim_amd.runtime import lib
    plan = (ctypes.c_int * 9)()
    assert lib.load().deepim_conv_wino_plan(None, B, cin, H, W, cout, out_nc8, s2d, plan) == 0      # host arithmetic: no device
    return list(plan)


# conv4 / conv5 / conv6 as the kernel sees them: (4 Cin, H/2, W/2, Cout) of the space-to-depth problem
_LAYERS = {"conv4": (1024, 30, 40, 512), "conv5": (2048, 15, 20, 512), "conv6": (2048, 8, 10, 1024)}


def _pieces(plan, slots):
    """The persistent blocks' piece walk (W8_PERSIST / w8_run_owner in csrc/wino.hip), restated: per block a list of
    (tile block, first granule, end granule, copy, pieces)."""
    _, _, _, ks, G_, q, F, grid0, rem = plan
    nlb = slots // 8

    def owner(u):
        big = rem * (q + 1)
        return u // (q + 1) if u < big else rem + (u - big) // q
    out = []
    for b in range(slots):
        lb, xcd = b >> 3, b & 7
        u = lb * q + min(lb, rem)
        uend = u + q + (1 if lb < rem else 0)
        mine = [((vb * nlb + lb) * 8 + xcd, 0, G_, -1, 0) for vb in range(F)]
        while u < uend:
            lt = u // G_
            g0 = u - lt * G_
            g1 = min(G_, g0 + uend - u)
            o0, o1 = owner(lt * G_), owner(lt * G_ + G_ - 1)
            n = o1 - o0 + 1
            mine.append(((F * nlb + lt) * 8 + xcd, g0, g1, -1 if n == 1 else lb - o0, 0 if n == 1 else n))
            u += g1 - g0
        out.append(mine)
    return out


@pytest.mark.parametrize("B", [32, 16, 8, 4])
def test_launch_plans_of_the_stride2_3x3_layers(B):
    """The phase walk needs K slices of whole eight-step bodies; stream-K (where the plan picks it) covers every granule once."""
    for name, (cin, H, W, cout) in _LAYERS.items():
        pl = _plan(B, cin, H, W, cout)
        assert pl[0] == 1 and pl[1] > 0, (B, name, pl)          # 128 channels x 32 tiles: the measured best block for this walk
        nK = cin // 8
        S, ks = pl[2], pl[3]
        assert ks % 8 == 0 and S * ks >= nK > (S - 1) * ks, (B, name, pl)
        G_, q, F, grid0 = pl[4], pl[5], pl[6], pl[7]
        if G_ == 0:
            continue
        assert S == 1 and F >= 2 and G_ * 8 == nK
        tiles = {}
        for blk in _pieces(pl, pl[1]):
            for bid, g0, g1, copy, n in blk:
                assert 0 <= bid < grid0 and 0 <= g0 < g1 <= G_
                tiles.setdefault(bid, []).append((g0, g1, copy, n))
        assert sorted(tiles) == list(range(grid0)), name
        for bid, ps in tiles.items():
            ps.sort()
            assert ps[0][0] == 0 and ps[-1][1] == G_ and all(a[1] == b[0] for a, b in zip(ps, ps[1:])), (name, bid, ps)
            if len(ps) > 1:
                assert [c for _, _, c, _ in ps] == list(range(len(ps))) and {n for *_, n in ps} == {len(ps)}
