"""CPU: the fp16 Winograd contract's numpy restatement (tests/fp16_wino_emulation.py) and the host side of network.FP16_WINOGRAD.
With the rounding replaced by the identity and float64 everywhere the emulation is the exact convolution; with fp16 rounding it stays
within 2^-9 of the layer's range of the direct fp16 path's result — four fp16 roundings (U, T, V, output) of 2^-11 each."""
import copy
import os
import re

import numpy as np
import pytest

import fp16_wino_emulation as emu
from oracle import net as onet
from oracle import pipeline as opipe
from mx_deepim_amd.config import default_config
from mx_deepim_amd.symbols import deepIM_flownet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conv64(x, w, b, slope):
    """Direct 3x3 stride-1 pad-1 convolution + bias + LeakyReLU in float64."""
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    y = np.zeros((B, w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            y += np.einsum("oc,bchw->bohw", w[:, :, ky, kx].astype(np.float64), xp[:, :, ky:ky + H, kx:kx + W])
    y += np.asarray(b, np.float64).reshape(1, -1, 1, 1)
    return np.where(y > 0, y, y * np.float64(np.float32(slope)))


@pytest.mark.parametrize("shape", [(2, 8, 6, 8, 16), (1, 5, 7, 9, 3), (2, 16, 1, 1, 4), (1, 4, 15, 20, 8)])
def test_identity_rounding_is_the_exact_convolution(shape):
    B, cin, H, W, cout = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((B, cin, H, W))
    w = rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)
    b = rng.standard_normal(cout).astype(np.float32)
    got = emu.conv_wino(x, w, b, 0.1, q=emu.identity, acc=np.float64, wdtype=np.float64)
    want = _conv64(x, w, b, 0.1)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("case", [(2, 64, 15, 20), (1, 256, 15, 20), (1, 1024, 8, 10)])
def test_fp16_contract_against_direct_fp16(case):
    """LeakyReLU-shaped activations, 1/sqrt(9 Cin) weights, 64 output channels: max |contract - q16(direct)| <= 2^-9 of the range."""
    B, cin, H, W = case
    cout = 64
    rng = np.random.default_rng(cin)
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    x = np.where(x > 0, x, 0.1 * x).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    want = opipe.q16(onet.conv2d(opipe.q16(x), opipe.q16(w), b, 1, 1, 0.1))
    rng_ = np.abs(want).max()
    got = emu.conv_wino(x, w, b, 0.1)
    err = np.abs(got - want).max() / rng_
    exact = _conv64(opipe.q16(x).astype(np.float64), opipe.q16(w).astype(np.float64), b, 0.1)
    pre = np.abs(emu.conv_wino(x, w, b, 0.1, pre_round=True) - exact).max() / rng_
    print("fp16 Winograd contract, Cin %4d: %.3g of the range from q16(direct), %.1f %% of elements differ; before the output rounding "
          "%.3g from the exact convolution (one fp16 rounding of it: %.3g)" %
          (cin, err, 100 * np.mean(got != want), pre, np.abs(opipe.q16(exact) - exact).max() / rng_))
    assert err <= 2.0 ** -9


def test_weight_transform_is_g_w_gt_rounded_once():
    """The fixed order of fp32 adds lands within one fp32 rounding or two of the float64 G g G^T; after the fp16 rounding almost all
    entries are the correctly rounded ones, none is more than one fp16 step away."""
    from oracle.wino import G
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((32, 16, 3, 3)) / 12).astype(np.float32)
    u = emu.transform_weights(w)
    ref = np.einsum("xa,ocab,nb->ocxn", G, opipe.q16(w).astype(np.float64), G)
    assert u.dtype == np.float32 and np.array_equal(u, opipe.q16(u))
    assert np.abs(u - ref).max() <= 2.0 ** -10 * np.abs(ref).max()
    assert np.mean(u != opipe.q16(ref)) < 0.01


def test_config_key_defaults_to_off():
    cfg = default_config()
    assert "FP16_WINOGRAD" in cfg.network and cfg.network.FP16_WINOGRAD is False


def test_header_declares_the_four_entries():
    txt = open(os.path.join(ROOT, "include", "deepim_hip.h")).read()
    for name in ("deepim_conv_wino_f16_supported", "deepim_conv_wino_f16_packed_size", "deepim_conv_wino_f16_pack_weights",
                 "deepim_conv2d_wino_f16_forward"):
        assert re.search(r"\b%s\s*\(" % name, txt), name


def test_only_the_fp16_test_symbol_reads_the_key():
    cfg = default_config()
    cfg.network.FP16_WINOGRAD = True
    assert deepIM_flownet().get_symbol(cfg).fp16_winograd is False              # fp32 graph
    c = copy.deepcopy(cfg); c.network.X3_CONV = True
    assert deepIM_flownet().get_symbol(c).fp16_winograd is False                # x3 graph
    c = copy.deepcopy(cfg); c.network.FP16_CONV = True
    assert deepIM_flownet().get_symbol(c).fp16_winograd is True
    c.network.FP16_WINOGRAD = False
    assert deepIM_flownet().get_symbol(c).fp16_winograd is False


def test_train_symbol_clears_the_flag():
    cfg = default_config()
    cfg.network.FP16_CONV = True
    cfg.network.FP16_WINOGRAD = True
    net = deepIM_flownet().get_train_symbol(cfg)
    assert net.fp16_conv and net.fp16_winograd is False
