"""CPU: the fp16-decoder emulation helper (tests/fp16_decoder_emulation.py) with the fp16 rounding replaced by the identity is the
oracle's fp32 decoder and heads exactly — pins the helper's wiring (concat order, which layers round, which weights)."""
import numpy as np

import fp16_decoder_emulation as emu
from oracle import pipeline as opipe
from mx_deepim_amd.config import default_config
from mx_deepim_amd.symbols import deepIM_flownet


def test_emulation_with_identity_rounding_is_the_oracle_decoder_and_heads():
    cfg = default_config()
    cfg.TEST.FAST_TEST = False
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=61)
    rng = np.random.default_rng(6)
    B, H, W = 1, 64, 80
    acts = {"conv4_1": rng.standard_normal((B, 512, 30, 40)).astype(np.float32),
            "conv5_1": rng.standard_normal((B, 512, 15, 20)).astype(np.float32),
            "conv6_1": rng.standard_normal((B, 1024, 8, 10)).astype(np.float32)}
    zf = np.array([[1.5, 1.5, 3.0, 2.0]], np.float32)
    ident = lambda x: np.asarray(x, np.float32)   # noqa: E731
    got = emu.decoder(params, acts, q=ident)
    want = opipe.decoder(params, acts)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    gh = emu.heads(params, got["Concat3"], zf, H, W, 20.0, q=ident)
    m = opipe.mask_head(params, want["Concat3"], zf, H, W)
    f = opipe.flow_head(params, want["Concat3"], zf, H, W, 20.0)
    for k, v in zip(("mask_lowres", "mask_logits", "mask_observed_pred"), m):
        np.testing.assert_array_equal(gh[k], v, err_msg=k)
    for k, v in zip(("flow_lowres", "zoom_flow_est", "flow_est"), f):
        np.testing.assert_array_equal(gh[k], v, err_msg=k)
    # and with fp16 rounding the deconvolution channels are fp16 values
    r = emu.decoder(params, acts)
    np.testing.assert_array_equal(r["Concat2"][:, 512:1026], emu.q16(r["Concat2"][:, 512:1026]))
    assert not np.array_equal(r["Concat3"], want["Concat3"])
