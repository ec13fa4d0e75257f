"""TRAIN.optimizer = "adam" without a GPU: the numpy restatement of MXNet's adam_update (tests/adam_emulation.py) against
torch.optim.Adam where the two formulas coincide and against closed forms where they do not; the float32 emulation inside the
bounds the GPU tests use, on their inputs; the configuration switch and the C ABI."""
import os

import numpy as np
import pytest
import torch

import adam_emulation as emu
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import parse_header
from mx_deepim_amd.symbols import deepIM_flownet


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_emulation_equals_torch_adam_where_epsilon_is_zero(wd):
    """With eps = 0 the two placements of epsilon coincide: 5 steps on 300 non-zero elements in float64, 1e-12 relative. (torch adds
    weight_decay * w to the gradient as MXNet does; rescale 1, no clip.)"""
    rng = np.random.default_rng(3)
    w0 = rng.standard_normal(300)
    w0[np.abs(w0) < 1e-3] = 1.0
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), eps=0.0, weight_decay=wd)
    w, m, v, t = w0.copy(), np.zeros(300), np.zeros(300), 0
    for _ in range(5):
        g = rng.standard_normal(300)
        g[np.abs(g) < 1e-3] = 1.0
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        w, m, v, t, _gp = emu.adam_update(w, m, v, g, 1e-2, t, wd=wd, epsilon=0.0, float_lr_t=False)
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-12, atol=0)
    assert t == 5


def test_epsilon_sits_outside_the_bias_correction():
    """t = 1 from zero moments: step = lr·sqrt(1-b2)·g' / (sqrt(1-b2)·|g'| + eps) — with an epsilon large enough to matter. torch's
    placement would give lr·g' / (|g'| + eps)."""
    g = np.array([1e-3, -2e-2, 0.5, -3.0])
    lr, eps, b2 = 0.1, 1e-3, 0.999
    w, m, v, t, _ = emu.adam_update(np.zeros(4), np.zeros(4), np.zeros(4), g, lr, 0, epsilon=eps)
    want = lr * np.sqrt(1 - b2) * g / (np.sqrt(1 - b2) * np.abs(g) + eps)
    np.testing.assert_allclose(-w, want, rtol=1e-6)                # (1e-6: lr_t is a float)
    torch_like = lr * g / (np.abs(g) + eps)
    assert np.abs(-w[0] - torch_like[0]) > 0.1 * np.abs(torch_like[0])
    assert t == 1


def test_clip_acts_after_the_weight_decay_term_and_zero_stays_zero():
    # g' = 0.5*1.0 + 0.1*8.0 = 1.3 -> clipped to 1.0; clipping first (the SGD kernel's order) would give min(0.5, 1) + 0.8 = 1.3
    w, m, v, t, gp = emu.adam_update(np.array([8.0]), np.zeros(1), np.zeros(1), np.array([1.0]), 1e-3, 0, wd=0.1, rescale=0.5, clip=1.0)
    assert gp[0] == 1.0 and m[0] == pytest.approx(0.1) and v[0] == pytest.approx(1e-3)
    # clip = 0 and None both mean no clip
    for clip in (0, 0.0, None):
        assert emu.adam_update(np.array([8.0]), np.zeros(1), np.zeros(1), np.array([1.0]), 1e-3, 0, wd=0.1, rescale=0.5, clip=clip)[4][0] == 1.3
    # g = m = v = 0, wd = 0: a step of exactly 0, not NaN; a skipped step moves nothing and keeps t
    for dt in (np.float32, np.float64):
        w, m, v, t, _ = emu.adam_update(np.array([0.25, -3.0]), np.zeros(2), np.zeros(2), np.zeros(2), 1e-3, 4, dtype=dt)
        assert w.tolist() == [0.25, -3.0] and not m.any() and not v.any() and t == 5
    w, m, v, t, _ = emu.adam_update(np.array([0.25]), np.array([0.5]), np.array([0.5]), np.array([np.inf]), 1e-3, 4, skip=True)
    assert (w[0], m[0], v[0], t) == (0.25, 0.5, 0.5, 4)


@pytest.mark.parametrize("clip", [0.0, 0.25])
def test_float32_emulation_stays_inside_the_gpu_tests_bounds_on_their_inputs(clip):
    """The bounds of tests/test_gpu_adam.py hold for a plain float32 evaluation in the kernel's operation order on exactly the
    inputs of the kernel test (same seeds): three updates of the 70-row table."""
    rng = np.random.default_rng(17)
    rows = emu.table_rows()
    assert len(rows) == 70 and sum(1 for r in rows if r[2]) == 3 and {r[1] for r in rows} == {0.0, 5e-4}
    w32 = emu.table_weights(rng)
    m32, v32 = [np.zeros_like(a) for a in w32], [np.zeros_like(a) for a in w32]
    t = 0
    for step in range(3):
        g = emu.table_gradients(rng)
        assert any((a == 0).any() for a in g) and all((a != 0).any() or a.size < 8 for a in g)
        for i, (n, wd, _tm) in enumerate(rows):
            ref = emu.adam_update(w32[i], m32[i], v32[i], g[i], 1e-3, t, wd=wd, rescale=0.5, clip=clip)
            got = emu.adam_update(w32[i], m32[i], v32[i], g[i], 1e-3, t, wd=wd, rescale=0.5, clip=clip, dtype=np.float32)
            assert got[0].dtype == np.float32
            if clip:
                assert step > 0 or i != 5 or (np.abs(ref[4]) == clip).any()      # the clip bites
            emu.check(got[0], got[1], got[2], ref, m32[i], emu.lr_t(1e-3, t + 1), "row %d update %d" % (i, step))
            w32[i], m32[i], v32[i] = got[0], got[1], got[2]
        t += 1


def test_train_symbol_honours_the_optimizer_key():
    cfg = default_config()
    assert cfg.TRAIN.optimizer == "sgd"
    assert deepIM_flownet().get_symbol(cfg, is_train=True).optimizer == "sgd"
    cfg.TRAIN.optimizer = "adam"
    assert deepIM_flownet().get_symbol(cfg, is_train=True).optimizer == "adam"
    for mode in ("FP16", "WINO", "X3"):        # every training mode takes it
        c = default_config()
        c.TRAIN.optimizer = "adam"
        c.network.FP16_CONV = mode == "FP16"
        c.TRAIN.WINOGRAD_CONV = mode == "WINO"
        c.TRAIN.X3_CONV = mode == "X3"
        assert deepIM_flownet().get_symbol(c, is_train=True).optimizer == "adam"
    cfg.TRAIN.optimizer = "nadam"
    with pytest.raises(ValueError, match="TRAIN.optimizer"):
        deepIM_flownet().get_symbol(cfg, is_train=True)


def test_header_declares_the_adam_entries():
    protos = parse_header()
    assert "deepim_adam_update" in protos and "deepim_adam_update_multi" in protos
    names = protos["deepim_adam_update_multi"][2]
    assert names[:5] == ["ctx", "table", "rows", "total_blocks", "opt_state"] and names[-1] == "amp_state"
    assert protos["deepim_adam_update"][2][:6] == ["ctx", "w", "mean", "var", "g", "lr_t"]


def test_optimizer_state_names_round_trip_through_nd_save(tmp_path):
    """optimizer_states() hands mx.nd.save a dict of float32 arrays and an int64 step count: the container carries both."""
    from mx_deepim_amd import mx
    d = {"mean:conv3_weight": np.arange(6, dtype=np.float32).reshape(2, 3), "var:conv3_weight": np.ones((2, 3), np.float32),
         "t": np.array([7], np.int64)}
    f = os.path.join(str(tmp_path), "opt.states")
    mx.nd.save(f, d)
    back = mx.nd.load(f)
    assert set(back) == set(d)
    for k in d:
        np.testing.assert_array_equal(back[k], d[k])
        assert back[k].dtype == d[k].dtype
