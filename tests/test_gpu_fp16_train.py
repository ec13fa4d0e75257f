"""§8f-4c — mixed-precision training (network.FP16_CONV in the training graph) on the GPU: the fp16 weight-gradient, data-gradient
and fused activation-gradient kernels against float64 references of the same fp16 operands; one training iteration against the
emulation of the numerics contract (tests/fp16_train_emulation.py, fed the GPU's own fp16 encoder activations) and against the fp32
oracle; the loss-scale state (overflow skip, halving, doubling); a full TRAIN_ITER_SIZE = 4 step."""
import ctypes

import numpy as np
import pytest
import torch

import fp16_train_emulation as emu
from oracle import pipeline as opipe
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import lib
from mx_deepim_amd.symbols import deepIM_flownet
from mx_deepim_amd.symbols.deepIM_flownet import ENCODER, _out_hw

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
MEANS_REV = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])


def _geoms(cin0=8, B=2, H=480, W=640):
    out, cin, hh, ww = [], cin0, H, W
    for name, cout, k, s, p in ENCODER:
        out.append((name, B, cin, hh, ww, cout, k, s, p))
        hh, ww = _out_hw(hh, ww, k, s, p)
        cin = cout
    return out


def _state(ctx, scale):
    st = np.zeros(4, np.uint32)
    st[:2] = np.array([scale, 1.0 / scale], np.float32).view(np.uint32)
    return ctx.array(st, np.uint32)


def _rand16(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float16)


WG = _geoms() + [("flow_conv1_c6", 2, 6, 480, 640, 64, 7, 2, 3), ("flow_conv1_c10", 2, 10, 480, 640, 64, 7, 2, 3)]


@pytest.mark.parametrize("case", WG, ids=[c[0] for c in WG])
def test_wgrad_f16_against_float64_sum_of_the_same_operands(ctx, case):
    name, B, cin, H, W, cout, k, s, p = case
    cpad = (cin + 7) // 8 * 8
    ho, wo = _out_hw(H, W, k, s, p)
    rng = np.random.default_rng(cin + cout + k)
    x = _rand16(rng, (B, H, W, cpad))
    x[..., cin:] = 0
    dz = _rand16(rng, (B, ho, wo, cout), 64.0)
    S = 256.0
    ref = torch.nn.grad.conv2d_weight(torch.from_numpy(x[..., :cin].astype(np.float64)).permute(0, 3, 1, 2), (cout, cin, k, k),
                                      torch.from_numpy(dz.astype(np.float64)).permute(0, 3, 1, 2), stride=s, padding=p).numpy() / S
    h = ctx.handle
    st = _state(ctx, S)
    xd, zd = ctx.array(x, np.float16), ctx.array(dz, np.float16)
    dw = ctx.empty((cout, cin, k, k))
    assert lib.deepim_conv2d_wgrad_f16(h, dw, xd, zd, st, B, cin, cpad, H, W, cout, k, s, p, 0) == 0
    got = dw.asnumpy()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err < 1e-5, err
    # tap-major layout (what the SGD table reads in place) = the natural one permuted; deterministic
    tm = ctx.empty((cout, k * k, cin))
    lib.deepim_conv2d_wgrad_f16(h, tm, xd, zd, st, B, cin, cpad, H, W, cout, k, s, p, 1)
    np.testing.assert_array_equal(tm.asnumpy(), got.reshape(cout, cin, k * k).transpose(0, 2, 1))
    assert st.asnumpy()[2] == 0


DG = [g for g in _geoms() if g[0] != "flow_conv1"]


@pytest.mark.parametrize("case", DG, ids=[c[0] for c in DG])
def test_dgrad_f16_within_one_fp16_rounding_of_float64(ctx, case):
    name, B, cin, H, W, cout, k, s, p = case
    ho, wo = _out_hw(H, W, k, s, p)
    rng = np.random.default_rng(cin * 3 + cout + k)
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    dz = _rand16(rng, (B, ho, wo, cout))
    ref = torch.nn.grad.conv2d_input((B, cin, H, W), torch.from_numpy(emu.q16(w).astype(np.float64)),
                                     torch.from_numpy(dz.astype(np.float64)).permute(0, 3, 1, 2), stride=s, padding=p)
    ref = ref.permute(0, 2, 3, 1).numpy()
    h = ctx.handle
    ws = ctx.empty(((lib.load().deepim_conv_dgrad_f16_workspace_size(B, cin, H, W, cout, k, s, p) + 1) // 2,), dtype=np.float16)
    dx = ctx.array(np.full((B, H, W, cin), 7.0), np.float16)      # every element written
    assert lib.deepim_conv2d_dgrad_f16(h, dx, ctx.array(dz, np.float16), ctx.array(w), ws, B, cin, H, W, cout, k, s, p) == 0
    got = dx.asnumpy().astype(np.float64)
    # one fp16 rounding of the float64 result, plus what the fp32 accumulation may add where the sum cancels (2^-20 of the sum of
    # the magnitudes of its products: matters only near zero, where the fp16 spacing is finer than the fp32 sum)
    mag = torch.nn.grad.conv2d_input((B, cin, H, W), torch.from_numpy(np.abs(emu.q16(w)).astype(np.float64)),
                                     torch.from_numpy(np.abs(dz.astype(np.float64))).permute(0, 3, 1, 2), stride=s, padding=p)
    tol = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64) + 2.0 ** -20 * mag.permute(0, 2, 3, 1).numpy()
    bad = np.abs(got - ref) > tol
    assert not bad.any(), (int(bad.sum()), float((np.abs(got - ref) / tol).max()))


@pytest.mark.parametrize("shape", [(2, 1024, 8, 10), (2, 512, 15, 20), (1, 64, 240, 320), (3, 128, 7, 9)])
@pytest.mark.parametrize("mode", ["d", "add", "both"])
def test_lrelu_bias_backward_f16_is_its_numpy_definition(ctx, shape, mode):
    B, C, H, W = shape
    rng = np.random.default_rng(B * C + H)
    y = _rand16(rng, (B, H, W, C))
    d = _rand16(rng, (B, H, W, C), 8.0) if mode != "add" else None
    add = (rng.standard_normal((B, C, H, W)) * 1e-3).astype(np.float32) if mode != "d" else None
    S = 1024.0
    e = np.zeros((B, H, W, C), np.float32) if d is None else d.astype(np.float32)
    if add is not None:
        e = (e + np.float32(S) * add.transpose(0, 2, 3, 1)).astype(np.float32) if d is not None else \
            (np.float32(S) * add.transpose(0, 2, 3, 1)).astype(np.float32)
    dz_ref = np.where(y.astype(np.float32) > 0, e, e * np.float32(0.1)).astype(np.float32).astype(np.float16)
    db_ref = dz_ref.astype(np.float64).sum(axis=(0, 1, 2)) / S
    h = ctx.handle
    st = _state(ctx, S)
    dd = ctx.array(d, np.float16) if d is not None else None
    dz = dd if dd is not None else ctx.empty((B, H, W, C), dtype=np.float16)      # in place over d, as the training graph runs it
    db = ctx.empty((C,))
    assert lib.deepim_lrelu_bias_backward_f16(h, dz, db, dd, ctx.array(add) if add is not None else None, ctx.array(y, np.float16), st,
                                              cf(0.1), B, C, H, W) == 0
    np.testing.assert_array_equal(dz.asnumpy(), dz_ref)
    err = np.abs(db.asnumpy() - db_ref).max() / max(1e-30, np.abs(db_ref).max())
    assert err < 1e-5, err
    assert st.asnumpy()[2] == 0
    if d is not None:    # an inf in the incoming gradient raises the flag
        d2 = d.copy()
        d2[0, 0, 0, 3] = np.inf
        lib.deepim_lrelu_bias_backward_f16(h, dz, db, ctx.array(d2, np.float16), None, ctx.array(y, np.float16), st, cf(0.1), B, C, H, W)
        assert st.asnumpy()[2] == 1


def _setup(ctx, B, seed, heads, input_mask=True, input_depth=False, fp16=True):
    d = synthetic.make_batch(B, seed=seed, n_frames=1)
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = heads
    cfg.network.INPUT_MASK, cfg.network.INPUT_DEPTH = input_mask, input_depth
    cfg.network.FP16_CONV = fp16
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    params = net.init_weights(cfg, seed=91)
    net.bind_train(ctx, B, params, num_points=3000)
    pco = np.stack([d["pose_tgt"][b][:, :3].astype(np.float64) @ d["point_cloud_model"][b].astype(np.float64) + d["pose_tgt"][b][:, 3:4]
                    for b in range(B)]).astype(np.float32)
    data_np = {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][0], "mask_observed": d["mask_observed"],
               "mask_rendered": d["mask_rendered"][0], "src_pose": d["src_pose"][0]}
    if input_depth:
        data_np.update(depth_observed=d["depth_gt_observed"], depth_rendered=d["depth_rendered"][0])
    label_np = {"mask_gt_observed": (d["depth_gt_observed"] > 0).astype(np.float32), "point_cloud_model": d["point_cloud_model"],
                "point_cloud_weights": np.ones((B, 3, 3000), np.float32), "point_cloud_observed": pco}
    if heads:
        from mx_deepim_amd.lib.pair_matching import data_pair
        flow, fw = data_pair.get_pair_flow({"depth_rendered": ctx.array(d["depth_rendered"][0]),
                                            "depth_gt_observed": ctx.array(d["depth_gt_observed"]),
                                            "pose_rendered": ctx.array(d["src_pose"][0]), "pose_observed": ctx.array(d["pose_tgt"])}, cfg)
        label_np["flow"], label_np["flow_weights"] = flow.asnumpy(), fw.asnumpy()
    data = {k: ctx.array(v) for k, v in data_np.items()}
    label = {k: ctx.array(v) for k, v in label_np.items()}
    return d, cfg, net, params, data_np, label_np, data, label


def _nchw(a):
    return np.ascontiguousarray(a.asnumpy().astype(np.float32).transpose(0, 3, 1, 2))


VARIANTS = [("pose", False, True, False), ("heads", True, True, False), ("c6", False, False, False), ("c10", False, True, True)]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_training_iteration_against_the_emulation_and_the_fp32_oracle(ctx, variant):
    tag, heads, input_mask, input_depth = variant
    d, cfg, net, params, data_np, label_np, data, label = _setup(ctx, 1, 921, heads, input_mask, input_depth)
    S = net.loss_scale()["scale"]
    assert S == cfg.TRAIN.FP16_LOSS_SCALE
    loss = float(net.forward_train(data, label).asnumpy()[0])
    grads = {k: v.asnumpy() for k, v in net.backward().items()}
    assert not net.loss_scale()["overflow"]
    acts = {name: _nchw(net.act[name + "_h"]) for name, *_ in ENCODER}
    np.testing.assert_array_equal(net.act["conv6_1"].asnumpy(), acts["conv6_1"])
    t = cfg.train_iter
    odata = dict(data_np)
    if not input_mask:
        odata["mask_observed"] = odata["mask_rendered"] = None
    args = (params, odata, label_np, d["K"], MEANS_REV, cfg.dataset.trans_means, cfg.dataset.trans_stds, cfg.network.ROT_COORD,
            t.LW_PM, t.NUM_3D_SAMPLE, cfg.dataset.NORMALIZE_3D_POINT, t.SE3_PM_LOSS_TYPE, t.SE3_PM_SL1_SCALAR)
    kw = dict(pred_flow=heads, pred_mask=heads, lw_flow=t.LW_FLOW, lw_mask=t.LW_MASK, normalize_flow=cfg.dataset.NORMALIZE_FLOW)
    e_loss, g_emu, _ = emu.train_iteration(*args, S=S, acts=acts, **kw)
    assert abs(loss - e_loss) <= 1e-3 * abs(e_loss), (loss, e_loss)
    assert set(grads) == set(g_emu)
    worst = {}
    for name in sorted(g_emu):
        if name.endswith("upsampling_weight"):
            assert not grads[name].any()
            continue
        ref = g_emu[name]
        err = float(np.abs(grads[name] - ref).max() / max(1e-30, np.abs(ref).max()))
        worst[name] = err
        assert err < 2e-3, (name, err)
    # against the fp32 oracle: cosine similarity per tensor
    _, g32, _ = opipe.train_iteration(*args, **kw)
    cos = {}
    for name in sorted(g32):
        if name.endswith("upsampling_weight"):
            continue
        a, b = grads[name].astype(np.float64).ravel(), g32[name].astype(np.float64).ravel()
        cos[name] = float(a @ b / max(1e-300, np.linalg.norm(a) * np.linalg.norm(b)))
    print("\n[fp16 training %s] S = %g, loss %.6g vs emulation %.6g; worst gradient error vs emulation %s = %.3g; lowest cosine vs fp32 "
          "%s = %.5f" % (tag, S, loss, e_loss, max(worst, key=worst.get), max(worst.values()), min(cos, key=cos.get), min(cos.values())))
    for name in sorted(cos):
        print("  %-26s err_emu %.2e  cos_fp32 %.6f" % (name, worst[name], cos[name]))
    assert min(cos.values()) >= 0.99, cos


def test_overflow_skips_the_step_and_the_scale_follows_the_window(ctx):
    d, cfg, net, params, data_np, label_np, data, label = _setup(ctx, 1, 922, True)
    net.forward_train(data, label)
    net.backward()
    net.update(lr=1e-3)                                      # one real step, so that the momenta are not all zero
    assert not net.loss_scale()["overflow"]
    st = np.zeros(4, np.uint32)
    st[:2] = np.array([2.0 ** 60, 2.0 ** -60], np.float32).view(np.uint32)   # numerically huge: S·e leaves fp16's range
    net.amp_state.copyfrom(st)
    net.forward_train(data, label)
    net.backward()
    assert net.loss_scale()["overflow"]
    w0 = {k: v.asnumpy() for k, v in net.params.items()}
    m0 = {k: v.asnumpy() for k, v in net.mom.items()}
    net.update(lr=1e-3)
    for k in w0:
        np.testing.assert_array_equal(net.params[k].asnumpy(), w0[k], err_msg=k)
        np.testing.assert_array_equal(net.mom[k].asnumpy(), m0[k], err_msg=k)
    ls = net.loss_scale()
    assert ls["scale"] == 2.0 ** 59 and ls["inv_scale"] == 2.0 ** -59 and not ls["overflow"] and ls["good_steps"] == 0
    # window 2: two clean steps double the scale
    net.loss_scale_window = 2
    net.set_loss_scale(1024.0)
    for i in range(2):
        net.forward_train(data, label)
        net.backward()
        assert not net.loss_scale()["overflow"]
        net.update(lr=1e-3)
        assert net.loss_scale()["scale"] == (1024.0 if i == 0 else 2048.0)
    assert net.loss_scale()["good_steps"] == 0
    assert not np.array_equal(net.params["conv3_weight"].asnumpy(), w0["conv3_weight"])


def test_training_reduces_all_three_losses_and_the_full_step_runs(ctx):
    """Six SGD steps on one fixed batch (B = 2): point-matching, flow and mask losses all go down; then the reference's whole step
    (TRAIN_ITER_SIZE = 4 iterations, device batch updater between them) stays finite."""
    from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import batchUpdaterPyMulti
    from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
    B = 2
    d, cfg, net, params, data_np, label_np, data, label = _setup(ctx, B, 77, True)

    def losses():
        pm = net.forward_train(data, label).asnumpy()[0]
        p, y = net.act["mask_prob"].asnumpy().astype(np.float64), net.act["zoom_mask_gt_observed"].asnumpy()
        bce = float(-(y * np.log(p + 1e-12) + (1 - y) * np.log(1 - p + 1e-12)).mean())
        return float(pm), float(net.act["flow_loss_sum"].asnumpy()[0]), bce

    first = losses()
    for _ in range(6):
        net.backward()
        net.update(lr=2e-3, wd=cfg.TRAIN.wd, momentum=0.5)
        last = losses()
    assert all(np.isfinite(last))
    assert last[0] < first[0] and last[1] < first[1] and last[2] < first[2], (first, last)
    assert not net.loss_scale()["overflow"]
    mesh = synthetic.ellipsoid_mesh([0.05, 0.04, 0.035], 24, 48)
    mesh.pop("uv")
    rm = Render_Py("unused", ["obj"], d["K"], 640, 480, meshes={"obj": mesh}, ctx=ctx, pixel_means=MEANS_REV.copy())
    upd = batchUpdaterPyMulti(cfg, 480, 640, render_machine=rm)
    data.update(tgt_pose=ctx.array(d["pose_tgt"]), depth_gt_observed=ctx.array(d["depth_gt_observed"]))
    assert cfg.network.TRAIN_ITER_SIZE == 4
    seen = []
    net.train_step(data, label, upd, lr=1e-4, on_iter=lambda it, dat, lab: seen.append(
        (float(net.act["pm_loss_sum"].asnumpy()[0]), float(net.act["flow_loss_sum"].asnumpy()[0]))))
    assert len(seen) == 4 and np.all(np.isfinite(seen)), seen
    assert all(np.isfinite(v.asnumpy()).all() for v in net.params.values())
