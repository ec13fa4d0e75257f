"""§8f-4e — split-fp16 training (TRAIN.X3_CONV) on the GPU: the x3 weight-gradient, data-gradient and fused activation-gradient
kernels against the oracle on the values of the same pairs; one training iteration against the oracle differentiated at the GPU's own
activations, against the unpatched oracle and against the plain fp16 mode on the same batch; the scale state (overflow skip, halving,
doubling); the re-pack, a full TRAIN_ITER_SIZE = 4 step, determinism; and that a default training net binds nothing of the mode.
Figures: none recorded yet — the wgrad and dgrad tests have passed on an MI355X, the rest has not run there
(profiles/r12_x3_train.md); the bars are the issue's, set before any run."""
import ctypes

import numpy as np
import pytest

import fp16_train_emulation as emu16
import x3_train_emulation as emu
from oracle import net as onet
from oracle import pipeline as opipe
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import DeviceArray, lib
from mx_deepim_amd.symbols import deepIM_flownet
from mx_deepim_amd.symbols.deepIM_flownet import ENCODER, _out_hw

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
f32 = np.float32
MEANS_REV = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])
ACT = 16.0


def _geoms(B, cin0=8, H=480, W=640):
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


def _to_split16(v, scale):
    """(B,C,H,W) fp32 -> split16 records (B,H,W,2C) fp16: per 16 channels [hi 16 | lo 16] of v·scale."""
    B, C, H, W = v.shape
    hi, lo = emu.split(v, scale)
    rec = np.stack([a.transpose(0, 2, 3, 1).reshape(B, H, W, C // 16, 16) for a in (hi, lo)], axis=4)
    return np.ascontiguousarray(rec.reshape(B, H, W, 2 * C)).astype(np.float16)


def _from_split16(a, scale=1.0):
    """split16 records (B,H,W,2C) -> the pair values (B,C,H,W) fp32: (hi + lo) / scale."""
    B, H, W, C2 = a.shape
    rec = a.reshape(B, H, W, C2 // 32, 2, 16).astype(f32)
    v = ((rec[..., 0, :] + rec[..., 1, :]).astype(f32) * f32(1.0 / scale)).astype(f32)
    return np.ascontiguousarray(v.reshape(B, H, W, C2 // 2).transpose(0, 3, 1, 2))


def _gradient_like(rng, shape, top, octaves=8.0):
    """Random signs, magnitudes spread over `octaves` octaves below `top`, one element at `top` itself."""
    v = (rng.choice([-1.0, 1.0], shape) * top * 2.0 ** -rng.uniform(0.0, octaves, shape)).astype(f32)
    v.flat[0] = top
    return v


def _wgrad_x3(ctx, case, x, dz_scaled, S):
    """The weight gradient of the training graph's route for this layer -> (natural (Cout,Cin,k,k), tap-major or None, overflow)."""
    name, B, cin, H, W, cout, k, s, p = case
    ho, wo = _out_hw(H, W, k, s, p)
    h, st = ctx.handle, _state(ctx, S)
    zd = ctx.array(_to_split16(dz_scaled, 1.0), np.float16)
    if cin % 16:      # conv1: dz in real units as NCHW fp32, then the fp32 weight gradient from the NCHW input
        dzf = ctx.empty((B, cout, ho, wo))
        assert lib.deepim_split16_to_nchw_f32_unscaled(h, dzf, zd, st, B, cout, ho, wo, cf(1.0)) == 0
        tm = ctx.empty((cout, k * k, cin))
        assert lib.deepim_conv2d_wgrad_tm(h, tm, ctx.array(x), dzf, B, cin, H, W, cout, k, k, s, p) == 0
        nat = ctx.empty((cout, cin, k, k))
        lib.deepim_weight_grad_to_natural(h, nat, tm, cout, cin, k * k)
        return nat.asnumpy(), tm.asnumpy(), int(st.asnumpy()[2])
    xd = ctx.array(_to_split16(x, ACT), np.float16)
    dw, tm = ctx.empty((cout, cin, k, k)), ctx.empty((cout, k * k, cin))
    assert lib.deepim_conv2d_wgrad_x3(h, dw, xd, zd, st, B, cin, H, W, cout, k, s, p, 0, cf(ACT)) == 0
    assert lib.deepim_conv2d_wgrad_x3(h, tm, xd, zd, st, B, cin, H, W, cout, k, s, p, 1, cf(ACT)) == 0
    return dw.asnumpy(), tm.asnumpy(), int(st.asnumpy()[2])


WG = _geoms(2)


@pytest.mark.parametrize("case", WG, ids=[c[0] for c in WG])
def test_wgrad_x3_against_the_oracle_on_the_pair_values(ctx, case):
    """Every encoder geometry at B = 2, both output layouts; flow_conv1 (Cin = 8, below one split16 record) by the route the training
    graph takes for it. Reference: the oracle's conv2d_backward (float64 sums) of the values the pairs carry. Operands inside the
    window: activations O(1) at scale 16, S·dz up to 200."""
    name, B, cin, H, W, cout, k, s, p = case
    ho, wo = _out_hw(H, W, k, s, p)
    rng = np.random.default_rng(cin + cout + k)
    x = rng.standard_normal((B, cin, H, W)).astype(f32)
    x = np.where(x > 0, x, 0.1 * x).astype(f32)
    S = 4096.0
    dz = _gradient_like(rng, (B, cout, ho, wo), 200.0)                     # already scaled by S
    xq = x if cin % 16 else emu.pair_value(x, ACT)
    ref = onet.conv2d_backward(xq, np.zeros((cout, cin, k, k), f32), emu.pair_value(dz, 1.0), s, p, need_dx=False)[1].astype(np.float64) / S
    got, tm, flag = _wgrad_x3(ctx, case, x, dz, S)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("\n[x3 wgrad %s] %.3g of the tensor maximum" % (name, err))
    assert err <= 1e-5, err
    # tap-major layout (what the SGD table reads in place) = the natural one permuted; deterministic
    np.testing.assert_array_equal(tm, got.reshape(cout, cin, k * k).transpose(0, 2, 1))
    assert flag == 0


def test_wgrad_x3_carries_small_gradients_once_scaled(ctx):
    """dz spanning 1e-6 … 1e-2 before scaling (conv3_1's geometry): S = 2^14 lifts it to 0.016 … 164, inside the window."""
    case = [c for c in WG if c[0] == "conv3_1"][0]
    name, B, cin, H, W, cout, k, s, p = case
    ho, wo = _out_hw(H, W, k, s, p)
    rng = np.random.default_rng(77)
    x = rng.standard_normal((B, cin, H, W)).astype(f32)
    x = np.where(x > 0, x, 0.1 * x).astype(f32)
    dz = (rng.choice([-1.0, 1.0], (B, cout, ho, wo)) * 10.0 ** rng.uniform(-6.0, -2.0, (B, cout, ho, wo))).astype(f32)
    S = 2.0 ** 14
    dzs = (dz * f32(S)).astype(f32)
    ref = onet.conv2d_backward(emu.pair_value(x, ACT), np.zeros((cout, cin, k, k), f32), dz, s, p, need_dx=False)[1].astype(np.float64)
    got, _, flag = _wgrad_x3(ctx, case, x, dzs, S)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("\n[x3 wgrad, dz 1e-6 … 1e-2, S = 2^14] %.3g of the tensor maximum" % err)
    assert err <= 1e-5 and flag == 0, (err, flag)


def _dgrad_x3(ctx, case, w, dz_scaled, ws_scale):
    """The data gradient by the training graph's route for this layer -> (pair values (B,Cin,H,W), overflow word)."""
    name, B, cin, H, W, cout, k, s, p = case
    ho, wo = _out_hw(H, W, k, s, p)
    h, st = ctx.handle, _state(ctx, 1.0)
    zd = ctx.array(_to_split16(dz_scaled, 1.0), np.float16)
    dx = ctx.array(np.full((B, H, W, 2 * cin), 7.0), np.float16)          # every element written
    if cin % 128:     # conv2: 64 output channels, below the x3 kernel's 128 → the fp32 data gradient over converted tensors
        dzf, dxf = ctx.empty((B, cout, ho, wo)), ctx.empty((B, cin, H, W))
        lib.deepim_split16_to_nchw_f32(h, dzf, zd, B, cout, ho, wo, cf(1.0))
        wt = ctx.empty((lib.load().deepim_conv_dgrad_packed_size(cout, cin, k, s, p) // 4 + lib.load().deepim_conv_packed_size(cin, cout, k, k) // 4,))
        lib.deepim_conv2d_dgrad(h, dxf, dzf, ctx.array(w), wt, B, cin, H, W, cout, k, s, p, None, None, cf(0.1))
        lib.deepim_nchw_f32_to_split16(h, dx, dxf, B, cin, H, W, cf(1.0))
        lib.deepim_x3_status_to_state(h, st)
    else:
        wsz = lib.load().deepim_conv_dgrad_x3_workspace_size(B, cin, H, W, cout, k, s, p)
        ws = ctx.empty(((wsz + 1) // 2,), dtype=np.float16)
        assert lib.deepim_conv2d_dgrad_x3(h, dx, zd, ctx.array(w), ws, st, B, cin, H, W, cout, k, s, p, cf(ws_scale)) == 0
    return _from_split16(dx.asnumpy()), int(st.asnumpy()[2])


DG = [g for B in (2, 4) for g in _geoms(B) if g[0] != "flow_conv1"]


@pytest.mark.parametrize("case", DG, ids=["%s-B%d" % (c[0], c[1]) for c in DG])
def test_dgrad_x3_against_the_oracle_on_the_pair_values(ctx, case):
    """Every geometry that has a data gradient (stride 2 and conv2's 64-channel output included) at B = 2 and B = 4, within 1e-5 of
    its range of the oracle's float64-accumulating data gradient of the pair values."""
    name, B, cin, H, W, cout, k, s, p = case
    ho, wo = _out_hw(H, W, k, s, p)
    rng = np.random.default_rng(cin * 3 + cout + k + B)
    w = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(f32)
    dz = _gradient_like(rng, (B, cout, ho, wo), 200.0)
    sw = emu.weight_scale(w)
    wq = w if cin % 128 else emu.pair_value(w, sw)
    ref = onet.conv2d_backward(np.zeros((B, cin, H, W), f32), wq, emu.pair_value(dz, 1.0), s, p)[0].astype(np.float64)
    got, flag = _dgrad_x3(ctx, case, w, dz, sw)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("\n[x3 dgrad %s B=%d] %.3g of the range" % (name, B, err))
    assert err <= 1e-5, err
    assert flag == 0


PK = [(256, 256, 3), (512, 256, 3), (256, 128, 5), (1024, 1024, 3)]


@pytest.mark.parametrize("case", PK)
def test_dgrad_pack_is_the_pack_of_the_transposed_flipped_weights(ctx, case):
    cout, cin, k = case
    rng = np.random.default_rng(cout + cin + k)
    w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(f32)
    sw = emu.weight_scale(w)
    h, st = ctx.handle, _state(ctx, 1.0)
    n = lib.load().deepim_conv_x3_packed_size(cin, cout, k, k) // 2
    a, b = DeviceArray(ctx, (n,), dtype=np.float16), DeviceArray(ctx, (n,), dtype=np.float16)
    assert lib.deepim_conv_x3_pack_dgrad(h, a, ctx.array(w), st, cout, cin, k, 0, 0, 1, k, k, cf(sw)) == 0
    wt = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
    lib.deepim_conv_x3_pack_weights(h, b, ctx.array(wt), cin, cout, k, k, cf(sw))
    np.testing.assert_array_equal(a.asnumpy().view(np.uint16), b.asnumpy().view(np.uint16))
    assert st.asnumpy()[2] == 0
    # a scale the weights do not fit (max |w|·sw is in [768, 1536], so 128 sw puts it at 98304 or more, past the clamp at 60000):
    # clamped, and the overflow word says so
    lib.deepim_conv_x3_pack_dgrad(h, a, ctx.array(w), st, cout, cin, k, 0, 0, 1, k, k, cf(sw * 128.0))
    assert st.asnumpy()[2] == 1


@pytest.mark.parametrize("shape", [(2, 1024, 8, 10), (2, 512, 15, 20), (1, 64, 240, 320), (3, 128, 7, 9)])
@pytest.mark.parametrize("mode", ["d", "add", "both"])
def test_lrelu_bias_backward_x3_is_its_numpy_definition(ctx, shape, mode):
    B, C, H, W = shape
    rng = np.random.default_rng(B * C + H)
    y = rng.standard_normal((B, C, H, W)).astype(f32)
    d = _gradient_like(rng, (B, C, H, W), 150.0) if mode != "add" else None
    add = (rng.standard_normal((B, C, H, W)) * 1e-3).astype(f32) if mode != "d" else None
    S = 1024.0
    ys, ds = _to_split16(y, ACT), (_to_split16(d, 1.0) if d is not None else None)
    e = np.zeros((B, C, H, W), f32) if d is None else _from_split16(ds)            # hi + lo in fp32
    if add is not None:
        e = (e + (f32(S) * add).astype(f32)).astype(f32) if d is not None else (f32(S) * add).astype(f32)
    yhi = emu.split(y, ACT)[0]
    t = np.where(yhi > 0, e, (e * f32(0.1)).astype(f32)).astype(f32)
    dz_ref = _to_split16(t, 1.0)
    db_ref = _from_split16(dz_ref).astype(np.float64).sum(axis=(0, 2, 3)) / S
    h, st = ctx.handle, _state(ctx, S)
    dd = ctx.array(ds, np.float16) if ds is not None else None
    dz = dd if dd is not None else ctx.empty((B, H, W, 2 * C), dtype=np.float16)   # in place over d, as the training graph runs it
    db = ctx.empty((C,))
    addd = ctx.array(add) if add is not None else None
    assert lib.deepim_lrelu_bias_backward_x3(h, dz, db, dd, addd, ctx.array(ys, np.float16), st, cf(0.1), B, C, H, W) == 0
    np.testing.assert_array_equal(dz.asnumpy().view(np.uint16), dz_ref.view(np.uint16))
    err = np.abs(db.asnumpy() - db_ref).max() / max(1e-30, np.abs(db_ref).max())
    assert err < 1e-5, err
    assert st.asnumpy()[2] == 0
    if add is not None:    # a gradient the scale does not hold raises the flag (and is clamped, not inf)
        a2 = add.copy()
        a2[0, 3, 0, 0] = 1e9
        d2 = ctx.array(ds, np.float16) if ds is not None else None
        out = d2 if d2 is not None else dz
        lib.deepim_lrelu_bias_backward_x3(h, out, db, d2, ctx.array(a2), ctx.array(ys, np.float16), st, cf(0.1), B, C, H, W)
        assert st.asnumpy()[2] == 1
        assert np.isfinite(out.asnumpy().astype(f32)).all()


def _setup(ctx, B, seed, heads, mode="x3"):
    d = synthetic.make_batch(B, seed=seed, n_frames=1)
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = heads
    cfg.TRAIN.X3_CONV = mode == "x3"
    cfg.network.FP16_CONV = mode == "fp16"
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    params = net.init_weights(cfg, seed=91)
    net.bind_train(ctx, B, params, num_points=3000)
    pco = np.stack([d["pose_tgt"][b][:, :3].astype(np.float64) @ d["point_cloud_model"][b].astype(np.float64) + d["pose_tgt"][b][:, 3:4]
                    for b in range(B)]).astype(np.float32)
    data_np = {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][0], "mask_observed": d["mask_observed"],
               "mask_rendered": d["mask_rendered"][0], "src_pose": d["src_pose"][0]}
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


def _worst(grads, ref):
    out = {}
    for name in sorted(ref):
        if name.endswith("upsampling_weight"):
            assert not grads[name].any()
            continue
        out[name] = float(np.abs(grads[name] - ref[name]).max() / max(1e-30, np.abs(ref[name]).max()))
    return out


@pytest.mark.parametrize("heads", [False, True], ids=["pose", "heads"])
def test_training_iteration_at_batch_4(ctx, heads):
    """One iteration at B = 4. Forward: every layer within 1e-5 of its maximum of the oracle. Backward against the oracle
    differentiated at the GPU's own activations: loss within 1e-4, every parameter gradient within 2e-4 of its maximum (the bars of
    §8f-4 / §8f-4d). Against the unpatched oracle: cosine >= 0.99 per gradient. And against the emulation of the contract fed the
    GPU's activations, the largest gradient error is at most a tenth of what the plain fp16 mode shows against ITS emulation on the
    same batch: the lo terms are in the sums."""
    B, seed = 4, 921
    d, cfg, net, params, data_np, label_np, data, label = _setup(ctx, B, seed, heads)
    S = net.loss_scale()["scale"]
    assert S == cfg.TRAIN.X3_GRAD_SCALE
    loss = float(net.forward_train(data, label).asnumpy()[0])
    grads = {k: v.asnumpy() for k, v in net.backward().items()}
    assert not net.loss_scale()["overflow"]
    acts = {name: _from_split16(net.act[name + "_x"].asnumpy(), ACT) for name, *_ in ENCODER}
    np.testing.assert_array_equal(net.act["conv6_1"].asnumpy(), acts["conv6_1"])
    t = cfg.train_iter
    args = (params, data_np, label_np, d["K"], MEANS_REV, cfg.dataset.trans_means, cfg.dataset.trans_stds, cfg.network.ROT_COORD,
            t.LW_PM, t.NUM_3D_SAMPLE, cfg.dataset.NORMALIZE_3D_POINT, t.SE3_PM_LOSS_TYPE, t.SE3_PM_SL1_SCALAR)
    kw = dict(pred_flow=heads, pred_mask=heads, lw_flow=t.LW_FLOW, lw_mask=t.LW_MASK, normalize_flow=cfg.dataset.NORMALIZE_FLOW)
    tag = "heads" if heads else "pose"
    # the unpatched oracle: forward per layer, cosine per gradient
    loss32, g32, f32w = opipe.train_iteration(*args, **kw)
    for name, *_ in ENCODER:
        err = float(np.abs(acts[name].astype(np.float64) - f32w[name]).max() / np.abs(f32w[name]).max())
        assert err <= 1e-5, (name, err)
    cos, rel = {}, {}
    for name in sorted(g32):
        if name.endswith("upsampling_weight"):
            continue
        a, b = grads[name].astype(np.float64).ravel(), g32[name].astype(np.float64).ravel()
        cos[name] = float(a @ b / max(1e-300, np.linalg.norm(a) * np.linalg.norm(b)))
        rel[name] = float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))
    # the oracle differentiated at the GPU's own activations (identity split: plain fp32 arithmetic, S = 1)
    o_loss, g_o, _ = emu.train_iteration(*args, split_value=emu.identity, S=1.0, acts=acts, **kw)
    assert abs(loss - o_loss) <= 1e-4 * abs(o_loss), (loss, o_loss)
    assert set(grads) == set(g_o)
    worst_o = _worst(grads, g_o)
    # the emulation of the contract at the same activations
    e_loss, g_e, fe = emu.train_iteration(*args, S=S, acts=acts, **kw)
    assert not fe["overflow"]
    worst_e = _worst(grads, g_e)
    dzmax = {name: float(np.abs(fe["dz_" + name]).max()) for name, *_ in ENCODER}
    # the plain fp16 mode on the same batch against its own emulation
    del net
    d2, cfg2, net16, params2, _, _, data2, label2 = _setup(ctx, B, seed, heads, mode="fp16")
    S16 = net16.loss_scale()["scale"]
    net16.forward_train(data2, label2)
    g16 = {k: v.asnumpy() for k, v in net16.backward().items()}
    assert not net16.loss_scale()["overflow"]
    acts16 = {name: np.ascontiguousarray(net16.act[name + "_h"].asnumpy().astype(f32).transpose(0, 3, 1, 2)) for name, *_ in ENCODER}
    _, g16e, _ = emu16.train_iteration(*args, S=S16, acts=acts16, **kw)
    worst16 = _worst(g16, g16e)
    print("\n[x3 training %s B=%d] S = %g, loss %.8g vs oracle at the GPU's activations %.8g (fp32 oracle %.8g)" % (tag, B, S, loss, o_loss, loss32))
    print("  largest gradient error vs the oracle at the GPU's activations: %s = %.3g" % (max(worst_o, key=worst_o.get), max(worst_o.values())))
    print("  largest gradient error vs the emulation: x3 %s = %.3g, plain fp16 %s = %.3g" % (
        max(worst_e, key=worst_e.get), max(worst_e.values()), max(worst16, key=worst16.get), max(worst16.values())))
    print("  vs the unpatched oracle: lowest cosine %s = %.7f, largest relative deviation %s = %.3g" % (
        min(cos, key=cos.get), min(cos.values()), max(rel, key=rel.get), max(rel.values())))
    for name, *_ in ENCODER:
        print("  %-12s max |S dz| %.4g (max |dz| %.4g)  dW err_oracle %.2e err_emu %.2e fp16 %.2e cos_fp32 %.7f" % (
            name, dzmax[name], dzmax[name] / S, worst_o[name + "_weight"], worst_e[name + "_weight"], worst16[name + "_weight"],
            cos[name + "_weight"]))
    for name in sorted(worst_o):
        assert worst_o[name] <= 2e-4, (name, worst_o[name])
    assert min(cos.values()) >= 0.99, cos
    assert max(worst_e.values()) <= 0.1 * max(worst16.values()), (max(worst_e.values()), max(worst16.values()))


def test_overflow_skips_the_step_and_the_scale_follows_the_window(ctx):
    d, cfg, net, params, data_np, label_np, data, label = _setup(ctx, 1, 922, True)
    net.forward_train(data, label)
    net.backward()
    net.update(lr=1e-3)                                      # one real step, so that the momenta are not all zero
    assert not net.loss_scale()["overflow"]
    st = np.zeros(4, np.uint32)
    st[:2] = np.array([2.0 ** 60, 2.0 ** -60], np.float32).view(np.uint32)   # numerically huge: S·e leaves the pairs' range
    net.amp_state.copyfrom(st)
    net.forward_train(data, label)
    net.backward()
    assert net.loss_scale()["overflow"]
    assert all(np.isfinite(v.asnumpy()).all() for v in net.grad.values())      # clamped and flagged, never inf
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


def test_a_clamp_in_the_forward_reaches_the_scale_state_on_the_device(ctx):
    """The x3 forward kernels report saturation through the context's status word; the backward moves the bit into the scale state."""
    d, cfg, net, params, data_np, label_np, data, label = _setup(ctx, 1, 923, False)
    b = net.params["conv3_bias"].asnumpy()
    b[5] = 1e6                                               # 1e6 · 16 leaves fp16's range: conv3's output is clamped
    net.params["conv3_bias"].copyfrom(b)
    net.forward_train(data, label)
    net.backward()
    assert net.loss_scale()["overflow"]
    st = ctypes.c_int(0)
    lib.deepim_zoom_status(ctx.handle, ctypes.byref(st))
    assert not st.value & 8                                  # the scale state carries it now


def test_update_repacks_training_reduces_the_losses_and_runs_are_bit_identical(ctx):
    """update() leaves packed_x3 equal to a fresh pack of the updated masters; six SGD steps on one fixed batch (B = 2) bring the
    point-matching, flow and mask losses down; the reference's whole step (TRAIN_ITER_SIZE = 4, device batch updater between the
    iterations) stays finite; two runs of an iteration give the same bits."""
    from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import batchUpdaterPyMulti
    from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
    B = 2
    d, cfg, net, params, data_np, label_np, data, label = _setup(ctx, B, 77, True)
    h = ctx.handle

    def losses():
        pm = net.forward_train(data, label).asnumpy()[0]
        p, y = net.act["mask_prob"].asnumpy().astype(np.float64), net.act["zoom_mask_gt_observed"].asnumpy()
        bce = float(-(y * np.log(p + 1e-12) + (1 - y) * np.log(1 - p + 1e-12)).mean())
        return float(pm), float(net.act["flow_loss_sum"].asnumpy()[0]), bce

    # determinism: the same iteration twice, bit for bit
    net.forward_train(data, label)
    g1 = {k: v.asnumpy() for k, v in net.backward().items()}
    net.forward_train(data, label)
    g2 = {k: v.asnumpy() for k, v in net.backward().items()}
    for k in g1:
        np.testing.assert_array_equal(g1[k], g2[k], err_msg=k)
    first = losses()
    for _ in range(6):
        net.backward()
        net.update(lr=2e-3, wd=cfg.TRAIN.wd, momentum=0.5)
        last = losses()
    assert all(np.isfinite(last))
    assert last[0] < first[0] and last[1] < first[1] and last[2] < first[2], (first, last)
    assert not net.loss_scale()["overflow"]
    # packed_x3 = a fresh pack of the updated masters at the bind-time scales
    cin = 64
    name0 = ENCODER[0][0]
    fresh = DeviceArray(ctx, (lib.load().deepim_conv1_x3_packed_size() // 2,), dtype=np.float16)
    lib.deepim_conv1_x3_pack_weights(h, fresh, net.params[name0 + "_weight"], cf(net.x3_wscale[name0]))
    np.testing.assert_array_equal(net.packed_x3[name0].asnumpy().view(np.uint16), fresh.asnumpy().view(np.uint16))
    assert not np.array_equal(net.params[name0 + "_weight"].asnumpy(), params[name0 + "_weight"])
    for name, cout, k, s_, p_ in ENCODER[1:]:
        fresh = DeviceArray(ctx, (lib.load().deepim_conv_x3_packed_size(cout, cin, k, k) // 2,), dtype=np.float16)
        lib.deepim_conv_x3_pack_weights(h, fresh, net.params[name + "_weight"], cout, cin, k, k, cf(net.x3_wscale[name]))
        np.testing.assert_array_equal(net.packed_x3[name].asnumpy().view(np.uint16), fresh.asnumpy().view(np.uint16), err_msg=name)
        cin = cout
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
    assert not net.loss_scale()["overflow"]


def test_a_weight_that_outgrows_its_scale_raises_the_overflow_word(ctx):
    d, cfg, net, params, data_np, label_np, data, label = _setup(ctx, 1, 924, False)
    net.forward_train(data, label)
    net.backward()
    w = net.params["conv4_weight"].asnumpy()
    w[0, 0, 0, 0] = 100.0 * 60000.0 / net.x3_wscale["conv4"]
    net.params["conv4_weight"].copyfrom(w)
    net.update(lr=0.0, wd=0.0)
    assert net.loss_scale()["overflow"]                      # set by the re-pack, after the scale step cleared the word


def test_a_default_training_net_binds_nothing_of_the_mode(ctx):
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = False
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    net.bind_train(ctx, 1, net.init_weights(cfg, seed=91), num_points=3000)
    assert not net.train_x3 and not net.x3_conv
    assert not hasattr(net, "packed_x3") and not hasattr(net, "amp_state") and not hasattr(net, "x3_wscale")
    assert not any(k.startswith("gx3") or k == "dgradx3" for k in net.ws)
    assert not any(k.endswith("_x") for k in net.act)
