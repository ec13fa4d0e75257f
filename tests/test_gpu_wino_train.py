"""§8f-4d — fp32 Winograd training (TRAIN.WINOGRAD_CONV) on the GPU: the three kernels that carry its layout contract, through the C
ABI, and the training graph built on them.
  * deepim_conv2d_wino_dgrad against the oracle's data gradient: <= 1e-5 of the range (the Winograd bar of DESIGN.md §4);
  * deepim_lrelu_bias_backward_nc8 and deepim_conv2d_wgrad_tm_nc8 against the NCHW kernels they stand in for: bit-identical
    (only loads and stores differ), the bias gradient within the bar of test_lrelu_bias_backward_equals_the_separate_passes;
  * one training iteration at B = 4 (every Winograd form except the 3x3 stride-2 one) and one at B = 8 (that one too) against the
    oracle, the per-step re-pack, a few SGD steps, a chained train_step.
close() = max |diff| / max |ref| as in tests/test_gpu_backward.py."""
import ctypes

import numpy as np
import pytest

from oracle import net as onet
from oracle import pipeline as opipe
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import DeviceArray, lib
from mx_deepim_amd.symbols import deepIM_flownet
from mx_deepim_amd.symbols.deepIM_flownet import ENCODER

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
MEANS_REV = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])
SLOPE = 0.1


def rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(1e-30, float(np.abs(ref).max()))


def to_nc8(ctx, x, mode):
    """NCHW numpy tensor -> device tensor in NC8 (mode 1) or NC8 space-to-depth order (mode 3)."""
    B, C, H, W = x.shape
    dst = ctx.empty(x.shape)
    if mode == 3:
        lib.deepim_relayout_nc8_s2d(ctx.handle, dst, ctx.array(x), B, C, H, W, 1)
    else:
        lib.deepim_relayout_nc8(ctx.handle, dst, ctx.array(x), B, C, H * W, 1)
    return dst


# ------------------------------------------------------------------------------------------- piece 3: Winograd data gradient
# (B, Cin, H, W, Cout) of the LAYER: the four 3x3 stride-1 encoder geometries at B = 2 and 4, and one Cin != Cout
DGRAD_CASES = [(B, c, h, w, c) for B in (2, 4) for c, h, w in ((256, 60, 80), (512, 30, 40), (512, 15, 20), (1024, 8, 10))] + \
              [(2, 128, 30, 40, 256)]


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_wino_dgrad_matches_oracle(ctx, case):
    B, cin, H, W, cout = case
    rng = np.random.default_rng(sum(case))
    w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    dz = rng.standard_normal((B, cout, H, W)).astype(np.float32)
    ref = np.asarray(onet.conv2d_backward(np.zeros((B, cin, H, W), np.float32), w, dz, 1, 1)[0], np.float64)
    h, L = ctx.handle, lib.load()
    pk = DeviceArray(ctx, (L.deepim_conv_wino_packed_size(cin, cout) // 4,))
    lib.deepim_conv_wino_pack_weights_dgrad(h, pk, ctx.array(w), cout, cin)
    dx = ctx.array(np.full((B, cin, H, W), 7.0, np.float32))
    lib.deepim_conv2d_wino_dgrad(h, dx, to_nc8(ctx, dz, 1), pk, B, cin, H, W, cout)
    err = rel(dx.asnumpy(), ref)
    print("wino dgrad %s: %.3g of the range" % (case, err))
    assert err <= 1e-5, err
    dx2 = ctx.empty((B, cin, H, W))                       # deterministic
    lib.deepim_conv2d_wino_dgrad(h, dx2, to_nc8(ctx, dz, 1), pk, B, cin, H, W, cout)
    np.testing.assert_array_equal(dx2.asnumpy(), dx.asnumpy())


@pytest.mark.parametrize("shape", [(256, 256), (512, 512), (1024, 1024), (256, 128), (64, 32)])
def test_dgrad_pack_is_the_pack_of_the_flipped_weights(ctx, shape):
    cout, cin = shape
    rng = np.random.default_rng(cout + cin)
    w = ctx.array(rng.standard_normal((cout, cin, 3, 3)).astype(np.float32))
    h, L = ctx.handle, lib.load()
    n = L.deepim_conv_wino_packed_size(cin, cout) // 4
    wt = ctx.empty((cin, cout, 3, 3))
    lib.deepim_conv_flip_weights(h, wt, w, cout, cin, 3, 3)
    ref, got = DeviceArray(ctx, (n,)), DeviceArray(ctx, (n,))
    lib.deepim_conv_wino_pack_weights(h, ref, wt, cin, cout)
    lib.deepim_conv_wino_pack_weights_dgrad(h, got, w, cout, cin)
    a, b = got.asnumpy(), ref.asnumpy()
    assert np.abs(b).max() > 0
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------- piece 1: activation-gradient walk
WALK_CASES = [((4, 64, 240, 320), 1), ((4, 64, 240, 320), 3), ((2, 256, 60, 80), 1), ((2, 256, 60, 80), 3), ((2, 1024, 8, 10), 1),
              ((2, 1024, 8, 10), 3), ((1, 512, 15, 20), 1), ((2, 1024, 8, 10), 0), ((2, 16, 5, 7), 1)]


@pytest.mark.parametrize("shape,mode", WALK_CASES)
def test_lrelu_bias_backward_nc8_equals_the_nchw_walk(ctx, shape, mode):
    """dz bit-identical to deepim_lrelu_bias_backward on the NCHW copy of the same y, dz_nc8 bit-identical to the relayout of that dz,
    db within rtol 2e-6 / atol 1e-6·sqrt(B·H·W) of the float64 sum; modes 1 and 3 (and 0: y already NCHW, taken for its dz_nc8
    output on the last layer), with and without `add`, in place and out of place; an odd plane and one whose size is no multiple of four."""
    B, C, H, W = shape
    rng = np.random.default_rng(sum(shape) + mode)
    dy = rng.standard_normal(shape).astype(np.float32)
    y = rng.standard_normal(shape).astype(np.float32)
    addn = rng.standard_normal(shape).astype(np.float32)
    h = ctx.handle
    y_dev = ctx.array(y) if mode == 0 else to_nc8(ctx, y, mode)
    for with_add in (False, True):
        add = ctx.array(addn) if with_add else None
        ref, db_ref = ctx.array(dy), ctx.empty((C,))
        lib.deepim_lrelu_bias_backward(h, ref, db_ref, ref, add, ctx.array(y), cf(SLOPE), B, C, H * W)
        ref_np = ref.asnumpy()
        ref_nc8 = to_nc8(ctx, ref_np, 1).asnumpy()
        host = ref_np.astype(np.float64).sum(axis=(0, 2, 3))
        for in_place in (True, False):
            for with_nc8 in (True, False):
                src = ctx.array(dy)
                dz = src if in_place else ctx.array(np.full(shape, 9.0, np.float32))
                z8 = ctx.array(np.full(shape, 9.0, np.float32)) if with_nc8 else None
                db = ctx.array(np.full((C,), 9.0, np.float32))
                lib.deepim_lrelu_bias_backward_nc8(h, dz, z8, db, src, add, y_dev, mode, cf(SLOPE), B, C, H, W)
                np.testing.assert_array_equal(dz.asnumpy().view(np.uint32), ref_np.view(np.uint32))
                if with_nc8:
                    np.testing.assert_array_equal(z8.asnumpy().view(np.uint32), ref_nc8.view(np.uint32))
                if not in_place:
                    np.testing.assert_array_equal(src.asnumpy(), dy)
                np.testing.assert_allclose(db.asnumpy(), host, rtol=2e-6, atol=1e-6 * np.sqrt(B * H * W))


def test_lrelu_bias_backward_nc8_on_an_empty_batch(ctx):
    x = ctx.array(np.zeros((1, 8, 4, 4), np.float32))
    db = ctx.array(np.full((8,), 7.0, np.float32))
    lib.deepim_lrelu_bias_backward_nc8(ctx.handle, x, None, db, x, None, x, 1, cf(SLOPE), 0, 8, 4, 4)
    np.testing.assert_array_equal(db.asnumpy(), np.zeros(8, np.float32))


# ------------------------------------------------------------------------------------------- piece 2: weight gradient, NC8 x
def _encoder_geometries(cin=8, H=480, W=640):
    out = []
    for name, cout, k, s, p in ENCODER:
        out.append((name, cin, H, W, cout, k, s, p))
        H, W, cin = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, cout
    return out


@pytest.mark.parametrize("geom", _encoder_geometries(), ids=lambda g: g[0])
def test_wgrad_tm_nc8_is_bit_identical_to_the_nchw_kernel(ctx, geom):
    name, cin, H, W, cout, k, s, p = geom
    B = 2
    rng = np.random.default_rng(cin + H + cout + k)
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dz = ctx.array(rng.standard_normal((B, cout, ho, wo)).astype(np.float32))
    h = ctx.handle
    ref = ctx.empty((cout, k * k, cin))
    lib.deepim_conv2d_wgrad_tm(h, ref, ctx.array(x), dz, B, cin, H, W, cout, k, k, s, p)
    ref_np = ref.asnumpy()
    assert np.abs(ref_np).max() > 0
    modes = [1] + ([3] if H % 2 == 0 and W % 2 == 0 else [])
    assert modes == [1, 3] or name in ("conv5_1", "conv6")        # the odd 15x20 planes
    for mode in modes:
        xs = to_nc8(ctx, x, mode)
        for _ in range(2):                                        # deterministic on a second call
            got = ctx.array(np.full((cout, k * k, cin), 3.0, np.float32))
            lib.deepim_conv2d_wgrad_tm_nc8(h, got, xs, mode, dz, B, cin, H, W, cout, k, k, s, p)
            np.testing.assert_array_equal(got.asnumpy().view(np.uint32), ref_np.view(np.uint32))


def test_wgrad_tm_nc8_refuses_what_it_cannot_address(ctx):
    x = ctx.array(np.zeros((1, 8, 5, 4), np.float32))
    dw = ctx.empty((8, 9, 8))
    with pytest.raises(RuntimeError):
        lib.deepim_conv2d_wgrad_tm_nc8(ctx.handle, dw, x, 3, x, 1, 8, 5, 4, 8, 3, 3, 1, 1)      # odd H in space-to-depth order
    with pytest.raises(RuntimeError):
        lib.deepim_conv2d_wgrad_tm_nc8(ctx.handle, dw, x, 2, x, 1, 8, 5, 4, 8, 3, 3, 1, 1)      # no such layout


# ------------------------------------------------------------------------------------------- the training graph
def _setup(ctx, B, seed, heads, wino=True):
    """As _train_setup of tests/test_gpu_backward.py, with TRAIN.WINOGRAD_CONV."""
    d = synthetic.make_batch(B, seed=seed, n_frames=1)
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = heads
    cfg.TRAIN.WINOGRAD_CONV = wino
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    params = net.init_weights(cfg, seed=91)
    net.bind_train(ctx, B, params, num_points=3000)
    gt = (d["depth_gt_observed"] > 0).astype(np.float32)
    pco = np.stack([d["pose_tgt"][b][:, :3].astype(np.float64) @ d["point_cloud_model"][b].astype(np.float64) + d["pose_tgt"][b][:, 3:4]
                    for b in range(B)]).astype(np.float32)
    data_np = {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][0], "mask_observed": d["mask_observed"],
               "mask_rendered": d["mask_rendered"][0], "src_pose": d["src_pose"][0]}
    label_np = {"mask_gt_observed": gt, "point_cloud_model": d["point_cloud_model"],
                "point_cloud_weights": np.ones((B, 3, 3000), np.float32), "point_cloud_observed": pco}
    if heads:
        from mx_deepim_amd.lib.pair_matching import data_pair
        flow, fw = data_pair.get_pair_flow({"depth_rendered": ctx.array(d["depth_rendered"][0]),
                                            "depth_gt_observed": ctx.array(d["depth_gt_observed"]),
                                            "pose_rendered": ctx.array(d["src_pose"][0]), "pose_observed": ctx.array(d["pose_tgt"])}, cfg)
        label_np["flow"], label_np["flow_weights"] = flow.asnumpy(), fw.asnumpy()
        assert np.count_nonzero(label_np["flow_weights"]) > 1000
    return d, cfg, net, params, data_np, label_np


def _oracle(cfg, d, params, data_np, label_np, heads):
    t = cfg.train_iter
    kw = dict(pred_flow=True, pred_mask=True, lw_flow=t.LW_FLOW, lw_mask=t.LW_MASK, normalize_flow=cfg.dataset.NORMALIZE_FLOW) if heads else {}
    return opipe.train_iteration(params, data_np, label_np, d["K"], MEANS_REV, cfg.dataset.trans_means, cfg.dataset.trans_stds,
                                 cfg.network.ROT_COORD, t.LW_PM, t.NUM_3D_SAMPLE, cfg.dataset.NORMALIZE_3D_POINT, t.SE3_PM_LOSS_TYPE,
                                 t.SE3_PM_SL1_SCALAR, **kw)


def _check_forward_layer_by_layer(net, params):
    """(a) every encoder activation against the oracle's direct convolution of the GPU's own previous activation: <= 1e-5 of its range."""
    prev = net.act["net_input"].asnumpy()
    acts = {}
    for name, s, p in opipe.ENCODER:
        got = net.activation_nchw(name).asnumpy().copy()
        ref = onet.conv2d(prev, params[name + "_weight"], params[name + "_bias"], s, p, SLOPE)
        err = rel(got, np.asarray(ref, np.float64))
        print("forward %s: %.3g of the range" % (name, err))
        assert err <= 1e-5, (name, err)
        acts[name] = prev = got
    return acts


def _no_relayout_calls(monkeypatch):
    """The layout contract: no conversion pass in forward_train / backward / update except the decoder's own skip slices."""
    calls = []
    for fn in ("deepim_relayout_nc8", "deepim_relayout_nc8_s2d"):
        monkeypatch.setattr(type(lib), fn, property(lambda self, fn=fn: (lambda *a: calls.append(fn))), raising=False)
    return calls


@pytest.mark.parametrize("heads", [False, True], ids=["pose", "heads"])
def test_training_iteration_with_winograd_matches_oracle(ctx, heads, monkeypatch):
    """B = 4: conv1 F(2x2,4x4), conv2 / conv3 over the space-to-depth input, conv3_1 … conv6_1 F(2x2,3x3), all four 3x3 stride-1 data
    gradients on the Winograd kernels. (a) forward layer by layer; (b) loss and all gradients against the oracle differentiated at the
    GPU's own encoder activations; (c) every gradient's cosine against the unpatched oracle >= 0.99."""
    B = 4
    d, cfg, net, params, data_np, label_np = _setup(ctx, B, 910 if not heads else 915, heads)
    assert net.train_winograd and net.nc8 and net.wino_conv1 is not None
    assert set(net.packed_wino) == {"conv2", "conv3", "conv3_1", "conv4_1", "conv5_1", "conv6_1"} and net.wino_s2d == {"conv2", "conv3"}
    assert set(net.packed_wino_dgrad) == {"conv3_1", "conv4_1", "conv5_1", "conv6_1"} and "dz_nc8" in net.ws
    data = {k: ctx.array(v) for k, v in data_np.items()}
    label = {k: ctx.array(v) for k, v in label_np.items()}
    with monkeypatch.context() as m:
        calls = _no_relayout_calls(m)
        loss = net.forward_train(data, label).asnumpy()[0]
        grads = net.backward()
        ctx.sync()
        assert calls == [], calls
    grads = {k: v.asnumpy() for k, v in grads.items()}
    acts = _check_forward_layer_by_layer(net, params)                                           # (a)
    with monkeypatch.context() as m:                                                            # (b)
        m.setattr(opipe, "encoder", lambda p_, x_, **kw: dict(acts))
        ref_loss, g_ref, fwd = _oracle(cfg, d, params, data_np, label_np, heads)
    np.testing.assert_array_equal(net.act["net_input"].asnumpy(), fwd["net_input"])
    print("loss %r oracle %r" % (float(loss), float(ref_loss)))
    assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss)
    assert set(grads) == set(g_ref)
    worst = 0.0
    for name in sorted(g_ref):
        if name.endswith("upsampling_weight"):
            assert not grads[name].any()
            continue
        assert np.abs(g_ref[name]).max() > 0, name
        worst = max(worst, rel(grads[name], g_ref[name]))
    print("worst gradient deviation from the oracle at the GPU's activations: %.3g" % worst)
    for name in sorted(g_ref):
        if not name.endswith("upsampling_weight"):
            err = rel(grads[name], g_ref[name])
            assert err < 2e-4, (name, err)
    _, g_free, _ = _oracle(cfg, d, params, data_np, label_np, heads)                            # (c)
    cos_min, dev_max = 1.0, 0.0
    for name in sorted(g_free):
        if name.endswith("upsampling_weight"):
            continue
        a, b = grads[name].astype(np.float64).ravel(), np.asarray(g_free[name], np.float64).ravel()
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
        cos_min, dev_max = min(cos_min, cos), max(dev_max, rel(grads[name], g_free[name]))
        assert cos >= 0.99, (name, cos)
    print("against the unpatched oracle: worst cosine %.9f, worst deviation %.3g of a gradient's range" % (cos_min, dev_max))


def test_training_iteration_at_batch_8_crosses_the_stride2_winograd_layouts(ctx):
    """B = 8, pose branch: conv4 and conv5 run as 3x3 stride-2 Winograd layers, so conv3_1 and conv4_1 write space-to-depth order and the
    walk / weight gradient read it. (a) forward layer by layer; (b) conv4 / conv4_1 / conv5 / conv5_1 / conv6_1 weight and bias
    gradients against the oracle differentiated at the GPU's activations (the oracle takes well under five minutes here)."""
    B = 8
    d, cfg, net, params, data_np, label_np = _setup(ctx, B, 911, False)
    assert set(net.wino_s2d3) == {"conv4", "conv5"} and net._s2d3_live(4) and net._s2d3_live(6)
    assert [net._enc_out_mode(li) for li in range(10)] == [3, 3, 1, 3, 1, 3, 1, 1, 1, 0]
    data = {k: ctx.array(v) for k, v in data_np.items()}
    label = {k: ctx.array(v) for k, v in label_np.items()}
    loss = net.forward_train(data, label).asnumpy()[0]
    grads = {k: v.asnumpy() for k, v in net.backward().items()}
    acts = _check_forward_layer_by_layer(net, params)
    with pytest.MonkeyPatch.context() as m:
        m.setattr(opipe, "encoder", lambda p_, x_, **kw: dict(acts))
        ref_loss, g_ref, _ = _oracle(cfg, d, params, data_np, label_np, False)
    assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss)
    for layer in ("conv4", "conv4_1", "conv5", "conv5_1", "conv6_1"):
        for part in ("_weight", "_bias"):
            err = rel(grads[layer + part], g_ref[layer + part])
            print("B=8 %s%s: %.3g" % (layer, part, err))
            assert err < 2e-4, (layer + part, err)


def _fresh_equals(ctx, buf, pack):
    """`buf` bit for bit equal to `pack(fresh)` where fresh starts as a copy of buf (a pack that writes only part of the buffer)."""
    fresh = DeviceArray(ctx, buf.shape, dtype=buf.dtype)
    fresh.copyfrom(buf.asnumpy())
    pack(fresh)
    np.testing.assert_array_equal(fresh.asnumpy().view(np.uint32), buf.asnumpy().view(np.uint32))


def test_update_repacks_what_the_winograd_graph_reads_and_training_converges(ctx):
    B = 4
    d, cfg, net, params, data_np, label_np = _setup(ctx, B, 77, True)
    data = {k: ctx.array(v) for k, v in data_np.items()}
    label = {k: ctx.array(v) for k, v in label_np.items()}
    h, P = ctx.handle, net.params

    def losses():
        pm = net.forward_train(data, label).asnumpy()[0]
        p, y = net.act["mask_prob"].asnumpy().astype(np.float64), net.act["zoom_mask_gt_observed"].asnumpy()
        bce = float(-(y * np.log(p + 1e-12) + (1 - y) * np.log(1 - p + 1e-12)).mean())
        return float(pm), float(net.act["flow_loss_sum"].asnumpy()[0]), bce

    first = losses()
    w_before = P["conv4_1_weight"].asnumpy()
    net.backward()
    net.update(lr=2e-3, wd=cfg.TRAIN.wd, momentum=0.5)
    assert not np.array_equal(P["conv4_1_weight"].asnumpy(), w_before)
    # every buffer the forward / backward of this mode reads equals a fresh pack of the updated parameters
    seen = set()
    for li, (name, cin, hh, ww, cout, k, s_, p_) in enumerate(net.enc_geom):
        w = P[name + "_weight"]
        if name in net.packed_wino and name in net.wino_s2d:
            _fresh_equals(ctx, net.packed_wino[name], lambda f: lib.deepim_conv_wino_pack_weights_s2d(h, f, w, cout, cin)); seen.add("s2d")
        elif name in net.packed_wino:
            _fresh_equals(ctx, net.packed_wino[name], lambda f: lib.deepim_conv_wino_pack_weights(h, f, w, cout, cin)); seen.add("wino")
        elif li == 0:
            _fresh_equals(ctx, net.wino_conv1, lambda f: lib.deepim_conv1_wino_pack_weights(h, f, w)); seen.add("conv1")
        else:
            _fresh_equals(ctx, net.packed[name], lambda f: lib.deepim_conv_pack_weights_ex(h, f, w, cout, cin, k, k, 4)); seen.add("nc8")
        if name in net.packed_wino_dgrad:
            _fresh_equals(ctx, net.packed_wino_dgrad[name], lambda f: lib.deepim_conv_wino_pack_weights_dgrad(h, f, w, cout, cin)); seen.add("dgrad")
    assert seen == {"s2d", "wino", "conv1", "nc8", "dgrad"}
    for name in ("deconv4", "Convolution3"):        # the decoder's packs are refreshed as before
        shape = net.arg_shape_dict()[name + "_weight"]
        if name.startswith("deconv"):
            _fresh_equals(ctx, net.packed[name], lambda f: lib.deepim_deconv_pack_weights(h, f, P[name + "_weight"], shape[0], shape[1]))
        else:
            order = net._train_pack_orders()[name]
            _fresh_equals(ctx, net.packed[name], lambda f: lib.deepim_conv_pack_weights_ex(h, f, P[name + "_weight"], *shape, order))
    second = losses()
    assert all(np.isfinite(second)) and second[0] != first[0]
    last = second
    for _ in range(5):
        net.backward()
        net.update(lr=2e-3, wd=cfg.TRAIN.wd, momentum=0.5)
        last = losses()
    assert all(np.isfinite(last))
    assert last[0] < first[0] and last[1] < first[1] and last[2] < first[2], (first, last)


def test_train_step_with_winograd_stays_finite_and_two_streams_agree(ctx):
    """A chained train_step of TRAIN_ITER_SIZE = 4 iterations under the key; and backward() on two streams gives the same bits."""
    from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import batchUpdaterPyMulti
    from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
    B, H, W = 4, 480, 640
    d, cfg, net, params, data_np, label_np = _setup(ctx, B, 77, True)
    data = {k: ctx.array(v) for k, v in data_np.items()}
    label = {k: ctx.array(v) for k, v in label_np.items()}
    net.forward_train(data, label)
    one = {k: v.asnumpy() for k, v in net.backward().items()}
    cfg2 = default_config()
    cfg2.network.PRED_FLOW = cfg2.network.PRED_MASK = True
    cfg2.TRAIN.WINOGRAD_CONV = True
    net2 = deepIM_flownet().get_symbol(cfg2, is_train=True)
    net2.two_streams = True
    net2.bind_train(ctx, B, params, num_points=3000)
    net2.forward_train(data, label)
    two = {k: v.asnumpy() for k, v in net2.backward().items()}
    for k in one:
        np.testing.assert_array_equal(one[k], two[k], err_msg=k)
    mesh = synthetic.ellipsoid_mesh([0.05, 0.04, 0.035], 24, 48)
    mesh.pop("uv")
    rm = Render_Py("unused", ["obj"], d["K"], W, H, meshes={"obj": mesh}, ctx=ctx, pixel_means=MEANS_REV.copy())
    upd = batchUpdaterPyMulti(cfg, H, W, render_machine=rm)
    data.update(tgt_pose=ctx.array(d["pose_tgt"]), depth_gt_observed=ctx.array(d["depth_gt_observed"]))
    seen = []
    net.train_step(data, label, upd, lr=1e-4, on_iter=lambda it, dat, lab: seen.append(
        (float(net.act["pm_loss_sum"].asnumpy()[0]), float(net.act["flow_loss_sum"].asnumpy()[0]))))
    assert len(seen) == 4 and np.isfinite(np.array(seen)).all(), seen


def test_without_the_key_nothing_of_the_mode_is_bound(ctx):
    d, cfg, net, params, data_np, label_np = _setup(ctx, 4, 910, False, wino=False)
    assert not net.train_winograd and not net.nc8
    assert net.packed_wino == {} and net.wino_s2d3 == {} and net.wino_conv1 is None and net.packed_wino_dgrad == {}
    assert "dz_nc8" not in net.ws


def test_the_key_needs_the_lds_weight_gradient(ctx):
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = False
    cfg.TRAIN.WINOGRAD_CONV = True
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    lib.deepim_set_option(ctx.handle, b"wgrad_lds", 0)
    try:
        with pytest.raises(NotImplementedError):
            net.bind_train(ctx, 2, net.init_weights(cfg, seed=91))
    finally:
        lib.deepim_set_option(ctx.handle, b"wgrad_lds", 1)
