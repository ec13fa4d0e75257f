"""Writes tests/golden/train_half_digests.json: SHA-256 digests of what the half-precision encoder backward (csrc/train_half.hip: the
fp16 and the split-fp16 "x3" mode) computes on seeded inputs — the raw output bytes of the C entry points on the smallest shapes that
reach every branch of the kernels and their launchers, and every gradient of one training iteration per mode. Needs the GPU.

    python tests/golden/make_train_half_digests.py [out.json] [note]   # after the library is built; the note goes into the file

tests/test_gpu_train_half_digests.py recomputes every digest with the tree's own library. The entry points are deterministic (fixed
slices, sums in a fixed order), so a digest moves only when a result bit moves: the file is regenerated only for a change that means
to alter the arithmetic, and its diff then names the cases that moved. The committed file was recorded with the library of the commit
before the two modes' sources were merged, so it also pins the merged kernels to the separate ones bit for bit.

A digest pins bits; it does not say they are right. tests/train_half_cases.py takes WGRAD, LRELU, DGRAD and DGRAD_CH from here and
tests/test_gpu_train_half_edges.py checks every one of these shapes against a float64 reference."""
import collections
import ctypes
import hashlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "train_half_digests.json")
cf, f16, f32 = ctypes.c_float, np.float16, np.float32
SLOPE, ACT, SCALE = 0.1, 16.0, 1024.0
MODES = ("f16", "x3")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _split16(v):
    """(B,H,W,C) fp32 values -> split16 records (B,H,W,2C) fp16: per 16 channels [hi 16 | lo 16]."""
    B, H, W, C = v.shape
    hi = v.astype(f16)
    lo = (v - hi.astype(f32)).astype(f16)
    rec = np.stack([a.reshape(B, H, W, C // 16, 16) for a in (hi, lo)], axis=4)
    return np.ascontiguousarray(rec.reshape(B, H, W, 2 * C))


def _tensor(rng, mode, shape, scale=1.0):
    """A seeded (B,H,W,C) tensor in the mode's layout: NHWC fp16, or split16."""
    v = (rng.standard_normal(shape) * scale).astype(f32)
    return _split16(v) if mode == "x3" else v.astype(f16)


def _state(ctx, scale=SCALE):
    """A fresh scale state {scale, 1 / scale, 0, 0}; the context's saturation bit is cleared first (into a state nobody reads), so
    that a case sees only what it raises itself."""
    from mx_deepim_amd.runtime import lib
    st = np.zeros(4, np.uint32)
    st[:2] = np.array([scale, 1.0 / scale], f32).view(np.uint32)
    sink = ctx.array(st, np.uint32)
    lib.deepim_x3_status_to_state(ctx.handle, sink)
    sink.asnumpy()      # (keeps `sink` alive until the launch has run)
    return ctx.array(st, np.uint32)


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ---- (a) weight gradient: both layouts -----------------------------------------------------------------------------------------
# (B, Cin, Cin_pad, H, W, Cout, k, stride, pad, modes)
WGRAD = [(1, 16, 16, 5, 6, 16, 3, 1, 1, MODES),      # npix 30: one ragged k-step, S = 1 (direct store), a 16-column second n-tile
         (2, 16, 16, 9, 11, 144, 3, 2, 1, MODES),    # npix 60, 4 tiles: S = 2 (partials + reduce), 16-row second m-tile, padding taps
         (1, 32, 32, 8, 10, 32, 5, 2, 2, MODES),
         (1, 6, 8, 12, 14, 24, 7, 2, 3, ("f16",))]   # the ci >= Cin mask and the Cout % 8 edge


def wgrad_case(ctx, mode, B, cin, cpad, H, W, cout, k, s, p):
    from mx_deepim_amd.runtime import lib
    rng, h = _rng("wgrad %s %s" % (mode, (B, cin, cpad, H, W, cout, k, s, p))), ctx.handle
    ho, wo = _out_hw(H, W, k, s, p)
    x = _tensor(rng, mode, (B, H, W, cpad))
    if cpad > cin:
        x[..., cin:] = 0
    xd, zd, st = ctx.array(x, f16), ctx.array(_tensor(rng, mode, (B, ho, wo, cout), 8.0), f16), _state(ctx)
    out = []
    for layout in (0, 1):
        dw = ctx.zeros((cout, cin, k, k) if layout == 0 else (cout, k * k, cin))
        if mode == "x3":
            lib.deepim_conv2d_wgrad_x3(h, dw, xd, zd, st, B, cin, H, W, cout, k, s, p, layout, cf(ACT))
        else:
            lib.deepim_conv2d_wgrad_f16(h, dw, xd, zd, st, B, cin, cpad, H, W, cout, k, s, p, layout)
        out.append(dw.asnumpy())
    return _digest(*out, st.asnumpy())


# ---- (b), (d) activation gradient + bias gradient, in place over d as the graph runs it ------------------------------------------
LRELU = [(3, 128, 7, 9),       # one slice
         (2, 64, 24, 30)]      # npix 1440: two slices, the second one ragged


def lrelu_case(ctx, mode, src, B, C, H, W, spike=False):
    """src: "d" (the gradient from the layer above), "add" (an fp32 NCHW term, scaled by S in the kernel) or "both"; spike: one
    element of `add` at 1e9, which the scale does not hold."""
    from mx_deepim_amd.runtime import lib
    rng, h = _rng("lrelu %s %s %s" % (mode, src, (B, C, H, W))), ctx.handle
    y = ctx.array(_tensor(rng, mode, (B, H, W, C)), f16)
    d = _tensor(rng, mode, (B, H, W, C), 4.0)
    add = (rng.standard_normal((B, C, H, W)) / 256.0).astype(f32)
    if spike:
        add[0, 3, 0, 0] = 1e9
    buf = ctx.array(d if src != "add" else np.zeros_like(d), f16)
    db, st = ctx.zeros((C,)), _state(ctx)
    fn = lib.deepim_lrelu_bias_backward_x3 if mode == "x3" else lib.deepim_lrelu_bias_backward_f16
    add_d = ctx.array(add) if src != "d" else None
    fn(h, buf, db, buf if src != "add" else None, add_d, y, st, cf(SLOPE), B, C, H, W)
    return _digest(buf.asnumpy().view(np.uint16), db.asnumpy(), st.asnumpy())


# ---- (c) data gradient -------------------------------------------------------------------------------------------------------
# (B, Hd, Wd, k, stride, pad); channels per mode
DGRAD = [(2, 6, 7, 3, 1, 1),
         (2, 7, 9, 3, 2, 1),       # both extents odd: the four parity classes have different windows
         (2, 7, 9, 5, 2, 2)]
DGRAD_CH = {"f16": (16, 24), "x3": (128, 32)}      # (Ci_l, Co_l)


def dgrad_case(ctx, mode, B, Hd, Wd, k, s, p):
    from mx_deepim_amd.runtime import lib
    L, h = lib.load(), ctx.handle
    ci, co = DGRAD_CH[mode]
    rng = _rng("dgrad %s %s" % (mode, (B, ci, Hd, Wd, co, k, s, p)))
    ho, wo = _out_hw(Hd, Wd, k, s, p)
    w = ctx.array((rng.standard_normal((co, ci, k, k)) / 12.0).astype(f32))
    zd, st = ctx.array(_tensor(rng, mode, (B, ho, wo, co), 4.0), f16), _state(ctx, 1.0)
    size = L.deepim_conv_dgrad_x3_workspace_size if mode == "x3" else L.deepim_conv_dgrad_f16_workspace_size
    nb = size(B, ci, Hd, Wd, co, k, s, p)
    ws = ctx.zeros(((nb + 1) // 2,), f16)
    dx = ctx.array(np.full((B, Hd, Wd, (2 if mode == "x3" else 1) * ci), 7.0), f16)      # every element is written
    if mode == "x3":
        lib.deepim_conv2d_dgrad_x3(h, dx, zd, w, ws, st, B, ci, Hd, Wd, co, k, s, p, cf(1024.0))
    else:
        lib.deepim_conv2d_dgrad_f16(h, dx, zd, w, ws, B, ci, Hd, Wd, co, k, s, p)
    return _digest(np.array([nb], np.uint64), dx.asnumpy().view(np.uint16), st.asnumpy())


# ---- (d) the saturation bit of an x3 forward reaches the scale state ---------------------------------------------------------------
def status_case(ctx):
    """A 1x1 x3 convolution whose bias (1e6, stored at scale 16) leaves fp16's range: the kernel clamps and raises the context's
    status bit; deepim_x3_status_to_state moves it into word 2, and a second call finds it cleared."""
    from mx_deepim_amd.runtime import lib
    L, h, rng = lib.load(), ctx.handle, _rng("status")
    B, cin, H, W, cout = 1, 32, 2, 2, 128
    pk = ctx.zeros((L.deepim_conv_x3_packed_size(cout, cin, 1, 1) // 2,), f16)
    w = ctx.array((rng.standard_normal((cout, cin, 1, 1)) / 8.0).astype(f32))
    lib.deepim_conv_x3_pack_weights(h, pk, w, cout, cin, 1, 1, cf(256.0))
    bias = np.zeros(cout, f32)
    bias[5] = 1e6
    bias_d, x = ctx.array(bias), ctx.array(_tensor(rng, "x3", (B, H, W, cin), ACT), f16)
    st, st2 = _state(ctx), _state(ctx)
    out = ctx.zeros((B, H, W, 2 * cout), f16)
    lib.deepim_conv2d_x3_forward(h, out, x, pk, bias_d, B, cin, H, W, cout, 1, 1, 1, 0, cf(SLOPE), cf(1.0 / (256.0 * ACT)), cf(ACT))
    lib.deepim_x3_status_to_state(h, st)
    lib.deepim_x3_status_to_state(h, st2)
    return _digest(st.asnumpy(), st2.asnumpy())


# ---- (e) one training iteration through the Python graph ------------------------------------------------------------------------------
def iteration_case(ctx, mode):
    """forward_train + backward at B = 1, pose branch, on the batch and the weights of tools/bench_train.py: every entry of net.grad
    in the parameter's own layout, and the scale state."""
    from mx_deepim_amd import synthetic
    from mx_deepim_amd.config import default_config
    from mx_deepim_amd.symbols import deepIM_flownet
    B = 1
    _state(ctx)      # (clears the saturation bit an earlier user of the context may have left)
    d = synthetic.make_batch(B, seed=910, n_frames=1)
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = False
    cfg.network.FP16_CONV = mode == "f16"
    cfg.TRAIN.X3_CONV = mode == "x3"
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    net.bind_train(ctx, B, net.init_weights(cfg, seed=91))
    gt = (d["depth_gt_observed"] > 0).astype(f32)
    pco = np.stack([d["pose_tgt"][b][:, :3] @ d["point_cloud_model"][b] + d["pose_tgt"][b][:, 3:4] for b in range(B)]).astype(f32)
    data = {k: ctx.array(v) for k, v in {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][0],
            "mask_observed": d["mask_observed"], "mask_rendered": d["mask_rendered"][0], "src_pose": d["src_pose"][0]}.items()}
    label = {k: ctx.array(v) for k, v in {"mask_gt_observed": gt, "point_cloud_model": d["point_cloud_model"],
             "point_cloud_weights": np.ones((B, 3, 3000), f32), "point_cloud_observed": pco}.items()}
    net.forward_train(data, label)
    net.backward()
    return _digest(*[net.grad[name].asnumpy() for name in sorted(net.grad)], net.amp_state.asnumpy())


def cases():
    """name -> function(ctx) -> digest, in the order of the file"""
    out = collections.OrderedDict()
    for B, cin, cpad, H, W, cout, k, s, p, modes in WGRAD:
        for mode in modes:
            out["wgrad_%s B%d Cin%d/%d %dx%d Cout%d k%d s%d p%d" % (mode, B, cin, cpad, H, W, cout, k, s, p)] = (
                lambda ctx, a=(mode, B, cin, cpad, H, W, cout, k, s, p): wgrad_case(ctx, *a))
    for shape in LRELU:
        for mode in MODES:
            for src in ("d", "add", "both"):
                out["lrelu_%s %s %dx%dx%dx%d" % ((mode, src) + shape)] = lambda ctx, a=(mode, src) + shape: lrelu_case(ctx, *a)
    for g in DGRAD:
        for mode in MODES:
            out["dgrad_%s B%d %dx%d k%d s%d p%d" % ((mode,) + g)] = lambda ctx, a=(mode,) + g: dgrad_case(ctx, *a)
    for mode in MODES:
        out["overflow_%s add 1e9 %dx%dx%dx%d" % ((mode,) + LRELU[0])] = (
            lambda ctx, a=(mode, "add") + LRELU[0]: lrelu_case(ctx, *a, spike=True))
    out["overflow_x3 status to state"] = status_case
    for mode in MODES:
        out["iteration_%s B1 pose" % mode] = lambda ctx, m=mode: iteration_case(ctx, m)
    return out


if __name__ == "__main__":
    from mx_deepim_amd.runtime import Context
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    ctx = Context.get(0)
    digests = collections.OrderedDict((name, fn(ctx)) for name, fn in cases().items())
    doc = collections.OrderedDict([
        ("header", "SHA-256 of the half-precision encoder backward's outputs on seeded inputs, written by "
                   "tests/golden/make_train_half_digests.py"),
        ("note", " ".join(sys.argv[2:])),
        ("digests", digests)])
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("%s: %d digests" % (path, len(digests)))
