"""Training metrics on the GPU (deepim_train_metrics and deepim_l2_norms_multi, csrc/metric.hip): time per call and achieved HBM
traffic, the reference's way on the same tensors (four asnumpy() copies plus the numpy expressions of deepim/core/metric.py), and
a training step with and without the metric update.

    python tools/bench_train_metrics.py [--batch N] [--reps 200] [--rounds 7] [--feed-rounds 7] [--no-step] [--json PATH]

Without --batch it measures B = 4 and B = 32. Method of tools/bench_flow_epe.py. Kernel time: HIP events around `reps`
back-to-back calls, `rounds` rounds after a warm-up, median and range; once rotating over enough buffer sets that twice the
256 MiB Infinity Cache passes between two uses of a buffer (the HBM figure), once on one set. Bytes are what the call has to
read: 4 per float of flow_loss, pm_loss, mask_prob and mask_gt (both heads, point-matching loss); the share is of the measured
copy rate of the device (6.29 TB/s). The comparison is host wall-clock around work that ends with the numbers on the host. The
training step is net.train_step at B = 4 with both heads (tools/bench_train.py's `4 heads step4`), alternating rounds with and
without CompositeEvalMetric.update behind it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.core import metric  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402

COPY_RATE = 6.29e12     # bytes/s, the measured device copy rate the project's notes use
H, W, NPTS = 480, 640, 3000


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def time_kernel(ctx, fn, reps, rounds, sets=1):
    for k in range(max(3, sets)):
        fn(k % sets)
    ctx.sync()
    us = []
    for _ in range(rounds):
        t = ctx.timer()
        t.start()
        for k in range(reps):
            fn(k % sets)
        t.stop()
        ctx.sync()
        us.append(t.elapsed_ms() / reps * 1e3)
    return stats(us)


def host_tensors(B, seed=21):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    p = rng.random((B, 1, H, W)).astype(f32)
    g = (rng.random((B, 1, H, W)) > 0.8).astype(f32)
    return {"flow_loss": (rng.random((B, 2, H, W)) ** 3).astype(f32), "point_matching_loss": (rng.random((B, 3, NPTS)) * 0.01).astype(f32),
            "mask_prob": p, "mask_gt": g}


def reference_way(preds):
    """deepim/core/metric.py:58-63, :73-77, :116-120, :130-137: four copies to the host and numpy."""
    t0 = time.perf_counter()
    flow_a = preds["flow_loss"].asnumpy()
    flow_b = preds["flow_loss"].asnumpy()
    pm = preds["point_matching_loss"].asnumpy()
    prob, gt = preds["mask_prob"].asnumpy(), preds["mask_gt"].asnumpy()
    t1 = time.perf_counter()
    out = [np.sum(flow_a), np.sum(flow_b), np.sum(pm),
           np.sum(-(gt * np.log(prob + 1e-19) + (1 - gt) * np.log(1 - prob + 1e-19)))]
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, out


def bench_kernels(ctx, B, a, res):
    host = host_tensors(B)
    nbytes = sum(v.nbytes for v in host.values())
    CACHE = 256 << 20
    cfg = default_config()

    def composite():
        return metric.CompositeEvalMetric([metric.Flow_L2LossMetric(cfg, 0), metric.Flow_CurLossMetric(cfg, 0),
                                           metric.PointMatchingLossMetric(cfg, 0), metric.MaskLossMetric(cfg, 0)])

    for mode, k in (("rotating", -(-2 * CACHE // nbytes) + 1), ("one set", 1)):
        sets = [{n: ctx.array(v) for n, v in host.items()} for _ in range(k)]
        comp = composite()
        st = time_kernel(ctx, lambda i: comp.update(None, sets[i]), a.reps, a.rounds, k)
        st["bytes"], st["sets"] = nbytes, k
        st["share_of_copy_rate"] = nbytes / (st["median"] * 1e-6) / COPY_RATE
        res["kernels"]["train_metrics B=%d (%s)" % (B, mode)] = st
        print("train_metrics B=%-2d %-9s %3d sets %8.1f us/call (min %.1f max %.1f)  %6.2f TB/s  %.2f of the copy rate" %
              (B, mode, k, st["median"], st["min"], st["max"], nbytes / st["median"] / 1e6, st["share_of_copy_rate"]))
        del sets
    preds = {n: ctx.array(v) for n, v in host.items()}
    comp = composite()

    def fused():
        t0 = time.perf_counter()
        comp.update(None, preds)
        values = comp.get()[1]
        return (time.perf_counter() - t0) * 1e3, 0.0, values

    v, r = fused()[2], reference_way(preds)[2]
    want = [r[0] / (H * W), r[1] / (H * W), r[2] / NPTS, r[3] / (H * W)]
    assert np.allclose(v, want, rtol=1e-5), ("the two evaluations disagree", v, want)
    fu, ho = [], []
    for _ in range(a.feed_rounds):
        comp.reset()
        fu.append(fused()[:2])
        ho.append(reference_way(preds)[:2])
    cmp_ = {"fused_update_and_get_ms": stats([x[0] for x in fu]), "reference_d2h_ms": stats([x[0] for x in ho]),
            "reference_numpy_ms": stats([x[1] for x in ho]), "reference_total_ms": stats([x[0] + x[1] for x in ho]),
            "bytes_d2h_reference": nbytes + host["flow_loss"].nbytes, "bytes_d2h_fused": 80}
    res["compare"]["B=%d" % B] = cmp_
    for k, v in cmp_.items():
        print("compare B=%-2d %-26s %s" % (B, k, v if not isinstance(v, dict) else "%.3f ms (min %.3f max %.3f)" % (v["median"], v["min"], v["max"])))


def bench_step(ctx, a, res, B=4):
    from mx_deepim_amd.core.module import MutableModule
    from mx_deepim_amd.lib.pair_matching import data_pair
    from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import batchUpdaterPyMulti
    from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
    from mx_deepim_amd.symbols import deepIM_flownet
    d = synthetic.make_batch(B, seed=910, n_frames=1)
    cfg = default_config()
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    net.bind_train(ctx, B, net.init_weights(cfg, seed=91))
    gt = (d["depth_gt_observed"] > 0).astype(np.float32)
    pco = np.stack([d["pose_tgt"][b][:, :3] @ d["point_cloud_model"][b] + d["pose_tgt"][b][:, 3:4] for b in range(B)]).astype(np.float32)
    data = {k: ctx.array(v) for k, v in {"image_observed": d["image_observed"], "image_rendered": d["image_rendered"][0],
            "mask_observed": d["mask_observed"], "mask_rendered": d["mask_rendered"][0], "src_pose": d["src_pose"][0],
            "tgt_pose": d["pose_tgt"], "depth_gt_observed": d["depth_gt_observed"]}.items()}
    label = {k: ctx.array(v) for k, v in {"mask_gt_observed": gt, "point_cloud_model": d["point_cloud_model"],
             "point_cloud_weights": np.ones((B, 3, NPTS), np.float32), "point_cloud_observed": pco}.items()}
    label["flow"], label["flow_weights"] = data_pair.get_pair_flow(
        {"depth_rendered": ctx.array(d["depth_rendered"][0]), "depth_gt_observed": ctx.array(d["depth_gt_observed"]),
         "pose_rendered": ctx.array(d["src_pose"][0]), "pose_observed": ctx.array(d["pose_tgt"])}, cfg)
    mesh = dict(synthetic.ellipsoid_mesh([0.05, 0.04, 0.035]), texture=synthetic.procedural_texture())
    mesh.pop("colors")
    rm = Render_Py("synthetic", ["ellipsoid"], d["K"], W, H, 0.25, 6.0, meshes={"ellipsoid": mesh}, ctx=ctx,
                   pixel_means=synthetic.PIXEL_MEANS[::-1].copy())
    upd = batchUpdaterPyMulti(cfg, H, W, render_machine=rm)
    comp = metric.CompositeEvalMetric([metric.Flow_L2LossMetric(cfg, 0), metric.Flow_CurLossMetric(cfg, 0),
                                       metric.PointMatchingLossMetric(cfg, 0), metric.MaskLossMetric(cfg, 0)])

    def run(with_metrics, n):
        t = ctx.timer()
        t.start()
        for _ in range(n):
            _d, lab = net.train_step(data, label, upd, lr=1e-6)
            if with_metrics:
                comp.update(lab, net.train_outputs())
        t.stop()
        ctx.sync()
        return t.elapsed_ms() / n

    for w in (False, True):
        run(w, 2)
    plain, with_m = [], []
    for _ in range(a.feed_rounds):
        plain.append(run(False, 5))
        with_m.append(run(True, 5))
    res["train_step"] = {"batch": B, "iterations": int(cfg.network.TRAIN_ITER_SIZE), "step_ms": stats(plain),
                         "step_with_metric_update_ms": stats(with_m)}
    print("train_step B=%d x%d heads: %.3f ms (min %.3f max %.3f); with the metric update %.3f ms (min %.3f max %.3f)" % (
        B, cfg.network.TRAIN_ITER_SIZE, res["train_step"]["step_ms"]["median"], min(plain), max(plain),
        res["train_step"]["step_with_metric_update_ms"]["median"], min(with_m), max(with_m)))
    # the weight-norm line over the net's parameter table: deepim_l2_norms_multi against a read-back and numpy per parameter
    mod = MutableModule(cfg, net)
    names = [n for n, _v in mod.weight_norms()]
    table, out = mod._norm_table
    nbytes = sum(net.params[n].nbytes for n in names)
    st = time_kernel(ctx, lambda i: lib.deepim_l2_norms_multi(ctx.handle, out, table, len(names)), 50, a.rounds)
    st.update(rows=len(names), bytes=nbytes, share_of_copy_rate=nbytes / (st["median"] * 1e-6) / COPY_RATE)
    res["kernels"]["l2_norms_multi"] = st
    print("l2_norms_multi %d rows %.1f MB %8.1f us/call (min %.1f max %.1f)  %6.2f TB/s  %.2f of the copy rate (parameters partly cache-resident)" % (
        len(names), nbytes / 1e6, st["median"], st["min"], st["max"], nbytes / st["median"] / 1e6, st["share_of_copy_rate"]))
    fu, ho = [], []
    for _ in range(a.feed_rounds):
        t0 = time.perf_counter()
        got = mod.weight_norms()
        fu.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ref = [np.linalg.norm(net.params[n].asnumpy().ravel()) for n in names]
        ho.append((time.perf_counter() - t0) * 1e3)
    # (numpy's float32 norm of 21 M elements is itself only good to about 1e-4: the check is against float64)
    ref64 = [np.linalg.norm(net.params[n].asnumpy().ravel().astype(np.float64)) for n in names]
    assert np.allclose([v for _n, v in got], ref64, rtol=1e-6, atol=0), "the two evaluations disagree"
    res["compare"]["weight_norms"] = {"fused_and_readback_ms": stats(fu), "reference_readback_and_numpy_ms": stats(ho)}
    print("weight-norm line: fused + read-back of %d floats %.3f ms; %d read-backs + numpy %.3f ms" % (
        len(names), stats(fu)["median"], len(names), stats(ho)["median"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--feed-rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = Context.get(0)
    res = {"reps": a.reps, "rounds": a.rounds, "kernels": {}, "compare": {}}
    for B in ([a.batch] if a.batch else [4, 32]):
        bench_kernels(ctx, B, a, res)
    if not a.no_step:
        bench_step(ctx, a, res)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
