"""Flow EPE of the test loop (deepim_flow_epe, csrc/flow.hip) on the GPU: time per call and achieved HBM traffic, and the
comparison with what evaluates the EPE without the kernel — deepim_calc_flow_forward, a device-to-host copy of the flow, the
visible map, the rendered depth and the prediction, and the numpy formula of tester.py:572-589 — alternating the two.

    python tools/bench_flow_epe.py [--batch 32] [--reps 200] [--rounds 7] [--feed-rounds 7] [--json PATH]

Method of tools/bench_ingest.py. Kernel time: HIP events around `reps` back-to-back calls, `rounds` rounds after a warm-up, median
and range; once rotating over enough buffer sets that twice the 256 MiB Infinity Cache passes between two uses of a buffer (the
HBM figure), once on one set. Bytes are what the algorithm has to move: 4 (rendered depth) + 8 (prediction) per pixel, plus one
4-byte gather of the observed depth per pixel with a rendered depth (counted as the frame's share of such pixels; an upper bound
of 16 B/pixel is printed too); the share is of the measured copy rate of the device (6.29 TB/s). The comparison is host
wall-clock around work that ends with the numbers on the host."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402

COPY_RATE = 6.29e12     # bytes/s, the measured device copy rate the project's notes use
THRESH = 3e-3


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


def inv3(K):
    """the library's own 3x3 inverse (adjugate in double, then float32), so that both evaluations see the same Kinv"""
    a, b, c, d, e, f, g, h, i = [float(v) for v in np.asarray(K, np.float32).reshape(9)]
    A, Bc, C = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * Bc + c * C
    o = [A / det, -(b * i - c * h) / det, (b * f - c * e) / det, Bc / det, (a * i - c * g) / det, -(a * f - c * d) / det,
         C / det, -(a * h - b * g) / det, (a * e - b * d) / det]
    return np.array(o, np.float64).astype(np.float32).reshape(3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--feed-rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, H, W = a.batch, 480, 640
    n = B * H * W
    ctx = Context.get(0)
    h = ctx.handle
    # four distinct synthetic pairs, tiled over the batch: object pixels (projection + gather) and background in a real ratio
    d = synthetic.make_batch(4, seed=20, n_frames=1)
    rep = -(-B // 4)
    dr = np.tile(d["depth_rendered"][0], (rep, 1, 1, 1))[:B]
    do = np.tile(d["depth_gt_observed"], (rep, 1, 1, 1))[:B]
    src = np.tile(d["src_pose"][0], (rep, 1, 1))[:B]
    tgt = np.tile(d["pose_tgt"], (rep, 1, 1))[:B]
    K = d["K"]
    est = (np.random.default_rng(20).standard_normal((B, 2, H, W)) * 3).astype(np.float32)
    obj_share = float((dr != 0).mean())
    nbytes = int(n * (12 + 4 * obj_share))
    CACHE = 256 << 20
    res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "object_pixel_share": obj_share, "kernels": {},
           "compare": {}}

    def make(k):
        sets = [(ctx.array(est), ctx.array(dr), ctx.array(do)) for _ in range(k)]
        ps, pt = ctx.array(src), ctx.array(tgt)
        out, totals = ctx.empty((B, 6), dtype=np.float64), ctx.zeros((6,), dtype=np.float64)
        return (lambda i: lib.deepim_flow_epe(h, out, totals, sets[i][0], sets[i][1], sets[i][2], ps, pt, K, None,
                                              ctypes.c_float(THRESH), 0, B, H, W)), sets

    for mode, k in (("rotating", -(-2 * CACHE // (n * 16)) + 1), ("one set", 1)):
        fn, keep = make(k)
        st = time_kernel(ctx, fn, a.reps, a.rounds, k)
        st["bytes"], st["bytes_upper_bound"], st["sets"] = nbytes, n * 16, k
        st["share_of_copy_rate"] = nbytes / (st["median"] * 1e-6) / COPY_RATE
        st["share_of_copy_rate_upper_bound_bytes"] = n * 16 / (st["median"] * 1e-6) / COPY_RATE
        res["kernels"]["flow_epe (%s)" % mode] = st
        print("flow_epe %-9s %3d sets %8.1f us/call (min %.1f max %.1f)  %6.2f TB/s  %.2f of the copy rate (%.2f at 16 B/pixel)" %
              (mode, k, st["median"], st["min"], st["max"], nbytes / st["median"] / 1e6, st["share_of_copy_rate"],
               st["share_of_copy_rate_upper_bound_bytes"]))
        del fn, keep

    # ---- comparison: the six totals of one batch on the host, (a) fused kernel, (b) calc_flow_forward + copies + numpy
    d_est, d_dr, d_do, d_src, d_tgt = ctx.array(est), ctx.array(dr), ctx.array(do), ctx.array(src), ctx.array(tgt)
    out, KT = ctx.empty((B, 6), dtype=np.float64), ctx.empty((B, 3, 4))
    flow, vis = ctx.empty((B, H, W, 2)), ctx.empty((B, H, W))
    Kinv = inv3(K)

    def fused():
        t0 = time.perf_counter()
        lib.deepim_flow_epe(h, out, None, d_est, d_dr, d_do, d_src, d_tgt, K, None, ctypes.c_float(THRESH), 0, B, H, W)
        rows = out.asnumpy()
        return (time.perf_counter() - t0) * 1e3, 0.0, rows

    def host():
        t0 = time.perf_counter()
        lib.deepim_calc_KT(h, KT, d_src, d_tgt, K, B)
        lib.deepim_calc_flow_forward(h, flow, vis, d_dr, d_do, KT, Kinv, ctypes.c_float(THRESH), 0, B, H, W)
        f, v, e, r = flow.asnumpy(), vis.asnumpy(), d_est.asnumpy(), d_dr.asnumpy()
        t1 = time.perf_counter()
        pred = e.transpose(0, 2, 3, 1).astype(np.float16)                        # tester.py:350-352
        x_diff = f[..., 0].astype(np.float64) - pred[..., 0]
        y_diff = f[..., 1].astype(np.float64) - pred[..., 1]
        point_diff = np.sqrt(np.square(x_diff) + np.square(y_diff))
        vizbg = np.logical_or(v, np.logical_and(v == 0, r[:, 0] == 0))
        rows = np.stack([point_diff.reshape(B, -1).sum(1), np.full(B, H * W, np.float64),
                         np.where(v == 1, point_diff, 0).reshape(B, -1).sum(1), v.reshape(B, -1).sum(1),
                         np.where(vizbg, point_diff, 0).reshape(B, -1).sum(1), vizbg.reshape(B, -1).sum(1)], 1)
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, rows

    ra, rb = fused()[2], host()[2]
    assert np.array_equal(ra[:, 1::2], rb[:, 1::2]), "the two evaluations count differently"
    # the host path rounds the ground truth to fp32 (deepim_calc_flow_forward's tensor): sums agree to fp32 grade only
    assert np.allclose(ra[:, 0::2], rb[:, 0::2], rtol=1e-6), "the two evaluations disagree"
    fu, ho = [], []
    for _ in range(a.feed_rounds):
        fu.append(fused()[:2])
        ho.append(host()[:2])
    res["compare"] = {"fused_kernel_and_readback_ms": stats([x[0] for x in fu]),
                      "host_kernel_and_d2h_ms": stats([x[0] for x in ho]), "host_numpy_ms": stats([x[1] for x in ho]),
                      "host_total_ms": stats([x[0] + x[1] for x in ho]), "bytes_d2h_host_path": n * 4 * 6, "bytes_d2h_fused": B * 48}
    for k, v in res["compare"].items():
        print("compare %-30s %s" % (k, v if not isinstance(v, dict) else "%.3f ms (min %.3f max %.3f)" % (v["median"], v["min"], v["max"])))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
