"""Frame ingest (csrc/ingest.hip) on the GPU: time per call and achieved HBM traffic of the four kernels, and the feed
comparison for a batch of pairs — (a) host numpy conversion to fp32 + deepim_h2d of the fp32 tensors, what a user does
without the kernels, against (b) deepim_h2d of the raw uint8 / uint16 frames + the kernels — alternating the two.

    python tools/bench_ingest.py [--batch 32] [--reps 200] [--rounds 7] [--feed-rounds 7] [--json PATH]

Kernel times: HIP events around `reps` back-to-back calls, `rounds` rounds after a warm-up, median and range; once rotating
over enough buffer sets that twice the 256 MiB Infinity Cache passes between two uses of a buffer (the HBM figure), once on
one set (which that cache holds). Bytes are what the algorithm has to move (inputs read once, outputs written once), computed
from the shapes; the share is of the measured copy rate of the device (6.29 TB/s). The feed comparison is host wall-clock
around work that ends in a device synchronise (deepim_h2d is synchronous, a deepim_sync follows the kernels)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd.lib.utils.mask_dilate import mask_dilate_draws  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402

COPY_RATE = 6.29e12     # bytes/s, the measured device copy rate the project's notes use
MEANS_RGB = np.array([103.939, 116.779, 123.68], np.float32)


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def time_kernel(ctx, fn, reps, rounds, sets=1):
    """fn(k) works on buffer set k: sets = 1 re-runs one set (which the 256 MiB Infinity Cache holds), more sets rotate"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--feed-rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, H, W = a.batch, a.height, a.width
    n = B * H * W
    ctx = Context.get(0)
    rng = np.random.default_rng(19)
    obs = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    ren = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    bg = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    depth = rng.integers(0, 3000, (B, H, W)).astype(np.uint16)
    labels = np.zeros((B, H, W), np.uint8)
    labels[:, H // 4:H // 2, W // 4:W // 2] = 1
    idx = np.ones(B, np.int32)
    draws = mask_dilate_draws(B, rng=np.random.RandomState(19))

    h, df = ctx.handle, ctypes.c_float(1000.0)
    d_idx, d_draws = ctx.array(idx, dtype=np.int32), ctx.array(draws, dtype=np.int32)
    CACHE = 256 << 20

    def n_sets(nbytes):     # enough sets that 2 x the Infinity Cache passes between two uses of a buffer
        return -(-2 * CACHE // nbytes) + 1

    def dev(host, dtype, k):
        return [ctx.array(host, dtype=dtype) for _ in range(k)]

    def bench(name, nbytes, make):
        for mode, k in (("rotating", n_sets(nbytes)), ("one set", 1)):
            fn = make(k)
            st = time_kernel(ctx, fn, a.reps, a.rounds, k)
            st["bytes"], st["sets"] = nbytes, k
            st["share_of_copy_rate"] = nbytes / (st["median"] * 1e-6) / COPY_RATE
            res["kernels"]["%s (%s)" % (name, mode)] = st
            print("%-24s %-9s %3d sets %8.1f us/call (min %.1f max %.1f)  %6.2f TB/s  %.2f of the copy rate" %
                  (name, mode, k, st["median"], st["min"], st["max"], nbytes / st["median"] / 1e6, st["share_of_copy_rate"]))
            del fn

    res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "kernels": {}, "feed": {}}

    def mk_bgr(with_bg):
        def make(k):
            fr, out = dev(obs, np.uint8, k), [ctx.empty((B, 3, H, W)) for _ in range(k)]
            bgs, lb = (dev(bg, np.uint8, k), dev(labels, np.uint8, k)) if with_bg else ([None] * k, [None] * k)
            return lambda i: lib.deepim_ingest_bgr8(h, out[i], fr[i], bgs[i], lb[i], None, MEANS_RGB, B, H, W)
        return make

    def mk_depth(with_labels):
        def make(k):
            dd, out = dev(depth, np.uint16, k), [ctx.empty((B, 1, H, W)) for _ in range(k)]
            lb = dev(labels, np.uint8, k) if with_labels else [None] * k
            ix = d_idx if with_labels else None
            return lambda i: lib.deepim_ingest_depth16(h, out[i], dd[i], lb[i], ix, df, B, H, W)
        return make

    def mk_label(k):
        lb, out = dev(labels, np.uint8, k), [ctx.empty((B, 1, H, W)) for _ in range(k)]
        return lambda i: lib.deepim_ingest_label_mask(h, out[i], lb[i], d_idx, B, H, W)

    def mk_dilate(k):
        m = (labels == 1).astype(np.float32)[:, None]
        ms, out = dev(m, np.float32, k), [ctx.empty((B, 1, H, W)) for _ in range(k)]
        return lambda i: lib.deepim_mask_dilate(h, out[i], ms[i], d_draws, B, H, W)

    bench("ingest_bgr8", n * (3 + 12), mk_bgr(False))
    bench("ingest_bgr8+bg", n * (7 + 12), mk_bgr(True))
    bench("ingest_depth16", n * (2 + 4), mk_depth(False))
    bench("ingest_depth16+labels", n * (3 + 4), mk_depth(True))
    bench("ingest_label_mask", n * (1 + 4), mk_label)
    bench("mask_dilate", n * (4 + 4), mk_dilate)

    # ---- feed comparison: one test-style batch (observed + rendered image, rendered depth, one label mask)
    def feed_host():
        t0 = time.perf_counter()
        imgs = []
        for fr in (obs, ren):
            t = np.empty((B, 3, H, W), np.float32)
            for i in range(3):
                t[:, i] = fr[..., 2 - i].astype(np.float32) - MEANS_RGB[i]
            imgs.append(t)
        dep = (depth.astype(np.float32) / np.float32(1000))[:, None]
        msk = (labels == idx[:, None, None]).astype(np.float32)[:, None]
        t1 = time.perf_counter()
        keep = [ctx.array(x) for x in imgs + [dep, msk]]
        ctx.sync()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, keep

    def feed_device():
        t0 = time.perf_counter()
        r_obs, r_ren = ctx.array(obs, dtype=np.uint8), ctx.array(ren, dtype=np.uint8)
        r_d, r_l = ctx.array(depth, dtype=np.uint16), ctx.array(labels, dtype=np.uint8)
        t1 = time.perf_counter()
        o1, o2 = ctx.empty((B, 3, H, W)), ctx.empty((B, 3, H, W))
        od, om = ctx.empty((B, 1, H, W)), ctx.empty((B, 1, H, W))
        lib.deepim_ingest_bgr8(h, o1, r_obs, None, None, None, MEANS_RGB, B, H, W)
        lib.deepim_ingest_bgr8(h, o2, r_ren, None, None, None, MEANS_RGB, B, H, W)
        lib.deepim_ingest_depth16(h, od, r_d, None, None, df, B, H, W)
        lib.deepim_ingest_label_mask(h, om, r_l, d_idx, B, H, W)
        ctx.sync()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (o1, o2, od, om)

    ka = feed_host()[2]
    kb = feed_device()[2]
    for x, y in zip(ka, kb):
        assert np.array_equal(x.asnumpy(), y.asnumpy()), "the two feeds disagree"
    del ka, kb
    host, devt = [], []
    for _ in range(a.feed_rounds):
        host.append(feed_host()[:2])
        devt.append(feed_device()[:2])
    res["feed"] = {
        "host_convert_ms": stats([x[0] for x in host]), "host_h2d_fp32_ms": stats([x[1] for x in host]),
        "host_total_ms": stats([x[0] + x[1] for x in host]),
        "device_h2d_raw_ms": stats([x[0] for x in devt]), "device_alloc_kernels_sync_ms": stats([x[1] for x in devt]),
        "device_total_ms": stats([x[0] + x[1] for x in devt]),
        "bytes_fp32": n * 4 * 8, "bytes_raw": n * (3 + 3 + 2 + 1)}
    for k, v in res["feed"].items():
        print("feed %-30s %s" % (k, v if not isinstance(v, dict) else "%.2f ms (min %.2f max %.2f)" % (v["median"], v["min"], v["max"])))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
