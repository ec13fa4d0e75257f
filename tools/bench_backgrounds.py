"""Background replacement on the device (csrc/ingest.hip deepim_ingest_bgr8_pool, csrc/sample.hip deepim_sample_backgrounds) at
480x640 with a pool of 64 seeded images of VOC-like sizes:

    python tools/bench_backgrounds.py [--batch 32] [--reps 200] [--rounds 7] [--feed-rounds 9] [--json PATH]

(a) The pool kernel and the draw kernel: HIP events around `reps` back-to-back calls, `rounds` rounds after a warm-up, median
    and range, rotating over enough frame / output sets that twice the 256 MiB Infinity Cache passes between two uses of a
    buffer, and on one set. Bytes are what the algorithm has to move: the frames and labels read once, the planes written once,
    and each pool image a batch draws read once (the taps of neighbouring pixels overlap; what they re-read is cache traffic).
    The share is of the measured copy rate of the device, the figure tools/bench_ingest.py uses.
(b) The only route there was before: deepim_h2d of a background already cropped and resized to (B,H,W,3) on the host, then
    deepim_ingest_bgr8 with bg_frames. The host resize is NOT charged to it. Against the new route for the same batch (the
    draws, then the pool kernel), alternating, host wall-clock around work that ends in a device synchronise; the frames and
    labels are on the device in both.
(c) A whole TrainDataLoader step (make_batch + synchronise) with and without backgrounds, alternating."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ingest import COPY_RATE, MEANS_RGB, stats, time_kernel  # noqa: E402
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.core.loader import TrainDataLoader  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py  # noqa: E402
from mx_deepim_amd.lib.utils import image as dimage  # noqa: E402
from mx_deepim_amd.lib.utils.background import BackgroundPool, background_draws_device  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402

POOL = 64


def voc_like_images(rng):
    """64 images with the sizes a VOC list has: 500 px on the long side, mostly landscape"""
    out = []
    for k in range(POOL):
        short = int(rng.integers(280, 421)) if k % 8 else 500
        out.append(rng.integers(0, 256, (500, short, 3) if k % 4 == 3 else (short, 500, 3), dtype=np.uint8))
    return out


def loader_world(ctx, cfg, B, H, W, rng):
    meshes = {"a": synthetic.ellipsoid_mesh([0.05, 0.04, 0.035], 12, 24)}
    meshes["a"].pop("uv")
    K = synthetic.K_LINEMOD.astype(np.float32)
    rm = Render_Py("unused", ["a"], K, W, H, meshes=meshes, ctx=ctx, pixel_means=np.asarray(dimage._means_rgb(cfg), np.float32))
    poses = np.stack([synthetic.sample_pose_pair(rng)[0] for _ in range(B)]).astype(np.float32)
    cls = np.zeros(B, np.int32)
    image, depth = rm.render_batch(ctx.array(cls, dtype=np.int32), ctx.array(poses))
    rgb = image.asnumpy() + rm.pixel_means.reshape(1, 3, 1, 1)
    bgr = np.ascontiguousarray(np.clip(np.rint(rgb), 0, 255).astype(np.uint8)[:, ::-1].transpose(0, 2, 3, 1))
    d16 = np.rint(depth.asnumpy()[:, 0] * 1000.0).astype(np.uint16)
    observed = {"image_observed": bgr, "depth_gt_observed": d16, "depth_observed": d16.copy(),
                "mask_gt_observed": (d16 > 0).astype(np.uint8), "mask_idx": np.ones(B, np.int32), "pose_observed": poses,
                "class_index": cls}
    points = {0: (synthetic.sample_model_points(rng, [0.05, 0.04, 0.035], 3000), np.ones((3, 3000), np.float32))}
    return rm, observed, points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--feed-rounds", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, H, W = a.batch, 480, 640
    n = B * H * W
    ctx = Context.get(0)
    h = ctx.handle
    rng = np.random.default_rng(25)
    images = voc_like_images(rng)
    pool = BackgroundPool(ctx, images, H, W)
    frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    labels = np.zeros((B, H, W), np.uint8)
    labels[:, H // 4:H // 2, W // 4:W // 2] = 1
    ids = ctx.array(np.arange(B), dtype=np.uint64)
    use_bg, bg_index = background_draws_device(ctx, B, 25, ids, 1.0, POOL)
    drawn = sorted(set(bg_index.asnumpy().tolist()))
    pool_read = sum(images[k].size for k in drawn)
    res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "pool_images": POOL, "pool_bytes": pool.nbytes,
           "images_drawn": len(drawn), "kernels": {}, "routes": {}, "loader": {}}

    # ---- (a) the kernels
    nbytes = n * (3 + 1 + 12) + pool_read
    for mode, k in (("rotating", -(-2 * (256 << 20) // (n * 16)) + 1), ("one set", 1)):
        fr = [ctx.array(frames, dtype=np.uint8) for _ in range(k)]
        lb = [ctx.array(labels, dtype=np.uint8) for _ in range(k)]
        out = [ctx.empty((B, 3, H, W)) for _ in range(k)]
        st = time_kernel(ctx, lambda i: lib.deepim_ingest_bgr8_pool(h, out[i], fr[i], lb[i], use_bg, bg_index, pool.pixels, pool.desc,
                                                                    pool.xtab, pool.ytab, POOL, MEANS_RGB, B, H, W),
                         a.reps, a.rounds, k)
        st.update(bytes=nbytes, sets=k, share_of_copy_rate=nbytes / (st["median"] * 1e-6) / COPY_RATE)
        res["kernels"]["ingest_bgr8_pool (%s)" % mode] = st
        print("ingest_bgr8_pool %-9s %3d sets %8.1f us/call (min %.1f max %.1f)  %6.2f TB/s  %.2f of the copy rate"
              % (mode, k, st["median"], st["min"], st["max"], nbytes / st["median"] / 1e6, st["share_of_copy_rate"]))
        if k > 1:       # the parent's composite on the same sets, its background a third stream from HBM
            bgs = [ctx.array(frames[::-1], dtype=np.uint8) for _ in range(k)]
            so = time_kernel(ctx, lambda i: lib.deepim_ingest_bgr8(h, out[i], fr[i], bgs[i], lb[i], use_bg, MEANS_RGB, B, H, W),
                             a.reps, a.rounds, k)
            so.update(bytes=n * (7 + 12), sets=k, share_of_copy_rate=n * 19 / (so["median"] * 1e-6) / COPY_RATE)
            res["kernels"]["ingest_bgr8+bg (rotating)"] = so
            print("ingest_bgr8+bg   rotating  %3d sets %8.1f us/call (min %.1f max %.1f)" % (k, so["median"], so["min"], so["max"]))
            del bgs
        del fr, lb, out
    u, x = ctx.empty((B,), np.int32), ctx.empty((B,), np.int32)
    st = time_kernel(ctx, lambda i: lib.deepim_sample_backgrounds(h, u, x, None, ctypes.c_double(0.5), POOL, 25, 0, ids, B), a.reps,
                     a.rounds)
    st["bytes"] = B * 16
    res["kernels"]["sample_backgrounds"] = st
    print("sample_backgrounds %8.2f us/call (min %.2f max %.2f)" % (st["median"], st["min"], st["max"]))

    # ---- (b) the two routes for one batch, frames and labels resident
    d_fr, d_lb = ctx.array(frames, dtype=np.uint8), ctx.array(labels, dtype=np.uint8)
    ready_bg = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)       # stands for the host's cropped and resized backgrounds
    out = ctx.empty((B, 3, H, W))

    def route_parent():
        t0 = time.perf_counter()
        d_bg = ctx.array(ready_bg, dtype=np.uint8)
        lib.deepim_ingest_bgr8(h, out, d_fr, d_bg, d_lb, use_bg, MEANS_RGB, B, H, W)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    def route_pool():
        t0 = time.perf_counter()
        ub, ix = background_draws_device(ctx, B, 25, ids, 1.0, POOL)
        lib.deepim_ingest_bgr8_pool(h, out, d_fr, d_lb, ub, ix, pool.pixels, pool.desc, pool.xtab, pool.ytab, POOL, MEANS_RGB, B, H, W)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(3):
        route_parent(), route_pool()
    old, new = [], []
    for _ in range(a.feed_rounds):
        old.append(route_parent())
        new.append(route_pool())
    res["routes"] = {"parent_upload_plus_composite_ms": stats(old), "pool_draws_plus_kernel_ms": stats(new),
                     "pcie_bytes_parent": n * 3, "pcie_bytes_pool": 0}
    for k in ("parent_upload_plus_composite_ms", "pool_draws_plus_kernel_ms"):
        v = res["routes"][k]
        print("route %-34s %.3f ms (min %.3f max %.3f)" % (k, v["median"], v["min"], v["max"]))

    # ---- (c) a whole loader step
    cfg = default_config()
    cfg.TRAIN.REPLACE_OBSERVED_BG_RATIO = 1.0
    rm, observed, points = loader_world(ctx, cfg, B, H, W, rng)
    loaders = {"without": TrainDataLoader(observed, cfg, rm, batch_size=B, seed=25, points=points),
               "with": TrainDataLoader(observed, cfg, rm, batch_size=B, seed=25, points=points, backgrounds=pool)}
    times = {"without": [], "with": []}
    for r in range(a.feed_rounds + 2):
        for name, ld in loaders.items():
            t0 = time.perf_counter()
            batch = ld.make_batch(ld.pairs[0], ld.draw_ids[0] + np.uint64(r))
            ctx.sync()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            del batch
    res["loader"] = {"step_ms_" + k: stats(v) for k, v in times.items()}
    for k, v in res["loader"].items():
        print("loader %-20s %.2f ms (min %.2f max %.2f)" % (k, v["median"], v["min"], v["max"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
