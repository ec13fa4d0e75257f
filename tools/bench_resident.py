"""Dev probe: what a device-resident observed set (mx_deepim_amd/core/resident.ResidentObserved) saves both loaders at 480x640.
usage: bench_resident.py [--batch 32] [--rounds 7] [--reps 100]

  train     one TrainDataLoader step (make_batch), host clock to a device synchronise, over the host set and over the resident
            set: same scene, same seed, alternating in one process
  test      the same for TestDataLoader (shared frames, two pairs per frame)
  bytes     what one batch of each uploads (Context.array / DeviceArray.copyfrom from the host, counted)
  bgr       deepim_ingest_bgr8_frames reading B frames of the resident set through a shuffled index, against deepim_ingest_bgr8 on
            B contiguous frames: HIP events around --reps back-to-back calls, per call
  points    deepim_gather_rows on the per-class point tables (model and weights), HIP events, against the stack + upload of the
            same rows it replaces, host clock to a device synchronise
Medians of --rounds rounds after a warm-up, min … max beside them; the last line is one JSON record. Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.core.loader import ResidentObserved, TestDataLoader, TrainDataLoader  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py  # noqa: E402
from mx_deepim_amd.runtime import Context, DeviceArray, lib  # noqa: E402

H, W = 480, 640
AXES = [0.05, 0.04, 0.035]


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


class Uploads(object):
    """Counts the bytes Context.array and DeviceArray.copyfrom move from the host while it is active."""

    def __enter__(self):
        self.bytes, self._array, self._copyfrom = 0, Context.array, DeviceArray.copyfrom
        me = self

        def array(ctx, host, dtype=np.float32):
            a = me._array(ctx, host, dtype)
            me.bytes += a.nbytes
            return a

        def copyfrom(dst, src):
            if not isinstance(src, DeviceArray):
                me.bytes += dst.nbytes
            return me._copyfrom(dst, src)

        Context.array, DeviceArray.copyfrom = array, copyfrom
        return self

    def __exit__(self, *exc):
        Context.array, DeviceArray.copyfrom = self._array, self._copyfrom


def alternate(ctx, steps, rounds):
    """[(median, min, max) ms per step] of the callables `steps`, run in turn `rounds` + 2 times, host clock to a synchronise"""
    ms = [[] for _ in steps]
    for r in range(rounds + 2):
        for i, step in enumerate(steps):
            ctx.sync()
            t0 = time.perf_counter()
            out = step(r)              # noqa: F841 (kept alive to the synchronise)
            ctx.sync()
            if r >= 2:
                ms[i].append(1e3 * (time.perf_counter() - t0))
    return [med(m) for m in ms]


def events(ctx, call, rounds, reps):
    """(median, min, max) us per call of `call`, HIP events around `reps` back-to-back calls"""
    for _ in range(5):
        call()
    t, per = ctx.timer(), []
    for _ in range(rounds):
        t.start()
        for _ in range(reps):
            call()
        t.stop()
        per.append(1e3 * t.elapsed_ms() / reps)
    return med(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    B = args.batch
    ctx = Context.get(0)
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = True
    K = np.ascontiguousarray(synthetic.K_LINEMOD, np.float32)
    mesh = dict(synthetic.ellipsoid_mesh(AXES), texture=synthetic.procedural_texture())
    mesh.pop("colors")
    rm = Render_Py("synthetic", ["ellipsoid"], K, W, H, 0.25, 6.0, meshes={"ellipsoid": mesh}, ctx=ctx,
                   pixel_means=synthetic.PIXEL_MEANS[::-1].copy())
    rng = np.random.default_rng(2333)
    M = 2 * B
    poses = np.stack([synthetic.sample_pose_pair(rng)[0] for _ in range(M)])
    image, depth = rm.render_batch(ctx.zeros((M,), np.int32), ctx.array(poses))
    rgb = image.asnumpy() + rm.pixel_means.reshape(1, 3, 1, 1)
    d16 = np.rint(depth.asnumpy()[:, 0] * 1000.0).astype(np.uint16)
    observed = {"image_observed": np.ascontiguousarray(np.clip(np.rint(rgb), 0, 255).astype(np.uint8)[:, ::-1].transpose(0, 2, 3, 1)),
                "depth_gt_observed": d16, "mask_gt_observed": (d16 > 0).astype(np.uint8), "mask_idx": np.ones(M, np.int32),
                "pose_observed": poses, "class_index": np.zeros(M, np.int32)}
    del image, depth, rgb
    n_pts = cfg.train_iter.NUM_3D_SAMPLE
    points = {0: (synthetic.sample_model_points(rng, AXES, n_pts), np.ones((3, n_pts), np.float32))}

    ctx.sync()
    t0 = time.perf_counter()
    res = ResidentObserved(observed, ctx, points=points)
    ctx.sync()
    build_ms = 1e3 * (time.perf_counter() - t0)

    # ---- the training loader
    kw = dict(batch_size=B, shuffle=True, seed=3, points=points)
    train = [TrainDataLoader(observed, cfg, rm, **kw), TrainDataLoader(res, cfg, rm, **kw)]
    train_ms = alternate(ctx, [lambda r, ld=ld: ld.make_batch(ld.pairs[r % len(ld)], ld.draw_ids[r % len(ld)]) for ld in train], args.rounds)
    train_up = []
    for ld in train:
        with Uploads() as up:
            ld.make_batch(ld.pairs[0], ld.draw_ids[0])
        train_up.append(up.bytes)

    # ---- the test loader: two pairs per frame, shared frames
    pairdb = [{"frame": p // 2, "gt_class": "ellipsoid", "mask_idx": 1, "pose_observed": poses[p // 2],
               "pose_rendered": synthetic.sample_pose_pair(rng)[0]} for p in range(2 * M)]
    test = [TestDataLoader(observed, pairdb, cfg, rm, batch_size=B), TestDataLoader(res, pairdb, cfg, rm, batch_size=B)]
    test_ms = alternate(ctx, [lambda r, ld=ld: ld.make_batch(ld.pairs[r % len(ld)]) for ld in test], args.rounds)
    test_up = []
    for ld in test:
        with Uploads() as up:
            ld.make_batch(ld.pairs[0])
        test_up.append(up.bytes)

    # ---- the BGR entry through an index against the per-sample entry on contiguous frames
    means = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1], np.float32)
    out = ctx.empty((B, 3, H, W))
    index = ctx.array(rng.permutation(M)[:B], dtype=np.int32)
    frames = res.arrays["image_observed"]
    contiguous = frames[0:B]
    bgr_idx = events(ctx, lambda: lib.deepim_ingest_bgr8_frames(ctx.handle, out, frames, index, res.rows, means, B, H, W), args.rounds, args.reps)
    bgr_seq = events(ctx, lambda: lib.deepim_ingest_bgr8(ctx.handle, out, contiguous, None, None, None, means, B, H, W), args.rounds, args.reps)
    bgr_idx2 = events(ctx, lambda: lib.deepim_ingest_bgr8_frames(ctx.handle, out, frames, index, res.rows, means, B, H, W), args.rounds, args.reps)

    # ---- the point tables: two gathers against the stack + upload of the same rows
    cls_host = np.zeros(B, np.int32)
    cls = ctx.array(cls_host, dtype=np.int32)
    o0, o1 = ctx.empty((B, 3, n_pts)), ctx.empty((B, 3, n_pts))

    def gather():
        lib.deepim_gather_rows(ctx.handle, o0, res.point_tables[0], cls, 1, 3 * n_pts, B)
        lib.deepim_gather_rows(ctx.handle, o1, res.point_tables[1], cls, 1, 3 * n_pts, B)

    gather_us = events(ctx, gather, args.rounds, args.reps)
    upload_ms = alternate(ctx, [lambda r: (ctx.array(np.stack([points[int(c)][0] for c in cls_host])),
                                           ctx.array(np.stack([points[int(c)][1] for c in cls_host])))], args.rounds)[0]

    print("resident set: %d frames, %.1f MB on the device, built in %.1f ms" % (M, res.nbytes / 1e6, build_ms))
    print("train loader step, B = %d: host set %.2f ms (%.2f … %.2f), resident %.2f ms (%.2f … %.2f)" % ((B,) + train_ms[0] + train_ms[1]))
    print("test loader step,  B = %d: host set %.2f ms (%.2f … %.2f), resident %.2f ms (%.2f … %.2f)" % ((B,) + test_ms[0] + test_ms[1]))
    print("uploaded per batch: train %d B -> %d B, test %d B -> %d B" % (train_up[0], train_up[1], test_up[0], test_up[1]))
    print("BGR ingest, B = %d: through the index %.1f us (%.1f … %.1f) and again %.1f us (%.1f … %.1f); contiguous per-sample "
          "%.1f us (%.1f … %.1f)" % ((B,) + bgr_idx + bgr_idx2 + bgr_seq))
    print("point clouds, B = %d x 2 x 3 x %d floats: two gathers %.1f us (%.1f … %.1f); stack + upload %.3f ms (%.3f … %.3f)"
          % ((B, n_pts) + gather_us + upload_ms))
    print(json.dumps({"batch": B, "frames": M, "resident_mb": res.nbytes / 1e6, "build_ms": build_ms,
                      "train_step_host_ms": train_ms[0][0], "train_step_resident_ms": train_ms[1][0],
                      "test_step_host_ms": test_ms[0][0], "test_step_resident_ms": test_ms[1][0],
                      "train_upload_bytes": train_up, "test_upload_bytes": test_up,
                      "bgr_indexed_us": bgr_idx[0], "bgr_indexed_again_us": bgr_idx2[0], "bgr_contiguous_us": bgr_seq[0],
                      "points_gather_us": gather_us[0], "points_upload_ms": upload_ms[0]}))


if __name__ == "__main__":
    main()
