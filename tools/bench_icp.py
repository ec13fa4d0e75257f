"""The depth ICP (csrc/icp.hip, lib/pair_matching/depth_icp.py) on the GPU at 480x640: time per call and achieved HBM traffic of
the normal pass and of one Gauss-Newton step, and a full DepthICP.refine as a share of a pred_eval batch.

    python tools/bench_icp.py [--batch 32] [--reps 200] [--rounds 7] [--feed-rounds 7] [--no-loop] [--json PATH]

Method of tools/bench_flow_epe.py. Kernel time: HIP events around `reps` back-to-back calls, `rounds` rounds after a warm-up,
median and range; once rotating over enough buffer sets that twice the 256 MiB Infinity Cache passes between two uses of a
buffer (the HBM figure), once on one set. Bytes are what the algorithm has to move. Normal pass: the depth read once and three
normal planes written, 16 B/pixel. Step: the source depth read once (4 B/pixel) plus, for a source pixel with a depth, one
gather of the target depth and normal (16 B; counted as the frame's share of such pixels, with 20 B/pixel printed as the upper
bound); the block partials and the finish are not counted. The share is of the measured copy rate of the device (6.29 TB/s).
The refine and the test loop are host wall clock around work that ends in a device synchronise (refine) or in pred_eval's own
read-backs: a test loop over two batches with TEST.DEPTH_ICP off and on, alternating, seeded weights and synthetic frames."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.lib.pair_matching.depth_icp import DepthICP  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402

COPY_RATE = 6.29e12     # bytes/s, the measured device copy rate the project's notes use
CLASSES = ["ape", "cat"]
MEANS_BGR = np.array([104.0, 117.0, 124.0])


class NullLogger(object):
    def info(self, *a):
        pass


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


def to_bgr8(t):
    rgb = t + synthetic.PIXEL_MEANS[::-1].reshape(1, 3, 1, 1)
    return np.ascontiguousarray(np.clip(np.rint(rgb), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)[..., ::-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--feed-rounds", type=int, default=7)
    ap.add_argument("--no-loop", action="store_true", help="kernels and refine only: no network, no pred_eval")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, H, W = a.batch, 480, 640
    n = B * H * W
    ctx = Context.get(0)
    h = ctx.handle
    # four distinct synthetic pairs, tiled over the batch: object pixels (projection + gather) and background in a real ratio
    d = synthetic.make_batch(4, seed=20, n_frames=1)
    order = [i % 4 for i in range(B)]
    dr = d["depth_rendered"][0][order]
    do = d["depth_gt_observed"][order]
    K = np.ascontiguousarray(d["K"], np.float32).reshape(3, 3)
    obj_share = float((dr != 0).mean())
    CACHE = 256 << 20
    res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "object_pixel_share": obj_share, "kernels": {}}
    identity = ctx.array(np.tile(np.eye(3, 4, dtype=np.float32), (B, 1, 1)))

    def make_normals(k):
        sets = [(ctx.array(do), ctx.empty((B, 3, H, W))) for _ in range(k)]
        return (lambda i: lib.deepim_depth_normals(h, sets[i][1], sets[i][0], K, ctypes.c_float(0.01), B, H, W)), sets

    def make_step(k):
        sets = []
        for _ in range(k):
            tgt, nrm = ctx.array(do), ctx.empty((B, 3, H, W))
            lib.deepim_depth_normals(h, nrm, tgt, K, ctypes.c_float(0.01), B, H, W)
            sets.append((ctx.array(dr), tgt, nrm))
        T, status = ctx.empty((B, 3, 4)), ctx.empty((B,), dtype=np.int32)

        def fn(i):
            T.copyfrom(identity)            # every call solves the same first step (a 1.5 KB copy on the stream)
            lib.deepim_icp_step(h, T, None, status, sets[i][0], sets[i][1], sets[i][2], K, None, ctypes.c_float(0.02), 12,
                                ctypes.c_double(1e-9), B, H, W)
        return fn, sets

    for name, make, per_set, nbytes, upper in (("depth_normals", make_normals, n * 16, n * 16, n * 16),
                                               ("icp_step", make_step, n * 20, int(n * (4 + 16 * obj_share)), n * 20)):
        for mode, k in (("rotating", -(-2 * CACHE // per_set) + 1), ("one set", 1)):
            fn, keep = make(k)
            st = time_kernel(ctx, fn, a.reps, a.rounds, k)
            st["bytes"], st["bytes_upper_bound"], st["sets"] = nbytes, upper, k
            st["share_of_copy_rate"] = nbytes / (st["median"] * 1e-6) / COPY_RATE
            st["share_of_copy_rate_upper_bound_bytes"] = upper / (st["median"] * 1e-6) / COPY_RATE
            res["kernels"]["%s (%s)" % (name, mode)] = st
            print("%-13s %-9s %3d sets %8.1f us/call (min %.1f max %.1f)  %6.2f TB/s  %.2f of the copy rate (%.2f at the upper bound)" %
                  (name, mode, k, st["median"], st["min"], st["max"], nbytes / st["median"] / 1e6, st["share_of_copy_rate"],
                   st["share_of_copy_rate_upper_bound_bytes"]))
            del fn, keep

    # ---- a full refine (outer = 2, inner = 5: one normal pass, two draws, ten steps, two applies) ---------------------------
    meshes = {}
    for i, c in enumerate(CLASSES):
        m = synthetic.ellipsoid_mesh(np.array([0.05, 0.04, 0.035]) * (1.0 + 0.2 * i), 12, 24)
        m.pop("uv")
        meshes[c] = m
    cfg = default_config()
    cfg.network.PIXEL_MEANS = MEANS_BGR.astype(np.float32)
    cfg.dataset.class_name = list(CLASSES)
    rm = Render_Py("unused", CLASSES, K, W, H, meshes=meshes, ctx=ctx, pixel_means=MEANS_BGR[::-1].astype(np.float32))
    icp = DepthICP(rm, cfg)
    poses = ctx.array(d["src_pose"][0][order])
    ids = ctx.array(np.array([i % 2 for i in range(B)], np.int32), dtype=np.int32)
    depth_obs, out = ctx.array(do), ctx.empty((B, 3, 4))
    ms = []
    for r in range(a.feed_rounds + 2):
        ctx.sync()
        t0 = time.perf_counter()
        icp.refine(poses, ids, depth_obs, K=K, out=out)
        ctx.sync()
        if r >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    res["refine_ms"] = stats(ms)
    print("refine (outer 2, inner 5) + sync   %.3f ms (min %.3f max %.3f)" % (res["refine_ms"]["median"], min(ms), max(ms)))

    # ---- the test loop over two batches, TEST.DEPTH_ICP off and on ---------------------------------------------------------
    if not a.no_loop:
        from mx_deepim_amd.core import tester
        from mx_deepim_amd.lib.dataset.LM6D_REFINE import LM6D_REFINE
        from mx_deepim_amd.lib.pair_matching import data_pair
        from mx_deepim_amd.symbols import deepIM_flownet

        cfg.TEST.test_iter, cfg.TEST.FAST_TEST = 2, True
        net = deepIM_flownet().get_symbol(cfg)
        params = net.init_weights(cfg, seed=20)
        params["trans_weight"] = params["trans_weight"] * np.float32(0.02)
        params["trans_bias"] = params["trans_bias"] * np.float32(0.02)
        net.bind(ctx, B, params)
        dep_o = do[:, 0]
        frames = {"image_observed": to_bgr8(d["image_observed"][order]), "image_rendered": to_bgr8(d["image_rendered"][0][order]),
                  "depth_rendered": np.rint(dr[:, 0] * 1000).astype(np.uint16),
                  "depth_gt_observed": np.rint(dep_o * 1000).astype(np.uint16), "depth_observed": np.rint(dep_o * 1000).astype(np.uint16),
                  "mask_gt_observed": ((dep_o > 0) * 3).astype(np.uint8), "mask_idx": np.full(B, 3, np.int32),
                  "pose_rendered": d["src_pose"][0][order].copy()}
        recs = [{"pose_rendered": d["src_pose"][0][i].copy(), "pose_observed": d["pose_tgt"][i].copy(), "gt_class": CLASSES[j % 2]}
                for j, i in enumerate(order)]
        points = {c: meshes[c]["vertices"][::7] for c in CLASSES}
        diameters = {c: 0.1 + 0.02 * i for i, c in enumerate(CLASSES)}
        log = NullLogger()
        tmp = tempfile.mkdtemp()
        imdb = LM6D_REFINE(CLASSES, points, diameters, ctx=ctx, logger=log, name="bench_icp", result_path=tmp)

        def loop(on):
            cfg.TEST.DEPTH_ICP = on
            data = [(data_pair.get_data_pair_test_batch(frames, cfg), frames, recs) for _ in range(2)]
            ctx.sync()
            t0 = time.perf_counter()
            tester.pred_eval(cfg, tester.Predictor(cfg, net), data, imdb, ignore_cache=True, logger=log, render_machine=rm)
            return (time.perf_counter() - t0) * 1e3 / 2

        loop(False), loop(True)
        off, on = [], []
        for _ in range(a.feed_rounds):
            off.append(loop(False))
            on.append(loop(True))
        res["pred_eval_batch_ms"] = {"off": stats(off), "on": stats(on)}
        res["refine_share_of_batch"] = res["refine_ms"]["median"] / res["pred_eval_batch_ms"]["off"]["median"]
        print("pred_eval per batch (with its evaluation), key off %.2f ms (min %.2f max %.2f), on %.2f ms (min %.2f max %.2f); "
              "refine = %.3f of a batch with the key off" % (stats(off)["median"], min(off), max(off), stats(on)["median"], min(on),
                                                            max(on), res["refine_share_of_batch"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
