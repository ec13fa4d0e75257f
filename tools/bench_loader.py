"""Dev probe: what the device loader (mx_deepim_amd/core/loader.TrainDataLoader) costs per batch at 480x640, next to the training
step it feeds.  usage: bench_loader.py [--batch 32] [--rounds 7] [--reps 200] [--pose]

  sampler   deepim_sample_rendered_poses alone on resident poses: HIP events around --reps back-to-back calls, per call
  draw      the pose draw as the loader pays for it, host clock to a device synchronise: upload of the draw ids + the kernel,
            against a HOST feed that draws the same rule in numpy (toolkit/LM6d_1_gen_rendered_pose.py:80-107) and uploads
            the poses
  loader    one whole loader step, host clock to a device synchronise: gather + upload of the uint8 / uint16 frames, ingest,
            draw, render, labels (make_batch)
  step      net.train_step of that batch (TRAIN_ITER_SIZE iterations, device batch updater), HIP events
Medians of --rounds rounds after a warm-up, min … max beside them; the last line is one JSON record. `--pose` trains the pose
branch only (no decoder, flow and mask heads). Needs a GPU: there is no host fall-back."""
import argparse
import ctypes
import json
import os
import sys
import time
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.core.loader import TrainDataLoader  # noqa: E402
from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import batchUpdaterPyMulti  # noqa: E402
from mx_deepim_amd.lib.pair_matching.pose_sampler import POSE_NOISE_DEFAULTS, noise_array, sample_rendered_poses  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402
from mx_deepim_amd.symbols import deepIM_flownet  # noqa: E402

H, W = 480, 640
AXES = [0.05, 0.04, 0.035]


def host_draw(rng, poses, K, n=POSE_NOISE_DEFAULTS):
    """The toolkit's loop in numpy for a batch of float32 poses -> float32 poses (the host feed the device draw replaces)."""
    out = poses.copy()
    for b, P in enumerate(poses.astype(np.float64)):
        R = P[:, :3]
        e = np.array([np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], np.hypot(R[0, 0], R[1, 0])), np.arctan2(R[1, 0], R[0, 0])])
        for _ in range(n["max_attempts"]):
            a = e + rng.normal(0, n["angle_std"] / 180 * pi, 3)
            t = P[:, 3] + rng.normal(0, 1, 3) * [n["x_std"], n["y_std"], n["z_std"]]
            (si, sj, sk), (ci, cj, ck) = np.sin(a), np.cos(a)
            Rt = np.array([[cj * ck, sj * si * ck - ci * sk, sj * ci * ck + si * sk],
                           [cj * sk, sj * si * sk + ci * ck, sj * ci * sk - si * ck], [-sj, cj * si, cj * ci]])
            M = R.T @ Rt
            s = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
            r_dist = np.degrees(np.arctan2(np.sqrt(s @ s), (np.trace(M) - 1) / 2))
            c = K @ t
            if r_dist <= n["angle_max"] and t[2] > 0 and n["border"] < c[0] / c[2] < W - n["border"] and n["border"] < c[1] / c[2] < H - n["border"]:
                out[b, :, :3], out[b, :, 3] = Rt, t
                break
    return out


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--pose", action="store_true")
    args = ap.parse_args()
    B = args.batch
    ctx = Context.get(0)
    cfg = default_config()
    cfg.network.PRED_FLOW = cfg.network.PRED_MASK = not args.pose
    K = np.ascontiguousarray(synthetic.K_LINEMOD, np.float32)
    mesh = dict(synthetic.ellipsoid_mesh(AXES), texture=synthetic.procedural_texture())
    mesh.pop("colors")
    rm = Render_Py("synthetic", ["ellipsoid"], K, W, H, 0.25, 6.0, meshes={"ellipsoid": mesh}, ctx=ctx,
                   pixel_means=synthetic.PIXEL_MEANS[::-1].copy())
    # the observed set: M = 2B frames rendered at random ground-truth poses and quantised as a camera would
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
    loader = TrainDataLoader(observed, cfg, rm, batch_size=B, shuffle=True, seed=3, points=points)

    # ---- sampler kernel alone
    pose_dev = ctx.array(poses[:B])
    pose_out, att_out = ctx.empty((B, 3, 4)), ctx.empty((B,), np.int32)      # resident outputs: nothing but the launch is timed
    noise5, border = noise_array(POSE_NOISE_DEFAULTS), ctypes.c_float(POSE_NOISE_DEFAULTS["border"])

    def draw(base):
        lib.deepim_sample_rendered_poses(ctx.handle, pose_out, att_out, None, pose_dev, K, noise5, W, H, border,
                                         POSE_NOISE_DEFAULTS["max_attempts"], 3, base, None, B)
    for i in range(10):
        draw(i * B)
    t, per_call = ctx.timer(), []
    for r in range(args.rounds):
        t.start()
        for i in range(args.reps):
            draw((r * args.reps + i) * B)
        t.stop()
        per_call.append(1e3 * t.elapsed_ms() / args.reps)
    sampler_us = med(per_call)
    attempts = sample_rendered_poses(pose_dev, K, W, H, 3)[1].asnumpy()

    # ---- the draw as a feed pays for it: device (ids up, kernel) against host (numpy draw, poses up), alternating
    dev_ms, host_ms, hrng = [], [], np.random.RandomState(3)
    for r in range(args.rounds + 1):
        ctx.sync()
        t0 = time.perf_counter()
        out = sample_rendered_poses(pose_dev, K, W, H, 3, draw_ids=np.arange(r * B, (r + 1) * B))
        ctx.sync()
        t1 = time.perf_counter()
        out = ctx.array(host_draw(hrng, poses[:B], K.astype(np.float64)))      # noqa: F841
        ctx.sync()
        t2 = time.perf_counter()
        if r:
            dev_ms.append(1e3 * (t1 - t0))
            host_ms.append(1e3 * (t2 - t1))
    dev_draw, host_feed = med(dev_ms), med(host_ms)

    # ---- the whole loader step and the training step it feeds
    net = deepIM_flownet().get_symbol(cfg, is_train=True)
    net.bind_train(ctx, B, net.init_weights(cfg, seed=91), num_points=n_pts)
    upd = batchUpdaterPyMulti(cfg, H, W, render_machine=rm)
    loader_ms, step_ms, ts = [], [], ctx.timer()
    for r in range(args.rounds + 2):
        nb = r % len(loader)
        ctx.sync()
        t0 = time.perf_counter()
        data, label = loader.make_batch(loader.pairs[nb], loader.draw_ids[nb])
        ctx.sync()
        t1 = time.perf_counter()
        ts.start()
        net.train_step(data, label, upd, lr=1e-6)
        ts.stop()
        if r >= 2:
            loader_ms.append(1e3 * (t1 - t0))
            step_ms.append(ts.elapsed_ms())
        if nb == len(loader) - 1:
            loader.reset()
    lo, st = med(loader_ms), med(step_ms)
    stats = loader.stats()
    up_mb = B * H * W * (3 + 2 + 1) / 1e6
    print("sampler kernel, B = %d: %.2f us per call (%.2f … %.2f), mean %.2f attempts per pair" % ((B,) + sampler_us + (attempts.mean(),)))
    print("pose draw as a feed: device %.3f ms (%.3f … %.3f), host numpy + upload %.3f ms (%.3f … %.3f)" % (dev_draw + host_feed))
    print("loader step, B = %d (%.1f MB uploaded): %.2f ms (%.2f … %.2f)" % ((B, up_mb) + lo))
    print("train_step x%d, %s: %.2f ms (%.2f … %.2f); the loader step is %.1f %% of it"
          % ((cfg.network.TRAIN_ITER_SIZE, "pose branch" if args.pose else "full graph") + st + (100 * lo[0] / st[0],)))
    print("loader totals: %s" % stats)
    print(json.dumps({"batch": B, "graph": "pose" if args.pose else "heads", "sampler_us": sampler_us[0], "device_draw_ms": dev_draw[0],
                      "host_feed_ms": host_feed[0], "loader_step_ms": lo[0], "train_step_ms": st[0], "loader_share_of_step": lo[0] / st[0],
                      "uploaded_mb": up_mb, "mean_attempts": float(attempts.mean()), "stats": stats}))


if __name__ == "__main__":
    main()
