"""The test-phase loader (core/loader.TestDataLoader, csrc/render.hip deepim_render_frames_forward, csrc/ingest.hip
deepim_mask_gate) at 480x640 with two ellipsoid meshes, one textured and one vertex-coloured:

    python tools/bench_test_loader.py [--batch 32] [--reps 100] [--rounds 7] [--feed-rounds 9] [--eval-batches 4] [--json PATH]

(a) The frame draw's launch group (memset of `covered`, project, raster, resolve): HIP events around `reps` back-to-back calls,
    `rounds` rounds after a warm-up, median and range, rotating over enough output sets that twice the 256 MiB Infinity Cache
    passes between two uses of a buffer, and on one set. The resolve pass alone is the same call with every class id outside the
    table: project and raster exit at once and the resolve pass still reads the whole z-buffer (8 B/px) and stores the two
    frames (5 B/px; 6 with a label map). Its share is of the copy rate tools/bench_ingest.py uses. (Per-kernel times of the
    drawn batch come from a kernel trace of this tool, see profiles/r29_test_loader.md.) deepim_mask_gate next to it, with none
    and with all of the planes empty.
(b) One loader step (make_batch + synchronise) against the host route there was before: the float draw
    (deepim_render_classes_forward), read-back, numpy quantisation, upload of the rendered frames and of the observed frame of
    every pair (B copies, as a per-pair batch has them), get_data_pair_test_batch. Alternating, host wall-clock.
(c) The loader's share of a pred_eval batch: pred_eval over ready-made batches against pred_eval over the loader, same pairs,
    default configuration (test_iter 4, FAST_TEST), wall-clock of the whole call divided by the number of batches."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ingest import COPY_RATE, stats, time_kernel  # noqa: E402
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.core import tester  # noqa: E402
from mx_deepim_amd.core.loader import TestDataLoader  # noqa: E402
from mx_deepim_amd.lib.dataset.LM6D_REFINE import LM6D_REFINE  # noqa: E402
from mx_deepim_amd.lib.pair_matching import data_pair  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py  # noqa: E402
from mx_deepim_amd.lib.utils import image as dimage  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402
from mx_deepim_amd.symbols import deepIM_flownet  # noqa: E402

AXES = ([0.05, 0.04, 0.035], [0.03, 0.06, 0.04])
CLASSES = ["a", "b"]
PER_FRAME = 4          # objects per camera frame


class _Quiet(object):
    def info(self, *a):
        pass


def world(ctx, cfg, n_pairs, H, W, rng):
    """(render machine, observed, pairdb): n_pairs pairs, PER_FRAME to a frame, observed frames made of the ground-truth draws."""
    meshes = {}
    for name, axes in zip(CLASSES, AXES):
        meshes[name] = synthetic.ellipsoid_mesh(axes, 24, 48)
    meshes["a"].pop("colors")
    meshes["a"]["texture"] = synthetic.procedural_texture()
    meshes["b"].pop("uv")
    rm = Render_Py("unused", CLASSES, cfg.dataset.INTRINSIC_MATRIX, W, H, meshes=meshes, ctx=ctx,
                   pixel_means=np.asarray(dimage._means_rgb(cfg), np.float32))
    F = -(-n_pairs // PER_FRAME)
    observed = {"image_observed": rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)}
    pairdb = []
    for p in range(n_pairs):
        gt, init = synthetic.sample_pose_pair(rng)[:2]
        pairdb.append({"frame": p // PER_FRAME, "gt_class": CLASSES[p % 2], "mask_idx": 1 + p % PER_FRAME,
                       "pose_observed": np.asarray(gt, np.float32), "pose_rendered": np.asarray(init, np.float32)})
    return rm, observed, pairdb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--feed-rounds", type=int, default=9)
    ap.add_argument("--eval-batches", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, H, W = a.batch, 480, 640
    n = B * H * W
    ctx = Context.get(0)
    h = ctx.handle
    cfg = default_config()
    rng = np.random.default_rng(29)
    rm, observed, pairdb = world(ctx, cfg, B * a.eval_batches, H, W, rng)
    res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "kernels": {}, "routes": {}, "pred_eval": {}}

    # ---- (a) the kernels
    cls_host = np.array([CLASSES.index(r["gt_class"]) for r in pairdb[:B]], np.int32)
    poses_host = np.stack([r["pose_rendered"] for r in pairdb[:B]])
    poses = ctx.array(poses_host)
    covered = ctx.empty((B,), np.int32)
    for what, ids in (("drawn", cls_host), ("empty: the resolve pass alone", np.full(B, -1, np.int32))):
        cls = ctx.array(ids, dtype=np.int32)
        for mode, k in (("rotating", -(-2 * (256 << 20) // (n * 5)) + 1), ("one set", 1)):
            sets = [(ctx.empty((B, H, W, 3), np.uint8), ctx.empty((B, H, W), np.uint16)) for _ in range(k)]
            st = time_kernel(ctx, lambda i: rm.render_frames_into(sets[i][0], sets[i][1], cls, poses, covered=covered), a.reps, a.rounds, k)
            st.update(bytes=n * (8 + 5), sets=k, share_of_copy_rate=n * 13 / (st["median"] * 1e-6) / COPY_RATE)
            res["kernels"]["render_frames_forward, %s (%s)" % (what, mode)] = st
            print("render_frames_forward %-30s %-9s %3d sets %8.1f us/call (min %.1f max %.1f)  %5.2f TB/s  %.2f of the copy rate"
                  % (what, mode, k, st["median"], st["min"], st["max"], n * 13 / st["median"] / 1e6, st["share_of_copy_rate"]))
            del sets
    rm.render_frames_into(ctx.empty((B, H, W, 3), np.uint8), ctx.empty((B, H, W), np.uint16), ctx.array(cls_host, dtype=np.int32), poses,
                          covered=covered)
    res["covered_mean_px"] = float(covered.asnumpy().mean())
    kf = -(-2 * (256 << 20) // (n * 16)) + 1
    fsets = [(ctx.empty((B, 3, H, W)), ctx.empty((B, 1, H, W))) for _ in range(kf)]
    cls = ctx.array(cls_host, dtype=np.int32)
    st = time_kernel(ctx, lambda i: rm.render_classes_into(fsets[i][0], fsets[i][1], cls, poses, pixel_means=None), a.reps, a.rounds, kf)
    st.update(bytes=n * 24, sets=kf, share_of_copy_rate=n * 24 / (st["median"] * 1e-6) / COPY_RATE)
    res["kernels"]["render_classes_forward, float tensors (rotating)"] = st
    print("render_classes_forward float tensors, rotating %3d sets %8.1f us/call (min %.1f max %.1f)  %.2f of the copy rate"
          % (kf, st["median"], st["min"], st["max"], st["share_of_copy_rate"]))
    del fsets
    mask = ctx.zeros((B, 1, H, W))
    for what, cov in (("no plane empty", np.ones(B, np.int32)), ("every plane empty", np.zeros(B, np.int32))):
        cov_d = ctx.array(cov, dtype=np.int32)
        st = time_kernel(ctx, lambda i: lib.deepim_mask_gate(h, mask, cov_d, B, H, W), a.reps, a.rounds)
        res["kernels"]["mask_gate, " + what] = st
        print("mask_gate %-18s %8.2f us/call (min %.2f max %.2f)" % (what, st["median"], st["min"], st["max"]))

    # ---- (b) one loader step against the host route
    loader = TestDataLoader(observed, pairdb, cfg, rm, batch_size=B)
    per_pair = TestDataLoader(observed, pairdb, cfg, rm, batch_size=B, shared_frames=False)
    pairs = loader.pairs[0]

    def route_host():
        t0 = time.perf_counter()
        recs = [pairdb[p] for p in pairs]
        ids = ctx.array(per_pair.class_index[pairs], dtype=np.int32)
        pose = ctx.array(per_pair.pose_rendered[pairs])
        image, depth = ctx.empty((B, 3, H, W)), ctx.empty((B, 1, H, W))
        rm.render_classes_into(image, depth, ids, pose, pixel_means=None)
        bgr = np.ascontiguousarray(np.rint(np.clip(image.asnumpy(), 0, 255)).astype(np.uint8)[:, ::-1].transpose(0, 2, 3, 1))
        d16 = (depth.asnumpy()[:, 0] * np.float32(1000)).astype(np.uint16)
        frames = {"image_observed": ctx.array(observed["image_observed"][per_pair.frame[pairs]], dtype=np.uint8),
                  "image_rendered": ctx.array(bgr, dtype=np.uint8), "depth_rendered": ctx.array(d16, dtype=np.uint16),
                  "mask_idx": ctx.array(per_pair.mask_idx[pairs], dtype=np.int32), "class_index": ids, "pose_rendered": pose}
        out = data_pair.get_data_pair_test_batch(frames, cfg), frames, recs
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def route(ld):
        t0 = time.perf_counter()
        out = ld.make_batch(pairs)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    (_t, old_out), (_t, new_out) = route_host(), route(per_pair)
    same = all(np.array_equal(old_out[0][k].asnumpy(), new_out[0][k].asnumpy())
               for k in ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "src_pose"))
    res["routes_give_the_same_batch"] = bool(same)
    print("the host route and the per-pair loader give the same batch:", same)
    del old_out, new_out
    times = {"host_float_draw_readback_quantise_upload_ms": [], "loader_shared_frames_ms": [], "loader_per_pair_ms": []}
    for r in range(a.feed_rounds + 2):
        for name, fn in (("host_float_draw_readback_quantise_upload_ms", route_host), ("loader_shared_frames_ms", lambda: route(loader)),
                         ("loader_per_pair_ms", lambda: route(per_pair))):
            t, out = fn()
            del out
            if r >= 2:
                times[name].append(t)
    res["routes"] = {k: stats(v) for k, v in times.items()}
    res["routes"].update(pcie_bytes_host=n * (16 + 5 + 3), pcie_bytes_loader_shared=(B // PER_FRAME) * H * W * 3,
                         pcie_bytes_loader_per_pair=n * 3)
    for k in times:
        v = res["routes"][k]
        print("route %-46s %.3f ms (min %.3f max %.3f)" % (k, v["median"], v["min"], v["max"]))

    # ---- (c) the loader's share of a pred_eval batch
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=20)
    params["trans_weight"] = params["trans_weight"] * np.float32(0.02)
    params["trans_bias"] = params["trans_bias"] * np.float32(0.02)
    net.bind(ctx, B, params)
    points = {c: rm.mesh_list[i].host["vertices"][::7] for i, c in enumerate(CLASSES)}
    diameters = {c: 0.1 for c in CLASSES}
    ready = list(loader)
    ctx.sync()
    walls = {"ready_made_batches": [], "loader": []}
    for r in range(3):
        for name, data in (("ready_made_batches", ready), ("loader", loader)):
            with tempfile.TemporaryDirectory() as tmp:
                imdb = LM6D_REFINE(CLASSES, points, diameters, ctx=ctx, logger=_Quiet(), name="bench", result_path=tmp)
                t0 = time.perf_counter()
                tester.pred_eval(cfg, tester.Predictor(cfg, net), data, imdb, logger=_Quiet(), render_machine=rm)
                ctx.sync()
                if r >= 1:
                    walls[name].append((time.perf_counter() - t0) * 1e3 / len(ready))
    a_ms, b_ms = stats(walls["ready_made_batches"])["median"], stats(walls["loader"])["median"]
    res["pred_eval"] = {"ms_per_batch_ready_made": stats(walls["ready_made_batches"]), "ms_per_batch_over_the_loader": stats(walls["loader"]),
                        "loader_share": (b_ms - a_ms) / b_ms, "test_iter": int(cfg.TEST.test_iter), "batches": len(ready)}
    print("pred_eval per batch: %.2f ms over ready-made batches, %.2f ms over the loader: the loader is %.1f %% of a batch"
          % (a_ms, b_ms, 100 * (b_ms - a_ms) / b_ms))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
