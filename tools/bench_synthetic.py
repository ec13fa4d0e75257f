"""Synthetic lit observed frames on the device (csrc/sample.hip deepim_sample_observed_poses / deepim_sample_lights, csrc/render.hip
deepim_render_observed_forward, lib/utils/synthetic_observed.py) at 480x640 with two textured ellipsoid meshes with normals:

    python tools/bench_synthetic.py [--batch 32] [--reps 100] [--rounds 7] [--feed-rounds 9] [--json PATH]

(a) The two sampler kernels and the new draw (its whole launch group: project, raster, resolve): HIP events around `reps`
    back-to-back calls, `rounds` rounds after a warm-up, median and range, the draw rotating over enough output sets that twice
    the 256 MiB Infinity Cache passes between two uses of a buffer, and on one set. Bytes are what the algorithm has to move: the
    z-buffer read once (8 B/px) and the three frames written once (6 B/px); the float draw of the same batch
    (deepim_render_classes_forward, one light) next to it writes 16 B/px. The share is of the copy rate tools/bench_ingest.py uses.
(b) One batch of synthetic frames by the new route (SyntheticObserved.frames: poses, lights, draw, nothing read back) against the
    only route there was before: one deepim_render_classes_forward call per light group (offset, ratio) into float tensors,
    read-back, numpy quantisation to uint8 BGR / uint16 / label frames, upload of the frames. The parent route gets its poses
    and lights for free (it has no sampler for either). Alternating, host wall-clock around work that ends in a synchronise.
(c) A whole TrainDataLoader step (make_batch + synchronise) without synthetic pairs and with half the batch synthetic,
    alternating.

    python tools/bench_synthetic.py --occluders N [--batch 32] ...

measures the occluded scenes instead (deepim_sample_occluders, deepim_render_scene_forward with S = N + 1 slots per frame,
deepim_occlusion_gate, SyntheticObserved(occluders=...)), every slot of every frame holding an object:
(d) The occluder sampler, the gate and the scene draw's launch group (project and raster over B S samples, one resolve pass over
    B frames), as in (a); the same launch group with every slot empty is the resolve pass over an untouched z-buffer, its
    memory floor. Bytes: 8 B/px of key read, 6 B/px stored, per FRAME.
(e) One batch of scenes by the scene entry against what there was before for the same frames: S deepim_render_observed_forward
    draws of B samples, one float draw of the B S samples for their depths (the uint16 depths are truncated and cannot order
    fragments), read-back, numpy composition (nearest float depth, lowest slot on ties) and upload. Alternating, as in (b).
(f) A TrainDataLoader step with half the batch synthetic, without and with occluders, alternating, as in (c)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_backgrounds import loader_world  # noqa: E402
from bench_ingest import COPY_RATE, stats, time_kernel  # noqa: E402
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.core.loader import TrainDataLoader  # noqa: E402
from mx_deepim_amd.lib.pair_matching.pose_sampler import BRIGHTNESS_RATIOS, sample_lights, sample_observed_poses  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi  # noqa: E402
from mx_deepim_amd.lib.pair_matching.pose_sampler import sample_occluders  # noqa: E402
from mx_deepim_amd.lib.utils.synthetic_observed import OccluderSpec, SyntheticObserved  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402

AXES = ([0.05, 0.04, 0.035], [0.03, 0.06, 0.04])
cf = ctypes.c_float


def lit_meshes(n_lat=24, n_lon=48):
    out = []
    for axes in AXES:
        m = synthetic.ellipsoid_mesh(axes, n_lat, n_lon)
        m.pop("colors")
        n = m["vertices"] / (np.asarray(axes, np.float32) ** 2)
        m["normals"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        m["texture"] = synthetic.procedural_texture()
        out.append(m)
    return out


def pose_stats():
    fallback = np.concatenate([np.eye(3), [[0.0], [0.0], [0.9]]], 1)
    return {c: dict(trans_mean=[0.0, 0.0, 0.9], trans_std=[0.08, 0.06, 0.12], pz_mean=[0.1, -0.2 + 0.3 * c, 0.9], angle_max=70.0,
                    fallback=fallback) for c in (0, 1)}


def occluded(ctx, a, rm, K, res):
    """(d), (e), (f): the scenes with a.occluders occluder slots, all of them filled."""
    B, H, W, S = a.batch, 480, 640, a.occluders + 1
    n, h, u64 = B * H * W, ctx.handle, ctypes.c_ulonglong
    spec = OccluderSpec([0, 1], {0: 0.10, 1: 0.12}, min_occluders=a.occluders, max_occluders=a.occluders)
    syn = SyntheticObserved(rm, pose_stats(), K, seed=31, occluders=spec)
    plain = SyntheticObserved(rm, pose_stats(), K, seed=31)
    t = rm.mesh_table()
    cls_host = (np.arange(B) % 2).astype(np.int32)
    cls, ids = ctx.array(cls_host, dtype=np.int32), ctx.array(np.arange(B), dtype=np.uint64)
    poses, _attempts = sample_observed_poses(cls, syn.pose_table, K, W, H, 31, draw_ids=ids)
    off, inten, ratio = sample_lights(ctx, B, 31, draw_ids=ids)
    res.update(occluders=a.occluders, slots=S)

    # ---- (d) the kernels
    o_out = ctx.empty((B, S), np.int32), ctx.empty((B, S, 3, 4)), ctx.empty((B, S), np.int32)
    st = time_kernel(ctx, lambda i: lib.deepim_sample_occluders(h, o_out[0], o_out[1], o_out[2], cls, poses, syn.occluder_classes,
                                                                syn.occluder_classes.size, syn.diameters, syn.diameters.size,
                                                                spec.min_occluders, spec.max_occluders, cf(0.2), cf(0.9), cf(0.5), cf(1.5),
                                                                u64(31), u64(0), ids, B), a.reps, a.rounds)
    res["kernels"]["sample_occluders"] = st
    print("sample_occluders      %8.2f us/call (min %.2f max %.2f)" % (st["median"], st["min"], st["max"]))
    ocls, oposes, olabel = sample_occluders(cls, poses, syn.occluder_classes, syn.diameters, 31, draw_ids=ids,
                                            min_occluders=spec.min_occluders, max_occluders=spec.max_occluders)
    res["live_slots"] = int((ocls.asnumpy() >= 0).sum())
    empty = ctx.array(np.full((B, S), -1, np.int32), dtype=np.int32)
    visible = ctx.empty((B, S), np.int32)
    nbytes = n * (8 + 6)
    k = -(-2 * (256 << 20) // (n * 6)) + 1
    sets = [(ctx.empty((B, H, W, 3), np.uint8), ctx.empty((B, H, W), np.uint16), ctx.empty((B, H, W), np.uint8)) for _ in range(k)]
    for name, c, nsets in (("scene, %d slots live (rotating)" % S, ocls, k), ("scene, %d slots live (one set)" % S, ocls, 1),
                           ("scene, every slot empty: the resolve pass alone (rotating)", empty, k)):
        st = time_kernel(ctx, lambda i: syn.scene_into(sets[i][0], sets[i][1], sets[i][2], c, oposes, off, inten, ratio, S,
                                                       label_value=olabel, visible=visible), a.reps, a.rounds, nsets)
        st.update(bytes=nbytes, sets=nsets, share_of_copy_rate=nbytes / (st["median"] * 1e-6) / COPY_RATE)
        res["kernels"][name] = st
        print("%-62s %8.1f us/call (min %.1f max %.1f)  %.2f of the copy rate" % (name, st["median"], st["min"], st["max"],
                                                                                 st["share_of_copy_rate"]))
    st = time_kernel(ctx, lambda i: syn.draw_into(sets[i][0], sets[i][1], sets[i][2], cls, poses, off, inten, ratio), a.reps, a.rounds, k)
    st.update(bytes=nbytes, sets=k, share_of_copy_rate=nbytes / (st["median"] * 1e-6) / COPY_RATE)
    res["kernels"]["render_observed_forward, one object (rotating)"] = st
    print("%-62s %8.1f us/call (min %.1f max %.1f)  %.2f of the copy rate" % ("render_observed_forward, one object (rotating)", st["median"],
                                                                             st["min"], st["max"], st["share_of_copy_rate"]))
    full, kept, totals = ctx.empty((B,), np.int32), ctx.empty((B,), np.int32), ctx.zeros((3,), np.uint64)
    alone = sets[0] if k == 1 else sets[1]
    syn.scene_into(alone[0], alone[1], alone[2], cls, poses, off, inten, ratio, 1, visible=full)
    syn.scene_into(sets[0][0], sets[0][1], sets[0][2], ocls, oposes, off, inten, ratio, S, label_value=olabel, visible=visible)
    for name, frac in (("occlusion_gate, min_visible 0 (every pair kept: the depth copy)", 0.0),
                       ("occlusion_gate, min_visible 1 (pairs fall back: four copies)", 1.0)):
        st = time_kernel(ctx, lambda i: lib.deepim_occlusion_gate(h, sets[0][0], sets[0][1], sets[0][2], None, kept, totals, None, B, alone[0],
                                                                  alone[1], alone[2], visible, full, ocls, cf(frac), B, S, H, W),
                         a.reps, a.rounds)
        res["kernels"][name] = st
        print("%-62s %8.1f us/call (min %.1f max %.1f)" % (name, st["median"], st["min"], st["max"]))
    res["kept_at_min_visible_1"] = int(kept.asnumpy().sum())
    del sets

    # ---- (e) one batch of scenes by the two routes
    flat_cls, flat_poses = ocls.reshape((B * S,)), oposes.reshape((B * S, 3, 4))
    per_slot = []           # slot s of every frame as a batch of B samples for the observed entry, staged before the clock starts
    oc_h, op_h, ol_h = ocls.asnumpy(), oposes.asnumpy(), olabel.asnumpy()
    for s_ in range(S):
        per_slot.append((ctx.array(oc_h[:, s_], dtype=np.int32), ctx.array(op_h[:, s_]), ctx.array(ol_h[:, s_], dtype=np.int32)))

    def route_parent():
        t0 = time.perf_counter()
        image, depth = ctx.empty((B * S, 3, H, W)), ctx.empty((B * S, 1, H, W))
        lib.deepim_render_classes_forward(h, image, depth, None, None, cf(0.0), flat_cls, t.mesh_desc, t.n_classes, t.max_V, t.max_F,
                                          t.vertices, t.vertex_attr, None, t.faces, t.textures, flat_poses, K, None, None, None, cf(0.0),
                                          B * S, H, W, cf(0.25), cf(6.0))
        z = depth.asnumpy().reshape(B, S, H, W)
        z[z == 0] = np.inf
        win = np.argmin(z, 1)
        frames = []
        for c, p, lab in per_slot:
            f = ctx.empty((B, H, W, 3), np.uint8), ctx.empty((B, H, W), np.uint16), ctx.empty((B, H, W), np.uint8)
            syn.draw_into(f[0], f[1], f[2], c, p, off, inten, ratio, label_value=lab)
            frames.append([x.asnumpy() for x in f])
        out = []
        for j, dt in enumerate((np.uint8, np.uint16, np.uint8)):
            stack = np.stack([fr[j] for fr in frames], 1)
            w = win.reshape((B, 1, H, W) + (1,) * (stack.ndim - 4))
            out.append(ctx.array(np.take_along_axis(stack, w, 1)[:, 0], dtype=dt))
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def route_new():
        t0 = time.perf_counter()
        f = ctx.empty((B, H, W, 3), np.uint8), ctx.empty((B, H, W), np.uint16), ctx.empty((B, H, W), np.uint8)
        syn.scene_into(f[0], f[1], f[2], ocls, oposes, off, inten, ratio, S, label_value=olabel, visible=visible)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, f

    (_t, old_out), (_t, new_out) = route_parent(), route_new()
    same = all(np.array_equal(x.asnumpy(), y.asnumpy()) for x, y in zip(old_out, new_out))
    res["routes_give_the_same_frames"] = bool(same)
    print("the two routes give the same frames:", same)
    del old_out, new_out
    old, new = [], []
    for r in range(a.feed_rounds + 1):
        to, tn = route_parent()[0], route_new()[0]
        if r:
            old.append(to)
            new.append(tn)
    res["routes"] = {"parent_S_draws_float_depths_readback_compose_upload_ms": stats(old), "scene_entry_ms": stats(new),
                     "pcie_bytes_parent": n * S * (4 + 6) + n * 6, "pcie_bytes_new": 0}
    for name in ("parent_S_draws_float_depths_readback_compose_upload_ms", "scene_entry_ms"):
        v = res["routes"][name]
        print("route %-56s %.3f ms (min %.3f max %.3f)" % (name, v["median"], v["min"], v["max"]))

    # ---- (f) a loader step with half the batch synthetic, without and with occluders
    cfg = default_config()
    unlit, observed, points = loader_world(ctx, cfg, B, H, W, np.random.default_rng(31))
    points[1] = points[0]
    loaders = {name: TrainDataLoader(observed, cfg, unlit, batch_size=B, seed=31, points=points, synthetic=g, num_synthetic=B,
                                     synthetic_classes=[0]) for name, g in (("half synthetic", plain), ("half synthetic, occluders", syn))}
    half_pairs = np.concatenate([np.arange(B // 2), B + np.arange(B - B // 2)])
    times = {name: [] for name in loaders}
    for r in range(a.feed_rounds + 2):
        for name, loader in loaders.items():
            t0 = time.perf_counter()
            batch = loader.make_batch(half_pairs, (half_pairs + r * 2 * B).astype(np.uint64))
            ctx.sync()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            del batch
    res["loader"] = {"step_ms " + name: stats(v) for name, v in times.items()}
    res["loader"]["stats"] = loaders["half synthetic, occluders"].stats()
    for name, v in res["loader"].items():
        if name != "stats":
            print("loader %-36s %.2f ms (min %.2f max %.2f)" % (name, v["median"], v["min"], v["max"]))
    print("loader stats", res["loader"]["stats"])


def finish(a, res):
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--feed-rounds", type=int, default=9)
    ap.add_argument("--json", default=None)
    ap.add_argument("--occluders", type=int, default=0, help="measure the occluded scenes with this many occluder slots (1..7) instead")
    a = ap.parse_args()
    B, H, W = a.batch, 480, 640
    n = B * H * W
    ctx = Context.get(0)
    h = ctx.handle
    K = synthetic.K_LINEMOD.astype(np.float32)
    rm = Render_Py_Light_ModelNet_Multi(["a", "b"], None, K, W, H, 0.25, 6.0, brightness_ratios=[0.7], meshes=lit_meshes(), ctx=ctx)
    if a.occluders:
        res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "kernels": {}, "routes": {}, "loader": {}}
        occluded(ctx, a, rm, K, res)
        return finish(a, res)
    syn = SyntheticObserved(rm, pose_stats(), K, seed=26)
    t = rm.mesh_table()
    cls_host = (np.arange(B) % 2).astype(np.int32)
    cls, ids = ctx.array(cls_host, dtype=np.int32), ctx.array(np.arange(B), dtype=np.uint64)
    res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "kernels": {}, "routes": {}, "loader": {}}

    # ---- (a) the kernels
    u64 = ctypes.c_ulonglong
    p_out, a_out = ctx.empty((B, 3, 4)), ctx.empty((B,), np.int32)
    st = time_kernel(ctx, lambda i: lib.deepim_sample_observed_poses(h, p_out, a_out, None, None, cls, syn.pose_table, syn.n_classes, K, W,
                                                                     H, cf(48.0), 100, u64(26), u64(0), ids, B), a.reps, a.rounds)
    st["bytes"] = B * (4 + 8 + 48 + 4)
    res["kernels"]["sample_observed_poses"] = st
    print("sample_observed_poses %8.2f us/call (min %.2f max %.2f)" % (st["median"], st["min"], st["max"]))
    l_out = ctx.empty((B, 3)), ctx.empty((B, 3)), ctx.empty((B,))
    ratios = np.asarray(BRIGHTNESS_RATIOS, np.float32)
    st = time_kernel(ctx, lambda i: lib.deepim_sample_lights(h, l_out[0], l_out[1], l_out[2], ratios, len(ratios), u64(26), u64(0), ids, B),
                     a.reps, a.rounds)
    st["bytes"] = B * (8 + 28)
    res["kernels"]["sample_lights"] = st
    print("sample_lights         %8.2f us/call (min %.2f max %.2f)" % (st["median"], st["min"], st["max"]))

    poses, attempts = sample_observed_poses(cls, syn.pose_table, K, W, H, 26, draw_ids=ids)
    off, inten, ratio = sample_lights(ctx, B, 26, draw_ids=ids)
    res["attempts_mean"] = float(attempts.asnumpy().mean())
    nbytes = n * (8 + 6)
    for mode, k in (("rotating", -(-2 * (256 << 20) // (n * 6)) + 1), ("one set", 1)):
        sets = [(ctx.empty((B, H, W, 3), np.uint8), ctx.empty((B, H, W), np.uint16), ctx.empty((B, H, W), np.uint8)) for _ in range(k)]
        st = time_kernel(ctx, lambda i: syn.draw_into(sets[i][0], sets[i][1], sets[i][2], cls, poses, off, inten, ratio), a.reps,
                         a.rounds, k)
        st.update(bytes=nbytes, sets=k, share_of_copy_rate=nbytes / (st["median"] * 1e-6) / COPY_RATE)
        res["kernels"]["render_observed_forward (%s)" % mode] = st
        print("render_observed_forward %-9s %3d sets %8.1f us/call (min %.1f max %.1f)  %6.2f TB/s  %.2f of the copy rate"
              % (mode, k, st["median"], st["min"], st["max"], nbytes / st["median"] / 1e6, st["share_of_copy_rate"]))
        del sets
    kf = -(-2 * (256 << 20) // (n * 16)) + 1
    fsets = [(ctx.empty((B, 3, H, W)), ctx.empty((B, 1, H, W))) for _ in range(kf)]
    one_off = np.array([0.0, 0.5, 0.5], np.float32)

    def float_draw(image, depth, c, p, it, o, r, nb):
        lib.deepim_render_classes_forward(h, image, depth, None, None, cf(0.0), c, t.mesh_desc, t.n_classes, t.max_V, t.max_F, t.vertices,
                                          t.vertex_attr, t.normals, t.faces, t.textures, p, K, None, o, it, cf(r), nb, H, W, cf(0.25),
                                          cf(6.0))

    st = time_kernel(ctx, lambda i: float_draw(fsets[i][0], fsets[i][1], cls, poses, inten, one_off, 0.3, B), a.reps, a.rounds, kf)
    st.update(bytes=n * (8 + 16), sets=kf, share_of_copy_rate=n * 24 / (st["median"] * 1e-6) / COPY_RATE)
    res["kernels"]["render_classes_forward, one light (rotating)"] = st
    print("render_classes_forward  rotating  %3d sets %8.1f us/call (min %.1f max %.1f)  %.2f of the copy rate"
          % (kf, st["median"], st["min"], st["max"], st["share_of_copy_rate"]))
    del fsets

    # ---- (b) one batch of synthetic frames by the two routes
    poses_h, off_h, inten_h, ratio_h = poses.asnumpy(), off.asnumpy(), inten.asnumpy(), ratio.asnumpy()
    groups = {}
    for b in range(B):
        groups.setdefault((tuple(off_h[b].tolist()), float(ratio_h[b])), []).append(b)
    staged = []          # per light group, on the device before the clock starts: the parent has no sampler to charge
    for (o, r), rows in groups.items():
        staged.append((np.asarray(o, np.float32), r, rows, ctx.array(cls_host[rows], dtype=np.int32), ctx.array(poses_h[rows]),
                       ctx.array(inten_h[rows])))
    res["light_groups"] = len(groups)

    def route_parent():
        t0 = time.perf_counter()
        bgr, d16 = np.empty((B, H, W, 3), np.uint8), np.empty((B, H, W), np.uint16)
        for o, r, rows, c, p, it in staged:
            image, depth = ctx.empty((len(rows), 3, H, W)), ctx.empty((len(rows), 1, H, W))
            float_draw(image, depth, c, p, it, o, r, len(rows))
            bgr[rows] = image.asnumpy()[:, ::-1].transpose(0, 2, 3, 1).astype(np.uint8)
            d16[rows] = (depth.asnumpy()[:, 0] * np.float32(1000)).astype(np.uint16)
        label = (d16 != 0).astype(np.uint8)
        out = ctx.array(bgr, dtype=np.uint8), ctx.array(d16, dtype=np.uint16), ctx.array(label, dtype=np.uint8)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def route_new():
        t0 = time.perf_counter()
        out = syn.frames(cls, ids)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    (_t, old_out), (_t, new_out) = route_parent(), route_new()
    same = all(np.array_equal(x.asnumpy(), new_out[k].asnumpy())
               for x, k in zip(old_out, ("image_observed", "depth_gt_observed", "mask_gt_observed")))
    res["routes_give_the_same_frames"] = bool(same)
    print("the two routes give the same frames:", same)
    for _ in range(2):
        route_parent(), route_new()
    old, new = [], []
    for _ in range(a.feed_rounds):
        old.append(route_parent()[0])
        new.append(route_new()[0])
    res["routes"] = {"parent_float_draws_readback_quantise_upload_ms": stats(old), "device_generator_ms": stats(new),
                     "pcie_bytes_parent": n * (16 + 6), "pcie_bytes_new": 0}
    for k in ("parent_float_draws_readback_quantise_upload_ms", "device_generator_ms"):
        v = res["routes"][k]
        print("route %-48s %.3f ms (min %.3f max %.3f)" % (k, v["median"], v["min"], v["max"]))

    # ---- (c) a whole loader step
    cfg = default_config()
    rng = np.random.default_rng(26)
    unlit, observed, points = loader_world(ctx, cfg, B, H, W, rng)
    points[1] = points[0]
    loader = TrainDataLoader(observed, cfg, unlit, batch_size=B, seed=26, points=points, synthetic=syn, num_synthetic=B,
                             synthetic_classes=[0])
    real_pairs = np.arange(B)
    half_pairs = np.concatenate([np.arange(B // 2), B + np.arange(B - B // 2)])
    times = {"S = 0": [], "half synthetic": []}
    for r in range(a.feed_rounds + 2):
        for name, pairs in (("S = 0", real_pairs), ("half synthetic", half_pairs)):
            t0 = time.perf_counter()
            batch = loader.make_batch(pairs, (pairs + r * 2 * B).astype(np.uint64))
            ctx.sync()
            if r >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            del batch
    res["loader"] = {"step_ms " + k: stats(v) for k, v in times.items()}
    res["loader"]["stats"] = loader.stats()
    for k, v in res["loader"].items():
        if k != "stats":
            print("loader %-24s %.2f ms (min %.2f max %.2f)" % (k, v["median"], v["min"], v["max"]))
    finish(a, res)


if __name__ == "__main__":
    main()
