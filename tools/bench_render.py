"""Time the HIP rasteriser at the bench geometry (B pairs, 480x640, LINEMOD-sized mesh) with HIP events.

--mixed: BASELINE config 3's render instead — 13 synthetic meshes of unequal size, B = 32 shuffled class ids — through
`Render_Py.render_batch` with host ids (one launch group per run of equal ids) and with device int32 ids (one launch group,
`deepim_render_classes_forward`), and both again on a single-class batch. Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.runtime import Context  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--lat", type=int, default=48)
ap.add_argument("--mixed", action="store_true", help="13 unequal meshes, shuffled ids: host-id runs vs device ids (default B = 32)")
args = ap.parse_args()
ctx = Context.get(0)


def mixed():
    B, H, W, n_cls = (32 if args.batch == 16 else args.batch), 480, 640, 13
    names = ["obj%02d" % k for k in range(n_cls)]
    meshes = {}
    for k, name in enumerate(names):                 # 1.1k .. 9.4k vertices; every other mesh textured, textures of two sizes
        lat = 24 + 4 * k
        m = synthetic.ellipsoid_mesh([0.05 + 0.002 * k, 0.04 + 0.001 * k, 0.035 + 0.0015 * k], lat, 2 * lat)
        if k % 2:
            m.pop("colors")
            m["texture"] = synthetic.procedural_texture(*((256, 512) if k % 4 == 1 else (128, 256)), seed=k)
        else:
            m.pop("uv")
        meshes[name] = m
    rm = Render_Py("unused", names, synthetic.K_LINEMOD, W, H, meshes=meshes, ctx=ctx, pixel_means=synthetic.PIXEL_MEANS[::-1].copy())
    rng = np.random.default_rng(0)
    poses = ctx.array(np.stack([synthetic.sample_pose_pair(rng)[1] for _ in range(B)]))
    out = (ctx.empty((B, 3, H, W)), ctx.empty((B, 1, H, W)))
    mask = ctx.empty((B, 1, H, W))
    shuffled = rng.integers(0, n_cls, B).astype(np.int32)
    single = np.full(B, n_cls // 2, np.int32)
    res = {"B": B, "H": H, "W": W, "n_classes": n_cls, "reps": args.reps, "V": [len(m["vertices"]) for m in meshes.values()],
           "F": [len(m["faces"]) for m in meshes.values()]}
    check = {}
    for tag, ids in (("mixed", shuffled), ("single", single)):
        runs = 1 + int(np.count_nonzero(np.diff(ids)))
        for where, ci in (("host", ids), ("device", ctx.array(ids, dtype=np.int32))):
            for _ in range(3):
                rm.render_batch(ci, poses, out=out, mask_rendered=mask)
            ms = []
            for _ in range(5):                       # five timed rounds: the median, and min..max as the run-to-run spread
                ctx.sync()
                t = ctx.timer()
                t.start()
                for _ in range(args.reps):
                    rm.render_batch(ci, poses, out=out, mask_rendered=mask)
                t.stop()
                ms.append(t.elapsed_ms() / args.reps)
            res["%s_%s_ids_ms" % (tag, where)] = round(float(np.median(ms)), 4)
            res["%s_%s_ids_ms_min_max" % (tag, where)] = [round(min(ms), 4), round(max(ms), 4)]
            res["%s_%s_ids_launches" % (tag, where)] = 3 * (runs if where == "host" else 1)     # project, raster, resolve
            check[tag, where] = (out[0].asnumpy(), out[1].asnumpy(), mask.asnumpy())
        res["%s_runs" % tag] = runs
        res["%s_same_bits" % tag] = bool(all(np.array_equal(a, b) for a, b in zip(check[tag, "host"], check[tag, "device"])))
        res["%s_covered_px_per_pose" % tag] = int((check[tag, "host"][1] > 0).sum() / B)
    print(json.dumps(res))


if args.mixed:
    mixed()
    sys.exit(0)
mesh = dict(synthetic.ellipsoid_mesh([0.05, 0.04, 0.035], args.lat, 2 * args.lat), texture=synthetic.procedural_texture())
mesh.pop("colors")
rm = Render_Py("unused", ["obj"], synthetic.K_LINEMOD, 640, 480, meshes={"obj": mesh}, ctx=ctx,
               pixel_means=synthetic.PIXEL_MEANS[::-1].copy())
rng = np.random.default_rng(0)
poses = ctx.array(np.stack([synthetic.sample_pose_pair(rng)[1] for _ in range(args.batch)]))
img, dep = ctx.empty((args.batch, 3, 480, 640)), ctx.empty((args.batch, 1, 480, 640))
for _ in range(3):
    rm.render_into(img, dep, 0, poses)
t = ctx.timer()
t.start()
for _ in range(args.reps):
    rm.render_into(img, dep, 0, poses)
t.stop()
ms = t.elapsed_ms() / args.reps
out_bytes = args.batch * 480 * 640 * 4 * 4            # image + depth written
zb_bytes = args.batch * 480 * 640 * 8 * 2              # z-buffer cleared + read back
print("render B=%d V=%d F=%d: %.3f ms per batch, %.1f us per pose, %.2f TB/s of (output + z-buffer) traffic"
      % (args.batch, len(mesh["vertices"]), len(mesh["faces"]), ms, 1e3 * ms / args.batch, (out_bytes + zb_bytes) / ms / 1e9))
print("covered pixels per pose:", int((dep.asnumpy() > 0).sum() / args.batch))
