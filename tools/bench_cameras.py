"""Per-pair cameras (deepim_bind_cameras, the K_host == NULL rule of include/deepim_hip.h) in one closed-loop iteration of the
test loop at 480x640 — forward (zoom front end, network), pose update, re-render with mask and rectangle from device class ids:

    python tools/bench_cameras.py [--batch 32] [--reps 20] [--rounds 7] [--json PATH]

(a) B pairs seen by four cameras shuffled over the batch, from the table: one network bound for B, one launch group per stage.
(b) The same pairs the only way there was before: four sub-batches of B/4, one per camera, with host K on a network bound for
    B/4 (its K and the render machine's K set before each sub-batch, which costs nothing on the device).
(c) B identical rows from the table against the host-K iteration on the same network: the cost of the table reads.
HIP events around `reps` back-to-back iterations in a synchronised window, `rounds` rounds after a warm-up, median and range.
Every iteration starts from the same batch, so the poses stay in frame however long the run is."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_ingest import time_kernel  # noqa: E402
from mx_deepim_amd import synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import update_test_batch  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402
from mx_deepim_amd.symbols import deepIM_flownet  # noqa: E402

H, W = 480, 640
CLASSES = ["a", "b"]


def four_cameras(K0):
    out = []
    for scale, shift in ((1.0, 0.0), (0.93, 3.5), (1.08, -2.25), (0.97, 1.75)):
        K = K0.copy()
        K[0, 0], K[1, 1] = K0[0, 0] * np.float32(scale), K0[1, 1] * np.float32(scale)
        K[0, 2], K[1, 2] = K0[0, 2] + np.float32(shift), K0[1, 2] + np.float32(shift)
        out.append(K)
    return out


def make_data(ctx, cfg, rm, tgt, src, ids, cams):
    """The test batch of the pairs (tgt, src): observed frame and mask drawn at tgt, rendered at src, pair b with cams[b]."""
    n = len(tgt)
    table = ctx.array(np.ascontiguousarray(cams))
    idd = ctx.array(ids, dtype=np.int32)
    image, depth = rm.render_batch(idd, ctx.array(tgt), K=table)
    mask = ctx.empty((n, 1, H, W))
    lib.deepim_depth_to_mask(ctx.handle, mask, depth, 0.0, mask.size)
    data = {"image_observed": image, "mask_observed": mask, "src_pose": ctx.array(src), "intrinsics": table}
    data = update_test_batch(cfg, data, rm, data["src_pose"], class_index=idd)
    data["mask_observed"] = mask
    return data, idd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B = a.batch
    if B % 4:
        raise SystemExit("--batch must be a multiple of 4 (four cameras, four equal sub-batches)")
    ctx = Context.get(0)
    cfg = default_config()
    K0 = np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32).reshape(3, 3).copy()
    cams4 = four_cameras(K0)
    rng = np.random.default_rng(28)
    cam_of = rng.permutation(np.arange(B) % 4)
    ids = (np.arange(B) % 2).astype(np.int32)
    pairs = [synthetic.sample_pose_pair(rng, K0, H, W) for _ in range(B)]
    tgt, src = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    meshes = {}
    for i, c in enumerate(CLASSES):
        m = synthetic.ellipsoid_mesh(np.array([0.05, 0.04, 0.035]) * (1.0 + 0.2 * i), 24, 48)
        m.pop("uv")
        meshes[c] = m
    rm = Render_Py("unused", CLASSES, K0, W, H, meshes=meshes, ctx=ctx, pixel_means=np.asarray(cfg.network.PIXEL_MEANS, np.float32)[::-1])

    def network(n):
        net = deepIM_flownet().get_symbol(cfg)
        params = net.init_weights(cfg, seed=3)
        params["trans_weight"] = params["trans_weight"] * np.float32(0.02)     # keep the object in frame (as bench.py does)
        params["trans_bias"] = params["trans_bias"] * np.float32(0.02)
        net.bind(ctx, n, params)
        rbuf = {k: ctx.empty((n, 3 if k == "image_rendered" else 1, H, W))
                for k in ("image_rendered", "depth_rendered", "mask_rendered", "mask_observed")}
        return net, rbuf

    def iteration(net, rbuf, data, idd):
        net.forward(data)
        pose = net.pose_update(data["src_pose"])
        return update_test_batch(cfg, data, rm, pose, class_index=idd, out=rbuf)

    net, rbuf = network(B)
    net_q, rbuf_q = network(B // 4)
    mixed, idd = make_data(ctx, cfg, rm, tgt, src, ids, [cams4[c] for c in cam_of])
    subs = []
    for c in range(4):
        rows = np.nonzero(cam_of == c)[0]
        d, i = make_data(ctx, cfg, rm, tgt[rows], src[rows], ids[rows], [cams4[c]] * len(rows))
        d.pop("intrinsics")
        subs.append((cams4[c], d, i, rows))
    same, idd_same = make_data(ctx, cfg, rm, tgt, src, ids, [K0] * B)
    same_host = dict(same)
    same_host.pop("intrinsics")

    def run_table(_):
        iteration(net, rbuf, mixed, idd)

    def run_sub_batches(_):
        for K, d, i, _rows in subs:
            net_q.K = rm.K = K
            iteration(net_q, rbuf_q, d, i)
        rm.K = K0

    # the two routes refine the same pairs: pose b of the table iteration against the pose of its sub-batch row
    # (not bit for bit: a network bound for another batch size may split its reductions differently)
    new = iteration(net, rbuf, mixed, idd)["src_pose"].asnumpy()
    worst = 0.0
    for K, d, i, rows in subs:
        net_q.K = rm.K = K
        worst = max(worst, float(np.abs(iteration(net_q, rbuf_q, d, i)["src_pose"].asnumpy() - new[rows]).max()))
    rm.K = K0
    res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "cameras": 4,
           "max_abs_pose_difference_between_routes": worst}
    print("largest |pose| difference between the table route and the sub-batch route: %.3g" % worst)
    order = (("table_one_launch_group_us", run_table), ("four_sub_batches_host_K_us", run_sub_batches),
             ("identical_rows_table_us", lambda _: iteration(net, rbuf, same, idd_same)),
             ("identical_rows_host_K_us", lambda _: iteration(net, rbuf, same_host, idd_same)))
    for name, fn in order:
        res[name] = time_kernel(ctx, fn, a.reps, a.rounds)
        v = res[name]
        print("%-32s %10.1f us/iteration (min %.1f max %.1f)" % (name, v["median"], v["min"], v["max"]))
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
