"""Shared-frame batches (several objects per camera frame) on the GPU: the zoom front end reading N uint8 frames in place
(deepim_zoom_concat_frames_forward) against the existing one reading B fp32 copies (deepim_zoom_concat_forward), at B pairs
of 480 x 640 and N in {32, 8, 4, 1}.

    python tools/bench_shared_frames.py [--batch 32] [--frames 32,8,4,1] [--reps 100] [--rounds 7] [--feed-rounds 7] [--json PATH]

1. The front end alone: HIP events around `reps` back-to-back calls, `rounds` rounds after a warm-up, median and range,
   rotating over enough buffer sets that twice the 256 MiB Infinity Cache passes between two uses of a buffer — an HBM figure.
   "bytes" is the upper bound of a call: every input read once in full and the net input written once. The resampler reads the
   crop region only, so the true read traffic is smaller by the same factor in both entries.
2. The feed of one batch, the two forms alternating: (a) today's — upload of the B replicated uint8 frames, deepim_ingest_bgr8,
   four front-end calls (four refinement iterations: the observed side does not change inside the closed loop); (b) upload of
   the N frames and of frame_index, four frames front-end calls. Host wall-clock around work that ends in a device synchronise.
3. Resident bytes of the observed side in each form.
The two entries are checked to give the same bits before anything is timed."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd.runtime import Context, lib  # noqa: E402

MEANS_RGB = np.array([103.939, 116.779, 123.68], np.float32)
K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]], np.float32)
CACHE = 256 << 20
ITERS = 4


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def time_calls(ctx, fn, reps, rounds, sets):
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
    ap.add_argument("--frames", default="32,8,4,1")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--feed-rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, H, W = a.batch, a.height, a.width
    hw = H * W
    ctx = Context.get(0)
    h = ctx.handle
    rng = np.random.default_rng(23)

    # per-pair side: an object of about 120 x 120 pixels per pair, scattered over the frame
    mo, mr, pose = np.zeros((B, 1, H, W), np.float32), np.zeros((B, 1, H, W), np.float32), np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        cy, cx = int(rng.integers(90, H - 90)), int(rng.integers(90, W - 90))
        mo[b, 0, cy - 60:cy + 60, cx - 60:cx + 60] = 1
        mr[b, 0, cy - 50:cy + 64, cx - 66:cx + 52] = 1
        z = 1.0
        pose[b, :, :3] = np.eye(3)
        pose[b, :, 3] = ((cx - K[0, 2]) / K[0, 0] * z, (cy - K[1, 2]) / K[1, 1] * z, z)
    ren = rng.uniform(-120, 120, (B, 3, H, W)).astype(np.float32)
    all_frames = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)

    res = {"batch": B, "height": H, "width": W, "reps": a.reps, "rounds": a.rounds, "front_end": {}, "feed": {}, "resident": {}}
    in_pair = hw * (3 + 1 + 1) * 4            # image_rendered + the two masks, fp32, per pair
    out_b = B * hw * 8 * 4
    old_bytes = B * hw * 3 * 4 + B * in_pair + out_b

    def n_sets(nbytes):
        return -(-2 * CACHE // nbytes) + 1

    sets = n_sets(old_bytes)
    d_ren = [ctx.array(ren) for _ in range(sets)]
    d_mo = [ctx.array(mo) for _ in range(sets)]
    d_mr = [ctx.array(mr) for _ in range(sets)]
    d_out = [ctx.empty((B, 8, H, W)) for _ in range(sets)]
    d_pose, zf = ctx.array(pose), ctx.empty((B, 4))

    def old_call(obs):
        return lambda i: lib.deepim_zoom_concat_forward(h, obs[i], d_ren[i], d_mo[i], d_mr[i], None, None, d_pose, K, MEANS_RGB,
                                                        d_out[i], zf, B, H, W)

    def new_call(fr, fi, N):
        return lambda i: lib.deepim_zoom_concat_frames_forward(h, fr[i], fi, N, d_ren[i], d_mo[i], d_mr[i], None, None, None,
                                                               ctypes.c_float(1000.0), None, d_pose, K, MEANS_RGB, d_out[i], zf,
                                                               B, H, W)

    for N in [int(x) for x in a.frames.split(",")]:
        fidx = (np.arange(B) % N).astype(np.int32)
        frames = np.ascontiguousarray(all_frames[:N])
        rep = np.ascontiguousarray(frames[fidx])
        d_fi = ctx.array(fidx, dtype=np.int32)
        # ---- 1. the front end alone
        obs = []
        for _ in range(sets):
            o = ctx.empty((B, 3, H, W))
            lib.deepim_ingest_bgr8(h, o, ctx.array(rep, dtype=np.uint8), None, None, None, MEANS_RGB, B, H, W)
            obs.append(o)
        fr = [ctx.array(frames, dtype=np.uint8) for _ in range(sets)]
        old_call(obs)(0)
        want = d_out[0].asnumpy().view(np.uint32)
        new_call(fr, d_fi, N)(0)
        assert np.array_equal(d_out[0].asnumpy().view(np.uint32), want), "the two front ends disagree"
        new_bytes = N * hw * 3 + B * in_pair + out_b
        row = {}
        for name, fn, nbytes in (("fp32 entry", old_call(obs), old_bytes), ("frames entry", new_call(fr, d_fi, N), new_bytes)):
            st = time_calls(ctx, fn, a.reps, a.rounds, sets)
            st["bytes_upper_bound"], st["sets"] = nbytes, sets
            row[name] = st
            print("N=%-3d front end %-13s %8.1f us/call (min %.1f max %.1f), <= %.1f MB/call, %d sets" %
                  (N, name, st["median"], st["min"], st["max"], nbytes / 1e6, sets))
        res["front_end"][str(N)] = row
        del obs, fr

        # ---- 2. the feed of one batch
        def feed_old():
            t0 = time.perf_counter()
            raw = ctx.array(rep, dtype=np.uint8)
            o = ctx.empty((B, 3, H, W))
            lib.deepim_ingest_bgr8(h, o, raw, None, None, None, MEANS_RGB, B, H, W)
            for _ in range(ITERS):
                lib.deepim_zoom_concat_forward(h, o, d_ren[0], d_mo[0], d_mr[0], None, None, d_pose, K, MEANS_RGB, d_out[0], zf,
                                               B, H, W)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3

        def feed_new():
            t0 = time.perf_counter()
            raw, fi = ctx.array(frames, dtype=np.uint8), ctx.array(fidx, dtype=np.int32)
            for _ in range(ITERS):
                lib.deepim_zoom_concat_frames_forward(h, raw, fi, N, d_ren[0], d_mo[0], d_mr[0], None, None, None,
                                                      ctypes.c_float(1000.0), None, d_pose, K, MEANS_RGB, d_out[0], zf, B, H, W)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3

        feed_old(), feed_new()
        o_ms, n_ms = [], []
        for _ in range(a.feed_rounds):
            o_ms.append(feed_old())
            n_ms.append(feed_new())
        res["feed"][str(N)] = {"replicated_ms": stats(o_ms), "shared_ms": stats(n_ms), "uploaded_bytes_replicated": B * hw * 3,
                               "uploaded_bytes_shared": N * hw * 3 + 4 * B}
        print("N=%-3d feed: replicated %.2f ms (min %.2f max %.2f), shared %.2f ms (min %.2f max %.2f)" %
              (N, stats(o_ms)["median"], min(o_ms), max(o_ms), stats(n_ms)["median"], min(n_ms), max(n_ms)))
        # ---- 3. resident bytes of the observed side
        res["resident"][str(N)] = {"replicated_fp32": B * hw * 3 * 4, "shared_uint8": N * hw * 3 + 4 * B}
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
