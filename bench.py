#!/usr/bin/env python
"""bench.py — pose-refinement iterations/sec of the DeepIM render-and-compare inner loop on MI355X.

Workload: BASELINE.json's metric is quoted on "4-iter loop, 480x640, bs32", which fits one GPU, so the default is
LINEMOD-'ape'-like pairs, batch 32 per GPU, 4 refinement iterations, 480x640, fp32 (`--batch 16` = configs[1],
`--batch 4` = the per-GPU share of configs[2]).  One *step* = one pass of the hot path over one batch = the
4-iteration loop over the 32 pairs (128 pose-refinement iterations): zoom → FlowNetS encoder → fc6/fc7 → rot/trans +
inverse ZoomTrans → RT_transform → re-render at the refined pose (HIP rasteriser standing in for the reference's
OpenGL window) + rendered-mask / observed-mask update (deepim/core/tester.py:420-455), the new frame
feeding the next iteration's ZoomMask.  `--prestaged` skips the re-render and feeds pre-staged frames instead.
Inputs are resident in HBM before the timed region.

A plain run sets up, warms up, times `--steps` steps, writes `--dump-outputs` and prints its line.  Everything else — the
auxiliary steps behind `roofline_zoom` / `render_ms` / `allgather_us`, the per-layer timings, the oracle parity replay, the CPU
baseline, the other configurations, at N>1 the weak-scaling figure and the all-gather checks — runs with `--full` only, after the
timed region.

N>1: one process per GPU (the driver launches them with torch.distributed.run; this file only reads the RANK /
WORLD_SIZE / LOCAL_RANK / MASTER_* variables it sets and never imports torch).  Pairs are independent; after every
refinement iteration the refined poses are all-gathered with ONE `ncclAllGather` (RCCL over xGMI, 48 B/pair)
enqueued on the library's own stream — no host sync inside the loop.  Default: 32 pairs per GPU (weak scaling, the
bs32 the metric is quoted on).  `--global-batch 32` is BASELINE config 3 as written: 32 pairs sharded 32/N per GPU
(strong scaling).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from mx_deepim_amd import parallel, synthetic  # noqa: E402
from mx_deepim_amd.config import default_config  # noqa: E402
from mx_deepim_amd.runtime import Context, lib  # noqa: E402
from mx_deepim_amd.symbols import deepIM_flownet  # noqa: E402
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py  # noqa: E402
from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import update_test_batch  # noqa: E402
from mx_deepim_amd.symbols.deepIM_flownet import ENCODER  # noqa: E402

FP32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: fp32 matrix == fp32 vector peak
HBM_PEAK_GBS = 8000.0
DUMP_CAP_BYTES = 64 << 20  # --dump-outputs: at most this many bytes of .npy payload in all


def dump_outputs(dirname, arrays, cap=DUMP_CAP_BYTES, seed=0):
    """--dump-outputs: every array as dirname/<name>.npy, float32 (float64 stays float64). Every array's leading axis is the pair.
    If they exceed `cap` together, each array above 1 MB keeps a fixed, seeded sample of its pairs (the same pairs for arrays of
    the same pair count), and the kept pair indices go to <name>_pairs.npy (float64). -> {name: shape} of what was written."""
    arrs = {k: np.ascontiguousarray(v, np.float64 if np.asarray(v).dtype == np.float64 else np.float32) for k, v in arrays.items()}
    big = [k for k, a in arrs.items() if a.nbytes > (1 << 20)]
    if sum(a.nbytes for a in arrs.values()) > cap:
        room = cap - sum(a.nbytes for k, a in arrs.items() if k not in big) - 4096 * len(big)   # index files and .npy headers
        scale = room / float(sum(arrs[k].nbytes for k in big))
        for k in big:
            rows = arrs[k].shape[0]
            idx = np.sort(np.random.default_rng(seed).choice(rows, max(1, int(rows * scale)), replace=False))
            arrs[k] = np.ascontiguousarray(arrs[k][idx])
            arrs[k + "_pairs"] = idx.astype(np.float64)
    os.makedirs(dirname, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(dirname, k + ".npy"), a)
    return {k: list(a.shape) for k, a in arrs.items()}


def encoder_flops_per_pair(cin=8, H=480, W=640):
    total, h, w = 0, H, W
    for _, cout, k, s, p in ENCODER:
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        total += 2 * cout * cin * k * k * h * w
        cin = cout
    return total


def layer_executed_flops_per_pair(net, geom):
    """MFMA FLOPs one encoder layer executes per pair: 16 positions per 2x2 output tile on the Winograd layers (49 of the 64 (position,
    phase) pairs on the stride-2 ones with Cin % 16 == 0), k*k taps per output on the direct ones."""
    name, cin, h, w, cout, k, s, p = geom
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    if name in getattr(net, "packed_wino", {}):
        pos_ch = 16 * cin
        if name in getattr(net, "wino_s2d", ()):     # stride 2: the four input phases as channels; with Cin % 16 == 0 the kernel
            pos_ch = (49 if cin % 16 == 0 else 64) * cin   # skips the identically-zero positions: 16 + 12 + 12 + 9 of 4 x 16
        return 2 * cout * pos_ch * ((ho + 1) // 2) * ((wo + 1) // 2)
    return 2 * cout * cin * k * k * ho * wo


def encoder_executed_flops_per_pair(net):
    """MFMA FLOPs the bound encoder actually executes per pair — the honest denominator for the matrix-pipe utilisation."""
    return sum(layer_executed_flops_per_pair(net, g) for g in net.enc_geom)


def physical_cores():
    """Physical cores of the host (psutil; half the hardware threads if it is not importable)."""
    try:
        import psutil
        return int(psutil.cpu_count(logical=False) or os.cpu_count() or 1)
    except ImportError:
        return max(1, (os.cpu_count() or 2) // 2)


def cpu_baseline(params, cfg, batch, budget_s=20.0, with_depth=False, min_runs=5, max_runs=15, pairs=8):
    """The stated CPU baseline: whole pair-iterations of the reference path on the host —
    the oracle's zoom front end (numpy, what the reference's CustomOps run on the host anyway) -> the N-group (10 convolutions + fc6 /
    fc7 / rot / trans with THIS run's weights) on oneDNN through torch-CPU, the library an MXNet-MKL build of the reference would call
    for those layers -> the oracle's inverse ZoomTrans + RT_transform; `pairs` pairs per call, threads pinned to the PHYSICAL cores.
    Protocol: one untimed warm-up call, then >= 5 timed ones (more while `budget_s` lasts), value = pairs / MEDIAN seconds per call.
    `gflops` = the encoder's 38.9 GFLOP per pair over the time inside the convolution stack. The bit-identical-to-the-checker build of the
    same loop (every convolution one fmaf chain on the oracle's cache-blocked OpenMP kernel) follows as `secondary_checker_build`;
    without torch it IS the baseline (kind stays "port": both are restatements, MXNet itself is not installable offline)."""
    from oracle import pipeline as opipe
    from oracle import net as onet
    from oracle import se3 as ose3
    from oracle import zoom as ozoom
    onet.build()
    means_rev = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])
    npairs = len(batch["image_observed"])
    cores = physical_cores()

    def slab(b, n):
        idx = [(b + i) % npairs for i in range(n)]
        data = {"image_observed": batch["image_observed"][idx], "image_rendered": batch["image_rendered"][0][idx],
                "mask_observed": batch["mask_observed"][idx], "mask_rendered": batch["mask_rendered"][0][idx],
                "src_pose": batch["src_pose"][0][idx]}
        if with_depth:
            data.update(depth_observed=batch["depth_gt_observed"][idx], depth_rendered=batch["depth_rendered"][0][idx])
        return data

    def checker_one(b):
        data = slab(b, 1)
        t0 = time.perf_counter()
        opipe.refine_iteration(params, data, batch["K"], means_rev, cfg.dataset.trans_means, cfg.dataset.trans_stds, cfg.network.ROT_COORD)
        return time.perf_counter() - t0

    def run(fn, min_r, max_r, budget):
        warm = fn(0)
        times, t_begin = [], time.perf_counter()
        while len(times) < min_r or (len(times) < max_r and time.perf_counter() - t_begin < budget):
            times.append(fn((1 + len(times)) % npairs))
        return warm, times

    res = None
    try:
        import torch
        import torch.nn.functional as F
    except ImportError:
        torch = None
    if torch is not None:
        torch.set_num_threads(cores)
        tw = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in params.items()
              if k.startswith(("flow_conv1", "conv", "fc", "rot", "trans"))}
        conv_s = [0.0]
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=max(1, min(pairs, cores)))

        def onednn_call(b):
            data = slab(b, pairs)
            t0 = time.perf_counter()
            def zoom_one(i):       # one pair per host thread: the pairs are independent, numpy releases the GIL in its kernels
                sl = slice(i, i + 1)
                return ozoom.net_input(data["image_observed"][sl], data["image_rendered"][sl], data["mask_observed"][sl],
                                       data["mask_rendered"][sl], data["src_pose"][sl], batch["K"], means_rev,
                                       data["depth_observed"][sl] if with_depth else None, data["depth_rendered"][sl] if with_depth else None)
            zs = list(pool.map(zoom_one, range(pairs)))
            x = np.concatenate([z[0] for z in zs], 0)
            zf = np.concatenate([z[1] for z in zs], 0)
            t1 = time.perf_counter()
            with torch.no_grad():
                y = torch.from_numpy(x)
                for name, cout, k, s_, p_ in ENCODER:
                    y = F.leaky_relu(F.conv2d(y, tw[name + "_weight"], tw[name + "_bias"], stride=s_, padding=p_), 0.1)
                t2 = time.perf_counter()
                y = F.leaky_relu(F.linear(y.flatten(1), tw["fc6_weight"], tw["fc6_bias"]), 0.1)
                y = F.leaky_relu(F.linear(y, tw["fc7_weight"], tw["fc7_bias"]), 0.1)
                rot = F.linear(y, tw["rot_weight"], tw["rot_bias"]).numpy()
                tr = F.linear(y, tw["trans_weight"], tw["trans_bias"]).numpy()
            tr = ozoom.zoom_trans(zf, tr, b_inv_zoom=True)
            for i in range(pairs):
                ose3.RT_transform(np.asarray(data["src_pose"][i], np.float32), rot[i], tr[i], cfg.dataset.trans_means,
                                  cfg.dataset.trans_stds, cfg.network.ROT_COORD)
            conv_s[0] += t2 - t1
            return time.perf_counter() - t0

        warm, times = run(onednn_call, min_runs, max_runs, budget_s * 0.6)
        conv_total = conv_s[0]
        med = float(np.median(times))
        # conv seconds of the timed calls only (the warm-up's share is subtracted by proportion of calls)
        conv_per_call = conv_total / (len(times) + 1)
        res = {"value": pairs / med, "unit": "pose-refinement iters/sec", "cores": cores, "threads": int(torch.get_num_threads()),
               "nproc": os.cpu_count(), "kind": "port",
               "gflops": encoder_flops_per_pair(8 + (2 if with_depth else 0)) * pairs / conv_per_call / 1e9,
               "n_group_share_of_time": conv_per_call / (float(np.mean(times + [warm]))),
               "protocol": "BASELINE.md section 3: 1 untimed warm-up call, then %d timed calls of %d pair-iterations; value = pairs / median" % (len(times), pairs),
               "seconds_per_call": {"median": med, "min": float(min(times)), "max": float(max(times)), "warmup": warm},
               "sample_short": "%d calls x %d pair-iterations (480x640, FAST_TEST) in %.1f s: numpy zoom + oneDNN conv/fc + oracle pose update"
                               % (len(times), pairs, float(sum(times))),
               "sample": "%d timed calls x %d pair-iterations (480x640, FAST_TEST graph: BASELINE config 1's unit of work) in %.1f s on pairs of "
                         "the same synthetic workload: oracle zoom front end (numpy, one pair per host thread) -> 10 convolutions + fc head on oneDNN (torch-CPU %s, this "
                         "run's weights) -> oracle inverse ZoomTrans + RT_transform; %d threads = the physical cores"
                         % (len(times), pairs, float(sum(times)), torch.__version__, int(torch.get_num_threads()))}
    # the checker build of the same pair-iteration: bit-identical convolutions, OpenMP threads pinned to the physical cores
    old_omp = os.environ.get("OMP_NUM_THREADS")
    onet.set_omp_threads(cores)
    onet.BLOCKED = True
    try:
        warm, times = run(checker_one, 2 if res else min_runs, 4 if res else max_runs, budget_s * (0.4 if res else 1.0))
    finally:
        onet.BLOCKED = False
    med = float(np.median(times))
    threads = onet.omp_threads()
    chk = {"value": 1.0 / med, "unit": "pose-refinement iters/sec", "cores": cores, "threads": threads, "nproc": os.cpu_count(),
           "omp_num_threads": old_omp or "unset: pinned to the %d physical cores through omp_set_num_threads" % cores,
           "gflops": encoder_flops_per_pair(8 + (2 if with_depth else 0)) / med / 1e9,
           "kind": "port", "protocol": "1 untimed warm-up pair-iteration, then %d timed; value = 1 / median" % len(times),
           "seconds_per_iteration": {"median": med, "min": float(min(times)), "max": float(max(times)), "warmup": warm},
           "sample": "%d timed pair-iterations (B = 1) in %.1f s; numpy + C oracle, every convolution the checker's own fmaf chain on its "
                     "cache-blocked fp32 OpenMP build (bit-identical to the parity oracle), %d threads; gflops counts the whole iteration's time"
                     % (len(times), float(sum(times)), threads)}
    if res is None:
        return chk
    res["secondary_checker_build"] = chk
    return res


def verify_parity(args, cfg, net, params, ctx, step, pose_cur, K, B):
    """Parity of the configuration that was just timed (same context, same plans, same batch): one more step with taps
    that copy, for `--verify` sampled pairs, the inputs of every refinement iteration (observed frame, the frame the GPU
    rendered, masks, [depth], the src pose of that iteration) and its outputs; each iteration is then replayed through the
    CPU oracle on exactly those inputs (tests/test_gpu_baseline_configs.py does the same at B = 4).  TEST-SIDE use of
    oracle/: checker only, after the timed region."""
    from oracle import pipeline as opipe
    from oracle import zoom as oz
    idx = sorted(set(int(i) for i in np.linspace(0, B - 1, max(1, args.verify))))
    in_keys = ("image_observed", "image_rendered", "mask_observed", "mask_rendered", "depth_observed", "depth_rendered", "src_pose")
    out_keys = ["zoom_factor", "se3", "net_input"] + (["flow_est", "mask_observed_pred"] if args.heads else [])
    snaps = {}

    def rows(a):
        return np.concatenate([a[i:i + 1].asnumpy() for i in idx])

    def tap(kind, it, data):
        if kind == "in":
            snaps[it] = {k: rows(data[k]) for k in in_keys if data.get(k) is not None}
        else:
            snaps[it]["out"] = {k: rows(net.act[k]) for k in out_keys}
            snaps[it]["out"]["pose_est"] = rows(pose_cur)
            zi = ctx.empty((B, 2, net.H, net.W), dtype=np.int32)
            lib.deepim_zoom_indices(ctx.handle, net.act["zoom_factor"], zi, B, net.H, net.W)
            snaps[it]["out"]["zoom_idx"] = rows(zi)

    step(tap=tap)
    ctx.sync()
    means_rev = np.ascontiguousarray(synthetic.PIXEL_MEANS[::-1])

    def rel(a, b):
        return float(np.abs(np.asarray(a, np.float64) - b).max() / max(1e-30, np.abs(b).max()))

    res = {"pairs": len(idx), "pair_index": idx, "iters": len(snaps), "pose_max_rel": 0.0, "se3_max_rel": 0.0,
           "zoom_factor_bit_exact": True, "zoom_idx_bit_exact": True, "net_input_bit_exact": True}
    if args.heads:
        res.update(flow_max_rel=0.0, mask_flip_frac=0.0)
    t0 = time.time()
    for it in sorted(snaps):
        d = {k: v for k, v in snaps[it].items() if k != "out"}
        got = snaps[it]["out"]
        ref = opipe.refine_iteration(params, d, K, means_rev, cfg.dataset.trans_means, cfg.dataset.trans_stds,
                                     cfg.network.ROT_COORD, heads=bool(args.heads), fp16_conv=bool(args.fp16), nc8=True)
        res["pose_max_rel"] = max(res["pose_max_rel"], rel(got["pose_est"], ref["pose_est"]))
        res["se3_max_rel"] = max(res["se3_max_rel"], rel(got["se3"], ref["se3"]))
        res["zoom_factor_bit_exact"] &= bool(np.array_equal(got["zoom_factor"], ref["zoom_factor"]))
        # fp16 mode: the front end writes fp16 pixel records — the fp32 net input rounded once
        want_in = ref["net_input"].astype(np.float16).astype(np.float32) if args.fp16 else ref["net_input"]
        res["net_input_bit_exact"] &= bool(np.array_equal(got["net_input"], want_in))
        res["zoom_idx_bit_exact"] &= bool(np.array_equal(got["zoom_idx"], oz.sample_indices(ref["zoom_factor"], net.H, net.W)))
        if args.heads:
            res["flow_max_rel"] = max(res["flow_max_rel"], rel(got["flow_est"], ref["flow_est"]))
            res["mask_flip_frac"] = max(res["mask_flip_frac"], float(np.mean(got["mask_observed_pred"] != ref["mask_observed_pred"])))
    if args.fp16:
        res["against"] = "oracle fp16 emulation (oracle/pipeline.py:encoder_fp16: fp16-rounded operands and outputs, fp32 accumulation)"
        # bars two orders of magnitude tighter than round 3's (2e-3 / 5e-3): observed pose 1e-6 … 5e-6, se3 2e-4 … 3e-4 —
        # both sides round the same fp16 operands, only the fp32 summation order differs
        res["bar"] = {"pose_max_rel": 1e-4, "se3_max_rel": 1e-3}
    else:
        res["against"] = ("CPU oracle, fp32 (float64-accumulating convolutions in the NC8 summation order), every iteration fed the GPU's own "
                          "inputs. The oracle's Z / S / F groups are pinned by outputs of the reference's own files (tests/golden); its N-group "
                          "(Convolution / FullyConnected / LeakyReLU) and the BilinearSampler restate third-party MXNet operators that "
                          "/root/reference does not hold: cross-checked against torch-CPU (tests/test_oracle_thirdparty.py), unpinned by the reference")
        res["bar"] = {"pose_max_rel": 1e-4, "se3_max_rel": 1e-4, "zoom": "bit-exact"}
        if args.heads:
            res["bar"].update(flow_max_rel=1e-4, mask_flip_frac=1e-4)
    ok = res["pose_max_rel"] <= res["bar"]["pose_max_rel"] and res["se3_max_rel"] <= res["bar"]["se3_max_rel"] and \
        res["zoom_factor_bit_exact"] and res["zoom_idx_bit_exact"] and res["net_input_bit_exact"]
    if args.heads and not args.fp16:
        ok = ok and res["flow_max_rel"] <= 1e-4 and res["mask_flip_frac"] <= 1e-4
    res["within_bar"] = bool(ok)
    res["oracle_seconds"] = time.time() - t0
    return res


def roofline_block(kernel, flops_alg, flops_exec, enc_ms, peak, wino_layers, traffic, traffic_src, per_kernel_path=None, batch=None, plain=True):
    """The `roofline` object of the bench line (pure: CPU-tested). `frac` is the PHYSICAL fraction — the FLOPs the matrix pipe executes
    over the dense peak, <= 1; the algorithmic figure (9 or 25 multiply-adds per output and input channel, of which the Winograd layers
    execute 16 per 2x2 tile) sits beside it as `algorithmic_tflops` / `algorithmic_over_peak` (> 1 is the algorithm, not the pipe).
    `per_kernel` / `roofline_hbm` come from the recorded rocprofv3 pass tools/profile_summary.py perkernel wrote (profiles/per_kernel.json),
    for the plain fp32 headline configuration at its batch size only."""
    executed = flops_exec / (enc_ms * 1e-3) / 1e12
    algorithmic = flops_alg / (enc_ms * 1e-3) / 1e12
    rl = {"bound": "mfma", "kernel": kernel, "achieved": executed, "peak": peak, "unit": "TFLOP/s", "frac": executed / peak,
          "achieved_counts": "FLOPs the matrix pipe executes (16 multiply-adds per 2x2 output tile, input and output channel on the "
                             "Winograd layers; 49 of 64 (position, phase) pairs on the 5x5 stride-2 ones; k*k per output on the direct ones)",
          "algorithmic_tflops": algorithmic, "algorithmic_over_peak": algorithmic / peak, "winograd_layers": wino_layers,
          "traffic": traffic, "traffic_source": traffic_src, "flop_per_launch_group": flops_alg,
          "executed_flop_per_launch_group": flops_exec, "ms_per_launch_group": enc_ms}
    hbm = None
    if plain and per_kernel_path and os.path.exists(per_kernel_path):
        pk = json.load(open(per_kernel_path))
        if pk.get("batch") == batch:
            rl["per_kernel"] = pk["per_kernel"]
            rl["per_kernel_source"] = pk["source"]
            rl["per_kernel_sum_ms"] = pk["sum_ms"]
            rl["per_kernel_run_ms_per_launch_group"] = pk.get("bench_ms_per_launch_group_same_run")
            hbm = pk.get("roofline_hbm")
    return rl, hbm


LINE_LIMIT = 4096      # bytes of the final stdout line (the driver parses the LAST line; round 5's 22.8 KB line came back unparsed)
STR_LIMIT = 120        # the driver's record clips strings at 128 characters


def _clip(s):
    return s if s is None or len(s) <= STR_LIMIT else s[:STR_LIMIT - 1] + "~"


def _pick(d, keys):
    return {k: d[k] for k in keys if d is not None and k in d}


def _r(x, n=6):
    """Floats at n significant digits (the line is read by people too)."""
    return float("%.*g" % (n, x)) if isinstance(x, float) else x


def compact_line(out):
    """The ONE line the driver parses (pure: CPU-tested in tests/test_host_logic.py): the contract's scalar keys, `config`, `roofline`,
    `roofline_zoom`, `cpu_baseline`, `parity`, `comm` — numbers and short strings only, no lists of dicts, < LINE_LIMIT bytes.
    Everything else (`other_configs`, the per-kernel table, the HBM entries of the Z / H / F kernels, the secondary CPU figures, the
    protocol prose) goes to bench_detail.json and to the '#'-prefixed lines printed BEFORE this one."""
    c = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                             "vs_baseline", "dtype", "data") if k in out}
    cfg = out.get("config") or {}
    c["config"] = _pick(cfg, ("workload", "pairs_per_gpu", "global_batch", "iters", "shard_counts", "encoder_launch", "parallelism"))
    rl = out.get("roofline")
    if rl:
        c["roofline"] = _pick(rl, ("bound", "kernel", "achieved", "peak", "unit", "frac", "algorithmic_over_peak", "traffic",
                                   "traffic_source", "ms_per_launch_group", "dominant_kernel", "dominant_ms", "dominant_achieved",
                                   "dominant_frac"))
        if c["roofline"].get("traffic_source"):       # the recorded PMC pass: file name only (the prose sits in the detail file)
            c["roofline"]["traffic_source"] = "recorded PMC pass, " + c["roofline"]["traffic_source"].split(" ")[0]
    else:
        c["roofline"] = None
    if out.get("roofline_zoom"):
        c["roofline_zoom"] = _pick(out["roofline_zoom"], ("bound", "kernel", "achieved", "peak", "unit", "frac", "ms"))
    cb = out.get("cpu_baseline")
    if cb:
        c["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "threads", "kind", "sample", "skipped"))
        if "sample_short" in cb:
            c["cpu_baseline"]["sample"] = cb["sample_short"]
    pa = out.get("parity")
    if pa:
        c["parity"] = _pick(pa, ("pose_max_rel", "se3_max_rel", "flow_max_rel", "mask_flip_frac", "zoom_idx_bit_exact",
                                 "net_input_bit_exact", "within_bar", "error"))
        if "pairs" in pa:
            c["parity"]["pairs"] = "%d of %d" % (pa["pairs"], cfg.get("pairs_per_gpu", 0))
            c["parity"]["iters"] = pa.get("iters")
    if out.get("comm"):
        c["comm"] = _pick(out["comm"], ("backend", "rccl_ranks", "rccl_version", "allgather_us", "ranks_reporting",
                                        "all_ranks_same_libraries", "note"))
    for k in ("render_ms", "dry_run"):
        if k in out:
            c[k] = out[k]
    c["detail"] = "bench_detail.json"

    def walk(v):
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        if isinstance(v, str):
            return _clip(v)
        if isinstance(v, float):
            return _r(v)
        return v
    c = walk(c)
    for k in ("value", "ms_per_step"):      # the two the driver cross-checks against its own clock: as measured
        if k in out:
            c[k] = out[k]
    line = json.dumps(c, separators=(",", ":"))
    assert len(line) < LINE_LIMIT, len(line)
    return line


def detail_lines(out):
    """'#'-prefixed, one per secondary figure: what other_configs / roofline_hbm / the per-kernel table hold, readable in the driver's
    stdout tail without being mistaken for the JSON line."""
    rows = []
    for name, r in sorted((out.get("other_configs") or {}).items()):
        if "value" in r:
            p = r.get("parity") or {}
            rows.append("# %s: %.1f %s%s%s%s" % (
                name, r["value"], r.get("unit", "it/s"), ", %.3f ms/step" % r["ms_per_step"] if "ms_per_step" in r else "",
                ", conv %.1f TF executed = %.3f of peak" % (r["conv_tflops_executed"], r["conv_frac"]) if "conv_frac" in r else "",
                ", parity pose %.2g se3 %.2g within_bar %s" % (p.get("pose_max_rel", float("nan")), p.get("se3_max_rel", float("nan")),
                                                              p.get("within_bar")) if p else ""))
        else:
            rows.append("# %s: %s" % (name, json.dumps(r)[:200]))
    for r in (out.get("roofline") or {}).get("layers_live") or []:
        rows.append("# layer %s: %.4f ms, %.1f TF executed = %.3f of peak" % (r["layer"], r["ms"], r["tflops_executed"], r["frac"]))
    return rows


def resolve_batches(args, world, rank):
    """-> (B, Bmax, counts, global_batch, scaling). Default = BASELINE.json's configuration at every N: a GLOBAL batch of
    `--batch` (32) pairs sharded in contiguous blocks over the GPUs — strong scaling, configs[2] as written ("batch 32 … sharded by
    object across 8xMI355X"; north_star: ">=10k it/s at batch 32 … on 8xMI355X"). `--global-batch G` overrides the total;
    `--weak` makes `--batch` the PER-GPU count (total = N x batch)."""
    if args.weak:
        return args.batch, args.batch, [args.batch] * world, world * args.batch, "weak"
    g = args.global_batch or args.batch
    counts = parallel.shard_counts(g, world)
    lo, hi = parallel.shard_bounds(g, world, rank)
    return hi - lo, max(counts), counts, g, "strong"


def headline(args, world, NIT, dt, pairs_total, scaling, steps, warmup, bs):
    """The part of the JSON line that does not depend on device measurements (shared by the real run and --dry-run)."""
    iters_total = pairs_total * NIT * steps
    return {
        "metric": "pose-refinement iters/sec (%d-iter loop, 480x640, bs%d)" % (NIT, bs),
        "value": iters_total / dt,
        "unit": "pose-refinement iters/sec",
        "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": dt / steps * 1e3,
        "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
        "dtype": "f16" if args.fp16 else ("f16x3" if args.x3 else "f32"), "data": "synthetic",
    }


def comm_record(ctx_handle):
    """deepim_comm_info of this process as a dict (what it really bound: RCCL rank count, version, library files)."""
    buf = ctypes.create_string_buffer(2048)
    lib.deepim_comm_info(ctx_handle, buf, 2048)
    rec = dict(kv.split("=", 1) for kv in buf.value.decode(errors="replace").split(";") if "=" in kv)
    for k in ("rccl_ranks", "rccl_version"):
        rec[k] = int(rec.get(k, "0") or 0)
    return rec


def dry_run(args, rank, world, rdzv):
    """No GPU: every rank owns its block of a global pose table; one 'refinement' = pose += 1 on the host; the per-iteration
    exchange, the ragged padding, the barrier-bracketed timing, the max over ranks and the rank-0 line are bench.py's own."""
    NIT = args.iters
    B, Bmax, counts, total, scaling = resolve_batches(args, world, rank)
    assert B > 0, "more GPUs than pairs"
    lo = sum(counts[:rank])
    if world > 1:       # the RCCL bootstrap's host half (parallel.PoseComm.__init__): rank 0's 128-byte id reaches every rank
        uid = rdzv.broadcast(bytes(range(128)) if rank == 0 else None, 0)
        assert isinstance(uid, bytes) and uid == bytes(range(128))
    table = np.arange(total * 12, dtype=np.float32).reshape(total, 3, 4)
    pose = table[lo:lo + B].copy()
    gathered = None

    def step():
        nonlocal pose, gathered
        pose = table[lo:lo + B].copy()
        for it in range(NIT):
            pose = pose + np.float32(1.0)
            if world > 1:
                src = np.zeros((Bmax, 3, 4), np.float32)
                src[:B] = pose
                gathered = np.concatenate(rdzv.all_gather(src), 0)

    for _ in range(1 + args.warmup):
        step()
    rdzv.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    rdzv.barrier()
    dt = rdzv.max(time.perf_counter() - t0) if world > 1 else time.perf_counter() - t0
    if world > 1:                                   # gather order: rank-major, each rank's block at r * Bmax, padding zero
        got = gathered.reshape(world, Bmax, 12)
        off = 0
        for r in range(world):
            want = (table[off:off + counts[r]] + np.float32(NIT)).reshape(counts[r], 12)
            assert np.array_equal(got[r, :counts[r]], want), "all-gather returned wrong poses for rank %d" % r
            assert not got[r, counts[r]:].any()
            off += counts[r]
    if args.dump_outputs and rank == 0:             # what the stand-in computed: every rank's poses, as gathered
        dump_outputs(args.dump_outputs, {"pose_est": np.concatenate([got[r, :counts[r]] for r in range(world)]).reshape(-1, 3, 4)
                                         if world > 1 else pose})
    # which GPU every rank's convenience calls would land on with a GPU per rank (Context.default(): DEEPIM_DEVICE, else LOCAL_RANK),
    # and what it has opened (nothing, here). Context.default_device_id() is not called: it counts the visible GPUs through HIP,
    # which would open the device in every rank of the rehearsal
    Context.set_default(int(os.environ.get("DEEPIM_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    my = dict(comm_record(None), default_device=Context.default_device_id(), opened=list(Context.opened))
    recs = rdzv.all_gather(json.dumps(my).encode()) if world > 1 else [json.dumps(my).encode()]
    if rank == 0:
        out = headline(args, world, NIT, dt, total, scaling, args.steps, args.warmup, total if scaling == "strong" else B)
        out["config"] = {"workload": "DRY RUN (no GPU): launch rehearsal of the %d-rank path" % world, "pairs_per_gpu": B,
                         "global_batch": total, "iters": NIT, "shard_counts": counts}
        c0 = json.loads(recs[0].decode())
        out["comm"] = {"backend": "host-dry-run" if world > 1 else "none", "rccl_ranks": 0, "rccl_version": c0["rccl_version"],
                       "librccl_path": c0.get("librccl_path") or None, "libamdhip64_path": c0.get("libamdhip64_path") or None,
                       "allgather_us": None, "ranks_reporting": len(recs),
                       "default_device_by_rank": [json.loads(r.decode())["default_device"] for r in recs],
                       "devices_opened_by_rank": [json.loads(r.decode())["opened"] for r in recs]}
        out["roofline"] = None
        out["dry_run"] = True
        print(json.dumps(out) if args.full_record else compact_line(out))
        sys.stdout.flush()
    rdzv.close()


class Loop(object):
    """One bound configuration of the refinement loop on this rank: network, synthetic batch (this rank's block), the closed-loop
    step, its HIP-event timers and the barrier-bracketed timing."""
    AUX_STEPS = 3

    def __init__(self, args, ctx, rdzv, comm, rank, world, B, Bmax, gbatch, strong, steps):
        self.args, self.ctx, self.rdzv, self.comm, self.rank, self.world = args, ctx, rdzv, comm, rank, world
        self.B, self.Bmax, self.NIT, self.steps = B, Bmax, args.iters, steps
        self.counts = parallel.shard_counts(gbatch, world) if strong else [B] * world
        self.outputs = None
        NIT, h = self.NIT, ctx.handle
        cfg = default_config()
        cfg.network.FP16_CONV = bool(args.fp16)
        cfg.network.X3_CONV = bool(args.x3)
        cfg.network.WINOGRAD_CONV = not args.no_winograd
        cfg.network.INPUT_DEPTH = bool(args.depth)
        if args.heads:
            cfg.TEST.FAST_TEST = False
        self.cfg = cfg
        net = self.net = deepIM_flownet().get_symbol(cfg)
        params = self.params = net.init_weights(cfg, seed=2333)
        # random-init translation head: damp it so 4 closed-loop iterations keep the object inside the frame
        params["trans_weight"] = params["trans_weight"] * np.float32(0.02)
        params["trans_bias"] = params["trans_bias"] * np.float32(0.02)
        net.bind(ctx, B, params)
        # only the pre-staged mode needs the later frames ray-cast on the host; the closed loop renders them on the device
        nfr = NIT if args.prestaged else 1
        if strong:   # every rank builds the same global batch and keeps its block (contiguous blocks)
            batch = parallel.shard_pairs(synthetic.make_batch(gbatch, seed=2333, n_frames=nfr, with_depth=args.depth),
                                         world, rank, gbatch)
        else:
            batch = synthetic.make_batch(B, seed=2333 + rank, n_frames=nfr, with_depth=args.depth)
        self.batch = batch
        self.image_observed = ctx.array(batch["image_observed"])
        self.depth_observed = ctx.array(batch["depth_gt_observed"]) if args.depth else None
        self.frames = [{"image_rendered": ctx.array(batch["image_rendered"][f]), "mask_rendered": ctx.array(batch["mask_rendered"][f]),
                        "mask_observed": ctx.array(batch["mask_observed_frames"][f])} for f in range(nfr)]
        if args.depth:
            for f in range(nfr):
                self.frames[f]["depth_rendered"] = ctx.array(batch["depth_rendered"][f])
        self.pose_init = ctx.array(batch["src_pose"][0])
        self.pose_cur = ctx.empty((B, 3, 4))
        # closed loop (tester.py:420-455): re-render at the refined pose on the device between iterations
        axes = [0.05, 0.04, 0.035]
        mesh = dict(synthetic.ellipsoid_mesh(axes), texture=synthetic.procedural_texture())
        mesh.pop("colors")
        self.light = None
        if args.lit:
            # BASELINE config 5 (ModelNet): the reference's loop draws through Render_Py_Light_ModelNet_Multi — per-fragment diffuse
            # term, light at 0.5·(0,1,1) + (t_x, −t_y, −t_z), per-render light colour U(0.9, 1.1) (tester.py:114-172); the colours
            # of every (iteration, pair) are drawn once, before the timed region, and stay on the device
            from mx_deepim_amd.lib.render_glumpy.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi
            nrm = mesh["vertices"] / (np.asarray(axes, np.float32) ** 2)
            mesh["normals"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
            self.render_machine = Render_Py_Light_ModelNet_Multi(["ellipsoid"], None, batch["K"], 640, 480, 0.25, 6.0,
                                                                 brightness_ratios=[0.7], meshes=[mesh], ctx=ctx,
                                                                 pixel_means=synthetic.PIXEL_MEANS[::-1].copy())
            rl = np.random.default_rng(77 + rank)
            self.light = [ctx.array(rl.uniform(0.9, 1.1, (B, 3)).astype(np.float32)) for _ in range(max(1, NIT - 1))]
        else:
            self.render_machine = Render_Py("synthetic", ["ellipsoid"], batch["K"], 640, 480, 0.25, 6.0,
                                            meshes={"ellipsoid": mesh}, ctx=ctx, pixel_means=synthetic.PIXEL_MEANS[::-1].copy())
        self.rbuf = {"image_rendered": ctx.empty((B, 3, 480, 640)), "depth_rendered": ctx.empty((B, 1, 480, 640)),
                     "mask_rendered": ctx.empty((B, 1, 480, 640)), "mask_observed": ctx.empty((B, 1, 480, 640))}
        # all-gather buffers: every rank contributes Bmax poses (ragged strong-scaling shards pad to the largest block)
        self.gather_in = ctx.zeros((Bmax, 3, 4)) if world > 1 else None
        self.gather_out = ctx.zeros((world * Bmax, 3, 4)) if world > 1 else None
        # HIP events inside the timed region: only the two that bracket the dominant kernel group (the 10 encoder launches) per
        # iteration — every event record costs the stream ~5 µs (profiles/r03_heads_b4_iteration_trace.txt: the gaps sit exactly at
        # the records), which is 1-2 % of a B = 4 iteration with six of them. The front end, the re-render and the pose gather are
        # timed by the same events over AUX_STEPS extra steps right after the timed region.
        # AUX_STEPS run with --full only: a plain run times its steps and nothing else
        aux = self.aux_steps = self.AUX_STEPS if args.full else 0
        self.enc_timers = [[ctx.timer() for _ in range(NIT)] for _ in range(max(steps, self.AUX_STEPS))]
        self.zoom_timers = [[ctx.timer() for _ in range(NIT)] for _ in range(aux)]
        self.render_timers = [[ctx.timer() for _ in range(NIT - 1)] for _ in range(aux)]
        self.gather_timers = [[ctx.timer() for _ in range(NIT)] for _ in range(aux)] if world > 1 else None
        self.use_graph = args.graph == "on"
        self.enc_graph = None
        # "step": the whole step as hipGraph segments (auto: where the launches are short enough for the host gaps and the event records
        # to show — per-GPU batches <= 8, the shards of an 8- / 4-GPU run; not with the host-side TCP exchange, which syncs anyway)
        self.graph_step = (args.graph == "step" or (args.graph == "auto" and B <= 8)) and (world == 1 or comm is not None)
        self.step_graphs, self._capturing = None, None

    def run_encoder(self):
        if self.enc_graph is not None:
            lib.deepim_graph_launch(self.ctx.handle, self.enc_graph)
        else:
            self.net.encoder()

    def step(self, timers=None, ztimers=None, rtimers=None, gtimers=None, tap=None):
        if self.step_graphs is not None and not (timers or ztimers or rtimers or gtimers or tap):
            return self.replay_step()
        args, net, h, NIT, B, Bmax = self.args, self.net, self.ctx.handle, self.NIT, self.B, self.Bmax
        pose_cur = self.pose_cur
        lib.deepim_d2d(h, pose_cur, self.pose_init, pose_cur.nbytes)
        data = {"image_observed": self.image_observed, "src_pose": pose_cur}
        if args.depth:
            data["depth_observed"] = self.depth_observed
        data.update(self.frames[0])
        cap = self._capturing
        for it in range(NIT):
            if args.prestaged:
                data.update(self.frames[it])
            if tap is not None:
                tap("in", it, data)
            if ztimers:
                ztimers[it].start()
            net.zoom(data)
            if ztimers:
                ztimers[it].stop()
            if timers:
                timers[it].start()
            self.run_encoder()
            if timers:
                timers[it].stop()
            if args.heads:
                net.decoder()
                net.heads()
            net.pose_head_update(pose_cur, pose_cur)   # fc6 → (fc7 → rot/trans → se3 → RT_transform in one launch): the refined pose becomes the next iteration's src_pose
            if tap is not None:
                tap("out", it, data)
            if self.world > 1:                     # every rank/host gets all refined poses
                if cap is not None:                # graph capture: the exchange stays a direct enqueue BETWEEN two graph segments
                    cap("cut")
                self.exchange(gtimers[it] if gtimers else None)
                if cap is not None:
                    cap("resume")
            if it < NIT - 1 and not args.prestaged:
                if rtimers:
                    rtimers[it].start()
                data = update_test_batch(self.cfg, data, self.render_machine, pose_cur, out=self.rbuf,
                                         light_intensity=self.light[it] if self.light else None)
                if rtimers:
                    rtimers[it].stop()

    def exchange(self, gtimer=None):
        """The per-iteration pose all-gather: ONE ncclAllGather enqueued on the library's stream (ragged shards pad to the largest)."""
        h, B, Bmax, pose_cur = self.ctx.handle, self.B, self.Bmax, self.pose_cur
        src = pose_cur
        if B != Bmax:
            lib.deepim_d2d(h, self.gather_in, pose_cur, pose_cur.nbytes)
            src = self.gather_in
        if gtimer:
            gtimer.start()
        if self.comm is not None:          # one enqueue on the library's stream, no host sync
            self.comm.all_gather_poses(self.gather_out, src)
        else:                              # host path: same exchange through the TCP rendezvous
            parts = self.rdzv.all_gather(src.asnumpy())
            self.gather_out.copyfrom(np.concatenate(parts, 0))
        if gtimer:
            gtimer.stop()

    def capture_step(self):
        """Record one whole step — pose reset, and per iteration front end, encoder, [decoder + heads], pose head + update, re-render +
        mask update — into hipGraph segments: ONE graph at N = 1; at N > 1 the segments between the pose exchanges (the all-gather is
        enqueued directly between two replays). Every buffer is bound once (bind()), so the graphs replay on the same memory."""
        h = self.ctx.handle
        graphs = []

        def begin():
            lib.deepim_graph_begin(h)

        def end():
            gid = ctypes.c_int(-1)
            lib.deepim_graph_end(h, ctypes.byref(gid))
            graphs.append(gid.value)

        def cap(what):
            if what == "cut":
                end()
            else:
                begin()
        self.ctx.sync()
        self._capturing = cap
        begin()
        try:
            self.step()
        finally:
            self._capturing = None
            end()
        self.step_graphs = graphs

    def replay_step(self):
        h, g = self.ctx.handle, self.step_graphs
        lib.deepim_graph_launch(h, g[0])
        for gid in g[1:]:
            self.exchange()
            lib.deepim_graph_launch(h, gid)

    def fence(self):          # device idle on every rank, then a barrier, then nothing pending before the clock is read
        self.ctx.sync()
        self.rdzv.barrier()
        self.ctx.sync()

    def time(self, warmup):
        """Priming pass + `warmup` untimed steps, then exactly `self.steps` steps between two fences; -> seconds, MAX over ranks."""
        ctx, h, net = self.ctx, self.ctx.handle, self.net
        self.step()   # priming pass, never timed: first-call work (tap tables, scratch growth, RCCL channel set-up)
        if self.use_graph:   # every first-call allocation has happened: record the encoder's launches once (same kernels, same plans)
            ctx.sync()
            gid = ctypes.c_int(-1)
            lib.deepim_graph_begin(h)
            try:
                net.encoder()
            finally:
                lib.deepim_graph_end(h, ctypes.byref(gid))
            self.enc_graph = gid.value
            self.step()
        if self.graph_step:
            try:
                self.capture_step()
            except Exception as e:      # noqa: BLE001 — a launch that cannot be captured: say so, time direct launches
                sys.stderr.write("[bench] whole-step graph capture failed (%s): direct launches\n" % (repr(e)[:200],))
                self.step_graphs = None
                ctx.sync()
            self.step()
        for _ in range(warmup):
            self.step()
        self.fence()
        t0 = time.perf_counter()
        for s_ in range(self.steps):
            self.step(None if self.step_graphs else self.enc_timers[s_])
        self.fence()
        dt = time.perf_counter() - t0
        if self.args.dump_outputs:                # the last timed step's results, before the auxiliary steps below recompute them
            self.outputs = self.last_outputs()
        if self.aux_steps:
            for s_ in range(self.aux_steps):      # outside the timed region: front end / re-render / pose gather, by HIP events
                self.step(self.enc_timers[s_] if self.step_graphs else None, self.zoom_timers[s_], self.render_timers[s_],
                          self.gather_timers[s_] if self.gather_timers else None)
            self.fence()
        if self.world > 1:
            dt_local = dt
            dt = self.comm.max_over_ranks(dt_local) if self.comm is not None else self.rdzv.max(dt_local)   # MAX over ranks
            if self.args.full:
                assert abs(dt - self.rdzv.max(dt_local)) < 1e-9, "device and host max-over-ranks disagree"
                # the gather really delivered every rank's poses, in rank order
                got = self.gather_out.asnumpy().reshape(self.world, self.Bmax, 12)
                mine = self.rdzv.all_gather(self.pose_cur.asnumpy().reshape(self.B, 12))
                for r in range(self.world):
                    assert np.array_equal(got[r, :len(mine[r])], mine[r]), "all-gather returned wrong poses for rank %d" % r
        # sanity: poses finite, zoom status clean (a figure measured on broken poses is no figure)
        st = ctypes.c_int(0)
        lib.deepim_zoom_status(h, ctypes.byref(st))
        assert np.all(np.isfinite(self.pose_cur.asnumpy())) and st.value == 0, ("bad poses / zoom status", st.value)
        return dt

    def last_outputs(self):
        """What the last step handed its caller, on the host: the refined poses (at N > 1 every rank's, from the all-gather, padding
        dropped) and the last iteration's network outputs (this rank's pairs): se3, zoom_factor, and with --heads the mask and flow."""
        A = self.net.act
        out = {"pose_est": self.pose_cur.asnumpy(), "se3": A["se3"].asnumpy(), "zoom_factor": A["zoom_factor"].asnumpy()}
        if self.args.heads:
            out["mask_observed_pred"] = A["mask_observed_pred"].asnumpy()
            out["flow_est"] = A["flow_est"].asnumpy()
        if self.world > 1:
            g = self.gather_out.asnumpy().reshape(self.world, self.Bmax, 3, 4)
            out["pose_est"] = np.concatenate([g[r, :c] for r, c in enumerate(self.counts)])
        return out

    def means(self):
        m = lambda rows: float(np.mean([t.elapsed_ms() for row in rows for t in row])) if rows and rows[0] else None   # noqa: E731
        return {"enc_ms": m(self.enc_timers[:self.aux_steps] if self.step_graphs else self.enc_timers[:self.steps]), "zoom_ms": m(self.zoom_timers), "render_ms": m(self.render_timers),
                "gather_ms": m(self.gather_timers) if self.gather_timers else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="pairs in the batch (bs32 of BASELINE.json's metric): the GLOBAL batch, "
                    "sharded over the GPUs in contiguous blocks (strong scaling, BASELINE configs[2] as written) — per GPU with --weak")
    ap.add_argument("--global-batch", type=int, default=0, help="strong scaling with this many pairs in total (overrides --batch)")
    ap.add_argument("--weak", action="store_true", help="weak scaling: --batch pairs PER GPU, N x batch in total (at N > 1 a --full "
                    "run appends this figure to `other_configs` next to the strong-scaling headline)")
    ap.add_argument("--allow-comm-fallback", action="store_true", help="N > 1 only: if RCCL cannot be brought up on every rank, run "
                    "the pose exchange through the TCP rendezvous instead of exiting non-zero (the line then says "
                    "comm.backend = tcp-fallback; never an xGMI number)")
    ap.add_argument("--iters", type=int, default=4, help="refinement iterations per step")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--fp16", action="store_true", help="BASELINE config 5 mode: conv stack on the fp16 matrix cores "
                    "(NOT the headline: reduced precision; reported with dtype f16)")
    ap.add_argument("--no-winograd", action="store_true", help="fp32 path: keep conv3_1 / conv4_1 / conv5_1 / conv6_1 on the direct "
                    "kernels (default: fp32 Winograd F(2x2,3x3) where the layer fills the chip — same fp32 arithmetic, 2.25x fewer "
                    "multiplies, <= 1e-5 of the layer's range from the direct sum; the roofline block then carries the EXECUTED "
                    "MFMA rate next to the algorithmic one)")
    ap.add_argument("--x3", action="store_true", help="split-fp16 conv mode: conv2 … conv6_1 as hi·hi + hi·lo + lo·hi on the "
                    "fp16 matrix cores with fp32 accumulation — fp32-grade results (≈1e-6 of the fp32 path, inside north_star's "
                    "1e-4), not bit-exact; reported with dtype f16x3 next to the bit-exact fp32 headline")
    ap.add_argument("--layers", action="store_true", help="with --full: also report the per-layer conv timings in the record")
    ap.add_argument("--heads", action="store_true", help="BASELINE config 4 mode: full test graph (FAST_TEST off) with the "
                    "FlowNetS decoder and the mask / flow heads in every iteration (NOT the headline)")
    ap.add_argument("--no-other-configs", action="store_true", help="--full: skip the short secondary runs of the other BASELINE "
                    "configurations (B=16, B=4 share of config 3, config 4 heads, config 5 fp16) that a default N=1 --full run "
                    "appends to its JSON line as `other_configs` (and, at N > 1, the weak-scaling figure)")
    ap.add_argument("--autotune", action="store_true", help="dev: let the library time split-K factors per conv geometry on "
                    "the first call instead of using the deterministic cost-model plan")
    ap.add_argument("--prestaged", action="store_true", help="feed pre-staged rendered frames instead of re-rendering "
                    "on the device between iterations (the pre-rasteriser behaviour of this bench)")
    ap.add_argument("--depth", action="store_true", help="BASELINE config 5 input as written: RGB-D pairs, network.INPUT_DEPTH "
                    "(ZoomDepth of observed + rendered depth inside the timed front end, C_in = 10)")
    ap.add_argument("--lit", choices=("auto", "on", "off"), default="auto", help="re-render between the iterations with the lit render "
                    "machine of the reference's ModelNet loops (render_py_light_modelnet_multi.py: per-fragment diffuse term); auto = on "
                    "for BASELINE config 5 as written (--fp16 --depth), off otherwise (LINEMOD loops draw unlit texture)")
    ap.add_argument("--graph", choices=("auto", "step", "on", "off"), default="off", help="step: the WHOLE step (pose reset, 4 x (front end, "
                    "encoder, pose head + update, re-render)) replayed from hipGraph segments — one graph at N = 1, cut at the pose exchanges at "
                    "N > 1; the conv group's HIP-event time then comes from 3 direct-launch steps right after the timed region. auto: "
                    "step for per-GPU batches <= 8, off above. off (default; measured in round 6, profiles/r06_b4_share.md: 3 425 vs 3 417 it/s at "
                    "B = 4 — the queue stays ahead of the GPU either way). on: replay the encoder's launches (10 convs + split-K "
                    "second passes + layout passes) from one captured hipGraph instead of issuing them one by one. Measured "
                    "(profiles/r03_fp16_config5.md): no gain at B = 8 / B = 4 — the kernel trace shows no idle gaps between the "
                    "encoder's launches, the queue stays ahead of the GPU — so direct launches stay the default")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE", help="dev: deepim_set_option on the context "
                    "before anything runs (labelled in the line)")
    ap.add_argument("--dry-run", action="store_true", help="launch rehearsal without a GPU: the same rank / rendezvous / shard / "
                    "per-iteration pose all-gather (host backend) / max-over-ranks / one-JSON-line-from-rank-0 code path with a "
                    "host stand-in for the refinement step; the line carries \"dry_run\": true and no roofline")
    ap.add_argument("--verify", type=int, default=2, help="--full: parity of THIS configuration, outside the timed region, N=1 only: "
                    "after the timed loop one more step is run and for this many sampled pairs every one of its refinement "
                    "iterations is replayed through the CPU oracle (fed the frames the GPU rendered) → `parity` in the JSON "
                    "line; 0 = off")
    ap.add_argument("--no-layer-timings", action="store_true", help="--full: skip the per-layer HIP-event timings after the timed region (6 extra launches per "
                    "encoder layer; the rocprofv3 passes of tools/run_profiles.sh cut the trace by iteration count and must not see them)")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure and check everything the headline does not "
                    "need: the auxiliary steps (front end / re-render / pose gather times, roofline_zoom), the per-layer timings, the "
                    "parity replay (--verify), the CPU baseline, the other configurations and, at N > 1, the weak-scaling figure and the "
                    "all-gather checks. Without it a run sets up, warms up, times the steps, dumps its outputs and prints its line")
    ap.add_argument("--full-record", action="store_true", help="print the full record (what bench_detail.json holds) as the final line "
                    "instead of the compact one the driver parses (used by the secondary runs and the tests that read its fields)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step "
                    "computed as DIR/<name>.npy (float32): pose_est (the refined poses; every rank's at N > 1), se3 and zoom_factor of its "
                    "last iteration, and with --heads mask_observed_pred and flow_est; at most 64 MB in all (above that the per-pixel "
                    "arrays keep a fixed, seeded sample of pairs, listed in <name>_pairs.npy). Inputs and weights are seeded, so the same "
                    "arguments give the same inputs on every run")
    ap.add_argument("--extras-budget", type=float, default=200.0, help="--full: wall-clock budget in seconds for everything after the "
                    "timed region (parity, CPU baseline, other configs); what does not fit is reported as skipped")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.layers and not args.full:
        ap.error("--layers reports the per-layer timings of a --full run: pass --full too")
    args.lit = args.lit == "on" or (args.lit == "auto" and args.fp16 and args.depth)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "launch with torch.distributed.run --nproc-per-node %d" % args.gpus
    # "rccl": device all-gather over RCCL; "host": the same exchange through the TCP rendezvous, on request (rehearsals with
    # several ranks on one visible GPU, where RCCL refuses duplicate devices)
    backend = os.environ.get("DEEPIM_BENCH_BACKEND", "rccl")
    rdzv = parallel.Rendezvous(rank, world)          # no-op at world == 1
    if args.dry_run:                                 # before any HIP call: a rehearsal's ranks never open a GPU
        return dry_run(args, rank, world, rdzv)
    ndev = ctypes.c_int(0)
    lib.load().deepim_device_count(ctypes.byref(ndev))
    device_id = local_rank % max(1, ndev.value)

    Context.set_default(device_id)                   # convenience calls of the host mirrors (RT_transform, nd.array, …) follow this rank's GPU
    ctx = Context.get(device_id)
    h = ctx.handle
    if args.autotune:
        lib.deepim_set_option(h, b"conv_autotune", 1)
    for o in args.opt:
        name, _, val = o.partition("=")
        lib.deepim_set_option(h, name.encode(), int(val))
    comm, comm_note = None, None
    if world > 1 and backend == "rccl":
        # bring RCCL up, prove the all-gather on rank-stamped poses, and let the ranks AGREE on the outcome: a failure on any of
        # them (library missing, init error, wrong bytes back) is a failure of the run — exit non-zero on every rank, so that a
        # TCP number can never be mistaken for an xGMI one — unless --allow-comm-fallback asks for the rendezvous exchange
        err = None
        try:
            comm = parallel.PoseComm(ctx, rdzv)
            probe_in = ctx.array(np.full((1, 3, 4), float(rank), np.float32))
            probe_out = ctx.zeros((world, 3, 4))
            comm.all_gather_poses(probe_out, probe_in)
            got = probe_out.asnumpy()[:, 0, 0]
            if not np.array_equal(got, np.arange(world, dtype=np.float32)):
                err = "all-gather returned %s" % got.tolist()
            nranks = comm_record(h)["rccl_ranks"]           # ncclCommCount of the communicator this rank really holds
            if err is None and nranks != world:
                err = "communicator has %d ranks, the launch has %d" % (nranks, world)
        except Exception as e:          # noqa: BLE001
            err = "%s: %s" % (type(e).__name__, e)
        errs = rdzv.all_gather((err or "").encode())
        bad = [(r, e.decode(errors="replace")) for r, e in enumerate(errs) if e]
        if bad:
            if comm is not None:
                try:
                    comm.close()
                except Exception:       # noqa: BLE001
                    pass
            comm = None
            comm_note = "RCCL unavailable (rank %d: %s)" % bad[0]
            if rank == 0:
                sys.stderr.write("bench: %s%s\n" % (comm_note, " — poses exchanged through the TCP rendezvous instead "
                                                    "(--allow-comm-fallback)" if args.allow_comm_fallback else
                                                    " — refusing to time a TCP exchange as if it were RCCL over xGMI; "
                                                    "pass --allow-comm-fallback to run anyway"))
            if not args.allow_comm_fallback:
                rdzv.barrier()
                rdzv.close()
                sys.exit(3)
    NIT = args.iters
    B, Bmax, counts, gbatch, scaling = resolve_batches(args, world, rank)
    assert B > 0, "more GPUs than pairs"
    L = Loop(args, ctx, rdzv, comm, rank, world, B, Bmax, gbatch, scaling == "strong", args.steps)
    dt = L.time(args.warmup)
    if args.dump_outputs and rank == 0:
        shapes = dump_outputs(args.dump_outputs, L.outputs)
        sys.stderr.write("[bench] last timed step's outputs -> %s: %s\n" % (args.dump_outputs, shapes))
    cfg, net, params, batch, pose_cur, step = L.cfg, L.net, L.params, L.batch, L.pose_cur, L.step
    use_graph = L.use_graph

    # what every rank bound (library files, RCCL's own rank count), gathered for the `comm` block
    my_rec = comm_record(h)
    recs = [json.loads(r.decode()) for r in rdzv.all_gather(json.dumps(my_rec).encode())] if world > 1 else [my_rec]

    # N > 1, default configuration, --full: the weak-scaling figure (--batch pairs PER GPU) next to the strong-scaling headline — a
    # second, short timed run of the same loop on every rank
    weak = None
    plain = not (args.fp16 or args.x3 or args.heads or args.prestaged or args.layers or args.depth or args.weak)
    if args.full and world > 1 and plain and not args.no_other_configs:
        Lw = Loop(args, ctx, rdzv, comm, rank, world, args.batch, args.batch, world * args.batch, False, 8)
        dtw = Lw.time(2)
        mw = Lw.means()
        weak = {"value": world * args.batch * NIT * 8 / dtw, "unit": "pose-refinement iters/sec", "scaling": "weak",
                "pairs_per_gpu": args.batch, "global_batch": world * args.batch, "steps": 8, "warmup": 2,
                "ms_per_step": dtw / 8 * 1e3, "allgather_us": None if mw["gather_ms"] is None else mw["gather_ms"] * 1e3,
                "conv_tflops": encoder_flops_per_pair(Lw.net.cin) * args.batch / (mw["enc_ms"] * 1e-3) / 1e12}
        del Lw

    if rank == 0:
        pairs_total = gbatch
        mm = L.means()
        enc_ms, zoom_ms = mm["enc_ms"], mm["zoom_ms"]
        flops = encoder_flops_per_pair(net.cin) * B
        wino_layers = sorted(getattr(net, "packed_wino", {}))
        peak = 2500.0 if args.fp16 else FP32_PEAK_TFLOPS   # dense fp16 MFMA peak, MI355X_MICROARCH.md
        if args.x3:   # three fp16 MFMA products per algorithmic multiply-add on conv2 … conv6_1: peak in algorithmic FLOPs
            peak = 2500.0 / 3.0
        zoom_bytes = 2 * (net.cin * 480 * 640 * 4) * B   # read + write every zoomed channel once
        traffic, traffic_src = None, None                # HBM bytes per conv launch group from a recorded PMC pass
        tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if os.path.exists(tpath) and not args.fp16:
            tj = json.load(open(tpath)).get(("x3_B%d" if args.x3 else ("wino_B%d" if getattr(net, "packed_wino", None) else "B%d")) % B)
            if tj:
                traffic, traffic_src = tj["conv_launch_group_bytes_corrected"], tj["source"]
        kname = ("encoder conv group: conv_f16_pp/dma_kernel + conv1 patch kernel (fp16 MFMA, fp32 accumulate)" if args.fp16 else
                 "encoder conv group: conv_f16_dma_kernel<X3> (3 fp16 MFMAs per product; peak = 2.5 PF / 3) + conv1_x3_kernel" if args.x3 else
                 "encoder conv group, 10 layers, fp32 MFMA: conv_direct, conv_nc8" +
                 (", conv_wino8/4 (F(2x2,3x3): %d layers)" % len(wino_layers) if wino_layers else "") + " kernels")
        rl, rl_hbm = None, None       # no encoder times without --full when the timed steps replay whole-step graphs (no events inside)
        if enc_ms is not None:
            rl, rl_hbm = roofline_block(kname, flops, encoder_executed_flops_per_pair(net) * B, enc_ms, peak, wino_layers, traffic,
                                        traffic_src, os.path.join(ROOT, "profiles", "per_kernel.json"), B,
                                        plain=not (args.fp16 or args.x3 or args.heads or args.depth) and bool(wino_layers))
        out = headline(args, world, NIT, dt, pairs_total, scaling, args.steps, args.warmup, gbatch if scaling == "strong" else B)
        cback = "none" if world == 1 else ("rccl" if comm is not None else ("tcp-fallback" if backend == "rccl" else "tcp-host-requested"))
        out["comm"] = {
            "backend": cback,
            "rccl_ranks": my_rec["rccl_ranks"] if comm is not None else 0,     # ncclCommCount of rank 0's communicator
            "rccl_version": my_rec["rccl_version"] or None,
            "librccl_path": my_rec.get("librccl_path") or None, "libamdhip64_path": my_rec.get("libamdhip64_path") or None,
            "allgather_us": None if mm["gather_ms"] is None else mm["gather_ms"] * 1e3,   # HIP-event mean of the per-iteration gather
            "ranks_reporting": len(recs),
            "all_ranks_same_libraries": all(r.get("librccl_path") == my_rec.get("librccl_path") and
                                            r.get("libamdhip64_path") == my_rec.get("libamdhip64_path") and
                                            r.get("rccl_ranks") == my_rec.get("rccl_ranks") for r in recs),
            "note": comm_note}
        out.update({
            "config": {"workload": "LINEMOD-ape-like synthetic, bs%d (%s/GPU, %s), %d iters, 480x640, %s, %s, %s" % (
                           gbatch, "/".join(str(c_) for c_ in sorted(set(counts), reverse=True)), scaling, NIT,
                           "decoder+heads" if args.heads else "FAST_TEST",
                           "RGB-D" if args.depth else "8-ch",
                           "pre-staged frames" if args.prestaged else "closed loop, %s GPU re-render" % ("lit" if args.lit else "unlit")),
                       "pairs_per_gpu": B, "global_batch": pairs_total, "iters": NIT, "shard_counts": counts,
                       "encoder_launch": "whole step from %d hipGraph segment(s)" % len(L.step_graphs) if L.step_graphs else
                                         "hipGraph replay" if use_graph else "direct launches",
                       "parallelism": ("%d process(es), one per GPU, contiguous pair blocks; one RCCL ncclAllGather of the poses per iteration" % world) if comm_note is None
                                      else "%d ranks; %s; poses through the TCP rendezvous" % (world, comm_note)},
            "roofline": rl,
        })
        if zoom_ms is not None:           # the auxiliary steps of a --full run
            out["roofline_zoom"] = {"bound": "hbm", "kernel": "bbox + zoom_factor + resample (fused front end)",
                                    "achieved": zoom_bytes / (zoom_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": zoom_bytes / (zoom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "ms": zoom_ms,
                                    "note": "algorithmic bytes = read + write of every zoomed channel once (SURVEY 8d); the fused "
                                            "front end keeps BilinearSampler's float/double blend bit for bit (VALU work ~ the "
                                            "HBM time), see profiles/r03_zoom_ablation.md"}
        if rl_hbm:
            out["roofline_hbm"] = rl_hbm      # the Z / H / F kernels SURVEY 8(d) lists, algorithmic bytes / recorded time / 8 TB/s each
        if not args.prestaged and NIT > 1 and mm["render_ms"] is not None:
            out["render_ms"] = mm["render_ms"]
        if weak is not None:
            out.setdefault("other_configs", {})["weak_scaling_batch%d_per_gpu" % args.batch] = weak
        # ---- everything below runs with --full only, OUTSIDE the timed region and bounded by --extras-budget; the headline
        # above is complete already, and is printed even if the process is told to stop while the extras run
        emitted = [False]

        def emit(*_sig):
            if not emitted[0]:
                emitted[0] = True
                try:
                    with open(os.path.join(os.environ.get("DEEPIM_BENCH_DETAIL_DIR", ROOT), "bench_detail.json"), "w") as f:
                        json.dump(out, f, indent=1)
                except OSError:
                    pass
                if args.full_record:
                    print(json.dumps(out))
                else:
                    for row in detail_lines(out):
                        print(row)
                    print(compact_line(out))
                sys.stdout.flush()
            if _sig:
                os._exit(0)
        if args.full:
            import signal
            for sg in (signal.SIGTERM, signal.SIGINT):
                signal.signal(sg, emit)
            deadline = time.time() + args.extras_budget
            sys.stderr.write("[bench] timed region complete; extras (parity, CPU baseline, other configs) run under a %.0f s budget\n"
                             % args.extras_budget)
            sys.stderr.flush()

            def left():
                return deadline - time.time()
            if not (args.fp16 or args.x3 or args.no_layer_timings):       # live, this run: every encoder layer alone -> the dominant kernel's own roofline fraction
                lt = layer_timings(ctx, net, peak=peak)
                dom = max(lt, key=lambda r: r["ms"])
                fam = [r for r in lt if r["kernel"] == dom["kernel"]]
                rl["layers_live"] = lt
                rl["dominant_kernel"] = "%s (%s)" % (dom["kernel"], ", ".join(r["layer"] for r in fam))
                rl["dominant_ms"] = sum(r["ms"] for r in fam)
                rl["dominant_achieved"] = sum(r["tflops_executed"] * r["ms"] for r in fam) / rl["dominant_ms"]
                rl["dominant_frac"] = rl["dominant_achieved"] / peak
                if args.layers:
                    out["layers"] = lt
            if world == 1 and args.verify > 0:
                try:
                    out["parity"] = verify_parity(args, cfg, net, params, ctx, step, pose_cur, batch["K"], B)
                except Exception as e:                       # a checker failure must not lose the measured line — but it is loud
                    out["parity"] = {"error": repr(e)[:300], "within_bar": False}
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(params, cfg, batch, with_depth=args.depth)
            default_run = (world == 1 and plain and not args.global_batch
                           and args.batch == 32 and not args.no_other_configs and not args.no_cpu_baseline)
            if default_run:
                out["other_configs"] = other_configs(left)
        emit()
    if comm is not None:
        comm.close()
    rdzv.close()


def other_configs(left=lambda: 1e9):
    """Short secondary runs (separate processes, after the timed region of the headline) of the other BASELINE.json
    configurations on this GPU, so that they are measured by the same driver command: configs[1] (batch 16), the per-GPU share
    of configs[2] (batch 4), configs[3] (decoder + mask / flow heads in every iteration) and configs[4] AS WRITTEN (RGB-D pairs,
    INPUT_DEPTH, fp16 conv path) at its per-GPU share (batch 8) and at batch 32, and the training-style iteration of SURVEY 8f-4
    (forward + backward + SGD step at batch 4, with and without the decoder and heads: `training_iteration_*`). Each entry: value (it/s), ms_per_step,
    conv-stack TFLOP/s and its fraction of the peak, and — where the run carries one — its own `parity` block.
    `left()` = seconds of the extras budget still available; runs that no longer fit are reported as skipped."""
    import subprocess
    runs = [("configs[1]_ape_batch16", ["--batch", "16", "--verify", "1"]),
            ("configs[2]_per_gpu_share_batch4", ["--batch", "4", "--verify", "1"]),
            ("configs[2]_per_gpu_share_of_4_gpus_batch8", ["--batch", "8", "--verify", "1"]),
            ("configs[3]_decoder_mask_flow_heads_batch32", ["--heads", "--verify", "1"]),
            ("configs[3]_decoder_mask_flow_heads_per_gpu_share_batch4", ["--heads", "--batch", "4", "--verify", "1"]),
            ("configs[4]_rgbd_fp16_conv_per_gpu_share_batch8", ["--fp16", "--depth", "--batch", "8", "--verify", "1"]),
            ("configs[4]_rgbd_fp16_conv_batch32", ["--fp16", "--depth", "--verify", "0"]),
            ("fp16_conv_8ch_batch32", ["--fp16", "--verify", "0"]),
            ("split_fp16_x3_conv_batch32", ["--x3", "--verify", "1"]),
            ("split_fp16_x3_conv_batch4", ["--x3", "--batch", "4", "--verify", "0"]),
            ("configs[3]_heads_split_fp16_x3_batch32", ["--x3", "--heads", "--verify", "0"])]
    res = {}

    def training():
        # SURVEY 8f-4 (module.backward + sgd of the reference's training loop) at the per-GPU share of config 4, tools/bench_train.py
        for name, extra in (("training_iteration_heads_batch4", ["4", "heads", "json"]), ("training_iteration_pose_branch_batch4", ["4", "json"]),
                            ("training_step_x4_batch4", ["4", "heads", "step4", "json"])):
            if left() < 30:
                res[name] = {"skipped": "extras budget spent"}
                continue
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_train.py")] + extra, capture_output=True, text=True,
                                   timeout=max(30.0, min(120.0, left())))
                res[name] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            except Exception as e:      # noqa: BLE001
                res[name] = {"error": repr(e)[:200]}

    for name, extra in runs:
        if name.startswith("configs[4]") and "training_iteration_heads_batch4" not in res:
            training()
        if left() < 30:
            res[name] = {"skipped": "extras budget spent"}
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", "8", "--warmup", "2", "--full", "--no-cpu-baseline",
                                "--no-other-configs", "--full-record"] + extra, capture_output=True, text=True, timeout=max(30.0, min(150.0, left())))
            j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            res[name] = {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "dtype": j["dtype"],
                         "workload": j["config"]["workload"], "conv_tflops_executed": j["roofline"]["achieved"],
                         "conv_tflops_algorithmic": j["roofline"]["algorithmic_tflops"],
                         "conv_peak_tflops": j["roofline"]["peak"], "conv_frac": j["roofline"]["frac"]}
            if "parity" in j:
                res[name]["parity"] = {k: j["parity"].get(k) for k in ("pairs", "iters", "pose_max_rel", "se3_max_rel", "flow_max_rel",
                                                                        "mask_flip_frac", "zoom_idx_bit_exact", "net_input_bit_exact",
                                                                        "within_bar", "bar", "error") if k in j["parity"]}
            if "--x3" in extra:
                res[name]["arithmetic"] = ("conv2-conv6_1 and conv1 as hi*hi + hi*lo + lo*hi on fp16 (hi, lo) pairs, fp32 accumulation: "
                                           "every layer <= 1e-5 of the fp32 oracle (observed 2.4e-6), pose ~1e-6 (north_star bar 1e-4), "
                                           "final poses of the 4-iteration closed loop within 1.2e-7 of the canonical fp32 run "
                                           "(tests/test_gpu_x3.py, tests/test_gpu_baseline_configs.py); not bit-exact, hence a labelled "
                                           "mode; conv_peak = 2.5 PF / 3 products")
            elif "--fp16" in extra:
                res[name]["arithmetic"] = "plain fp16 operands, fp32 accumulation: pose ~2e-3 of the fp32 oracle, outside the 1e-4 bar (BASELINE config 5)"
        except Exception as e:      # a secondary figure must never break the headline line
            res[name] = {"error": repr(e)[:200]}
    return res


def layer_kernel_name(net, name, k, s):
    """Which kernel family the bound fp32 encoder runs a layer on (csrc/conv.hip, csrc/wino.hip)."""
    if name in getattr(net, "packed_wino", {}):
        return "conv_wino8/4_kernel<s2d>" if name in getattr(net, "wino_s2d", ()) else "conv_wino8/4_kernel"
    return "conv_direct_kernel" if name == ENCODER[0][0] else "conv_nc8_kernel"


def layer_timings(ctx, net, reps=5, peak=FP32_PEAK_TFLOPS):
    """Every encoder layer alone, HIP events around `reps` back-to-back launches on the library's stream (after the timed region): ms,
    algorithmic and executed TFLOP/s, fraction of the peak. The layer with the largest share is the `dominant_*` of the roofline."""
    res = []
    src = net.conv1_input()
    for li, geom in enumerate(net.enc_geom):
        name, cin, h, w, cout, k, s, p = geom
        t = ctx.timer()
        net.encoder_layer(li, src)
        t.start()
        for _ in range(reps):
            net.encoder_layer(li, src)
        t.stop()
        ms = t.elapsed_ms() / reps
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        fl = 2.0 * cout * cin * k * k * ho * wo * net.B
        ex = float(layer_executed_flops_per_pair(net, geom)) * net.B
        res.append({"layer": name, "kernel": layer_kernel_name(net, name, k, s), "ms": ms, "tflops": fl / (ms * 1e-3) / 1e12,
                    "tflops_executed": ex / (ms * 1e-3) / 1e12, "frac": ex / (ms * 1e-3) / 1e12 / peak})
        src = net.act[name]
    return res


if __name__ == "__main__":
    main()
