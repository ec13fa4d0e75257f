"""bench.py contract checks on the GPU box: the one JSON line the driver parses, at N = 1 and — launched exactly as the
driver launches it (torch.distributed.run) with both ranks on the one visible GPU — the N = 2 code path incl. the
per-iteration all-gather validation, weak and strong (--global-batch) scaling.  RCCL refuses two ranks on one device, so
the two-rank runs route the same exchange through the host rendezvous (DEEPIM_BENCH_BACKEND=host); the RCCL entry points
themselves are exercised with a world-size-1 communicator."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline")


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def test_bench_line_single_gpu():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "1", "--warmup", "1", "--batch", "2", "--full", "--no-cpu-baseline",
                        "--verify", "0"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) < 4096, len(last)          # the compact line the driver parses; detail in bench_detail.json
    d = json.loads(last)
    assert d == _last_json(r.stdout)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "pose-refinement iters/sec" and d["dtype"] == "f32" and d["scaling"] == "strong"
    assert d["comm"]["backend"] == "none" and d["comm"]["rccl_ranks"] == 0
    full = json.load(open(os.path.join(ROOT, "bench_detail.json")))
    assert "libamdhip64" in full["comm"]["libamdhip64_path"] and full["value"] == pytest.approx(d["value"], rel=1e-5)
    assert 0 < d["roofline"]["dominant_frac"] < 1 and len(full["roofline"]["layers_live"]) == 10
    assert abs(d["value"] - 2 * 4 * 1 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4
    assert 0 < rf["frac"] < 1 and d["config"]["workload"]


def test_plain_run_times_its_steps_and_nothing_else():
    """Without --full a run sets up, warms up, times its steps and prints the line: the contract's keys and the encoder roofline
    from the HIP events inside the timed steps, but no auxiliary steps (roofline_zoom, render_ms), no per-layer timings, no parity
    replay, no CPU baseline and no other configurations."""
    r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--batch", "2"], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) < 4096, len(last)
    d = json.loads(last)
    for k in REQUIRED:
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert abs(d["value"] - 2 * 4 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    rf = d["roofline"]
    assert 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4 and "dominant_frac" not in rf
    for k in ("roofline_zoom", "render_ms", "parity", "cpu_baseline", "other_configs"):
        assert k not in d, k
    assert "timed region complete" not in r.stderr and d["comm"]["allgather_us"] is None


def test_bench_dump_outputs_of_the_last_timed_step(tmp_path):
    """--dump-outputs: the last timed step's results as float32 .npy files — the refined poses and the last iteration's se3 /
    zoom_factor — identical in two runs with the same arguments (seeded inputs), and with --steps the number of timed steps."""
    got = []
    for name, steps in (("a", "3"), ("b", "2")):
        r = subprocess.run([sys.executable, "bench.py", "--steps", steps, "--warmup", "1", "--batch", "2", "--no-cpu-baseline",
                            "--verify", "0", "--no-other-configs", "--no-layer-timings", "--dump-outputs", str(tmp_path / name)],
                           cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        assert _last_json(r.stdout)["steps"] == int(steps)
        files = sorted(os.listdir(str(tmp_path / name)))
        assert files == ["pose_est.npy", "se3.npy", "zoom_factor.npy"], files
        got.append({f[:-4]: np.load(str(tmp_path / name / f)) for f in files})
    a, b = got
    assert a["pose_est"].shape == (2, 3, 4) and a["se3"].shape[0] == 2 and a["zoom_factor"].shape[0] == 2
    for k in a:
        assert a[k].dtype == np.float32 and np.all(np.isfinite(a[k])), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("extra,bar", [([], 1e-4), (["--batch", "16"], 1e-4)], ids=["bs32_headline", "bs16_configs1"])
def test_bench_reports_parity_of_the_timed_configuration(extra, bar):
    """BASELINE.md §3's "max rel. error vs oracle" column, measured by bench.py itself on the configuration it times:
    B = 32 (the headline) and B = 16 (configs[1]) under the DEFAULT split-K plan, all 4 closed-loop iterations of two
    sampled pairs replayed through the CPU oracle.  Bars: pose and se3 <= 1e-4 relative, zoom factors / crop indices /
    net input bit-exact."""
    r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-other-configs",
                        "--full", "--full-record", "--verify", "2"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    p = d["parity"]
    print("bench parity %s: pose %.2e se3 %.2e (pairs %s, %d iterations, oracle %.0f s)" % (
        extra, p["pose_max_rel"], p["se3_max_rel"], p["pair_index"], p["iters"], p["oracle_seconds"]))
    assert "error" not in p, p
    assert p["pairs"] == 2 and p["iters"] == 4
    assert p["pose_max_rel"] <= bar and p["se3_max_rel"] <= bar
    assert p["zoom_factor_bit_exact"] and p["zoom_idx_bit_exact"] and p["net_input_bit_exact"] and p["within_bar"]


def test_bench_parity_heads_and_config5_modes():
    """The same field for `--heads` (config 4 mode: + flow <= 1e-4, mask flips <= 1e-4 of the pixels) and for config 5 as
    written (`--fp16 --depth`: RGB-D input, against the oracle's fp16 emulation, bars 1e-4 / 1e-3)."""
    for extra in (["--heads", "--batch", "4"], ["--fp16", "--depth", "--batch", "8"]):
        r = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-other-configs",
                            "--full", "--full-record", "--verify", "1"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        d = _last_json(r.stdout)
        p = d["parity"]
        print("bench parity %s: %s" % (extra, {k: v for k, v in p.items() if k not in ("against", "bar")}))
        assert "error" not in p and p["within_bar"], p
        if "--depth" in extra:
            assert d["dtype"] == "f16" and "RGB-D" in d["config"]["workload"] and p["net_input_bit_exact"]
        else:
            assert p["flow_max_rel"] <= 1e-4 and p["mask_flip_frac"] <= 1e-4


def test_headline_survives_a_sigterm_during_the_extras():
    """the measured line must not be lost if the process is stopped while the secondary figures run. bench.py
    announces the end of the timed region on stderr; SIGTERM after that → exactly one JSON line on stdout, exit code 0."""
    import signal
    import time
    p = subprocess.Popen([sys.executable, "bench.py", "--steps", "1", "--warmup", "1", "--batch", "2", "--full", "--verify", "2",
                          "--no-other-configs"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    t0 = time.time()
    seen = False
    while time.time() - t0 < 600:
        line = p.stderr.readline()
        if not line:
            break
        if "timed region complete" in line:
            seen = True
            break
    assert seen, "bench.py never announced the end of the timed region"
    time.sleep(1.0)                      # inside verify_parity / cpu_baseline now (both take >= 10 s)
    p.send_signal(signal.SIGTERM)
    out, _ = p.communicate(timeout=120)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, out[-500:])
    d = json.loads(lines[0])
    assert d["value"] > 0 and "roofline" in d and "cpu_baseline" not in d


def _run_two_ranks(port, extra):
    env = dict(os.environ, DEEPIM_BENCH_BACKEND="host", MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "1",
                        "--warmup", "1", "--full"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return _last_json(r.stdout)


def test_bench_two_ranks_weak_scaling_dry_run():
    d = _run_two_ranks(29671, ["--weak", "--batch", "2"])
    assert d["n_gpus"] == 2 and "cpu_baseline" not in d and d["scaling"] == "weak"
    assert abs(d["value"] - 2 * 2 * 4 * 1 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["comm"]["backend"] == "tcp-host-requested" and d["comm"]["rccl_ranks"] == 0 and d["comm"]["allgather_us"] > 0


def test_bench_two_ranks_default_is_strong_scaling_of_the_global_batch():
    """What the driver passes is `--gpus N` only: the batch is then GLOBAL (here --batch 4 → 2 per rank), strong scaling, and the
    default run appends the weak-scaling figure (--batch per GPU) to other_configs."""
    d = _run_two_ranks(29673, ["--batch", "4", "--full-record"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["global_batch"] == 4 and d["config"]["shard_counts"] == [2, 2]
    assert abs(d["value"] - 4 * 4 * 1 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"] and "bs4" in d["metric"]
    w = d["other_configs"]["weak_scaling_batch4_per_gpu"]
    assert w["scaling"] == "weak" and w["global_batch"] == 8 and w["value"] > 0


def test_bench_two_ranks_strong_scaling_ragged_dry_run():
    """--global-batch 3 over 2 ranks: shards of 2 and 1 pairs (padded all-gather), value counts the 3 global pairs."""
    d = _run_two_ranks(29675, ["--global-batch", "3"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["global_batch"] == 3
    assert abs(d["value"] - 3 * 4 * 1 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]


def test_bench_two_ranks_default_backend_agrees_on_the_rendezvous_fallback():
    """The driver's own command line (RCCL backend) with two ranks on ONE visible GPU: RCCL refuses the duplicate device at
    communicator init and every rank learns it over the rendezvous. Without --allow-comm-fallback the run REFUSES (exit code 3 on
    every rank, no JSON line: a TCP number must not pass for an xGMI one); with it all ranks fall back to the rendezvous exchange
    and the line says so, machine-readably (`comm.backend`). (On a multi-GPU node the same code path keeps RCCL.)"""
    import ctypes
    from mx_deepim_amd.runtime import lib
    ndev = ctypes.c_int(0)
    lib.load().deepim_device_count(ctypes.byref(ndev))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.pop("DEEPIM_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29679", "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "1", "--batch", "4", "--no-other-configs", "--full",
           "--full-record"]
    if ndev.value < 2:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
        assert r.returncode != 0 and not [l for l in r.stdout.splitlines() if l.startswith("{")], (r.stdout[-1500:], r.stderr[-1500:])
        assert "RCCL unavailable" in r.stderr and "--allow-comm-fallback" in r.stderr
        cmd[cmd.index("29679")] = "29683"
        cmd.append("--allow-comm-fallback")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "strong" and d["config"]["shard_counts"] == [2, 2]
    if ndev.value < 2:
        assert d["comm"]["backend"] == "tcp-fallback" and d["comm"]["rccl_ranks"] == 0 and "RCCL unavailable" in d["comm"]["note"]
        assert "RCCL unavailable" in d["config"]["parallelism"] and "rendezvous" in d["config"]["parallelism"], d["config"]
        assert "RCCL unavailable" in r.stderr
    else:
        assert d["comm"]["backend"] == "rccl" and d["comm"]["rccl_ranks"] == 2 and d["comm"]["allgather_us"] > 0
        assert "librccl" in d["comm"]["librccl_path"] and d["comm"]["all_ranks_same_libraries"]
        assert "ncclAllGather" in d["config"]["parallelism"], d["config"]


def test_rccl_entry_points_world_size_one(ctx):
    """deepim_comm_unique_id / comm_init / allgather_poses / comm_allreduce_f64 / comm_destroy through librccl.so itself
    (dlopen'ed by the library) with a one-rank communicator, plus the communicator-less copy path."""
    import ctypes
    import numpy as np
    from mx_deepim_amd.runtime import lib
    rng = np.random.default_rng(3)
    poses = rng.standard_normal((5, 3, 4)).astype(np.float32)
    src, dst = ctx.array(poses), ctx.zeros((5, 3, 4))
    lib.deepim_allgather_poses(ctx.handle, dst, src, 5)            # no communicator: plain copy
    np.testing.assert_array_equal(dst.asnumpy(), poses)
    uid = ctypes.create_string_buffer(128)
    lib.deepim_comm_unique_id(uid)
    assert any(uid.raw)
    lib.deepim_comm_init(ctx.handle, 0, 1, uid)
    try:
        dst2 = ctx.zeros((5, 3, 4))
        lib.deepim_allgather_poses(ctx.handle, dst2, src, 5)       # ncclAllGather on the library's stream
        t = ctx.array(np.array([1.25, -3.0]), dtype=np.float64)
        lib.deepim_comm_allreduce_f64(ctx.handle, t, 2, 0)
        np.testing.assert_array_equal(dst2.asnumpy(), poses)
        np.testing.assert_array_equal(t.asnumpy(), [1.25, -3.0])
        with __import__("pytest").raises(RuntimeError):
            lib.deepim_comm_init(ctx.handle, 0, 1, uid)             # already initialised
        # what this process bound: RCCL's own rank count, its version and the files the symbols in use live in
        buf = ctypes.create_string_buffer(2048)
        lib.deepim_comm_info(ctx.handle, buf, 2048)
        rec = dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))
        assert rec["backend"] == "rccl" and rec["rccl_ranks"] == "1" and int(rec["rccl_version"]) > 20000, rec
        assert "librccl" in rec["librccl_path"] and "libamdhip64" in rec["libamdhip64_path"], rec
    finally:
        lib.deepim_comm_destroy(ctx.handle)
