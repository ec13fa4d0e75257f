"""Host-side logic that needs no GPU: Prop string-kwarg parsing, shape inference, op registry,
pair sharding and the world_size-2 gloo all-gather of refined poses."""
import os
import types

import numpy as np
import pytest

import mx_deepim_amd.operator_py  # noqa: F401  (registers the ops)
from mx_deepim_amd import mx, parallel
from mx_deepim_amd.config import default_config
from mx_deepim_amd.mx.nd import _attr_to_str
from mx_deepim_amd.symbols import deepIM_flownet


def test_registry_matches_reference_op_types():
    assert mx.operator.registered_ops() == sorted(
        ["ZoomMask", "ZoomImage", "ZoomImageWithFactor", "ZoomDepth", "ZoomFlow", "ZoomMaskWithFactor", "ZoomTrans",
         "Transform3D", "FlowUpdater", "GroupPicker"])


def test_props_parse_string_kwargs_like_mxnet():
    cfg = default_config()
    K = cfg.dataset.INTRINSIC_MATRIX.flatten()
    p = mx.operator.get_registered("ZoomMask")(K=_attr_to_str(K), height="480", width="640")
    np.testing.assert_array_equal(p.K, cfg.dataset.INTRINSIC_MATRIX)
    assert p.list_arguments() == ["mask_observed", "mask_gt_observed", "mask_rendered", "src_pose"]
    assert p.list_outputs() == ["zoom_mask_observed", "zoom_mask_gt_observed", "zoom_mask_rendered", "zoom_factor"]
    _, out, aux = p.infer_shape([[4, 1, 480, 640]] * 3 + [[4, 3, 4]])
    assert out == [[4, 1, 480, 640]] * 3 + [[4, 4]] and aux == []
    q = mx.operator.get_registered("ZoomImageWithFactor")(pixel_means=_attr_to_str(cfg.network.PIXEL_MEANS.flatten()))
    np.testing.assert_allclose(q.pixel_means, cfg.network.PIXEL_MEANS[::-1])   # reversal, zoom_image_with_factor.py:80
    f = mx.operator.get_registered("ZoomFlow")(b_inv_zoom="True")
    assert f.list_arguments() == ["zoom_factor", "flow"] and f.list_outputs() == ["zoom_flow"]
    f = mx.operator.get_registered("ZoomFlow")()
    assert f.list_arguments() == ["zoom_factor", "flow", "flow_weights"]
    t = mx.operator.get_registered("Transform3D")(T_means="[0.0 0.0 0.0]", T_stds="[1.0 1.0 1.0]", rot_coord="CAMERA")
    assert t.list_arguments() == ["point_cloud", "rotation", "translation", "pose_src"]
    with pytest.raises(AssertionError):  # b_project_2d is NOT_IMPLEMENTED in the reference too (transform3d.py:32)
        mx.operator.get_registered("Transform3D")(T_means="[0 0 0]", T_stds="[1 1 1]", b_project_2d="True").create_operator(
            None, None, None)
    g = mx.operator.get_registered("GroupPicker")(group_num="13")
    assert g.infer_shape([[8, 52], [8]])[1] == [[8, 4]]
    u = mx.operator.get_registered("FlowUpdater")(K=_attr_to_str(K))
    assert u.infer_shape([[2, 1, 480, 640]] * 2 + [[2, 3, 4]] * 2)[1] == [[2, 2, 480, 640]] * 2


def test_symbol_graph_flags_follow_config():
    cfg = default_config()
    net = deepIM_flownet().get_symbol(cfg)
    assert net.cin == 8 and not net.with_decoder                      # shipped config: FAST_TEST prunes the decoder
    shapes = net.arg_shape_dict()
    assert shapes["flow_conv1_weight"] == (64, 8, 7, 7) and shapes["fc6_weight"] == (256, 81920)
    assert sum(int(np.prod(s)) for s in shapes.values()) == 45096391  # 45.09 M encoder parameters
    cfg.TEST.FAST_TEST = False
    net = deepIM_flownet().get_symbol(cfg)
    assert net.with_mask_head and net.with_flow_head
    assert net.arg_shape_dict()["deconv4_weight"] == (1026, 256, 4, 4)
    cfg.network.INPUT_DEPTH = True
    assert deepIM_flownet().get_symbol(cfg).cin == 10
    cfg.network.REGRESSOR_NUM = 2
    with pytest.raises(Exception):
        deepIM_flownet().get_symbol(cfg)
    w = deepIM_flownet().get_symbol(default_config()).init_weights(seed=1, names=("rot_weight", "trans_weight"))
    assert w["rot_weight"][0].min() >= 0.01 and abs(w["rot_weight"][1:]).max() <= 0.01   # deepIM_flownet.py:795-800


def test_shard_bounds_cover_all_pairs():
    for n, world in ((32, 8), (13, 8), (8, 8), (5, 2), (3, 4)):
        spans = [parallel.shard_bounds(n, world, r) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1
    batch = {"image_observed": np.zeros((6, 3, 4, 4)), "image_rendered": np.zeros((2, 6, 3, 4, 4)), "K": np.eye(3)}
    s = parallel.shard_pairs(batch, 4, 1)
    assert s["image_observed"].shape[0] == 2 and s["image_rendered"].shape[:2] == (2, 2) and s["K"].shape == (3, 3)
    three = {"image_observed": np.zeros((3, 3, 4, 4)), "K": np.eye(3)}        # 3 pairs: K (3,3) must not be taken for a per-pair array
    assert parallel.shard_pairs(three, 2, 1)["K"].shape == (3, 3) and parallel.shard_pairs(three, 2, 1)["image_observed"].shape[0] == 1


def _rdzv_worker(rank, world, port, counts, q):
    try:
        rd = parallel.Rendezvous(rank, world, "127.0.0.1", port)
        allp = np.arange(sum(counts) * 12, dtype=np.float32).reshape(-1, 3, 4)
        lo, hi = parallel.shard_bounds(sum(counts), world, rank)
        got = parallel.gather_padded(rd, allp[lo:hi], counts)
        uid = rd.broadcast(bytes(range(128)) if rank == 0 else None)          # the RCCL unique-id bootstrap
        ok = np.array_equal(got, allp) and uid == bytes(range(128)) and rd.max(rank * 1.5) == (world - 1) * 1.5
        rd.barrier()
        rd.close()
        q.put((rank, bool(ok)))
    except Exception as e:   # surface the failure instead of a queue timeout
        q.put((rank, repr(e)))


@pytest.mark.parametrize("counts", [[4, 4], [3, 2]])
def test_rendezvous_all_gather_world2(counts):
    """The N > 1 host path without torch: two processes, TCP star on 127.0.0.1, even and ragged pose shards."""
    import multiprocessing as mp
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = 31000 + os.getpid() % 2000 + len(set(counts))
    procs = [ctxm.Process(target=_rdzv_worker, args=(r, 2, port, counts, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


class _FailingLib(object):
    """Stands in for the C library: rank 0 cannot make the RCCL id (librccl missing, …)."""

    def deepim_comm_unique_id(self, buf):
        raise RuntimeError("librccl.so: cannot open shared object file")

    def deepim_comm_init(self, *a):
        raise AssertionError("must not be reached: nobody got an id")


def _posecomm_worker(rank, port, q):
    try:
        import mx_deepim_amd.runtime as rt
        rt.lib = _FailingLib()                       # PoseComm imports `lib` from the runtime module at construction
        rd = parallel.Rendezvous(rank, 2, "127.0.0.1", port)
        try:
            parallel.PoseComm(types.SimpleNamespace(handle=None), rd)
            q.put((rank, "no error"))
        except RuntimeError as e:
            errs = rd.all_gather(str(e).encode())    # what bench.py does next: the ranks agree on the verdict
            q.put((rank, [x.decode() for x in errs]))
        rd.close()
    except Exception as e:   # surface the failure instead of a queue timeout
        q.put((rank, repr(e)))


def test_rccl_id_failure_on_rank0_reaches_every_rank():
    """Rank 0's failure to make the RCCL id travels to the peers in the id's place: every rank raises the same RuntimeError
    (nobody waits for an id that never comes, nobody enters the collective init) and the rendezvous stays usable for the
    fallback exchange."""
    import multiprocessing as mp
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = 33000 + os.getpid() % 2000
    procs = [ctxm.Process(target=_posecomm_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert set(res) == {0, 1}
    for r in (0, 1):
        assert isinstance(res[r], list) and len(res[r]) == 2, res
        assert all("librccl.so" in m for m in res[r]), res


def test_rendezvous_single_rank_is_a_no_op():
    rd = parallel.Rendezvous(0, 1)
    assert rd.all_gather("x") == ["x"] and rd.max(2.5) == 2.5 and rd.broadcast(b"id") == b"id"
    rd.barrier()
    rd.close()


@pytest.mark.parametrize("counts", ["2,2", "3,2"])
def test_rendezvous_under_torchrun_matches_gloo(counts):
    """Launched the way the driver launches bench.py (torch.distributed.run, 2 ranks): the Rendezvous picks up RANK /
    WORLD_SIZE / MASTER_* from the launcher and its pose gather equals torch.distributed's gloo all-gather."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 33000 + os.getpid() % 2000 + len(counts) + int(counts[0])
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "_rdzv_worker.py"),
                        counts], cwd=root, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "rank 0 ok" in r.stdout and "rank 1 ok" in r.stdout


def test_rendezvous_wire_format_is_typed_binary_not_pickle():
    """nothing a peer sends may be unpickled.  Values round-trip through the typed codec; malformed or
    oversized frames raise instead of being interpreted."""
    src = open(parallel.__file__).read()
    assert "import pickle" not in src and "pickle.loads" not in src
    vals = [None, 3, -7, 2.5, b"\x00\x01id", np.arange(24, dtype=np.float32).reshape(2, 3, 4), np.zeros((0, 3, 4), np.float32),
            np.array([1.5, 2.5]), [None, 1.0, b"x", np.ones((2, 2), np.int32)]]
    for v in vals:
        back = parallel._decode(parallel._encode(v))
        if isinstance(v, np.ndarray):
            assert back.dtype == v.dtype and back.shape == v.shape and np.array_equal(back, v)
        elif isinstance(v, list):
            assert len(back) == len(v) and back[1] == 1.0 and back[2] == b"x" and np.array_equal(back[3], v[3])
        else:
            assert back == v and type(back) is type(v)
    import pickle
    for bad in (b"", b"Z", b"F\x00", b"A\x09\x01", b"A\x00\x01\x05\x00\x00\x00abc", b"L\x02\x00\x00\x00", pickle.dumps({"a": 1})):
        with pytest.raises(ValueError):
            parallel._decode(bad)
    with pytest.raises(TypeError):
        parallel._encode({"a": 1})


def _token_worker(rank, port, token, q):
    try:
        rd = parallel.Rendezvous(rank, 2, "127.0.0.1", port, timeout=20.0, token=token)
        got = rd.all_gather(float(rank))
        rd.close()
        q.put((rank, got))
    except Exception as e:
        q.put((rank, type(e).__name__))


def test_rendezvous_rejects_a_peer_with_the_wrong_token():
    """A process that does not hold the job token cannot take a rank's slot: the hub drops it and keeps waiting for
    the real rank 1, which then joins normally."""
    import multiprocessing as mp
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = 35000 + os.getpid() % 2000
    hub = ctxm.Process(target=_token_worker, args=(0, port, "job-secret", q))
    hub.start()
    intruder = ctxm.Process(target=_token_worker, args=(1, port, "guess", q))
    intruder.start()
    r = q.get(timeout=60)
    assert r == (1, "RuntimeError"), r             # the intruder is told no
    intruder.join(timeout=30)
    real = ctxm.Process(target=_token_worker, args=(1, port, "job-secret", q))
    real.start()
    res = sorted([q.get(timeout=60), q.get(timeout=60)])
    hub.join(timeout=30)
    real.join(timeout=30)
    assert res == [(0, [0.0, 1.0]), (1, [0.0, 1.0])], res


def test_rendezvous_moves_to_the_next_candidate_port_when_the_first_is_taken():
    """MASTER_PORT + 1 belongs to somebody else (a listener that never speaks): the hub binds the next port of the candidate list,
    the spoke skips the silent one and finds it; the exchange then works as usual."""
    import multiprocessing as mp
    import socket
    port = 37000 + os.getpid() % 2000
    squat = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    squat.bind(("127.0.0.1", port))
    squat.listen(4)
    try:
        ctxm = mp.get_context("spawn")
        q = ctxm.Queue()
        procs = [ctxm.Process(target=_token_worker, args=(r, port, "job-secret", q)) for r in range(2)]
        for p in procs:
            p.start()
        res = sorted([q.get(timeout=90), q.get(timeout=90)])
        for p in procs:
            p.join(timeout=30)
        assert res == [(0, [0.0, 1.0]), (1, [0.0, 1.0])], res
    finally:
        squat.close()


def _foreign_hub(port, q):
    try:
        parallel.Rendezvous(0, 2, "127.0.0.1", port, timeout=8.0, token="somebody-elses-job")
        q.put("joined")
    except Exception as e:      # noqa: BLE001 — its rank 1 never comes: times out, which is what the test expects
        q.put(type(e).__name__)


def test_rendezvous_skips_another_jobs_hub_on_the_first_port():
    """Another deepim job of this host owns MASTER_PORT + 1 and speaks the protocol: its hub refuses our spoke (wrong token). The
    spoke must go on to the next candidate port — where this job's hub had to move — instead of aborting on the refusal
    (ADVICE r3), and the foreign hub must not be blocked by our stray connection."""
    import multiprocessing as mp
    import socket
    import time
    port = 39000 + os.getpid() % 2000
    ctxm = mp.get_context("spawn")
    qf, q = ctxm.Queue(), ctxm.Queue()
    foreign = ctxm.Process(target=_foreign_hub, args=(port, qf))
    foreign.start()
    for _ in range(200):                      # wait until the foreign hub listens
        try:
            socket.create_connection(("127.0.0.1", port), timeout=0.2).close()
            break
        except OSError:
            time.sleep(0.05)
    procs = [ctxm.Process(target=_token_worker, args=(r, port, "job-secret", q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=90), q.get(timeout=90)])
    for p in procs:
        p.join(timeout=30)
    assert res == [(0, [0.0, 1.0]), (1, [0.0, 1.0])], res
    assert qf.get(timeout=30) == "RuntimeError"          # the foreign hub just timed out waiting for ITS rank 1
    foreign.join(timeout=30)


def test_rendezvous_needs_a_token_on_a_routable_address(monkeypatch):
    monkeypatch.delenv("DEEPIM_RDZV_TOKEN", raising=False)
    monkeypatch.delenv("LOCAL_WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="DEEPIM_RDZV_TOKEN"):
        parallel.Rendezvous(1, 2, "10.1.2.3", 29999, timeout=1.0)


@pytest.mark.parametrize("global_batch,counts", [(None, [4] * 8), (32, [4] * 8), (13, [2, 2, 2, 2, 2, 1, 1, 1])])
def test_eight_rank_launch_rehearsal(global_batch, counts):
    """The driver's 8-GPU command line, without GPUs: `python -m torch.distributed.run --nproc-per-node 8 bench.py --gpus 8
    --global-batch G --dry-run` — bench.py's own rank/env handling, rendezvous, RCCL-id broadcast, shard bounds, padded
    per-iteration pose gather (order checked inside on every rank), barrier-bracketed max-over-ranks timing, and exactly ONE
    JSON line, from rank 0 only.  (No RCCL run with N > 1 ranks exists yet: gpurun boxes have one GPU.)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # global_batch None = what the DRIVER passes (`--gpus 8` and nothing else about the batch): the default must be BASELINE
    # configs[2] as written — a global batch of 32 sharded 4 per GPU, strong scaling
    port = 36000 + os.getpid() % 2000 + (global_batch or 57)
    extra = [] if global_batch is None else ["--global-batch", str(global_batch)]
    global_batch = global_batch or 32
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "8", "--steps", "2", "--warmup", "1",
                        "--dry-run", "--full-record"] + extra, cwd=root, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines                       # rank 0 only
    d = json.loads(lines[0])
    assert d["dry_run"] is True and d["n_gpus"] == 8 and d["scaling"] == "strong" and d["steps"] == 2
    assert d["config"]["shard_counts"] == counts and d["config"]["global_batch"] == global_batch
    assert d["config"]["pairs_per_gpu"] == counts[0]
    assert abs(d["value"] - global_batch * 4 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    assert ("bs%d" % global_batch) in d["metric"]
    # the machine-readable exchange record (a dry run has no RCCL: says so, names the HIP runtime every rank would bind)
    c = d["comm"]
    assert c["backend"] == "host-dry-run" and c["rccl_ranks"] == 0 and c["ranks_reporting"] == 8 and c["allgather_us"] is None
    assert "libamdhip64" in (c["libamdhip64_path"] or "")
    # every rank's default context is ITS GPU (LOCAL_RANK), not GPU 0 — and a rehearsal opens none
    assert c["default_device_by_rank"] == list(range(8)) and c["devices_opened_by_rank"] == [[]] * 8


def test_default_context_follows_local_rank(monkeypatch):
    """The host mirrors' convenience calls (RT_transform, mx.nd.array, Render_Py, …) default to Context.default(): DEEPIM_DEVICE, else
    LOCAL_RANK (one process per GPU), else 0 — never a hard-wired GPU 0."""
    import re
    from mx_deepim_amd.runtime import Context
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setattr(Context, "visible_devices", staticmethod(lambda: 0))    # the selection alone; folding is checked below
    for env, want in (({}, 0), ({"LOCAL_RANK": "5"}, 5), ({"LOCAL_RANK": "5", "DEEPIM_DEVICE": "2"}, 2), ({"LOCAL_RANK": "x"}, 0)):
        monkeypatch.delenv("LOCAL_RANK", raising=False)
        monkeypatch.delenv("DEEPIM_DEVICE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setattr(Context, "_default_id", None)
        assert Context.default_device_id() == want
    # launchers that mask the GPUs per rank (one visible device, LOCAL_RANK = 5): the rank folds onto the visible devices instead of
    # failing in deepim_create with 'no such device' (ADVICE r5); an explicit DEEPIM_DEVICE is taken as written
    for ndev, env, want in ((1, {"LOCAL_RANK": "5"}, 0), (4, {"LOCAL_RANK": "5"}, 1), (8, {"LOCAL_RANK": "5"}, 5),
                            (1, {"LOCAL_RANK": "5", "DEEPIM_DEVICE": "2"}, 2)):
        monkeypatch.delenv("LOCAL_RANK", raising=False)
        monkeypatch.delenv("DEEPIM_DEVICE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setattr(Context, "_default_id", None)
        monkeypatch.setattr(Context, "visible_devices", staticmethod(lambda n=ndev: n))
        assert Context.default_device_id() == want, (ndev, env)
    monkeypatch.undo()
    monkeypatch.setattr(Context, "_default_id", None)
    Context.set_default(3)
    assert Context.default_device_id() == 3
    monkeypatch.setattr(Context, "_default_id", None)
    for dirpath, _, files in os.walk(os.path.join(root, "mx_deepim_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"Context\.get\(0\)", src), os.path.join(dirpath, f)


def test_operator_props_parse_boolean_kwargs_like_the_reference():
    """`s.lower() == "true"` everywhere (zoom_trans.py:81-82, zoom_flow.py:85, zoom_mask_with_factor.py:77, flow_updater.py:118) but in
    Transform3D, which uses distutils' strtobool (transform3d.py:290)."""
    from mx_deepim_amd.operator_py._common import istrue, strtobool
    assert istrue("True") and istrue("TRUE") and istrue(True) and not istrue("1") and not istrue("yes") and not istrue("on") and not istrue("False")
    assert strtobool("1") and strtobool("yes") and not strtobool("off")
    with pytest.raises(ValueError):
        strtobool("maybe")
    f = mx.operator.get_registered("ZoomFlow")(b_inv_zoom="1")
    assert f.b_inv_zoom is False
    z = mx.operator.get_registered("ZoomTrans")(b_inv_zoom="true", b_zoom_grad="yes")
    assert z.b_inv_zoom is True and z.b_zoom_grad is False


def test_graph_flags_are_wired_or_refused():
    """ROT_TYPE (deepIM_flownet.py:715, :791-793), SE3_DIST_LOSS / TRANS_LOSS_TYPE (:238-262): honoured or refused, never ignored."""
    from mx_deepim_amd.config import default_config
    from mx_deepim_amd.symbols import deepIM_flownet
    cfg = default_config()
    cfg.network.ROT_TYPE = "EULER"
    net = deepIM_flownet().get_symbol(cfg)
    sh = net.arg_shape_dict()
    assert net.rot_param == 3 and sh["rot_weight"] == (3, 256) and sh["rot_bias"] == (3,)
    assert not net.init_weights(cfg, seed=1)["rot_weight"].any()
    with pytest.raises(NotImplementedError):
        deepIM_flownet().get_symbol(cfg, is_train=True)
    cfg.network.ROT_TYPE = "AXIS"
    with pytest.raises(Exception, match="rot_type"):
        deepIM_flownet().get_symbol(cfg)
    cfg.network.ROT_TYPE = "QUAT"
    cfg.train_iter.SE3_DIST_LOSS = True
    tnet = deepIM_flownet().get_symbol(cfg, is_train=True)
    assert tnet.se3_dist_loss and tnet.trans_loss_type == "L2"
    cfg.train_iter.TRANS_LOSS_TYPE = "huber"
    with pytest.raises(Exception, match="TRANS_LOSS_TYPE"):
        deepIM_flownet().get_symbol(cfg, is_train=True)
    cfg.network.REGRESSOR_NUM = 2
    with pytest.raises(Exception, match="NOT IMPLEMENTED"):
        deepIM_flownet().get_symbol(cfg)


def test_weak_scaling_is_opt_in():
    """`--weak`: --batch pairs PER rank (the pre-round-4 default), labelled weak."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 38100 + os.getpid() % 1500
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--weak", "--batch", "3", "--dry-run"], cwd=root, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["scaling"] == "weak" and d["config"]["global_batch"] == 6 and d["config"]["shard_counts"] == [3, 3] and "bs3" in d["metric"]


def test_cpu_baseline_follows_the_stated_protocol():
    """bench.py's `cpu_baseline`: whole pair-iterations = oracle zoom -> the N-group on oneDNN
    (torch-CPU) -> oracle pose update, threads pinned to the physical cores, one untimed warm-up call then the timed ones, value = pairs /
    median, GFLOP/s of the convolution stack stated; the checker's own (bit-identical) build of the same iteration rides along as the
    secondary figure. (Two timed calls here; the bench takes >= 5.)"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from mx_deepim_amd import synthetic
    from mx_deepim_amd.config import default_config
    from mx_deepim_amd.symbols import deepIM_flownet
    cfg = default_config()
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=5)
    batch = synthetic.make_batch(2, seed=7, n_frames=1)
    r = bench.cpu_baseline(params, cfg, batch, budget_s=0.0, min_runs=2, max_runs=2, pairs=2)
    cores = bench.physical_cores()
    assert 1 <= cores <= os.cpu_count()
    assert r["kind"] == "port" and r["cores"] == cores and r["threads"] == cores and r["nproc"] == os.cpu_count()
    sp = r["seconds_per_call"]
    assert abs(r["value"] - 2.0 / sp["median"]) < 1e-9 * r["value"] and sp["min"] <= sp["median"] <= sp["max"]
    assert r["gflops"] > 1.0 and 0 < r["n_group_share_of_time"] < 1
    assert "1 untimed warm-up" in r["protocol"] and "2 timed" in r["protocol"] and "oneDNN" in r["sample"]
    c = r["secondary_checker_build"]
    si = c["seconds_per_iteration"]
    assert c["kind"] == "port" and c["threads"] == cores and "omp_num_threads" in c and c["gflops"] > 0.1
    assert abs(c["value"] - 1.0 / si["median"]) < 1e-9 * c["value"] and si["min"] <= si["median"] <= si["max"]
    assert r["value"] > c["value"]            # the library convolutions beat the one-chain-per-output checker build
    from oracle import net as onet
    assert onet.BLOCKED is False            # the timing switch is reset: the checker stays the checker


def test_bench_final_line_is_compact_and_parseable():
    """the driver parses the LAST stdout line; round 5's 22.8 KB line (lists of dicts) came back `parsed: null`. The
    final line is now `compact_line(record)`: < 4 KB, scalars and short strings only, with the contract's keys, `roofline.frac` and
    `cpu_baseline.value`; the full record goes to bench_detail.json. Checked on round 5's own full record and end to end on a dry run."""
    import json
    import subprocess
    import sys
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full = [l for l in open(os.path.join(root, "profiles", "r05_bench_default_n1.json.log")).read().splitlines() if l.startswith("{")][-1]
    assert len(full) > 20000
    rec = json.loads(full)
    rec["roofline"].update(layers_live=[{"layer": "conv2", "kernel": "k", "ms": 1.0, "tflops": 200.0, "tflops_executed": 120.0, "frac": 0.76}],
                           dominant_kernel="k (conv2)", dominant_ms=1.0, dominant_achieved=120.0, dominant_frac=0.76)
    line = bench.compact_line(rec)
    assert len(line) < 4096 and "\n" not in line
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "parity", "comm"):
        assert k in d, k
    assert d["value"] == pytest.approx(rec["value"], rel=1e-5) and d["roofline"]["frac"] == pytest.approx(rec["roofline"]["frac"], rel=1e-5)
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 128 and d["cpu_baseline"]["kind"] == "port"
    assert d["parity"]["pairs"] == "2 of 32" and d["parity"]["within_bar"] is True
    assert d["roofline"]["dominant_frac"] == 0.76 and "per_kernel" not in d["roofline"] and "other_configs" not in d

    def flat(v):
        if isinstance(v, dict):
            for x in v.values():
                yield from flat(x)
        else:
            yield v
    for v in flat(d):        # no lists of dicts, no string the driver's 128-character clip would cut
        assert not (isinstance(v, list) and any(isinstance(x, (dict, list)) for x in v))
        assert not isinstance(v, str) or len(v) <= 120
    rows = bench.detail_lines(rec)
    assert rows and all(r.startswith("# ") for r in rows) and any("configs[2]_per_gpu_share_batch4" in r for r in rows)
    # end to end: the default output of a (dry) run ends in exactly that kind of line
    r = subprocess.run([sys.executable, "bench.py", "--dry-run", "--steps", "2", "--warmup", "1"], cwd=root, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) < 4096 and json.loads(last)["dry_run"] is True


def test_bench_dump_outputs_stays_under_the_cap_with_a_fixed_sample(tmp_path):
    """bench.py --dump-outputs: float32 .npy files (float64 kept), small arrays whole, and above the cap every large array keeps
    the same seeded sample of pairs, recorded in <name>_pairs.npy, so that two runs write identical files."""
    import bench
    rng = np.random.default_rng(1)
    arrays = {"pose_est": rng.standard_normal((8, 3, 4)), "se3": rng.standard_normal((8, 7)).astype(np.float32),
              "mask": rng.standard_normal((8, 1, 240, 320)).astype(np.float32),
              "flow": rng.standard_normal((8, 2, 240, 320)).astype(np.float16)}
    cap = 4 << 20                                        # 7.4 MB of arrays
    shapes = bench.dump_outputs(str(tmp_path / "a"), arrays, cap=cap)
    bench.dump_outputs(str(tmp_path / "b"), arrays, cap=cap)
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == sorted(k + ".npy" for k in shapes) == sorted(os.listdir(str(tmp_path / "b")))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= cap
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in files}
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.array_equal(v, np.load(str(tmp_path / "b" / (k + ".npy")))), k
    assert got["pose_est"].dtype == np.float64 and np.array_equal(got["pose_est"], arrays["pose_est"])
    assert np.array_equal(got["se3"], arrays["se3"])
    idx = got["mask_pairs"].astype(int)
    assert np.array_equal(idx, got["flow_pairs"]) and 0 < len(idx) < 8 and np.all(np.diff(idx) > 0)
    assert np.array_equal(got["mask"], arrays["mask"][idx])
    assert np.array_equal(got["flow"], arrays["flow"][idx].astype(np.float32))
    small = bench.dump_outputs(str(tmp_path / "c"), arrays, cap=64 << 20)       # under the cap: everything whole, no index files
    assert small == {k: list(v.shape) for k, v in arrays.items()}


def test_bench_dry_run_dumps_outputs(tmp_path):
    """--dump-outputs end to end without a GPU: the dry run's stand-in poses, identical from run to run; --steps below 1 is refused."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, "bench.py", "--dry-run", "--steps", "3", "--warmup", "1", "--batch", "5",
                            "--dump-outputs", str(tmp_path / name)], cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert os.listdir(str(tmp_path / name)) == ["pose_est.npy"]
        outs.append(np.load(str(tmp_path / name / "pose_est.npy")))
    assert outs[0].dtype == np.float32 and outs[0].shape == (5, 3, 4) and np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], np.arange(60, dtype=np.float32).reshape(5, 3, 4) + 4)      # 4 refinement iterations of pose += 1
    r = subprocess.run([sys.executable, "bench.py", "--dry-run", "--steps", "0"], cwd=root, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_bench_layers_needs_full():
    """--layers adds the per-layer timings of a --full run to its record: alone it is refused, before anything runs."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "bench.py", "--dry-run", "--layers"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--full" in r.stderr


def test_bench_roofline_block_is_physical(tmp_path):
    """bench.py's `roofline` object: `frac` = executed FLOPs over the dense peak (<= 1); the algorithmic figure —
    which the Winograd layers push past the peak — sits beside it; the per-kernel table is read from the recorded pass when it was
    taken at this batch size."""
    import json
    import bench
    pk = {"batch": 32, "source": "test", "sum_ms": 6.0, "bench_ms_per_launch_group_same_run": 6.01,
          "per_kernel": [{"layer": "conv1", "frac": 0.78}], "roofline_hbm": [{"kernel": "flow_kernel", "frac": 0.43}]}
    path = str(tmp_path / "per_kernel.json")
    json.dump(pk, open(path, "w"))
    rl, hbm = bench.roofline_block("k", 1242.7e9, 734.0e9, 6.1, 157.3, ["conv2"], None, None, path, 32)
    assert abs(rl["achieved"] - 734.0e9 / 6.1e-3 / 1e12) < 1e-9 and abs(rl["frac"] - rl["achieved"] / 157.3) < 1e-12 and rl["frac"] <= 1.0
    assert rl["algorithmic_over_peak"] > 1.0 and abs(rl["algorithmic_tflops"] - 1242.7e9 / 6.1e-3 / 1e12) < 1e-9
    assert rl["per_kernel"] == pk["per_kernel"] and hbm == pk["roofline_hbm"]
    rl4, hbm4 = bench.roofline_block("k", 155.3e9, 100e9, 1.2, 157.3, ["conv2"], None, None, path, 4)
    assert "per_kernel" not in rl4 and hbm4 is None                      # recorded at another batch size: not quoted
    rlx, hbmx = bench.roofline_block("k", 100e9, 100e9, 1.0, 2500.0, [], None, None, path, 32, plain=False)
    assert "per_kernel" not in rlx and hbmx is None and rlx["frac"] == rlx["algorithmic_over_peak"]


def test_recorded_per_kernel_table_is_consistent():
    """profiles/per_kernel.json (tools/profile_summary.py perkernel, from the rocprofv3 pass of the default bench command): every fraction is
    <= 1, the per-layer times sum to the conv launch group bench.py's own HIP events measured in the SAME run within 2 %, and every kernel
    SURVEY 8(d) lists has its HBM entry."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "profiles", "per_kernel.json")
    if not os.path.exists(path):
        pytest.skip("no recorded pass committed yet")
    d = json.load(open(path))
    assert [r["layer"] for r in d["per_kernel"]] == ["conv1", "conv2", "conv3", "conv3_1", "conv4", "conv4_1", "conv5", "conv5_1", "conv6", "conv6_1"]
    for r in d["per_kernel"]:
        assert 0 < r["frac"] <= 1.0 and r["executed_tflops"] <= r["algorithmic_tflops"] + 1e-9, r
        assert r["mfma_busy"] is None or 0 < r["mfma_busy"] <= 1.0
    assert abs(sum(r["ms"] + r["split_k_reduce_ms"] for r in d["per_kernel"]) - d["sum_ms"]) < 1e-9
    assert abs(d["sum_ms"] - d["bench_ms_per_launch_group_same_run"]) <= 0.02 * d["bench_ms_per_launch_group_same_run"]
    names = {r["kernel"].split("<")[0].replace("upsample16x4", "upsample16") for r in d["roofline_hbm"]}
    assert {"flow_kernel", "resolve_kernel", "upsample16_kernel", "resample4_kernel", "conv_fewout_kernel"} <= names
    assert all(0 < r["frac"] <= 1.0 for r in d["roofline_hbm"])


def test_bench_executed_flops_count_what_the_winograd_layers_run():
    """bench.py's `roofline.executed`: 16 positions per 2x2 tile and channel pair on the 3x3 Winograd layers, 49 of the 64 (position,
    phase) pairs on the stride-2 ones (Cin % 16 == 0), 9 / 25 / 49 taps per output on the direct layers."""
    import bench
    from mx_deepim_amd.symbols.deepIM_flownet import ENCODER

    class Net(object):
        pass
    net = Net()
    net.enc_geom, h, w, cin = [], 480, 640, 8
    for name, cout, k, s, p in ENCODER:
        net.enc_geom.append((name, cin, h, w, cout, k, s, p))
        h, w, cin = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, cout
    net.packed_wino, net.wino_s2d = {}, set()
    assert bench.encoder_executed_flops_per_pair(net) == bench.encoder_flops_per_pair(8)
    net.packed_wino = {n: None for n in ("conv2", "conv3", "conv3_1", "conv4_1", "conv5_1", "conv6_1")}
    net.wino_s2d = {"conv2", "conv3"}
    direct = {g[0]: 2 * g[4] * g[1] * g[5] ** 2 * ((g[2] + 2 * g[7] - g[5]) // g[6] + 1) * ((g[3] + 2 * g[7] - g[5]) // g[6] + 1) for g in net.enc_geom}
    want = sum(v for n, v in direct.items() if n not in net.packed_wino)
    want += 2 * 128 * 49 * 64 * 60 * 80 + 2 * 256 * 49 * 128 * 30 * 40                     # conv2, conv3: 49 positions x Cin per 2x2 tile
    want += 2 * 256 * 256 * 16 * 30 * 40 + 2 * 512 * 512 * 16 * 15 * 20                   # conv3_1, conv4_1
    want += 2 * 512 * 512 * 16 * 8 * 10 + 2 * 1024 * 1024 * 16 * 4 * 5                    # conv5_1 (15x20 -> 8x10 tiles), conv6_1
    assert bench.encoder_executed_flops_per_pair(net) == want
    assert 0.55 < want / bench.encoder_flops_per_pair(8) < 0.62
