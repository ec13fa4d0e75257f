"""Per-pair cameras on the GPU: `deepim_bind_cameras` and the K_host == NULL rule (include/deepim_hip.h) through the zoom front
ends, the draws, deepim_pose_error, the flow entries, the render machines and pred_eval.

The contract is exact: sample b of a call that reads the bound table has the bits the SAME call (same B, same inputs) gives
with K_host = row b. So every comparison is np.array_equal on bits, against one host-K call per distinct camera, from which the
rows of that camera are taken. Batch: B = 5 with rows [K0, K1, K0, K2, K1] (tests/cameras_scene.py); frames 48 x 64 unless noted.
Only arp_2d is also compared with a float64 restatement, at the tolerance of the existing pose-error test."""
import ctypes

import numpy as np
import pytest

import cameras_scene as cs
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import tester
from mx_deepim_amd.lib.dataset.LM6D_REFINE import LM6D_REFINE
from mx_deepim_amd.lib.pair_matching import data_pair
from mx_deepim_amd.lib.render_glumpy.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
from mx_deepim_amd.runtime import lib
from mx_deepim_amd.symbols import deepIM_flownet

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
H, W, B, ROWS = 48, 64, cs.B, cs.ROWS
MEANS = cs.MEANS


def bits(a):
    a = a.asnumpy() if hasattr(a, "asnumpy") else np.asarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def check_rows(call, table_dev, cams, ctx, rows=ROWS):
    """call(K) → list of (n, ...) arrays. The table call (K = None, table bound) equals, row by row, the call with that row's
    camera as K_host."""
    ctx.bind_cameras(table_dev)
    got = [bits(a) for a in call(None)]
    ctx.bind_cameras(None)
    seen = 0
    for c in sorted(set(rows.tolist())):
        want = [bits(a) for a in call(cams[c])]
        sel = np.nonzero(rows == c)[0]
        for g, w in zip(got, want):
            assert g.shape == w.shape
            np.testing.assert_array_equal(g[sel], w[sel])
        seen += len(sel)
    assert seen == len(rows)
    return got


@pytest.fixture(scope="module")
def cams():
    return cs.cameras(H, W)


@pytest.fixture(scope="module")
def table_dev(ctx):
    return ctx.array(cs.table(H, W))


# ----------------------------------------------------------------------------------------------------------------- 1. zoom --
def _zoom_inputs(ctx, s):
    return {k: ctx.array(v) for k, v in s.items()}


@pytest.mark.parametrize("Wz", [64, 45], ids=["W64", "W45"])
def test_zoom_concat_and_image_forward(ctx, Wz):
    """the planes front end with masks and depth (W = 45: the generic plan kernels) and the mask-less deepim_zoom_image_forward;
    pair 3 has no rendered object (the rend[1] < 0 branch)"""
    s = cs.zoom_scene(H, Wz, seed=5)
    d = _zoom_inputs(ctx, s)
    cams_w, tab = cs.cameras(H, Wz), ctx.array(cs.table(H, Wz))
    for K in cams_w:
        assert np.isfinite(cs.zoom_factors_oracle(s, K)).all()              # no pair has an empty box under any camera

    def concat(K):
        out, zf = ctx.empty((B, 10, H, Wz)), ctx.empty((B, 4))
        lib.deepim_zoom_concat_forward(ctx.handle, d["image_observed"], d["image_rendered"], d["mask_observed"], d["mask_rendered"],
                                       d["depth_observed"], d["depth_rendered"], d["src_pose"], K, MEANS, out, zf, B, H, Wz)
        return [zf, out]

    def image(K):
        zo, zr, zf = ctx.empty((B, 3, H, Wz)), ctx.empty((B, 3, H, Wz)), ctx.empty((B, 4))
        lib.deepim_zoom_image_forward(ctx.handle, d["image_observed"], d["image_rendered"], d["src_pose"], K, MEANS, zo, zr, zf,
                                      B, H, Wz)
        return [zf, zo, zr]

    for call in (concat, image):
        got = check_rows(call, tab, cams_w, ctx)
        zf = got[0].view(np.float32)
        assert np.isfinite(zf).all()
        assert not np.array_equal(zf[0, 2:], zf[1, 2:])
    zf = check_rows(concat, tab, cams_w, ctx)[0].view(np.float32)
    for c, K in enumerate(cams_w):                                            # and the factors are the oracle's for each camera
        sel = np.nonzero(ROWS == c)[0]
        np.testing.assert_array_equal(bits(zf[sel]), bits(cs.zoom_factors_oracle(s, K)[sel]))
    # the camera matters where the rendered box exists (centre from K·t) and not where it does not (centre of the observed box)
    host = [concat(K)[0].asnumpy() for K in cams_w]
    assert not np.array_equal(host[0][0], host[1][0])
    np.testing.assert_array_equal(host[0][3], host[1][3])


def test_zoom_h16_and_frames(ctx, cams, table_dev):
    s = cs.zoom_scene(H, W, seed=6)
    d = _zoom_inputs(ctx, s)
    rng = np.random.default_rng(9)
    frames = ctx.array(rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8), dtype=np.uint8)
    fidx = ctx.array(np.array([1, 0, 0, 1, 1], np.int32), dtype=np.int32)

    def h16(K):
        main8, x2, zf = ctx.empty((B, H, W, 8), dtype=np.float16), ctx.empty((B, H, W, 2), dtype=np.float16), ctx.empty((B, 4))
        lib.deepim_zoom_concat_forward_h16(ctx.handle, d["image_observed"], d["image_rendered"], d["mask_observed"],
                                           d["mask_rendered"], d["depth_observed"], d["depth_rendered"], d["src_pose"], K, MEANS,
                                           main8, x2, zf, B, H, W)
        return [zf, main8, x2]

    def from_frames(K):
        out, zf = ctx.empty((B, 8, H, W)), ctx.empty((B, 4))
        lib.deepim_zoom_concat_frames_forward(ctx.handle, frames, fidx, 2, d["image_rendered"], d["mask_observed"],
                                              d["mask_rendered"], None, None, None, cf(1000.0), None, d["src_pose"], K, MEANS,
                                              out, zf, B, H, W)
        return [zf, out]

    for call in (h16, from_frames):
        got = check_rows(call, table_dev, cams, ctx)
        assert np.isfinite(got[0].view(np.float32)).all() and got[1].any()


# --------------------------------------------------------------------------------------------------------------- 2. render --
@pytest.fixture(scope="module")
def machines(ctx, cams):
    ell, box = cs.ellipsoid(), cs.box_mesh()
    plain = {"ell": {k: ell[k] for k in ("vertices", "faces", "colors")}, "box": {k: box[k] for k in ("vertices", "faces", "colors")}}
    rm = Render_Py("unused", ["ell", "box"], cams[0], W, H, meshes=plain, ctx=ctx, pixel_means=MEANS)
    tex = synthetic.procedural_texture(16, 32, seed=3)
    lit = [dict(vertices=m["vertices"], faces=m["faces"], uv=m["uv"], normals=m["normals"], texture=tex) for m in (ell, box)]
    rml = Render_Py_Light_ModelNet_Multi(["ell", "box"], None, cams[0], W, H, meshes=lit, ctx=ctx, pixel_means=MEANS)
    return rm, rml


def _bufs(ctx, n):
    return [ctx.empty((n, 3, H, W)), ctx.empty((n, 1, H, W)), ctx.empty((n, 1, H, W)), ctx.empty((n, 1, H, W))]


def test_render_machines_take_a_device_table(ctx, cams, table_dev, machines):
    rm, rml = machines
    poses = ctx.array(cs.poses(B, H, W, seed=31)[0])
    ids = ctx.array(np.array([0, 1, 1, 0, 1], np.int32), dtype=np.int32)
    inten = ctx.array(np.random.default_rng(4).uniform(0.9, 1.1, (B, 3)).astype(np.float32))

    def dev_or_host(K, sl=slice(0, B)):
        return table_dev[sl] if K is None else K

    def classes(K):          # two meshes, device ids: one launch group
        o = _bufs(ctx, B)
        rm.render_classes_into(o[0], o[1], ids, poses, K=dev_or_host(K), mask_rendered=o[2], mask_box=o[3])
        return o

    def one_mesh_slice(K):   # render_into on the slice [1:4]: the table binds with its offset
        o = _bufs(ctx, 3)
        rm.render_into(o[0], o[1], 1, poses[1:4], K=dev_or_host(K, slice(1, 4)), mask_rendered=o[2], mask_box=o[3])
        return o

    def lit(K):
        o = _bufs(ctx, B)
        rml.render_into(o[0], o[1], 0, poses, K=dev_or_host(K), mask_rendered=o[2], mask_box=o[3], light_intensity=inten)
        return o

    def lit_classes(K):
        o = _bufs(ctx, B)
        rml.render_classes_into(o[0], o[1], ids, poses, K=dev_or_host(K), mask_rendered=o[2], mask_box=o[3], light_intensity=inten)
        return o

    def batch_host_ids(K):   # render_batch with host ids: runs [0], [1, 1], [0], [1], each with its slice of the table
        o = _bufs(ctx, B)
        rm.render_batch([0, 1, 1, 0, 1], poses, K=dev_or_host(K), out=(o[0], o[1]), mask_rendered=o[2])
        return o[:3]

    for call, rows in ((classes, ROWS), (one_mesh_slice, ROWS[1:4]), (lit, ROWS), (lit_classes, ROWS), (batch_host_ids, ROWS)):
        got = check_rows(call, None, cams, ctx, rows=rows)
        mask = got[2].view(np.float32)
        assert all(mask[b].sum() >= 4 for b in range(len(rows))), call.__name__        # nothing passes on empty frames
    a, b = classes(cams[0])[1].asnumpy(), classes(cams[1])[1].asnumpy()
    assert not np.array_equal(a[0], b[0])                                              # the camera matters
    with pytest.raises(ValueError, match="batch"):
        rm.render_into(*_bufs(ctx, 3)[:2], 0, poses[1:4], K=table_dev)


def test_graph_replay_reads_the_tables_new_contents(ctx, cams, machines):
    """one captured table draw, replayed after the table was overwritten in place, equals the host-K draws with the new cameras"""
    rm, _ = machines
    poses = ctx.array(cs.poses(B, H, W, seed=32)[0])
    ids = ctx.array(np.array([1, 0, 1, 1, 0], np.int32), dtype=np.int32)
    tab = ctx.array(cs.table(H, W))
    o = _bufs(ctx, B)

    def draw(K, out):
        rm.render_classes_into(out[0], out[1], ids, poses, K=K, mask_rendered=out[2], mask_box=out[3])

    draw(tab, o)                                                              # eagerly first: scratch and z-buffer are sized
    first = [bits(a) for a in o]
    gid = ctypes.c_int(-1)
    lib.deepim_graph_begin(ctx.handle)
    try:
        draw(tab, o)
    finally:
        lib.deepim_graph_end(ctx.handle, ctypes.byref(gid))
    new_rows = np.array([2, 2, 1, 0, 0])
    tab.copyfrom(np.stack([cams[c] for c in new_rows]))                        # in place: the graph holds this address
    for a in o:
        a.copyfrom(np.float32(7.0))
    lib.deepim_graph_launch(ctx.handle, gid.value)
    got = [bits(a) for a in o]
    assert not np.array_equal(got[1], first[1])
    for c in range(3):
        w = _bufs(ctx, B)
        draw(cams[c], w)
        for g, x in zip(got, w):
            np.testing.assert_array_equal(g[new_rows == c], bits(x)[new_rows == c])


# ----------------------------------------------------------------------------------------------------------- 3. pose error --
@pytest.mark.parametrize("shared", [0, 1], ids=["per_sample_points", "shared_points"])
def test_pose_error(ctx, cams, table_dev, shared):
    N = 7
    rng = np.random.default_rng(17)
    gt, est = cs.poses(B, H, W, seed=33)
    pts = (rng.standard_normal((3, N) if shared else (B, 3, N)) * 0.04).astype(np.float32)
    e, g, p = ctx.array(est), ctx.array(gt), ctx.array(pts)

    def call(K):
        out = ctx.empty((B, 5))
        lib.deepim_pose_error(ctx.handle, out, e, g, p, shared, K, B, N)
        return [out]

    got = check_rows(call, table_dev, cams, ctx)[0].view(np.float32)
    want = [cs.arp_2d(est[b], gt[b], (pts if shared else pts[b]).T, cams[ROWS[b]]) for b in range(B)]
    np.testing.assert_allclose(got[:, 4], want, rtol=2e-4, atol=1e-6)       # the bar of tests/test_gpu_se3_heads.py's pose-error test
    assert not np.isclose(got[0, 4], call(cams[1])[0].asnumpy()[0, 4], rtol=1e-3)    # arp_2d depends on the camera


# ------------------------------------------------------------------------------------------------------------------ 4. flow --
@pytest.mark.parametrize("shape", [(48, 64), (30, 45)], ids=["48x64", "30x45_tail"])
def test_calc_KT_flow_epe_and_pair_flow_labels(ctx, shape):
    """30 x 45: H·W % 4 == 2, the EPE kernel's cnt < 4 tail. Pair 2 is skipped in the EPE. Five identical rows against the K_host
    call pit the device's inverse intrinsics against the host's."""
    Hf, Wf = shape
    cams_f, rows = cs.cameras(Hf, Wf), cs.table(Hf, Wf)
    s = cs.flow_scene(Hf, Wf, seed=40 + Hf)
    d = {k: ctx.array(v) for k, v in s.items()}
    skip = ctx.array(np.array([0, 0, 1, 0, 0], np.int32), dtype=np.int32)

    def kt(K):
        out = ctx.empty((B, 3, 4))
        lib.deepim_calc_KT(ctx.handle, out, d["pose_rendered"], d["pose_observed"], K, B)
        return [out]

    def epe(K):
        out, tot = ctx.empty((B, 6), dtype=np.float64), ctx.zeros((6,), dtype=np.float64)
        lib.deepim_flow_epe(ctx.handle, out, tot, d["flow_est"], d["depth_rendered"], d["depth_observed"], d["pose_rendered"],
                            d["pose_observed"], K, skip, cf(3e-3), 1, B, Hf, Wf)
        return [out]

    def labels(K):
        flow, wts = ctx.empty((B, 2, Hf, Wf)), ctx.empty((B, 2, Hf, Wf))
        lib.deepim_pair_flow_labels(ctx.handle, flow, wts, d["depth_rendered"], d["depth_observed"], d["pose_rendered"],
                                    d["pose_observed"], K, cf(3e-3), 0, 1, B, Hf, Wf)
        return [flow, wts]

    for c in (1, 2, 0):                                                       # five identical rows == the K_host call, all rows
        same = ctx.array(np.ascontiguousarray(np.stack([cams_f[c]] * B)))
        for call in (kt, epe, labels):
            check_rows(call, same, {0: cams_f[c]}, ctx, rows=np.zeros(B, int))
    tab = ctx.array(rows)
    check_rows(kt, tab, cams_f, ctx)
    e = check_rows(epe, tab, cams_f, ctx)[0].view(np.float64)
    assert (e[2] == 0).all() and (e[[0, 1, 3, 4], 3] > Hf * Wf / 4).all()     # the skipped row; the others see their object
    fl = check_rows(labels, tab, cams_f, ctx)
    assert all(fl[1].view(np.float32)[b].sum() > Hf * Wf / 2 for b in range(B))
    assert not np.array_equal(bits(epe(cams_f[0])[0])[1], bits(epe(cams_f[1])[0])[1])   # the camera matters


# ---------------------------------------------------------------------------------------------------------------- 5. errors --
def test_errors_come_from_the_host_and_name_the_entry(ctx, cams, table_dev):
    s = cs.flow_scene(H, W, seed=3)
    d = {k: ctx.array(v) for k, v in s.items()}
    kt = ctx.empty((B, 3, 4))
    ctx.bind_cameras(None)
    with pytest.raises(RuntimeError, match="deepim_calc_KT: K_host is NULL and no camera table is bound"):
        lib.deepim_calc_KT(ctx.handle, kt, d["pose_rendered"], d["pose_observed"], None, B)
    out = ctx.empty((B, 5))
    with pytest.raises(RuntimeError, match="deepim_pose_error: .*no camera table"):
        lib.deepim_pose_error(ctx.handle, out, d["pose_rendered"], d["pose_observed"], ctx.zeros((3, 1)), 1, None, B, 1)
    zf = ctx.empty((B, 4))
    img = ctx.zeros((B, 3, H, W))
    with pytest.raises(RuntimeError, match="deepim_zoom_image_forward: .*no camera table"):
        lib.deepim_zoom_image_forward(ctx.handle, img, img, d["pose_rendered"], None, MEANS, ctx.empty((B, 3, H, W)),
                                      ctx.empty((B, 3, H, W)), zf, B, H, W)
    ctx.bind_cameras(table_dev[0:3])                                          # n = 3 < B = 5
    with pytest.raises(RuntimeError, match="deepim_calc_KT: .*3 rows for a batch of 5"):
        lib.deepim_calc_KT(ctx.handle, kt, d["pose_rendered"], d["pose_observed"], None, B)
    with pytest.raises(RuntimeError, match="deepim_flow_epe: .*3 rows for a batch of 5"):
        lib.deepim_flow_epe(ctx.handle, ctx.empty((B, 6), dtype=np.float64), None, d["flow_est"], d["depth_rendered"],
                            d["depth_observed"], d["pose_rendered"], d["pose_observed"], None, None, cf(3e-3), 1, B, H, W)
    lib.deepim_calc_KT(ctx.handle, kt[0:3], d["pose_rendered"], d["pose_observed"], None, 3)      # n = 3 serves B = 3
    # the entries that keep requiring their K: an error code, not a host crash, whatever is bound
    ctx.bind_cameras(table_dev)
    noise = np.zeros(6, np.float32)
    with pytest.raises(RuntimeError, match="deepim_sample_rendered_poses failed.*K"):
        lib.deepim_sample_rendered_poses(ctx.handle, ctx.empty((B, 3, 4)), ctx.empty((B,), dtype=np.int32), None,
                                         d["pose_rendered"], None, noise, W, H, cf(0.0), 4, 1, 0, None, B)
    with pytest.raises(RuntimeError, match="deepim_flow_updater_forward: K_host is required"):
        lib.deepim_flow_updater_forward(ctx.handle, ctx.empty((B, 2, H, W)), ctx.empty((B, 2, H, W)), d["depth_rendered"],
                                        d["depth_observed"], d["pose_rendered"], d["pose_observed"], None, cf(3e-3), 0, B, H, W)
    assert ctx.bind_cameras(None) is None
    want = kt.copy()
    lib.deepim_calc_KT(ctx.handle, want, d["pose_rendered"], d["pose_observed"], cams[1], B)      # a host-K call still works
    ctx.bind_cameras(np.stack([cams[1]] * B))                                 # a numpy table: validated, uploaded, returned
    lib.deepim_calc_KT(ctx.handle, kt, d["pose_rendered"], d["pose_observed"], None, B)
    np.testing.assert_array_equal(bits(kt), bits(want))
    with pytest.raises(ValueError, match="finite"):
        ctx.bind_cameras(np.full((2, 3, 3), np.nan, np.float32))
    ctx.bind_cameras(None)


# ------------------------------------------------------------------------------------------------------------ 7. end to end --
HE, WE, BE = 480, 640, 3
MEANS_BGR = np.array([104.0, 117.0, 124.0])


class ListLogger(object):
    def __init__(self):
        self.lines = []

    def info(self, msg, *a):
        self.lines.append(str(msg))


def _to_bgr8(t, means_rgb):
    rgb = t + means_rgb.reshape(1, 3, 1, 1)
    return np.ascontiguousarray(np.clip(np.rint(rgb), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)[..., ::-1])


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16_conv"])
def test_pred_eval_with_a_camera_per_pair(ctx, tmp_path, fp16):
    """480 x 640, B = 3, test_iter = 2, PRED_FLOW on, FAST_TEST off: pred_eval over records carrying K0, K1, K2 against three
    runs of the same batch with config.dataset.INTRINSIC_MATRIX = K_b and no record K (same batch size, so the same per-sample
    bits): pair b's poses, errors and calc_EPE_batch row come from run b."""
    cfg = default_config()
    cfg.network.PIXEL_MEANS = MEANS_BGR.astype(np.float32)
    cfg.TEST.test_iter, cfg.TEST.FAST_TEST = 2, False
    cfg.dataset.class_name = ["ape"]
    if fp16:
        cfg.network.FP16_CONV = True
    K_cfg = np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32).reshape(3, 3).copy()
    cams3 = cs.cameras(HE, WE, K_cfg)
    np.testing.assert_array_equal(cams3[0], K_cfg)
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=20)
    params["trans_weight"] = params["trans_weight"] * np.float32(0.02)       # keep the object in frame (as bench.py does)
    params["trans_bias"] = params["trans_bias"] * np.float32(0.02)
    net.bind(ctx, BE, params)
    mesh = synthetic.ellipsoid_mesh(np.array([0.05, 0.04, 0.035]), 12, 24)
    mesh.pop("uv")
    means_rgb = MEANS_BGR[::-1].astype(np.float32)
    rm = Render_Py("unused", ["ape"], K_cfg, WE, HE, meshes={"ape": mesh}, ctx=ctx, pixel_means=means_rgb)
    points, diameters = {"ape": mesh["vertices"][::7]}, {"ape": 0.1}
    tgt, src = cs.poses(BE, HE, WE, seed=77)
    # every frame is drawn per pair with host-K calls: observed at pose_observed, rendered at pose_rendered, with the pair's camera
    frames = {"pose_rendered": src.copy(), "mask_idx": np.full(BE, 3, np.int32)}
    img, dep = ctx.empty((1, 3, HE, WE)), ctx.empty((1, 1, HE, WE))
    drawn = {}
    for kind, poses in (("observed", tgt), ("rendered", src)):
        im, de = [], []
        for b in range(BE):
            rm.render_into(img, dep, 0, ctx.array(poses[b:b + 1]), K=cams3[b])
            im.append(img.asnumpy()[0])
            de.append(dep.asnumpy()[0, 0])
        drawn[kind] = (np.stack(im), np.stack(de))
        assert all((d > 0).sum() > 500 for d in de)
    frames["image_observed"], frames["image_rendered"] = _to_bgr8(drawn["observed"][0], means_rgb), _to_bgr8(drawn["rendered"][0], means_rgb)
    frames["depth_rendered"] = np.rint(drawn["rendered"][1] * 1000).astype(np.uint16)
    frames["depth_gt_observed"] = np.rint(drawn["observed"][1] * 1000).astype(np.uint16)
    frames["mask_gt_observed"] = ((drawn["observed"][1] > 0) * 3).astype(np.uint8)
    recs = [{"pose_rendered": src[b].copy(), "pose_observed": tgt[b].copy(), "gt_class": "ape"} for b in range(BE)]
    recs_K = [dict(r, K=cams3[b]) for b, r in enumerate(recs)]

    def run(records, name, intrinsics=None):
        log = ListLogger()
        imdb = LM6D_REFINE(["ape"], points, diameters, ctx=ctx, logger=log, name=name, result_path=str(tmp_path / name))
        f = dict(frames) if intrinsics is None else dict(frames, intrinsics=intrinsics)
        data = data_pair.get_data_pair_test_batch(f, cfg)
        res = tester.pred_eval(cfg, tester.Predictor(cfg, net), [(data, f, records)], imdb, logger=log, render_machine=rm)
        out = net.forward(data)                                               # the first forward again, for the pair's EPE rows
        Kd = data.get("intrinsics")
        rows = tester.calc_EPE_batch(cfg, out["flow_est_crop"], tester.par_generate_gt(cfg, f), data["src_pose"], tgt, K=Kd).asnumpy()
        return res, rows, imdb

    res, rows, imdb = run(recs_K, "per_pair", intrinsics=np.stack(cams3))
    assert len(res["all_K"]) == 1 and len(res["all_K"][0]) == BE
    np.testing.assert_array_equal(np.stack(res["all_K"][0]), np.stack(cams3))
    np.testing.assert_array_equal([res["epe"][k] for k in tester.EPE_KEYS], (rows[0] + rows[1]) + rows[2])
    assert (rows[:, 3] > 100).all()
    try:
        for b in range(BE):
            cfg.dataset.INTRINSIC_MATRIX = cams3[b].copy()
            net.K, rm.K = cams3[b].copy(), cams3[b].copy()
            one, rows_b, _ = run(recs, "camera%d" % b)
            assert one["all_K"] is None
            for it in range(2):
                np.testing.assert_array_equal(bits(np.asarray(res["all_poses_est"][0][it][b])), bits(np.asarray(one["all_poses_est"][0][it][b])))
                assert res["all_rot_err"][0][it][b] == one["all_rot_err"][0][it][b]
                assert res["all_trans_err"][0][it][b] == one["all_trans_err"][0][it][b]
            np.testing.assert_array_equal(rows[b], rows_b[b])
            if b > 0:                                                         # another camera gives pair b other bits
                assert not np.array_equal(np.asarray(res["all_poses_est"][0][1][0]), np.asarray(one["all_poses_est"][0][1][0]))
    finally:
        cfg.dataset.INTRINSIC_MATRIX = K_cfg
        net.K, rm.K = K_cfg.copy(), K_cfg.copy()
    # the evaluation used every pair's own camera: arp_2d differs from the one taken with the config camera alone
    est, gt = res["all_poses_est"], res["all_poses_gt"]
    own, alone = imdb.pose_metrics(cfg, est, gt, res["all_K"])["ape"], imdb.pose_metrics(cfg, est, gt)["ape"]
    np.testing.assert_array_equal(own[:, 0], alone[:, 0])                     # pair 0 has the config camera
    assert (own[:, 1:, 3] != alone[:, 1:, 3]).all()
    np.testing.assert_array_equal(own[:, :, :3], alone[:, :, :3])             # re, te and ADD do not read K
    t_alone = imdb.evaluate_pose_arp_2d(cfg, est, gt)
    assert not np.array_equal(res["tables"]["arp_2d"]["count_correct"]["mean"], t_alone["count_correct"]["mean"])
    # the cache and its sidecar give the same tables back
    again = tester.pred_eval(cfg, None, None, imdb, logger=imdb.logger)
    assert again["from_cache"]
    np.testing.assert_array_equal(np.stack(again["all_K"][0]), np.stack(cams3))
    np.testing.assert_array_equal(again["tables"]["arp_2d"]["count_correct"]["mean"], res["tables"]["arp_2d"]["count_correct"]["mean"])
    # intrinsics in the batch without a K in the records: refused
    f = dict(frames, intrinsics=np.stack(cams3))
    with pytest.raises(ValueError, match="no pair record has a 'K'"):
        tester.pred_eval(cfg, tester.Predictor(cfg, net), [(data_pair.get_data_pair_test_batch(f, cfg), f, recs)], imdb,
                         ignore_cache=True, logger=imdb.logger, render_machine=rm)
