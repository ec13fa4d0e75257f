"""Mixed-class batches in one launch group from device-resident class ids: `deepim_render_classes_forward` and its Python
surface (`Render_Py.render_batch` / `render_classes_into`, `update_test_batch`, `batchUpdaterPyMulti.forward`) against the
per-class entries (bit for bit: same arithmetic, order-independent visibility) and against oracle/render.py.
Quarter-size frames (120 x 160, K scaled by 0.25) and the four-class table of tests/render_classes_table.py."""
import ctypes

import numpy as np
import pytest

from oracle import flow as oflow
from oracle import render as orender
from mx_deepim_amd.config import default_config
from mx_deepim_amd.runtime import DeviceArray, lib
from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import batchUpdaterPyMulti, update_test_batch
from mx_deepim_amd.lib.render_glumpy.render_py_light_modelnet_multi import LIGHT_OFFSET, Render_Py_Light_ModelNet_Multi
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py, pack_mesh_table

import render_classes_table as rct

pytestmark = pytest.mark.gpu
cf = ctypes.c_float
H, W, K, MEANS = rct.H, rct.W, rct.K, rct.MEANS
ZN, ZF = 0.25, 6.0
IDS = np.array([2, 0, 0, 3, 1, 3, 2], np.int32)


class _Dev(object):
    """The four meshes on the device, one by one (for the per-class entries) and as the packed table."""

    def __init__(self, ctx, lit=False):
        self.meshes = rct.meshes(normals=lit)
        self.one = []
        for m in self.meshes:
            tex = m.get("texture")
            self.one.append(dict(vertices=ctx.array(m["vertices"]), attr=ctx.array(rct.attr(m)),
                                 faces=ctx.array(m["faces"], dtype=np.int32), texture=None if tex is None else ctx.array(tex),
                                 th=0 if tex is None else tex.shape[0], tw=0 if tex is None else tex.shape[1],
                                 normals=ctx.array(m["normals"]) if lit else None, V=len(m["vertices"]), F=len(m["faces"])))
        t = pack_mesh_table(self.meshes, with_normals=lit)
        self.n, self.max_V, self.max_F = len(t["mesh_desc"]), t["max_V"], t["max_F"]
        self.vertices, self.vertex_attr = ctx.array(t["vertices"]), ctx.array(t["vertex_attr"])
        self.normals = ctx.array(t["normals"]) if lit else None
        self.faces, self.textures = ctx.array(t["faces"], dtype=np.int32), ctx.array(t["textures"])
        self.desc = ctx.array(t["mesh_desc"], dtype=np.int32)


@pytest.fixture(scope="module")
def dev(ctx):
    return _Dev(ctx)


def _bufs(ctx, B):
    return ctx.empty((B, 3, H, W)), ctx.empty((B, 1, H, W)), ctx.empty((B, 1, H, W)), ctx.empty((B, 1, H, W))


def _classes(ctx, d, ids_dev, poses_dev, bufs, mask=True, box=True, light_offset=None, inten=None, ratio=0.0):
    img, dep, mr, mb = bufs
    lib.deepim_render_classes_forward(ctx.handle, img, dep, mr if mask else None, mb if box else None, cf(0.2), ids_dev, d.desc,
                                      d.n, d.max_V, d.max_F, d.vertices, d.vertex_attr, d.normals, d.faces, d.textures,
                                      poses_dev, K, MEANS, light_offset, inten, cf(ratio), poses_dev.shape[0], H, W, cf(ZN), cf(ZF))


def _per_run(ctx, d, ids, poses_dev, mask=True, box=True):
    """Today's path: one launch group of a single-mesh entry per run of equal ids."""
    B = len(ids)
    img, dep, mr, mb = _bufs(ctx, B)
    b0 = 0
    while b0 < B:
        b1 = b0 + 1
        while b1 < B and ids[b1] == ids[b0]:
            b1 += 1
        m = d.one[ids[b0]]
        tail = (m["vertices"], m["attr"], m["faces"], m["texture"], m["th"], m["tw"], poses_dev[b0:b1], K, MEANS, m["V"], m["F"],
                b1 - b0, H, W, cf(ZN), cf(ZF))
        if mask:
            lib.deepim_render_update_forward(ctx.handle, img[b0:b1], dep[b0:b1], mr[b0:b1], mb[b0:b1] if box else None, cf(0.2), *tail)
        else:
            lib.deepim_render_forward(ctx.handle, img[b0:b1], dep[b0:b1], *tail)
        b0 = b1
    return [a.asnumpy() for a in ((img, dep, mr, mb) if mask else (img, dep))]


@pytest.fixture(scope="module")
def mixed(ctx, dev):
    """The B = 7 mixed batch drawn by the per-class entries, computed once and left unchanged."""
    poses = rct.poses(len(IDS), seed=21)
    return poses, _per_run(ctx, dev, IDS, ctx.array(poses))


def _clear_status(ctx):
    st = ctypes.c_int(-1)
    lib.deepim_zoom_status(ctx.handle, ctypes.byref(st))
    return st.value


def test_same_bits_as_the_per_class_entries(ctx, dev, mixed):
    poses, want = mixed
    bufs = _bufs(ctx, len(IDS))
    pd, idd = ctx.array(poses), ctx.array(IDS, dtype=np.int32)
    _clear_status(ctx)                                                       # the status word is sticky across tests
    _classes(ctx, dev, idd, pd, bufs)
    for got, ref in zip(bufs, want):
        np.testing.assert_array_equal(got.asnumpy(), ref)
    assert all((want[2][b] > 0).sum() > 200 for b in range(len(IDS)))      # nothing passes on empty frames
    assert _clear_status(ctx) == 0
    # without mask and rectangle: the plain draw
    bufs2 = _bufs(ctx, len(IDS))
    _classes(ctx, dev, idd, pd, bufs2, mask=False, box=False)
    img, dep = _per_run(ctx, dev, IDS, pd, mask=False)
    np.testing.assert_array_equal(bufs2[0].asnumpy(), img)
    np.testing.assert_array_equal(bufs2[1].asnumpy(), dep)
    np.testing.assert_array_equal(img, want[0])
    # mask without rectangle
    bufs3 = _bufs(ctx, len(IDS))
    _classes(ctx, dev, idd, pd, bufs3, box=False)
    np.testing.assert_array_equal(bufs3[2].asnumpy(), want[2])


def test_against_the_oracle(ctx, dev):
    ids = np.array([3, 1, 2, 0], np.int32)                                  # one sample of each class, out of order
    poses = rct.poses(4, seed=33)
    bufs = _bufs(ctx, 4)
    _classes(ctx, dev, ctx.array(ids, dtype=np.int32), ctx.array(poses), bufs)
    img, dep, mr, mb = (a.asnumpy() for a in bufs)
    for b in range(4):
        m = dev.meshes[ids[b]]
        ri, rd = orender.render(m["vertices"], rct.attr(m), m["faces"], poses[b], K, H, W, texture=m.get("texture"), pixel_means=MEANS)
        np.testing.assert_array_equal(dep[b, 0], rd)                        # same fp32 expression order
        np.testing.assert_allclose(img[b], ri, rtol=0, atol=1e-3)           # 0..255 scale
        np.testing.assert_array_equal(mr[b, 0], (rd > 0.2).astype(np.float32))
        np.testing.assert_array_equal(mb[b, 0], oflow.mask_box(mr[b, 0]))
        assert 200 < mr[b].sum() < H * W / 2


def test_out_of_range_ids_give_empty_frames(ctx, dev, mixed):
    poses, want = mixed
    ids = IDS.copy()
    ids[2], ids[4] = -1, dev.n                                               # both sides of [0, n_classes), mid-batch
    bufs = _bufs(ctx, len(ids))
    for a in bufs:
        a.copyfrom(np.float32(7.0))                                         # every output element has to be written
    _clear_status(ctx)
    _classes(ctx, dev, ctx.array(ids, dtype=np.int32), ctx.array(poses), bufs)
    img, dep, mr, mb = (a.asnumpy() for a in bufs)
    for b in (2, 4):
        np.testing.assert_array_equal(img[b], np.broadcast_to(-MEANS[:, None, None], (3, H, W)))
        assert not dep[b].any() and not mr[b].any() and not mb[b].any()
    assert _clear_status(ctx) == 4                                          # what an empty mask gives today: status bit 2
    keep = [0, 1, 3, 5, 6]
    for got, ref in zip((img, dep, mr, mb), want):
        np.testing.assert_array_equal(got[keep], ref[keep])
    # the z-buffer was left all-ones: an ordinary draw on the same context is correct
    again = _per_run(ctx, dev, IDS, ctx.array(poses))
    for got, ref in zip(again, want):
        np.testing.assert_array_equal(got, ref)
    assert _clear_status(ctx) == 0


def test_capture_and_replay_with_other_ids(ctx, dev, mixed):
    poses, want = mixed
    B = len(IDS)
    ids2 = np.array([1, 3, 2, 2, 0, 1, 0], np.int32)
    poses2 = rct.poses(B, seed=45)
    idd, pd, bufs = ctx.array(IDS, dtype=np.int32), ctx.array(poses), _bufs(ctx, B)
    _classes(ctx, dev, idd, pd, bufs)                                       # eagerly first: scratch and z-buffer are sized
    np.testing.assert_array_equal(bufs[0].asnumpy(), want[0])
    gid = ctypes.c_int(-1)
    lib.deepim_graph_begin(ctx.handle)
    try:
        _classes(ctx, dev, idd, pd, bufs)
    finally:
        lib.deepim_graph_end(ctx.handle, ctypes.byref(gid))
    idd.copyfrom(ids2)                                                       # in place: the graph holds these addresses
    pd.copyfrom(poses2)
    for a in bufs:
        a.copyfrom(np.float32(7.0))
    lib.deepim_graph_launch(ctx.handle, gid.value)
    got = [a.asnumpy() for a in bufs]
    eager = _bufs(ctx, B)
    _classes(ctx, dev, ctx.array(ids2, dtype=np.int32), ctx.array(poses2), eager)
    for g, e in zip(got, eager):
        np.testing.assert_array_equal(g, e.asnumpy())
    assert not np.array_equal(got[1], want[1])                              # it is the second batch
    per_run = _per_run(ctx, dev, ids2, ctx.array(poses2))
    for g, r in zip(got, per_run):
        np.testing.assert_array_equal(g, r)


def test_lit_machine_matches_per_class_lit_draws(ctx):
    d = _Dev(ctx, lit=True)
    B = len(IDS)
    poses = rct.poses(B, seed=57)
    inten = np.random.default_rng(3).uniform(0.9, 1.1, (B, 3)).astype(np.float32)
    pd, it = ctx.array(poses), ctx.array(inten)
    bufs = _bufs(ctx, B)
    _classes(ctx, d, ctx.array(IDS, dtype=np.int32), pd, bufs, light_offset=LIGHT_OFFSET, inten=it, ratio=0.7)
    img, dep, mr, mb = _bufs(ctx, B)
    for b in range(B):                                                      # one launch group per sample
        m = d.one[IDS[b]]
        lib.deepim_render_lit_forward(ctx.handle, img[b:b + 1], dep[b:b + 1], mr[b:b + 1], mb[b:b + 1], cf(0.2), m["vertices"],
                                      m["attr"], m["normals"], m["faces"], m["texture"], m["th"], m["tw"], pd[b:b + 1], K, MEANS,
                                      LIGHT_OFFSET, it[b:b + 1], cf(0.7), m["V"], m["F"], 1, H, W, cf(ZN), cf(ZF))
    for got, ref in zip(bufs, (img, dep, mr, mb)):
        np.testing.assert_array_equal(got.asnumpy(), ref.asnumpy())
    assert all(mr.asnumpy()[b].sum() > 200 for b in range(B))
    # the shading is there: not the unlit draw
    unlit = _bufs(ctx, B)
    lib.deepim_render_classes_forward(ctx.handle, unlit[0], unlit[1], None, None, cf(0.2), ctx.array(IDS, dtype=np.int32), d.desc, d.n,
                                      d.max_V, d.max_F, d.vertices, d.vertex_attr, None, d.faces, d.textures, pd, K, MEANS, None,
                                      None, cf(0.0), B, H, W, cf(ZN), cf(ZF))
    np.testing.assert_array_equal(unlit[1].asnumpy(), dep.asnumpy())
    assert not np.array_equal(unlit[0].asnumpy(), img.asnumpy())
    # the lit render machine: device ids == host ids
    rm = Render_Py_Light_ModelNet_Multi(rct.NAMES, None, K, W, H, ZN, ZF, brightness_ratios=[0.7], meshes=d.meshes, ctx=ctx,
                                        pixel_means=MEANS)
    a = rm.render_batch(IDS, pd, light_intensity=it)
    b_ = rm.render_batch(ctx.array(IDS, dtype=np.int32), pd, light_intensity=it)
    np.testing.assert_array_equal(b_[0].asnumpy(), a[0].asnumpy())
    np.testing.assert_array_equal(b_[0].asnumpy(), img.asnumpy())
    np.testing.assert_array_equal(b_[1].asnumpy(), dep.asnumpy())


def _machine(ctx, dev):
    return Render_Py("unused", rct.NAMES, K, W, H, ZN, ZF, meshes=dict(zip(rct.NAMES, dev.meshes)), ctx=ctx, pixel_means=MEANS)


def test_render_batch_takes_device_ids_without_a_read_back(ctx, dev, mixed, monkeypatch):
    poses, want = mixed
    rm = _machine(ctx, dev)
    pd = ctx.array(poses)
    img_h, dep_h = rm.render_batch(IDS, pd)
    np.testing.assert_array_equal(img_h.asnumpy(), want[0])
    idd = ctx.array(IDS, dtype=np.int32)
    out = (ctx.empty((len(IDS), 3, H, W)), ctx.empty((len(IDS), 1, H, W)))
    mr = ctx.empty((len(IDS), 1, H, W))
    rm.mesh_table()                                                          # built lazily once, outside the guarded call
    with monkeypatch.context() as mp:
        def boom(self):
            raise AssertionError("read-back of a device array inside render_batch")
        mp.setattr(DeviceArray, "asnumpy", boom)
        got = rm.render_batch(idd, pd, out=out, mask_rendered=mr, mask_thresh=0.2)
    assert got[0] is out[0] and got[1] is out[1]
    np.testing.assert_array_equal(out[0].asnumpy(), img_h.asnumpy())
    np.testing.assert_array_equal(out[1].asnumpy(), dep_h.asnumpy())
    np.testing.assert_array_equal(mr.asnumpy(), want[2])
    assert rm.mesh_table() is rm.mesh_table()
    # other device dtypes keep today's behaviour (read back, split into runs)
    img_f, _ = rm.render_batch(ctx.array(IDS.astype(np.float32)), pd)
    np.testing.assert_array_equal(img_f.asnumpy(), img_h.asnumpy())
    # the explicit method insists on device int32 ids
    with pytest.raises(TypeError):
        rm.render_classes_into(out[0], out[1], IDS, pd)


def test_updaters_agree_for_host_and_device_ids(ctx, dev, monkeypatch):
    rm = _machine(ctx, dev)
    cfg = default_config()
    cfg.dataset.INTRINSIC_MATRIX = K
    B = 4
    ids = np.array([3, 3, 1, 0], np.int32)
    idd = ctx.array(ids, dtype=np.int32)
    poses = rct.poses(B, seed=69)
    pd = ctx.array(poses)
    # test loop: one fused pass (draw + mask + rectangle)
    names = ("image_rendered", "depth_rendered", "mask_rendered", "mask_observed")
    out_h = {n: ctx.empty((B, 3 if n == "image_rendered" else 1, H, W)) for n in names}
    out_d = {n: ctx.empty((B, 3 if n == "image_rendered" else 1, H, W)) for n in names}
    new_h = update_test_batch(cfg, {}, rm, pd, class_index=ids, out=out_h)
    with monkeypatch.context() as mp:
        def boom(self):
            raise AssertionError("read-back of a device array inside update_test_batch")
        mp.setattr(DeviceArray, "asnumpy", boom)
        new_d = update_test_batch(cfg, {}, rm, pd, class_index=idd, out=out_d)
    assert new_d["mask_observed"] is out_d["mask_observed"] and new_d["src_pose"] is pd
    for n in names:
        np.testing.assert_array_equal(out_d[n].asnumpy(), out_h[n].asnumpy())
    assert all(out_h["mask_rendered"].asnumpy()[b].sum() > 200 for b in range(B))
    assert sorted(new_d) == sorted(new_h)
    # training loop's updater, with fresh allocations and with its workspace (fused mask)
    upd = batchUpdaterPyMulti(cfg, H, W, render_machine=rm)
    rng = np.random.default_rng(4)
    se3 = np.concatenate([[[1, 0.02, -0.01, 0.03]] * B, rng.standard_normal((B, 3)) * 0.05], 1).astype(np.float32)
    depth_obs = out_h["depth_rendered"].asnumpy()          # the observed frame = the objects at `poses`, which is the target pose
    keys = ("image_rendered", "depth_rendered", "mask_rendered", "flow", "flow_weights", "src_pose")
    for use_ws in (False, True):
        res = []
        for ci in (ids, idd):
            batch = {"src_pose": ctx.array(poses), "tgt_pose": ctx.array(poses), "depth_gt_observed": ctx.array(depth_obs),
                     "class_index": ci}
            new = upd.forward(batch, {"se3": ctx.array(se3)}, out=upd.workspace(ctx, B) if use_ws else None)
            assert new["class_index"] is ci
            res.append({k: new[k].asnumpy() for k in keys})
        for k in keys:
            np.testing.assert_array_equal(res[1][k], res[0][k])
        assert res[0]["flow_weights"].any() and res[0]["mask_rendered"].any()


def test_host_checks_of_the_entry(ctx, dev):
    B = 2
    bufs = _bufs(ctx, B)
    idd, pd = ctx.array(IDS[:B], dtype=np.int32), ctx.array(rct.poses(B, seed=81))
    with pytest.raises(RuntimeError):                                       # rectangle without its mask
        _classes(ctx, dev, idd, pd, bufs, mask=False, box=True)
    with pytest.raises(RuntimeError):                                       # lit without normals
        _classes(ctx, dev, idd, pd, bufs, light_offset=LIGHT_OFFSET, ratio=0.7)
    args = [ctx.handle, bufs[0], bufs[1], None, None, cf(0.2), idd, dev.desc, dev.n, 0, dev.max_F, dev.vertices, dev.vertex_attr, None,
            dev.faces, dev.textures, pd, K, MEANS, None, None, cf(0.0), B, H, W, cf(ZN), cf(ZF)]
    with pytest.raises(RuntimeError):                                       # max_V = 0
        lib.deepim_render_classes_forward(*args)
    args[9], args[10] = dev.max_V, 0
    with pytest.raises(RuntimeError):                                       # max_F = 0
        lib.deepim_render_classes_forward(*args)
    # none of them launched anything: the next draw is an ordinary one, and B = 0 is a no-op
    args[10] = dev.max_F
    lib.deepim_render_classes_forward(*args)
    assert (bufs[1].asnumpy() > 0).sum() > 400
    args[22] = 0
    lib.deepim_render_classes_forward(*args)
