"""The closed loop's shortcut: update_test_batch exports the two mask boxes from its box-fill pass and deepIM_flownet.zoom()
takes them instead of searching both masks again. Everything the front end writes must have the bits of the mask-reading path.
24x32 scene of tests/closed_loop_scene.py (an ordinary object, one over the right and bottom edges, a single rendered pixel
column = empty rectangle, nothing rendered); the network object is bound for the front end only (fc6 fixes the full network's
frame at 480x640, which only the capture test below needs)."""
import ctypes

import numpy as np
import pytest

import closed_loop_scene as cls
from mx_deepim_amd import synthetic
from mx_deepim_amd.config import default_config
from mx_deepim_amd.lib.pair_matching.batch_updater_py_multi import update_test_batch
from mx_deepim_amd.lib.render_glumpy.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
from mx_deepim_amd.runtime import Context, lib
from mx_deepim_amd.symbols import deepIM_flownet

pytestmark = pytest.mark.gpu
H, W, B = cls.H, cls.W, cls.B
INT_MAX = np.iinfo(np.int32).max


def status(ctx):
    st = ctypes.c_int(0)
    lib.deepim_zoom_status(ctx.handle, ctypes.byref(st))
    return st.value


def front_net(ctx, form="nchw", cfg=None):
    """A network object bound for its zoom front end only: the buffers zoom() writes, at the scene's size"""
    net = deepIM_flownet().get_symbol(cfg or default_config())
    net.ctx, net.B, net.H, net.W, net.K, net.pixel_means = ctx, B, H, W, cls.K.astype(np.float32), cls.MEANS.astype(np.float32)
    net.act["net_input"], net.act["zoom_factor"] = ctx.empty((B, net.cin, H, W)), ctx.empty((B, 4))
    if form == "h16":
        net.fp16_conv = net.fp16_fused_input = True
        net.act["net_input_h8"] = ctx.empty((B, H, W, 8), dtype=np.float16)
    return net


def machine(ctx, lit=False):
    if lit:
        return Render_Py_Light_ModelNet_Multi(cls.NAMES, None, cls.K, W, H, meshes=cls.meshes(normals=True), ctx=ctx,
                                              pixel_means=cls.MEANS)
    return Render_Py("unused", cls.NAMES, cls.K, W, H, meshes=dict(zip(cls.NAMES, cls.meshes())), ctx=ctx, pixel_means=cls.MEANS)


def observed(ctx):
    rng = np.random.default_rng(5)
    return ctx.array(rng.uniform(-120, 130, (B, 3, H, W)).astype(np.float32))


def loop_step(ctx, net, rm, poses, ids, seeded, cams=None, light=None, cfg=None, out=None):
    """update_test_batch then zoom(); seeded=False hands the masks over as fresh copies, so the identity check fails.
    -> dict(zoom_factor bits, net input bits, status word, bbox launches, the batch)"""
    status(ctx)
    data = {"image_observed": observed(ctx), "src_pose": ctx.array(poses)}
    if cams is not None:
        data["intrinsics"] = ctx.array(cams)
    new = update_test_batch(cfg or default_config(), data, rm, data["src_pose"], class_index=ids, light_intensity=light, out=out)
    if not seeded:
        new["mask_observed"], new["mask_rendered"] = new["mask_observed"].copy(), new["mask_rendered"].copy()
    n0 = ctx.bbox_launches()
    net.zoom(new)
    launches = ctx.bbox_launches() - n0
    raw = dict.__getitem__(net.act, "net_input_h8" if net.fp16_conv else "net_input").asnumpy()
    return {"zoom_factor": net.act["zoom_factor"].asnumpy().view(np.uint32), "launches": launches, "status": status(ctx),
            "net_input": raw.view(np.uint16 if net.fp16_conv else np.uint32), "batch": new}


def check_equal(a, b):
    assert a["launches"] == 0 and b["launches"] == 1
    np.testing.assert_array_equal(a["zoom_factor"], b["zoom_factor"])
    np.testing.assert_array_equal(a["net_input"], b["net_input"])
    assert a["status"] == b["status"]


def host_ids(ctx):
    return cls.IDS


def device_ids(ctx):
    return ctx.array(cls.IDS, dtype=np.int32)


@pytest.mark.parametrize("form", ["nchw", "h16"])
@pytest.mark.parametrize("ids", [host_ids, device_ids])
def test_seeded_equals_unseeded(ctx, form, ids):
    """host ids: one deepim_render_update_forward per run of equal ids, each exporting its slice of the boxes; device ids: the
    mesh-table draw. Pairs 2 and 3 have an empty observed box (NaN factor, status bit 0), pair 3 also status bit 2."""
    net, rm = front_net(ctx, form), machine(ctx)
    a = loop_step(ctx, net, rm, cls.poses(), ids(ctx), True)
    b = loop_step(ctx, net, rm, cls.poses(), ids(ctx), False)
    check_equal(a, b)
    zf = a["zoom_factor"].view(np.float32)
    assert np.isfinite(zf[:2]).all() and np.isnan(zf[2:]).all()
    assert a["status"] == 1 | 4
    assert a["net_input"].any()


def test_seeded_equals_unseeded_with_a_camera_table(ctx):
    net, rm = front_net(ctx), machine(ctx)
    cams = cls.cameras()
    poses = cls.poses(cams=cams)
    a = loop_step(ctx, net, rm, poses, device_ids(ctx), True, cams=cams)
    b = loop_step(ctx, net, rm, poses, device_ids(ctx), False, cams=cams)
    check_equal(a, b)
    assert np.isfinite(a["zoom_factor"].view(np.float32)[:2]).all()
    ctx.bind_cameras(None)


@pytest.mark.parametrize("ids", [host_ids, device_ids])
def test_seeded_equals_unseeded_through_the_lit_draw(ctx, ids):
    net, rm = front_net(ctx), machine(ctx, lit=True)
    light = ctx.array(np.random.default_rng(3).uniform(0.9, 1.1, (B, 3)).astype(np.float32))
    a = loop_step(ctx, net, rm, cls.poses(), ids(ctx), True, light=light)
    b = loop_step(ctx, net, rm, cls.poses(), ids(ctx), False, light=light)
    check_equal(a, b)
    assert a["status"] == 1 | 4


@pytest.mark.parametrize("ids", [host_ids, device_ids])
def test_exported_boxes_are_those_numpy_finds_on_the_masks(ctx, ids):
    rm = machine(ctx)
    new = update_test_batch(default_config(), {}, rm, ctx.array(cls.poses()), class_index=ids(ctx))
    boxes = new["zoom_boxes"].asnumpy()
    assert boxes.dtype == np.int32 and boxes.shape == (B, 2, 4)
    mo, mr = new["mask_observed"].asnumpy(), new["mask_rendered"].asnumpy()
    want = np.array([[cls.numpy_box(mo[b, 0], 0.3), cls.numpy_box(mr[b, 0], 0.2)] for b in range(B)], np.int64)
    np.testing.assert_array_equal(boxes, want)
    # the scene is what it claims to be
    assert want[0, 0, 1] >= 0 and want[0, 1, 1] < W - 1 and want[0, 1, 3] < H - 1            # inside the frame
    assert want[1, 1, 1] == W - 1 and want[1, 1, 3] == H - 1 and want[1, 0, 1] == W - 2      # over the right and bottom edges
    assert want[2, 1, 0] == want[2, 1, 1] == cls.SLIVER_COL and want[2, 1, 3] > want[2, 1, 2]   # one column: empty rectangle
    assert want[2, 0].tolist() == [INT_MAX, -1, INT_MAX, -1] and not mo[2].any()
    assert want[3].tolist() == [[INT_MAX, -1, INT_MAX, -1]] * 2 and not mr[3].any()          # nothing rendered
    assert new["zoom_boxes"].masks[0] is new["mask_observed"] and new["zoom_boxes"].masks[1] is new["mask_rendered"]
    status(ctx)


def test_boxes_live_in_out_and_follow_its_masks(ctx):
    rm = machine(ctx)
    out = {n: ctx.empty((B, 3 if n == "image_rendered" else 1, H, W))
           for n in ("image_rendered", "depth_rendered", "mask_rendered", "mask_observed")}
    new = update_test_batch(default_config(), {}, rm, ctx.array(cls.poses()), class_index=cls.IDS, out=out)
    assert new["zoom_boxes"] is out["zoom_boxes"] and new["mask_observed"] is out["mask_observed"]
    first = out["zoom_boxes"].asnumpy()
    again = update_test_batch(default_config(), new, rm, ctx.array(cls.poses(shift=3.0)), class_index=cls.IDS, out=out)
    assert again["zoom_boxes"] is out["zoom_boxes"]
    second = out["zoom_boxes"].asnumpy()
    np.testing.assert_array_equal(second[0, 1, :2], first[0, 1, :2] + 3)       # the object moved three pixels to the right
    cfg = default_config()
    cfg.TEST.UPDATE_MASK = "init"
    kept = update_test_batch(cfg, dict(again), rm, ctx.array(cls.poses()), class_index=cls.IDS, out=out)
    assert "zoom_boxes" not in kept                     # the rendered mask was redrawn without its boxes: none are handed on
    status(ctx)


def test_accumulators_stay_armed(ctx):
    """a seeded call, then an unseeded one on other masks on the same context = the unseeded call of a fresh context"""
    net, rm = front_net(ctx), machine(ctx)
    loop_step(ctx, net, rm, cls.poses(), device_ids(ctx), True)
    after = loop_step(ctx, net, rm, cls.poses(shift=3.0), device_ids(ctx), False)
    fresh = Context(0)
    want = loop_step(fresh, front_net(fresh), machine(fresh), cls.poses(shift=3.0), device_ids(fresh), False)
    assert after["launches"] == want["launches"] == 1
    for k in ("zoom_factor", "net_input", "status"):
        np.testing.assert_array_equal(after[k], want[k])
    # and once more unseeded on the first masks: the seeded call's boxes were read, not left in the accumulators
    again = loop_step(ctx, net, rm, cls.poses(), device_ids(ctx), False)
    first = loop_step(fresh, front_net(fresh), machine(fresh), cls.poses(), device_ids(fresh), False)
    for k in ("zoom_factor", "net_input", "status"):
        np.testing.assert_array_equal(again[k], first[k])


def test_guard_takes_the_mask_reading_path(ctx):
    """bbox launches counted on the context: none for the render pass's own masks, one for anything else"""
    rm = machine(ctx)
    net = front_net(ctx)
    assert loop_step(ctx, net, rm, cls.poses(), device_ids(ctx), True)["launches"] == 0
    # pre-staged frames: masks that no render call of this loop wrote, no boxes in the batch
    made = update_test_batch(default_config(), {}, rm, ctx.array(cls.poses()), class_index=cls.IDS)
    staged = {"image_observed": observed(ctx), "image_rendered": made["image_rendered"], "src_pose": made["src_pose"],
              "mask_observed": made["mask_observed"], "mask_rendered": made["mask_rendered"]}
    n0 = ctx.bbox_launches()
    net.zoom(staged)
    assert ctx.bbox_launches() - n0 == 1
    # one mask object replaced, the boxes still in the batch
    for name in ("mask_observed", "mask_rendered"):
        swapped = dict(made, image_observed=staged["image_observed"])
        swapped[name] = made[name].copy()
        n0 = ctx.bbox_launches()
        net.zoom(swapped)
        assert ctx.bbox_launches() - n0 == 1, name
    # UPDATE_MASK == "init": the observed mask is the caller's, the render pass exports nothing
    cfg = default_config()
    cfg.TEST.UPDATE_MASK = "init"
    net_init = front_net(ctx, cfg=cfg)
    new = update_test_batch(cfg, dict(staged), rm, made["src_pose"], class_index=cls.IDS)
    assert "zoom_boxes" not in new and new["mask_observed"] is staged["mask_observed"]
    n0 = ctx.bbox_launches()
    net_init.zoom(new)
    assert ctx.bbox_launches() - n0 == 1
    # a network configured for "init" ignores boxes that a batch still carries
    both = dict(made, image_observed=staged["image_observed"])
    n0 = ctx.bbox_launches()
    net_init.zoom(both)
    assert ctx.bbox_launches() - n0 == 1
    status(ctx)


def test_one_shot_requests_do_not_outlive_a_failed_call(ctx):
    rm, net = machine(ctx), front_net(ctx)
    boxes = ctx.empty((B, 2, 4), dtype=np.int32)
    img, dep = ctx.empty((B, 3, H, W)), ctx.empty((B, 1, H, W))
    poses = ctx.array(cls.poses())
    lib.deepim_render_export_boxes(ctx.handle, boxes)
    with pytest.raises(RuntimeError):                     # an entry that draws no mask_box refuses, and clears the request
        rm.render_into(img, dep, 0, poses)
    rm.render_into(img, dep, 0, poses)
    made = update_test_batch(default_config(), {"image_observed": observed(ctx)}, rm, poses, class_index=cls.IDS)
    lib.deepim_zoom_seed_boxes(ctx.handle, made["zoom_boxes"])
    with pytest.raises(RuntimeError):                     # any refusal after the seed is taken will do: here W % 4 != 0 for NC8
        lib.deepim_zoom_concat_forward_nc8(ctx.handle, made["image_observed"], made["image_rendered"], made["mask_observed"],
                                           made["mask_rendered"], made["src_pose"], net.K, net.pixel_means,
                                           net.act["net_input"], net.act["zoom_factor"], B, H, W - 1)
    swapped = dict(made, mask_observed=made["mask_observed"].copy())
    n0 = ctx.bbox_launches()
    net.zoom(swapped)                                     # no stale seed: this call searches its masks
    assert ctx.bbox_launches() - n0 == 1
    status(ctx)


def test_bbox_pass_by_quads_equals_the_row_sweep(ctx):
    """the mask-reading path itself: 16-byte loads over whole rows (aligned masks, W % 4 == 0) against the row-by-row sweep, which
    a mask 4 bytes off alignment takes. Sparse masks with values on both sides of the two thresholds (0.3 observed, 0.2 rendered),
    so every position inside a quad is somewhere the first or the last pixel of a box; 24 rows = three blocks."""
    from mx_deepim_amd.runtime import DeviceArray
    rng = np.random.default_rng(17)
    net = front_net(ctx)
    n = B * H * W
    for trial in range(4):
        host = []
        for _ in range(2):
            m = np.zeros((B, 1, H, W), np.float32)
            for b in range(B):
                k = int(rng.integers(1, 4))
                m[b, 0, rng.integers(0, H, k), rng.integers(0, W, k)] = rng.choice([0.25, 0.35, 1.0], k)
                m[b, 0, rng.integers(0, H, 3), rng.integers(0, W, 3)] = 0.15
            host.append(m)
        image = observed(ctx)
        pose = ctx.array(cls.poses())
        got = []
        for offset in (0, 1):
            masks = []
            for m in host:
                whole = ctx.zeros((n + 4,))
                view = DeviceArray(ctx, (B, 1, H, W), np.float32, ptr=whole.ptr + 4 * offset, base=whole)
                view.copyfrom(m)
                masks.append(view)
            data = {"image_observed": image, "image_rendered": image, "mask_observed": masks[0], "mask_rendered": masks[1],
                    "src_pose": pose}
            n0 = ctx.bbox_launches()
            net.zoom(data)
            assert ctx.bbox_launches() - n0 == 1
            got.append((net.act["zoom_factor"].asnumpy().view(np.uint32), dict.__getitem__(net.act, "net_input").asnumpy().view(np.uint32)))
        np.testing.assert_array_equal(got[0][0], got[1][0])
        np.testing.assert_array_equal(got[0][1], got[1][1])
    status(ctx)


def test_capture_and_replay_one_iteration(ctx, small_batch):
    """render update → zoom → pose tail recorded into one graph and replayed on other device-resident poses: the eager results.
    At 480x640, B = 2: the pose tail needs the bound network. conv6_1 holds fixed values (no encoder run: not what is tested)."""
    HH, WW, BB = 480, 640, 2
    cfg = default_config()
    net = deepIM_flownet().get_symbol(cfg)
    params = net.init_weights(cfg, seed=20)
    params["trans_weight"] = params["trans_weight"] * np.float32(0.02)
    params["trans_bias"] = params["trans_bias"] * np.float32(0.02)
    net.bind(ctx, BB, params)
    net.act["conv6_1"].copyfrom(np.random.default_rng(8).standard_normal(net.act["conv6_1"].shape).astype(np.float32) * 0.1)
    mesh = synthetic.ellipsoid_mesh(np.array([0.05, 0.04, 0.035]), 12, 24)
    mesh.pop("uv")
    means = synthetic.PIXEL_MEANS[::-1].copy()
    rm = Render_Py("unused", ["obj"], cfg.dataset.INTRINSIC_MATRIX, WW, HH, meshes={"obj": mesh}, ctx=ctx, pixel_means=means)
    names = ("image_rendered", "depth_rendered", "mask_rendered", "mask_observed")
    rbuf = {n: ctx.empty((BB, 3 if n == "image_rendered" else 1, HH, WW)) for n in names}
    image_observed = ctx.array(small_batch["image_observed"])
    pose_in, pose_out = ctx.empty((BB, 3, 4)), ctx.empty((BB, 3, 4))
    ids = ctx.array(np.zeros(BB, np.int32), dtype=np.int32)
    launches = []

    def iteration():
        n0 = ctx.bbox_launches()
        data = update_test_batch(cfg, {"image_observed": image_observed}, rm, pose_in, class_index=ids, out=rbuf)
        net.zoom(data)
        net.pose_head_update(pose_in, pose_out)
        launches.append(ctx.bbox_launches() - n0)

    def results():
        return [a.asnumpy().view(np.uint32) for a in (pose_out, net.act["se3"], net.act["zoom_factor"],
                                                      dict.__getitem__(net.act, "net_input"), rbuf["mask_observed"])]

    p0, p1 = small_batch["pose_tgt"].astype(np.float32), small_batch["src_pose"][0].astype(np.float32)
    pose_in.copyfrom(p1)
    iteration()
    want = results()
    pose_in.copyfrom(p0)
    iteration()
    first = results()
    assert not np.array_equal(first[0], want[0]) and not np.array_equal(first[2], want[2])
    ctx.sync()
    gid = ctypes.c_int(-1)
    lib.deepim_graph_begin(ctx.handle)
    try:
        iteration()
    finally:
        lib.deepim_graph_end(ctx.handle, ctypes.byref(gid))
    assert launches == [0, 0, 0]
    pose_in.copyfrom(p1)
    lib.deepim_graph_launch(ctx.handle, gid.value)
    for got, w in zip(results(), want):
        np.testing.assert_array_equal(got, w)
    pose_in.copyfrom(p0)
    lib.deepim_graph_launch(ctx.handle, gid.value)
    for got, w in zip(results(), first):
        np.testing.assert_array_equal(got, w)
    assert status(ctx) == 0
