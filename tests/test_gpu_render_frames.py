"""deepim_render_frames_forward and deepim_mask_gate on the GPU. Two small meshes — a textured ellipsoid and a vertex-coloured one
whose colours leave 0..255 on both sides, so the clamp is exercised — at 24x32 (768 pixels: the four-pixels-per-lane dword path)
and 15x21 (315 pixels, not a multiple of 4: the single-pixel path with a partial last block), B = 4. The reference of every byte
is the numpy quantisation of what the parent's deepim_render_classes_forward (unlit, pixel_means NULL) returns: exact."""
import ctypes

import numpy as np
import pytest

from mx_deepim_amd import synthetic
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
from mx_deepim_amd.runtime import lib

pytestmark = pytest.mark.gpu
ZN, ZF = 0.25, 6.0
SIZES = [(24, 32), (15, 21)]
cf = ctypes.c_float
CLS = np.array([0, 1, 1, 0], np.int32)


def _K(h, w, f=None):
    f = 2.6 * h if f is None else f
    return np.array([[f, 0, w / 2.0], [0, f * 1.01, h / 2.0], [0, 0, 1]], np.float32)


def _meshes():
    tex = synthetic.ellipsoid_mesh([0.05, 0.04, 0.035], 8, 16)
    tex.pop("colors")
    tex["texture"] = synthetic.procedural_texture(32, 64)
    col = synthetic.ellipsoid_mesh([0.03, 0.06, 0.04], 8, 16)
    col.pop("uv")
    col["colors"] = (col["colors"] * np.float32(1.5) - np.float32(60.0)).astype(np.float32)     # about -60 .. 322
    return {"tex": tex, "col": col}


_MACHINES = {}


def _machine(ctx, h, w):
    if (h, w) not in _MACHINES:
        _MACHINES[(h, w)] = Render_Py("unused", ["tex", "col"], _K(h, w), w, h, ZN, ZF, meshes=_meshes(), ctx=ctx)
    return _MACHINES[(h, w)]


def _poses(n=4, seed=3):
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        poses[i, :, :3] = synthetic.random_rotation(rng)
        poses[i, :, 3] = [rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.36, 0.42)]
    return poses


def _frames(ctx, rm, cls, poses, K=None, rows=None, N=None, label=True, label_value=None, covered=True, fill=None, depth_factor=1000.0):
    """Render_Py.render_frames_into → {"image", "depth", "label", "covered"} on the host (None where not asked for)."""
    B, h, w = len(cls), rm.height, rm.width
    N = B if N is None else N
    out = {"image": ctx.empty((N, h, w, 3), np.uint8), "depth": ctx.empty((N, h, w), np.uint16),
           "label": ctx.empty((N, h, w), np.uint8) if label else None}
    if fill is not None:
        for a in out.values():
            if a is not None:
                lib.deepim_memset(ctx.handle, a, fill, a.nbytes)
    out["covered"] = ctx.array(np.full(B, 12345, np.int32), dtype=np.int32) if covered else None      # the call overwrites it
    rm.render_frames_into(out["image"], out["depth"], ctx.array(cls, dtype=np.int32), ctx.array(poses), K=K,
                          rows=None if rows is None else ctx.array(rows, dtype=np.int32), label=out["label"],
                          label_value=None if label_value is None else ctx.array(label_value, dtype=np.int32),
                          covered=out["covered"], depth_factor=depth_factor)
    return {k: None if v is None else v.asnumpy() for k, v in out.items()}


def _float_draw(ctx, rm, cls, poses, K=None):
    """The parent's entry: deepim_render_classes_forward, unlit, pixel_means NULL → (levels (B,3,h,w) RGB, depth (B,h,w)) float32."""
    B, h, w = len(cls), rm.height, rm.width
    image, depth = ctx.empty((B, 3, h, w)), ctx.empty((B, 1, h, w))
    t = rm.mesh_table()
    lib.deepim_render_classes_forward(ctx.handle, image, depth, None, None, cf(0.0), ctx.array(cls, dtype=np.int32), t.mesh_desc,
                                      t.n_classes, t.max_V, t.max_F, t.vertices, t.vertex_attr, None, t.faces, t.textures,
                                      ctx.array(poses), rm.K if K is None else np.ascontiguousarray(K, np.float32), None, None, None,
                                      cf(0.0), B, h, w, cf(ZN), cf(ZF))
    return image.asnumpy(), depth.asnumpy()[:, 0]


def _quantise(levels, depth, factor=1000.0):
    """cv2.imwrite of the float BGR image (saturate, round to nearest even) and (depth * factor).astype(uint16) of
    toolkit/LM6d_3_gen_PoseCNN_pred_rendered.py:149-155"""
    image = np.ascontiguousarray(np.rint(np.clip(levels, 0, 255)).astype(np.uint8)[:, ::-1].transpose(0, 2, 3, 1))
    prod = depth * np.float32(factor)
    assert prod.dtype == np.float32
    return image, (prod.astype(np.int32) & 0xffff).astype(np.uint16)


@pytest.mark.parametrize("h,w", SIZES)
def test_bytes_equal_the_quantised_float_draw(ctx, h, w):
    rm = _machine(ctx, h, w)
    poses = _poses()
    label_value = np.array([1, 2, 200, 255], np.int32)
    got = _frames(ctx, rm, CLS, poses, label_value=label_value)
    levels, depth = _float_draw(ctx, rm, CLS, poses)
    image, depth16 = _quantise(levels, depth)
    np.testing.assert_array_equal(got["image"], image)
    np.testing.assert_array_equal(got["depth"], depth16)
    np.testing.assert_array_equal(got["label"], ((depth16 != 0) * label_value[:, None, None]).astype(np.uint8))
    np.testing.assert_array_equal(got["covered"], np.count_nonzero(depth16.reshape(4, -1), axis=1))
    # the inputs reach every branch of the quantisation: each sample is drawn, levels fall between whole numbers on both sides of
    # one half (a truncating or a flooring store fails), below 0 and above 255 (an unclamped store fails), and the depth
    # product is not whole (a rounding store fails)
    hit = np.repeat((depth != 0)[:, None], 3, 1)
    frac = levels[hit] - np.floor(levels[hit])
    assert (got["covered"] > 20).all()
    assert (frac > 0.5).any() and ((frac > 0) & (frac < 0.5)).any()
    assert (levels[hit] < -0.5).any() and (levels[hit] > 255.5).any()
    prod = depth * np.float32(1000)
    assert np.count_nonzero(np.rint(prod) != np.floor(prod)) > 0
    # a second call gives the same bytes: the z-buffer was left clean and covered is written, not accumulated
    again = _frames(ctx, rm, CLS, poses, label_value=label_value)
    for k in got:
        np.testing.assert_array_equal(again[k], got[k], err_msg=k)
    # label and covered are optional; NULL label_value = 1; another depth factor
    bare = _frames(ctx, rm, CLS, poses, label=False, covered=False)
    np.testing.assert_array_equal(bare["image"], image)
    np.testing.assert_array_equal(bare["depth"], depth16)
    ones = _frames(ctx, rm, CLS, poses, depth_factor=2500.0)
    np.testing.assert_array_equal(ones["label"], (depth16 != 0).astype(np.uint8))
    np.testing.assert_array_equal(ones["depth"], _quantise(levels, depth, 2500.0)[1])
    np.testing.assert_array_equal(ones["covered"], got["covered"])


@pytest.mark.parametrize("h,w", SIZES)
def test_bad_class_id_and_pose_behind_the_camera_give_empty_rows(ctx, h, w):
    rm = _machine(ctx, h, w)
    poses = _poses()
    whole = _frames(ctx, rm, CLS, poses)
    cls = CLS.copy()
    cls[1], cls[3] = 2, -1                       # outside the table on both sides
    poses2 = poses.copy()
    poses2[2] = -1.0                             # the detector's "nothing found" sentinel: every vertex behind the camera
    got = _frames(ctx, rm, cls, poses2, fill=0xAB)
    for b in (1, 2, 3):
        assert not got["image"][b].any() and not got["depth"][b].any() and not got["label"][b].any()
    np.testing.assert_array_equal(got["covered"], [np.count_nonzero(whole["depth"][0]), 0, 0, 0])
    assert got["covered"][0] > 20
    for k in ("image", "depth", "label"):
        np.testing.assert_array_equal(got[k][0], whole[k][0])


@pytest.mark.parametrize("h,w", SIZES)
def test_destination_rows(ctx, h, w):
    rm = _machine(ctx, h, w)
    poses = _poses()
    ident = _frames(ctx, rm, CLS, poses)
    rows = np.array([7, 0, 3, 5], np.int32)
    got = _frames(ctx, rm, CLS, poses, rows=rows, N=9, fill=0xAB)
    others = [r for r in range(9) if r not in rows.tolist()]
    for k in ("image", "depth", "label"):
        np.testing.assert_array_equal(got[k][rows], ident[k], err_msg=k)
        assert (got[k][others].view(np.uint8) == 0xAB).all()
    np.testing.assert_array_equal(got["covered"], ident["covered"])             # per sample, not per row
    # a row outside [0, N) is not written, its pixels are still counted and the z-buffer is still put back
    off = rows.copy()
    off[1] = 9
    got = _frames(ctx, rm, CLS, poses, rows=off, N=9, fill=0xAB)
    assert (got["image"][[0, 8]] == 0xAB).all() and (got["depth"][[0, 8]].view(np.uint8) == 0xAB).all()
    np.testing.assert_array_equal(got["covered"], ident["covered"])
    again = _frames(ctx, rm, CLS, poses)
    for k in ident:
        np.testing.assert_array_equal(again[k], ident[k], err_msg=k)
    with pytest.raises(RuntimeError, match="N >= B"):
        _frames(ctx, rm, CLS, poses, N=3)


@pytest.mark.parametrize("h,w", SIZES)
def test_per_sample_cameras_from_a_bound_table(ctx, h, w):
    rm = _machine(ctx, h, w)
    poses = _poses()
    table = np.stack([_K(h, w, f) for f in (2.6 * h, 2.2 * h, 3.0 * h, 2.4 * h)])
    table[1, 0, 2] += 1.5
    table[2, 1, 2] -= 2.25
    got = _frames(ctx, rm, CLS, poses, K=ctx.array(table))
    for b in range(4):
        one = _frames(ctx, rm, CLS, poses, K=table[b])
        for k in got:
            np.testing.assert_array_equal(got[k][b], one[k][b], err_msg="%s %d" % (k, b))
    assert len({got["image"][b].tobytes() for b in range(4)}) == 4 and (got["covered"] > 8).all()
    assert not np.array_equal(got["depth"][1], _frames(ctx, rm, CLS, poses)["depth"][1])      # the table, not the machine's K


def test_depth_range_beyond_uint16_is_a_host_error(ctx):
    rm = _machine(ctx, 24, 32)
    with pytest.raises(RuntimeError, match="65536"):
        _frames(ctx, rm, CLS, _poses(), depth_factor=11000.0)                                  # 6 x 11000 = 66000
    assert _frames(ctx, rm, CLS, _poses(), depth_factor=10000.0)["depth"].any()              # 60000 < 65536: served
    with pytest.raises(TypeError, match="device int32"):
        rm.render_frames_into(ctx.empty((4, 24, 32, 3), np.uint8), ctx.empty((4, 24, 32), np.uint16), CLS, ctx.array(_poses()))
    with pytest.raises(TypeError, match="uint16"):
        rm.render_frames_into(ctx.empty((4, 24, 32, 3), np.uint8), ctx.empty((4, 24, 32), np.float32),
                              ctx.array(CLS, dtype=np.int32), ctx.array(_poses()))


def test_the_draw_and_the_gate_replay_from_a_captured_graph(ctx):
    """After one eager call the buffers have grown: the launch group (memset of covered included) and the gate are captured
    once and replayed on other poses and ids, which the graph reads from the device at replay."""
    h, w = 24, 32
    rm = _machine(ctx, h, w)
    poses_a, poses_b = _poses(seed=3), _poses(seed=9)
    poses_b[1] = -1.0
    cls_b = np.array([1, 0, 0, 1], np.int32)
    image, depth, covered = ctx.empty((4, h, w, 3), np.uint8), ctx.empty((4, h, w), np.uint16), ctx.empty((4,), np.int32)
    cls_d, poses_d = ctx.array(CLS, dtype=np.int32), ctx.array(poses_a)
    mask = ctx.array(np.ones((4, 1, h, w), np.float32))
    rm.render_frames_into(image, depth, cls_d, poses_d, covered=covered)
    gid = ctypes.c_int(-1)
    lib.deepim_graph_begin(ctx.handle)
    try:
        rm.render_frames_into(image, depth, cls_d, poses_d, covered=covered)
        lib.deepim_mask_gate(ctx.handle, mask, covered, 4, h, w)
    finally:
        lib.deepim_graph_end(ctx.handle, ctypes.byref(gid))
    cls_d.copyfrom(cls_b)
    poses_d.copyfrom(poses_b)
    for _ in range(2):                            # twice: covered does not accumulate across replays either
        lib.deepim_graph_launch(ctx.handle, gid.value)
    want = _frames(ctx, rm, cls_b, poses_b)
    np.testing.assert_array_equal(image.asnumpy(), want["image"])
    np.testing.assert_array_equal(depth.asnumpy(), want["depth"])
    np.testing.assert_array_equal(covered.asnumpy(), want["covered"])
    assert want["covered"][1] == 0 and (want["covered"][[0, 2, 3]] > 20).all()
    np.testing.assert_array_equal(mask.asnumpy().reshape(4, -1).max(1), [1, 0, 1, 1])


@pytest.mark.parametrize("h,w", SIZES)
def test_mask_gate_zeroes_only_the_uncovered_planes(ctx, h, w):
    rng = np.random.default_rng(h)
    bits = rng.integers(1, 2 ** 32, (5, 1, h, w), dtype=np.uint64).astype(np.uint32)      # any bit pattern, NaNs included
    covered = np.array([3, 0, -1, 0, h * w], np.int32)
    mask = ctx.array(bits.view(np.float32))
    lib.deepim_mask_gate(ctx.handle, mask, ctx.array(covered, dtype=np.int32), 5, h, w)
    got = mask.asnumpy().view(np.uint32)
    want = bits.copy()
    want[[1, 3]] = 0
    np.testing.assert_array_equal(got, want)
    # a leading-axis view that is only 4-byte aligned takes the single-store path: the same result
    if (h * w) % 4:
        view = ctx.array(bits.view(np.float32))[1:4]
        lib.deepim_mask_gate(ctx.handle, view, ctx.array(np.array([0, 5, 0], np.int32), dtype=np.int32), 3, h, w)
        want = bits[1:4].copy()
        want[[0, 2]] = 0
        np.testing.assert_array_equal(view.asnumpy().view(np.uint32), want)
    lib.deepim_mask_gate(ctx.handle, mask, ctx.array(covered, dtype=np.int32), 0, h, w)      # B = 0: nothing to do
