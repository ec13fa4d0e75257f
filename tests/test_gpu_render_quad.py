"""The resolve and box-fill passes with four pixels per lane (context option render_quad = 1, the default) against one pixel per
lane (render_quad = 0): image, depth, mask, box words and rectangle bit for bit. 24x32 takes the four-pixel kernels; 23x31 (a
plane that is no multiple of 4) and a misaligned output take the one-pixel kernels under either setting. Five samples: an object
in each corner of the frame and an empty frame."""
import ctypes

import numpy as np
import pytest

import closed_loop_scene as cls
from mx_deepim_amd.lib.render_glumpy.render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi
from mx_deepim_amd.lib.render_glumpy.render_py_multi import Render_Py
from mx_deepim_amd.runtime import DeviceArray, lib

pytestmark = pytest.mark.gpu
N = 5


def corner_poses(H, W):
    p = np.zeros((N, 3, 4), np.float32)
    c, s = np.cos(0.4), np.sin(0.4)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    for b, (u, v) in enumerate([(1.0, 1.0), (W - 2.0, 1.0), (1.0, H - 2.0), (W - 2.0, H - 2.0), (900.0, 5.0)]):
        p[b, :, :3], p[b, :, 3] = R, cls.back_project(u, v)
    return p


def draw(ctx, rm, H, W, quad, device_ids, offset=0):
    """-> the five outputs and the exported boxes, as uint32 / int32 bits; offset: floats by which every output is misaligned"""
    st = ctypes.c_int(0)
    lib.deepim_zoom_status(ctx.handle, ctypes.byref(st))      # reading clears what earlier tests left
    lib.deepim_set_option(ctx.handle, b"render_quad", quad)
    try:
        def buf(c):
            whole = ctx.zeros((N * c * H * W + 4,))
            return DeviceArray(ctx, (N, c, H, W), np.float32, ptr=whole.ptr + 4 * offset, base=whole)
        img, dep, mr, mb = buf(3), buf(1), buf(1), buf(1)
        boxes = ctx.zeros((N, 2, 4), dtype=np.int32)
        poses = ctx.array(corner_poses(H, W))
        if device_ids:
            rm.render_classes_into(img, dep, ctx.array(np.zeros(N, np.int32), dtype=np.int32), poses, mask_rendered=mr, mask_box=mb,
                                   boxes=boxes)
        else:
            rm.render_into(img, dep, 0, poses, mask_rendered=mr, mask_box=mb, boxes=boxes)
        lib.deepim_zoom_status(ctx.handle, ctypes.byref(st))
        return [a.asnumpy().view(np.uint32) for a in (img, dep, mr, mb)] + [boxes.asnumpy(), st.value]
    finally:
        lib.deepim_set_option(ctx.handle, b"render_quad", 1)


def check(one, four, H, W):
    for a, b in zip(one, four):
        np.testing.assert_array_equal(a, b)
    img, dep, mr, mb, boxes, st = four
    dep, mr, mb = dep.view(np.float32), mr.view(np.float32), mb.view(np.float32)
    np.testing.assert_array_equal(mr, (dep > 0.2).astype(np.float32))
    for b in range(N):
        assert boxes[b, 1].tolist() == cls.numpy_box(mr[b, 0], 0.2) and boxes[b, 0].tolist() == cls.numpy_box(mb[b, 0], 0.3)
        xs, xe, ys, ye = boxes[b, 1]
        want = np.zeros((H, W), np.float32)
        if xe >= 0:
            want[ys:ye, xs:xe] = 1
        np.testing.assert_array_equal(mb[b, 0], want)
    # an object in each corner, touching both of its edges, and an empty frame
    assert boxes[0, 1, 0] == 0 and boxes[0, 1, 2] == 0 and boxes[1, 1, 1] == W - 1 and boxes[1, 1, 2] == 0
    assert boxes[2, 1, 0] == 0 and boxes[2, 1, 3] == H - 1 and boxes[3, 1, 1] == W - 1 and boxes[3, 1, 3] == H - 1
    assert not mr[4].any() and not mb[4].any() and (dep[4] == 0).all() and st == 4


@pytest.mark.parametrize("H,W,offset", [(24, 32, 0), (23, 31, 0), (24, 32, 1)])
@pytest.mark.parametrize("device_ids", [False, True])
def test_four_pixels_per_lane_equal_one(ctx, H, W, offset, device_ids):
    rm = Render_Py("unused", cls.NAMES, cls.K, W, H, meshes=dict(zip(cls.NAMES, cls.meshes())), ctx=ctx, pixel_means=cls.MEANS)
    one = draw(ctx, rm, H, W, 0, device_ids, offset)
    four = draw(ctx, rm, H, W, 1, device_ids, offset)
    check(one, four, H, W)


def test_four_pixels_per_lane_equal_one_lit(ctx):
    H, W = 24, 32
    rm = Render_Py_Light_ModelNet_Multi(cls.NAMES, None, cls.K, W, H, meshes=cls.meshes(normals=True), ctx=ctx,
                                        pixel_means=cls.MEANS)
    check(draw(ctx, rm, H, W, 0, False), draw(ctx, rm, H, W, 1, False), H, W)


def test_option_reads_back(ctx):
    v = ctypes.c_int(-1)
    lib.deepim_get_option(ctx.handle, b"render_quad", ctypes.byref(v))
    assert v.value == 1
