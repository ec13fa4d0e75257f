"""The four-pair 24x32 scene of tests/test_gpu_closed_loop_boxes.py and tests/test_gpu_render_quad.py: every case of the boxes
that the render pass hands to the zoom front end.
  pair 0  an ordinary object inside the frame
  pair 1  an object hanging over the right and bottom edges
  pair 2  a sliver whose rendered mask is a single pixel column: the half-open rectangle is empty
  pair 3  an object outside the frame: nothing rendered
Two classes: 0 an ellipsoid, 1 the sliver (a thin upright quad); the per-pair ids are IDS."""
import numpy as np

from mx_deepim_amd import synthetic

H, W, B = 24, 32, 4
K = synthetic.K_LINEMOD.copy()
K[:2] *= 0.05                                        # LINEMOD intrinsics for a 1/20-size frame
MEANS = synthetic.PIXEL_MEANS[::-1].copy()
NAMES = ["ball", "sliver"]
IDS = np.array([0, 0, 1, 0], np.int32)
Z = 0.6
SLIVER_COL = 10


def back_project(u, v, z=Z, k=K):
    return np.array([(u - k[0, 2]) / k[0, 0] * z, (v - k[1, 2]) / k[1, 1] * z, z], np.float32)


def meshes(normals=False):
    ball = synthetic.ellipsoid_mesh([0.10, 0.09, 0.08], 8, 16)
    ball.pop("uv")
    # the sliver: 0.6 pixels wide around a pixel-index column, 9.6 pixels high between two rows: covers column SLIVER_COL only
    w, h = 0.3 * Z / K[0, 0], 4.8 * Z / K[1, 1]
    v = np.array([[-w, -h, 0], [w, -h, 0], [w, h, 0], [-w, h, 0]], np.float32)
    sliver = {"vertices": v, "faces": np.array([[0, 1, 2], [0, 2, 3]], np.int32),
              "colors": np.array([[200, 40, 40], [40, 200, 40], [40, 40, 200], [200, 200, 40]], np.float32)}
    out = [ball, sliver]
    if normals:
        n = ball["vertices"] / (np.asarray([0.10, 0.09, 0.08], np.float32) ** 2)
        ball["normals"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        sliver["normals"] = np.tile(np.array([[0, 0, -1]], np.float32), (4, 1))
    return out


def poses(shift=0.0, cams=None):
    """(B,3,4): identity rotations (a small turn about z for the balls), the four placements above; `shift` moves the objects
    by that many pixels in x (other poses of the same cases). cams: (B,3,3) per-pair cameras the placements are meant for."""
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    k = [K] * B if cams is None else cams
    p = np.zeros((B, 3, 4), np.float32)
    p[0, :, :3], p[0, :, 3] = R, back_project(13.0 + shift, 11.0, k=k[0])
    p[1, :, :3], p[1, :, 3] = R, back_project(29.0 + shift, 21.0, k=k[1])
    p[2, :, :3], p[2, :, 3] = np.eye(3), back_project(float(SLIVER_COL + int(shift)), 10.0, k=k[2])
    p[3, :, :3], p[3, :, 3] = R, back_project(400.0, 11.0, k=k[3])
    return p


def cameras():
    """(B,3,3): a camera of its own for every pair, close to K"""
    t = np.repeat(K[None], B, 0).astype(np.float32)
    for b in range(B):
        t[b, 0, 0] *= 1.0 + 0.01 * b
        t[b, 1, 1] *= 1.0 - 0.01 * b
        t[b, 0, 2] += 0.25 * b
    return t


def numpy_box(m, thresh):
    """{minx, maxx, miny, maxy} of m > thresh as the zoom front end's bbox pass defines it; empty: {INT_MAX, -1, INT_MAX, -1}"""
    ys, xs = np.nonzero(m > thresh)
    if len(xs) == 0:
        i = np.iinfo(np.int32).max
        return [i, -1, i, -1]
    return [xs.min(), xs.max(), ys.min(), ys.max()]
