"""The four-class mesh table shared by tests/test_render_mesh_table_host.py and tests/test_gpu_render_classes.py, chosen so that
every field of a descriptor row matters: V and F differ (max_V / max_F padding), vertex colours and textures alternate (mixed
3-float / 2-float attribute blocks, tex_off −1 / 0 / > 0) and the two textures differ in size."""
import numpy as np

from mx_deepim_amd import synthetic

H, W = 120, 160
K = synthetic.K_LINEMOD.copy()
K[:2] *= 0.25                                        # LINEMOD intrinsics for a quarter-size frame
MEANS = synthetic.PIXEL_MEANS[::-1].copy()
NAMES = ["c0", "c1", "c2", "c3"]
# (axes, n_lat, n_lon, texture size or None = vertex colours)
SPEC = [([0.10, 0.09, 0.08], 6, 12, None), ([0.09, 0.10, 0.08], 12, 24, (16, 32)),
        ([0.08, 0.09, 0.10], 24, 48, None), ([0.10, 0.08, 0.09], 12, 24, (64, 128))]


def meshes(normals=False):
    """One dict(vertices, faces, uv + texture | colors [, normals]) per class."""
    out = []
    for k, (axes, n_lat, n_lon, tex) in enumerate(SPEC):
        m = synthetic.ellipsoid_mesh(axes, n_lat, n_lon)
        if tex is None:
            m.pop("uv")
        else:
            m.pop("colors")
            m["texture"] = synthetic.procedural_texture(tex[0], tex[1], seed=7 + k)
        if normals:
            n = m["vertices"] / (np.asarray(axes, np.float32) ** 2)
            m["normals"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        out.append(m)
    return out


def attr(m):
    return m["uv"] if "texture" in m else m["colors"]


def poses(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([synthetic.sample_pose_pair(rng, K, H, W)[1] for _ in range(n)]).astype(np.float32)
