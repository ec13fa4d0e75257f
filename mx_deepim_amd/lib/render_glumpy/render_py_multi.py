"""`Render_Py` with the constructor and `render()` signature of lib/render_glumpy/render_py_multi.py:21-129,
drawn by the HIP rasteriser (csrc/render.hip, `deepim_render_forward`) instead of an off-screen OpenGL window.

    render_machine = Render_Py(model_dir, classes, K, width, height, zNear, zFar)
    bgr, depth = render_machine.render(cls_idx, quat_or_mat, t)          # reference call (:101), host arrays
    image, depth = render_machine.render_batch(class_index, poses)       # device tensors for the batch updater
    render_machine.render_classes_into(image, depth, class_index_dev, poses)   # mixed-class batch, ids on the device

`render` returns what the reference returns (:121-129): (H,W,3) float32 BGR on the 0..255 scale and (H,W)
metric depth with 0 background. `render_batch` skips that host round trip: it writes the network-input tensors
(RGB − reversed PIXEL_MEANS, NCHW; batch_updater_py_multi.py:117-133) straight into HBM.

Meshes come from `<model_dir>/<class>/textured.obj` + `texture_map.png` like the reference (:68-77), or from
memory through `meshes={class: dict(vertices, faces, uv, texture | colors)}` (what the tests and bench use:
there are no model files offline).

A batch whose samples belong to different classes is one launch group when its class ids are a device int32 array
(`deepim_render_classes_forward` over the mesh table `pack_mesh_table` builds): the host never reads the ids.
"""
import ctypes
import os

import numpy as np

from ...runtime import Context, DeviceArray, lib


def quat2mat(q):
    """(w,x,y,z) → 3x3 rotation, any non-zero norm (argument staging for `render`; the reference takes it from
    lib/pair_matching/RT_transform.py:quat2mat). A near-zero quaternion gives the identity, as there."""
    w, x, y, z = (float(c) for c in np.asarray(q, dtype=np.float64).reshape(4))
    n = w * w + x * x + y * y + z * z
    if n < np.finfo(np.float64).eps:
        return np.eye(3)
    s = 2.0 / n
    return np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                     [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                     [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]])


def load_obj(path):
    """Minimal Wavefront reader for the `v` / `vt` / `f` records of the LINEMOD `textured.obj` files.
    Like glumpy's data.objload (used at render_py_multi.py:72) every distinct (position, texcoord) pair becomes
    one vertex; polygons are fanned into triangles."""
    pos, tex, corner, faces = [], [], {}, []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                pos.append([float(x) for x in tok[1:4]])
            elif tok[0] == "vt":
                tex.append([float(x) for x in tok[1:3]])
            elif tok[0] == "f":
                idx = []
                for c in tok[1:]:
                    parts = c.split("/")
                    vi = int(parts[0])
                    ti = int(parts[1]) if len(parts) > 1 and parts[1] else 0
                    key = (vi - 1 if vi > 0 else len(pos) + vi, (ti - 1 if ti > 0 else len(tex) + ti) if ti else -1)
                    idx.append(corner.setdefault(key, len(corner)))
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    keys = sorted(corner, key=corner.get)
    vertices = np.array([pos[k[0]] for k in keys], dtype=np.float32).reshape(-1, 3)
    uv = np.array([tex[k[1]] if k[1] >= 0 else [0.0, 0.0] for k in keys], dtype=np.float32).reshape(-1, 2)
    return vertices, uv, np.array(faces, dtype=np.int32).reshape(-1, 3)


def load_texture(path):
    """(h,w,3) float32 on the 0..255 scale, flipped so row 0 is v = 0 (render_py_multi.py:76)."""
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGB"), dtype=np.float32)
    return np.ascontiguousarray(img[::-1])


DESC_FIELDS = ("v_off", "V", "f_off", "F", "attr_off", "tex_off", "tex_h", "tex_w")


def pack_mesh_table(meshes, with_normals=False):
    """Host packer of the mesh table of `deepim_render_classes_forward` (layout: include/deepim_hip.h). `meshes`: one
    dict(vertices, faces, uv + texture | colors [, normals]) per class, in class-id order. Returns a dict of numpy arrays:
    vertices (ΣV,3), vertex_attr (flat: each mesh's own (V,2) uv or (V,3) colour block back to back), normals (ΣV,3) or None,
    faces (ΣF,3) int32 with indices local to their mesh, textures (flat: each textured mesh's (h,w,3) block) or None,
    mesh_desc (n,8) int32 rows of DESC_FIELDS (offsets of attr / tex in floats, tex_off −1 = vertex colours), max_V, max_F.
    The device trusts this table, so everything it indexes with is checked here."""
    if len(meshes) == 0:
        raise ValueError("mesh table needs at least one mesh")
    verts, attrs, nrms, faces, texs, desc = [], [], [], [], [], []
    v_off = f_off = attr_off = tex_off = 0
    for m in meshes:
        v = np.ascontiguousarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(m["faces"], dtype=np.int32).reshape(-1, 3)
        V, F = len(v), len(f)
        if V == 0 or F == 0:
            raise ValueError("empty mesh")
        if f.min() < 0 or f.max() >= V:
            raise ValueError("face index out of range")
        texture = m.get("texture")
        if texture is not None:
            texture = np.ascontiguousarray(texture, dtype=np.float32)
            if m.get("uv") is None or texture.ndim != 3 or texture.shape[2] != 3 or texture.size == 0:
                raise ValueError("textured mesh needs uv (V,2) and texture (h,w,3)")
            a = np.ascontiguousarray(m["uv"], dtype=np.float32).reshape(V, 2)
            row_tex = (tex_off, texture.shape[0], texture.shape[1])
            texs.append(texture.reshape(-1))
            tex_off += texture.size
        else:
            if m.get("colors") is None:
                raise ValueError("mesh needs a texture or per-vertex colors")
            a = np.ascontiguousarray(m["colors"], dtype=np.float32).reshape(V, 3)
            row_tex = (-1, 0, 0)
        if with_normals:
            n = np.ascontiguousarray(m["normals"], dtype=np.float32).reshape(-1, 3)
            if len(n) != V:
                raise ValueError("one normal per vertex")
            nrms.append(n)
        desc.append((v_off, V, f_off, F, attr_off) + row_tex)
        verts.append(v)
        faces.append(f)
        attrs.append(a.reshape(-1))
        v_off, f_off, attr_off = v_off + V, f_off + F, attr_off + a.size
    if max(3 * v_off, 3 * f_off, attr_off, tex_off) >= 2 ** 31:
        raise ValueError("mesh table too large for int32 offsets")
    desc = np.asarray(desc, dtype=np.int32).reshape(-1, 8)
    return {"vertices": np.concatenate(verts), "vertex_attr": np.concatenate(attrs),
            "normals": np.concatenate(nrms) if with_normals else None, "faces": np.concatenate(faces),
            "textures": np.concatenate(texs) if texs else None, "mesh_desc": desc,
            "max_V": int(desc[:, 1].max()), "max_F": int(desc[:, 3].max())}


class _MeshTable(object):
    """The packed table on the device, uploaded once."""

    def __init__(self, ctx, host):
        self.n_classes, self.max_V, self.max_F = len(host["mesh_desc"]), host["max_V"], host["max_F"]
        self.vertices, self.vertex_attr = ctx.array(host["vertices"]), ctx.array(host["vertex_attr"])
        self.normals = None if host["normals"] is None else ctx.array(host["normals"])
        self.faces = ctx.array(host["faces"], dtype=np.int32)
        self.textures = None if host["textures"] is None else ctx.array(host["textures"])
        self.mesh_desc = ctx.array(host["mesh_desc"], dtype=np.int32)


def is_device_ids(class_index):
    """True for what takes the one-launch-group path: a device array of dtype int32."""
    return hasattr(class_index, "asnumpy") and hasattr(class_index, "ptr") and class_index.dtype == np.int32


class _Mesh(object):
    def __init__(self, ctx, vertices, faces, uv=None, texture=None, colors=None):
        vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        if faces.size and (faces.min() < 0 or faces.max() >= len(vertices)):
            raise ValueError("face index out of range")
        self.V, self.F = len(vertices), len(faces)
        self.host = dict(vertices=vertices, faces=faces, uv=uv, texture=texture, colors=colors)    # what pack_mesh_table reads
        self.vertices = ctx.array(vertices)
        self.faces = ctx.array(faces, dtype=np.int32)
        if texture is not None:
            texture = np.ascontiguousarray(texture, dtype=np.float32)
            if uv is None or texture.ndim != 3 or texture.shape[2] != 3:
                raise ValueError("textured mesh needs uv (V,2) and texture (h,w,3)")
            self.attr = ctx.array(np.ascontiguousarray(uv, dtype=np.float32).reshape(self.V, 2))
            self.texture, self.tex_h, self.tex_w = ctx.array(texture), texture.shape[0], texture.shape[1]
        else:
            if colors is None:
                raise ValueError("mesh needs a texture or per-vertex colors")
            self.attr = ctx.array(np.ascontiguousarray(colors, dtype=np.float32).reshape(self.V, 3))
            self.texture, self.tex_h, self.tex_w = None, 0, 0


class Render_Py(object):
    def __init__(self, model_dir, classes, K, width=640, height=480, zNear=0.25, zFar=6.0, meshes=None, ctx=None,
                 pixel_means=None):
        self.width, self.height, self.zNear, self.zFar = int(width), int(height), float(zNear), float(zFar)
        self.K = np.ascontiguousarray(K, dtype=np.float32).reshape(3, 3)
        self.model_dir, self.classes = model_dir, list(classes)
        self.ctx = ctx or Context.default()
        # tensor-channel order (RGB): the updater subtracts PIXEL_MEANS[[2,1,0]] (batch_updater_py_multi.py:124-127)
        self.pixel_means = None if pixel_means is None else np.ascontiguousarray(pixel_means, np.float32).reshape(3)
        self.mesh_list = []
        self._table = None
        for cls in self.classes:
            if meshes is not None and cls in meshes:
                self.mesh_list.append(_Mesh(self.ctx, **meshes[cls]))
                continue
            folder = os.path.join(model_dir, cls)
            vertices, uv, faces = load_obj(os.path.join(folder, "textured.obj"))
            self.mesh_list.append(_Mesh(self.ctx, vertices, faces, uv=uv,
                                        texture=load_texture(os.path.join(folder, "texture_map.png"))))

    # -- device API ----------------------------------------------------------------------------------------------
    def _camera(self, K, n):
        """`K=` of the draw methods → the C entry's K_host: the machine's K (None), a host (3,3), or — for a DeviceArray (n,3,3)
        whose leading axis is the call's batch, sample b drawn with row b — NULL after binding it as the context's camera table
        (a leading-axis slice binds with its offset)."""
        if K is None:
            return self.K
        if isinstance(K, DeviceArray):
            if K.ndim != 3 or K.shape[0] != n:
                raise ValueError("a device K must be (n,3,3) with n = the call's batch (%d), got %s" % (n, K.shape))
            self.ctx.bind_cameras(K)
            return None
        return np.ascontiguousarray(K, dtype=np.float32).reshape(3, 3)

    def render_into(self, image, depth, cls_idx, poses, K=None, pixel_means="default", mask_rendered=None, mask_box=None,
                    mask_thresh=0.2, light_intensity=None, boxes=None):
        """image (n,3,H,W), depth (n,1,H,W), poses (n,3,4): all device arrays; one mesh. With `mask_rendered` (n,1,H,W)
        the same pass also writes depth > mask_thresh, and with `mask_box` its box_rendered rectangle. (`light_intensity` belongs
        to the lit ModelNet machine, render_py_light_modelnet_multi.py; this unlit draw ignores it.) `K`: None (the machine's), a
        host (3,3), or a DeviceArray (n,3,3) of per-sample cameras (`_camera`). `boxes`: None, or a device int32 (n,2,4) array
        that receives the zoom front end's boxes of `mask_box` and `mask_rendered` (`deepim_render_export_boxes`; needs both)."""
        m = self.mesh_list[int(cls_idx)]
        n = poses.shape[0]
        K = self._camera(K, n)
        means = self.pixel_means if isinstance(pixel_means, str) else pixel_means
        tail = (m.vertices, m.attr, m.faces, m.texture, m.tex_h, m.tex_w, poses, K, means, m.V, m.F, n, self.height,
                self.width, ctypes.c_float(self.zNear), ctypes.c_float(self.zFar))
        if mask_rendered is None:
            if mask_box is not None:
                raise ValueError("mask_box needs mask_rendered")
            if boxes is not None:
                raise ValueError("boxes needs mask_box")
            lib.deepim_render_forward(self.ctx.handle, image, depth, *tail)
        else:
            self._export_boxes(boxes, mask_box, n)
            lib.deepim_render_update_forward(self.ctx.handle, image, depth, mask_rendered, mask_box,
                                             ctypes.c_float(mask_thresh), *tail)

    def _export_boxes(self, boxes, mask_box, n):
        """Arm the one-shot boxes export for the draw that follows at once (the C entry clears it, also when it fails)."""
        if boxes is None:
            return
        if mask_box is None:
            raise ValueError("boxes needs mask_box")
        if not isinstance(boxes, DeviceArray) or boxes.dtype != np.int32 or boxes.shape != (n, 2, 4):
            raise ValueError("boxes must be a device int32 array (%d,2,4)" % n)
        lib.deepim_render_export_boxes(self.ctx.handle, boxes)

    _lit = False         # the lit machine's mesh table carries the normals

    def mesh_table(self):
        """The device mesh table of `render_classes_into`: packed and uploaded once per render machine, on first use."""
        if self._table is None:
            self._table = _MeshTable(self.ctx, pack_mesh_table([m.host for m in self.mesh_list], with_normals=self._lit))
        return self._table

    def _draw_classes(self, image, depth, class_index, poses, K, pixel_means, mask_rendered, mask_box, mask_thresh,
                      light_offset=None, light_intensity=None, ratio=0.0, boxes=None):
        if not is_device_ids(class_index):
            raise TypeError("render_classes_into needs class_index as a device int32 array")
        if mask_rendered is None and mask_box is not None:
            raise ValueError("mask_box needs mask_rendered")
        t = self.mesh_table()
        K = self._camera(K, poses.shape[0])
        means = self.pixel_means if isinstance(pixel_means, str) else pixel_means
        self._export_boxes(boxes, mask_box, poses.shape[0])
        lib.deepim_render_classes_forward(self.ctx.handle, image, depth, mask_rendered, mask_box, ctypes.c_float(mask_thresh),
                                          class_index, t.mesh_desc, t.n_classes, t.max_V, t.max_F, t.vertices, t.vertex_attr,
                                          t.normals, t.faces, t.textures, poses, K, means, light_offset, light_intensity,
                                          ctypes.c_float(ratio), poses.shape[0], self.height, self.width,
                                          ctypes.c_float(self.zNear), ctypes.c_float(self.zFar))

    def render_classes_into(self, image, depth, class_index, poses, K=None, pixel_means="default", mask_rendered=None,
                            mask_box=None, mask_thresh=0.2, light_intensity=None, boxes=None):
        """As `render_into` for a batch of mixed classes: `class_index` (n) is a DEVICE int32 array and sample b draws mesh
        class_index[b], all in one launch group. The ids are never read on the host; a sample whose id is outside
        [0, len(classes)) comes out as an empty frame (see include/deepim_hip.h). (`light_intensity`: ignored, as in `render_into`.)"""
        self._draw_classes(image, depth, class_index, poses, K, pixel_means, mask_rendered, mask_box, mask_thresh, boxes=boxes)

    def render_frames_into(self, image_u8, depth_u16, class_index_dev, poses, K=None, rows=None, label=None, label_value=None,
                           covered=None, depth_factor=1000.0):
        """The unlit mixed-class draw stored as DECODED frames (`deepim_render_frames_forward`): what the reference's
        toolkit/LM6d_3_gen_PoseCNN_pred_rendered.py writes to disk for every initial pose and lib/utils/image.py reads back.
        image_u8 (N,H,W,3) uint8 BGR = rint(clip(level, 0, 255)), depth_u16 (N,H,W) uint16 = the float32 depth * depth_factor
        truncated, label (N,H,W) uint8 or None = label_value[b] (device int32 (n), None = 1) where the depth is non-zero.
        Sample b goes to row rows[b] (device int32 (n), None = b) of the N >= n rows. covered: device int32 (n) or None, written
        with each sample's count of non-zero depth pixels (never read here). `K`: as in `render_into`."""
        if not is_device_ids(class_index_dev):
            raise TypeError("render_frames_into needs class_index as a device int32 array")
        n, H, W = poses.shape[0], self.height, self.width
        if image_u8.dtype != np.uint8 or image_u8.ndim != 4 or image_u8.shape[1:] != (H, W, 3):
            raise TypeError("render_frames_into: image must be uint8 (N,%d,%d,3), got %s %s" % (H, W, image_u8.dtype, image_u8.shape))
        N = image_u8.shape[0]
        if depth_u16.dtype != np.uint16 or depth_u16.shape != (N, H, W):
            raise TypeError("render_frames_into: depth must be uint16 %s, got %s %s" % ((N, H, W), depth_u16.dtype, depth_u16.shape))
        if label is not None and (label.dtype != np.uint8 or label.shape != (N, H, W)):
            raise TypeError("render_frames_into: label must be uint8 %s, got %s %s" % ((N, H, W), label.dtype, label.shape))
        for name, a in (("rows", rows), ("label_value", label_value), ("covered", covered)):
            if a is not None and (not is_device_ids(a) or a.size != n):
                raise TypeError("render_frames_into: %s must be a device int32 array of %d values" % (name, n))
        if class_index_dev.size != n:
            raise TypeError("render_frames_into: %d class ids for %d poses" % (class_index_dev.size, n))
        t = self.mesh_table()
        K = self._camera(K, n)
        lib.deepim_render_frames_forward(self.ctx.handle, image_u8, depth_u16, label, covered, rows, N, label_value,
                                         ctypes.c_float(depth_factor), class_index_dev, t.mesh_desc, t.n_classes, t.max_V, t.max_F,
                                         t.vertices, t.vertex_attr, t.faces, t.textures, poses, K, n, H, W,
                                         ctypes.c_float(self.zNear), ctypes.c_float(self.zFar))

    def render_batch(self, class_index, poses, K=None, out=None, mask_rendered=None, mask_thresh=0.2, light_intensity=None):
        """poses (B,3,4) device; class_index: scalar, host sequence of B class ids, None (= class 0), or a device array.
        Host ids: samples of the same class in consecutive runs are drawn by one launch group each. A DEVICE int32 array of B ids:
        the whole batch is one launch group (`render_classes_into`) and the ids are never read back. (A device array of another
        dtype is read back and split into runs like host ids.) `out` = (image, depth) preallocated device tensors;
        `mask_rendered` (B,1,H,W): also written, = depth > mask_thresh, by the same pass. `K`: as in `render_into`; a device
        (B,3,3) table is sliced with the runs on the host-id path."""
        B = poses.shape[0]
        image, depth = out if out is not None else (self.ctx.empty((B, 3, self.height, self.width)),
                                                    self.ctx.empty((B, 1, self.height, self.width)))
        if is_device_ids(class_index) and class_index.size == B:
            self.render_classes_into(image, depth, class_index, poses, K=K, mask_rendered=mask_rendered, mask_thresh=mask_thresh,
                                     light_intensity=light_intensity)
            return image, depth
        if class_index is None:
            ids = np.zeros(B, np.int64)
        else:
            ids = class_index.asnumpy() if hasattr(class_index, "asnumpy") else np.asarray(class_index)
            ids = np.broadcast_to(ids.astype(np.int64).reshape(-1), (B,)) if ids.size == 1 else ids.astype(np.int64).reshape(B)
        b0 = 0
        while b0 < B:
            b1 = b0 + 1
            while b1 < B and ids[b1] == ids[b0]:
                b1 += 1
            self.render_into(image[b0:b1], depth[b0:b1], ids[b0], poses[b0:b1], K=K[b0:b1] if isinstance(K, DeviceArray) else K,
                             mask_rendered=None if mask_rendered is None else mask_rendered[b0:b1], mask_thresh=mask_thresh,
                             light_intensity=None if light_intensity is None else light_intensity[b0:b1])
            b0 = b1
        return image, depth

    # -- reference API -------------------------------------------------------------------------------------------
    def render(self, cls_idx, r, t, r_type="quat", K=None):
        if r_type == "quat":
            R = quat2mat(r)
        elif r_type == "mat":
            R = np.asarray(r)
        else:
            raise ValueError("r_type must be 'quat' or 'mat'")
        pose = np.zeros((1, 3, 4), np.float32)
        pose[0, :, :3] = np.asarray(R, np.float32).reshape(3, 3)
        pose[0, :, 3] = np.asarray(t, np.float32).reshape(3)
        image = self.ctx.empty((1, 3, self.height, self.width))
        depth = self.ctx.empty((1, 1, self.height, self.width))
        self.render_into(image, depth, cls_idx, self.ctx.array(pose), K=K, pixel_means=None)
        rgb = image.asnumpy()[0]
        bgr = np.ascontiguousarray(rgb[::-1].transpose(1, 2, 0))
        return bgr, depth.asnumpy()[0, 0]
