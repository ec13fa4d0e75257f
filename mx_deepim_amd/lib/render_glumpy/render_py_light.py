"""`Render_Py_Light` with the constructor and `render()` signature of lib/render_glumpy/render_py_light.py:82-172 — the render
machine toolkit/LM6d_ds_1_gen_observed.py draws its synthetic observed frames with — over the lit machine of
render_py_light_modelnet_multi.py and the HIP rasteriser instead of an off-screen OpenGL window.

    rm = Render_Py_Light(model_folder, K, width, height, zNear, zFar, brightness_ratios=[0.2, 0.25, 0.3, 0.35, 0.4])
    bgr, depth = rm.render(r, t, light_position, light_intensity, brightness_k=2, r_type="quat")      # reference call (:123)
    SyntheticObserved(rm, stats, K, seed)                   # lib/utils/synthetic_observed.py: whole batches, on the device

One model, class id 0: `<model_folder>/textured.obj` (positions, texcoords, normals; NOT rescaled, :92) + `texture_map.png`, or
from memory through `meshes=[dict(vertices, faces, uv, normals, texture)]`.

The fragment stage is the one csrc/render.hip has, texture * ((1 - r) + r brightness) * intensity (the ModelNet machine's,
render_py_light_modelnet_multi.py:74); this file's own shader (:74) multiplies the intensity into the diffuse term only,
texture * ((1 - r) + r brightness intensity). KNOWN DIFFERENCE: the two agree for a white light of intensity 1.
"""
import numpy as np

from .render_py_light_modelnet_multi import Render_Py_Light_ModelNet_Multi, load_obj_with_normals
from .render_py_multi import load_texture, quat2mat


class Render_Py_Light(Render_Py_Light_ModelNet_Multi):
    def __init__(self, model_folder, K, width=640, height=480, zNear=0.25, zFar=6.0, brightness_ratios=[0.4, 0.3, 0.2], meshes=None,
                 ctx=None, pixel_means=None):
        if meshes is None:
            vertices, uv, normals, faces = load_obj_with_normals("{}/textured.obj".format(model_folder))
            meshes = [dict(vertices=vertices, faces=faces, uv=uv, normals=normals,
                           texture=load_texture("{}/texture_map.png".format(model_folder)))]
        if len(meshes) != 1:
            raise ValueError("Render_Py_Light draws one model")
        super(Render_Py_Light, self).__init__([model_folder], None, K, width, height, zNear, zFar, brightness_ratios=brightness_ratios,
                                              meshes=meshes, ctx=ctx, pixel_means=pixel_means)
        self.model_folder = model_folder

    def render(self, r, t, light_position, light_intensity, brightness_k=0, r_type="quat"):
        """-> (bgr (H,W,3) uint8, depth (H,W) float32 metres, 0 = background) as :123-172. `light_position` is the absolute
        position in OpenGL camera coordinates, as LM6d_ds_1_gen_observed.py:131-135 computes it: offset + (t_x, -t_y, -t_z). The
        offset is taken back out in float64, so an offset that is a float32 comes back exactly."""
        if r_type == "quat":
            R = quat2mat(r)
        elif r_type == "mat":
            R = np.asarray(r)
        else:
            raise ValueError("r_type must be 'quat' or 'mat'")
        t32 = np.asarray(t, np.float32).reshape(3)
        pose = np.zeros((1, 3, 4), np.float32)
        pose[0, :, :3] = np.asarray(R, np.float32).reshape(3, 3)
        pose[0, :, 3] = t32
        flip = np.array([1.0, -1.0, -1.0])
        off = (np.asarray(light_position, np.float64).reshape(3) - flip * t32.astype(np.float64)).astype(np.float32)
        image = self.ctx.empty((1, 3, self.height, self.width))
        depth = self.ctx.empty((1, 1, self.height, self.width))
        inten = self.ctx.array(np.asarray(light_intensity, np.float32).reshape(1, 3))
        self.render_into(image, depth, 0, self.ctx.array(pose), pixel_means=None, light_offset=off, light_intensity=inten,
                         brightness_k=brightness_k)
        rgb = image.asnumpy()[0]
        return np.ascontiguousarray(rgb[::-1].transpose(1, 2, 0)).astype(np.uint8), depth.asnumpy()[0, 0]
