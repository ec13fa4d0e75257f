"""Host packer of the mesh table that `deepim_render_classes_forward` draws mixed-class batches from
(mx_deepim_amd/lib/render_glumpy/render_py_multi.py `pack_mesh_table`; layout: include/deepim_hip.h). Pure numpy: no GPU."""
import numpy as np
import pytest

from mx_deepim_amd.lib.render_glumpy.render_py_multi import DESC_FIELDS, pack_mesh_table
from mx_deepim_amd.runtime import parse_header

import render_classes_table as rct


@pytest.fixture(scope="module")
def meshes():
    return rct.meshes(normals=True)


@pytest.fixture(scope="module")
def table(meshes):
    return pack_mesh_table(meshes)


def test_descriptor_rows_and_offsets(meshes, table):
    assert DESC_FIELDS == ("v_off", "V", "f_off", "F", "attr_off", "tex_off", "tex_h", "tex_w")
    d = table["mesh_desc"]
    assert d.dtype == np.int32 and d.shape == (4, 8) and d.flags["C_CONTIGUOUS"]
    Vs, Fs = [len(m["vertices"]) for m in meshes], [len(m["faces"]) for m in meshes]
    assert len(set(Vs)) == 3 and len(set(Fs)) == 3                      # the table really has unequal meshes
    np.testing.assert_array_equal(d[:, 1], Vs)
    np.testing.assert_array_equal(d[:, 3], Fs)
    np.testing.assert_array_equal(d[:, 0], np.concatenate([[0], np.cumsum(Vs)[:-1]]))
    np.testing.assert_array_equal(d[:, 2], np.concatenate([[0], np.cumsum(Fs)[:-1]]))
    assert table["max_V"] == max(Vs) and table["max_F"] == max(Fs)
    assert table["vertices"].shape == (sum(Vs), 3) and table["vertices"].dtype == np.float32
    assert table["faces"].shape == (sum(Fs), 3) and table["faces"].dtype == np.int32
    for k, m in enumerate(meshes):
        np.testing.assert_array_equal(table["vertices"][d[k, 0]:d[k, 0] + d[k, 1]], m["vertices"])
        np.testing.assert_array_equal(table["faces"][d[k, 2]:d[k, 2] + d[k, 3]], m["faces"])    # local indices, not rebased
        assert table["faces"][d[k, 2]:d[k, 2] + d[k, 3]].max() < d[k, 1]
    assert table["normals"] is None                                      # the unlit machine's table carries none


def test_mixed_attribute_blocks(meshes, table):
    d, a = table["mesh_desc"], table["vertex_attr"]
    assert a.ndim == 1 and a.dtype == np.float32
    widths = [2 if "texture" in m else 3 for m in meshes]
    assert widths == [3, 2, 3, 2]
    sizes = [w * len(m["vertices"]) for w, m in zip(widths, meshes)]
    np.testing.assert_array_equal(d[:, 4], np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    assert a.size == sum(sizes)
    for k, m in enumerate(meshes):
        block = a[d[k, 4]:d[k, 4] + sizes[k]].reshape(-1, widths[k])
        np.testing.assert_array_equal(block, rct.attr(m))


def test_texture_offsets(meshes, table):
    d, t = table["mesh_desc"], table["textures"]
    np.testing.assert_array_equal(d[:, 5], [-1, 0, -1, 16 * 32 * 3])
    np.testing.assert_array_equal(d[:, 6], [0, 16, 0, 64])
    np.testing.assert_array_equal(d[:, 7], [0, 32, 0, 128])
    assert t.ndim == 1 and t.dtype == np.float32 and t.size == (16 * 32 + 64 * 128) * 3
    for k in (1, 3):
        np.testing.assert_array_equal(t[d[k, 5]:d[k, 5] + d[k, 6] * d[k, 7] * 3].reshape(d[k, 6], d[k, 7], 3), meshes[k]["texture"])
    only_colours = pack_mesh_table([meshes[0], meshes[2]])
    assert only_colours["textures"] is None
    np.testing.assert_array_equal(only_colours["mesh_desc"][:, 5], [-1, -1])


def test_normals_of_the_lit_machine(meshes):
    table = pack_mesh_table(meshes, with_normals=True)
    d = table["mesh_desc"]
    assert table["normals"].shape == table["vertices"].shape and table["normals"].dtype == np.float32
    for k, m in enumerate(meshes):
        np.testing.assert_array_equal(table["normals"][d[k, 0]:d[k, 0] + d[k, 1]], m["normals"])
    np.testing.assert_array_equal(d, pack_mesh_table(meshes)["mesh_desc"])
    short = dict(meshes[1], normals=meshes[1]["normals"][:-1])
    with pytest.raises(ValueError):
        pack_mesh_table([meshes[0], short], with_normals=True)


def test_rejects_face_index_outside_its_mesh(meshes):
    # the index is valid in the packed vertex array (the next mesh's vertices follow) but not in its own mesh
    bad = dict(meshes[0], faces=meshes[0]["faces"].copy())
    bad["faces"][5, 1] = len(meshes[0]["vertices"])
    with pytest.raises(ValueError):
        pack_mesh_table([bad, meshes[1]])
    bad["faces"][5, 1] = -1
    with pytest.raises(ValueError):
        pack_mesh_table([bad, meshes[1]])
    with pytest.raises(ValueError):
        pack_mesh_table([])
    with pytest.raises(ValueError):
        pack_mesh_table([dict(meshes[1], uv=None)])                     # textured mesh without uv


def test_entry_is_declared_with_the_table_layout():
    ret, argtypes, names = parse_header()["deepim_render_classes_forward"]
    assert names == ["ctx", "image", "depth", "mask_rendered", "mask_box", "mask_thresh", "class_index", "mesh_desc", "n_classes",
                     "max_V", "max_F", "vertices", "vertex_attr", "normals", "faces", "textures", "poses", "K_host",
                     "pixel_means_host", "light_offset_host", "light_intensity", "brightness_ratio", "B", "H", "W", "znear", "zfar"]
