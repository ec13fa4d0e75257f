"""Per-pair cameras, the host side: the table helper and its validation (mx_deepim_amd/cameras.py), the sidecar of the result
cache (core/tester.py) and pose_metrics' stacking of all_K over the iterations and the eggbox half-turn subset (a stub stands in
for the device call). No GPU."""
import os
import pickle

import numpy as np
import pytest

import cameras_scene as cs
from mx_deepim_amd import cameras
from mx_deepim_amd.config import default_config
from mx_deepim_amd.core import tester
from mx_deepim_amd.lib.dataset.LM6D_REFINE import LM6D_REFINE

K0, K1, K2 = cs.cameras(48, 64)


def test_the_three_cameras_differ_as_stated_and_every_pair_has_a_box_under_each():
    assert K1[0, 0] == K0[0, 0] * np.float32(0.93) and K2[1, 1] == K0[1, 1] * np.float32(1.08)
    assert K1[0, 2] == K0[0, 2] + np.float32(3.5) and K2[1, 2] == K0[1, 2] - np.float32(2.25)
    t = cs.table(48, 64)
    assert t.shape == (5, 3, 3) and t.dtype == np.float32 and t.flags["C_CONTIGUOUS"]
    for b, c in enumerate(cs.ROWS):
        np.testing.assert_array_equal(t[b], (K0, K1, K2)[c])
    for W in (64, 45):
        s = cs.zoom_scene(48, W, seed=5)
        for K in cs.cameras(48, W):
            zf = cs.zoom_factors_oracle(s, K)              # raises on an empty observed box
            assert np.isfinite(zf).all() and (zf[:, 0] > 0).all() and (np.abs(zf[:, 2:]) < 1).all()


def test_table_helper_falls_back_to_the_config_camera():
    recs = [{"K": K1}, {}, {"K": None}, {"K": K2.astype(np.float64).tolist()}]
    t = cameras.camera_table(recs, K0.astype(np.float64))
    assert t.shape == (4, 3, 3) and t.dtype == np.float32 and t.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(t, np.stack([K1, K0, K0, K2]))
    assert cameras.has_cameras(recs) and not cameras.has_cameras([{}, {"K": None}])
    # a transposed view comes back contiguous
    v = cameras.validate_cameras(np.stack([K0.T, K1.T]).transpose(0, 2, 1))
    assert v.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(v, np.stack([K0, K1]))


@pytest.mark.parametrize("bad, word", [("nan", "finite"), ("inf", "finite"), ("k22", r"K\[2,2\]"), ("singular", "singular")])
def test_validation_errors(bad, word):
    K = K1.copy()
    if bad == "nan":
        K[0, 2] = np.nan
    elif bad == "inf":
        K[1, 1] = np.inf
    elif bad == "k22":
        K[2, 2] = 0
    else:                                   # K[2,2] stays 1: only the determinant is zero
        K = np.array([[500, 3, 0], [1000, 6, 0], [0, 0, 1]], np.float32)
    with pytest.raises(ValueError, match=word):
        cameras.validate_cameras(np.stack([K0, K]))
    with pytest.raises(ValueError, match="camera 1 .*" + word):
        cameras.camera_table([{}, {"K": K}], K0)
    with pytest.raises(ValueError, match="shape"):
        cameras.validate_cameras(K0)


def test_sidecar_is_written_only_when_cameras_were_used_and_loaded_with_the_cache(tmp_path):
    path = str(tmp_path / "imdb_pose_iter2.pkl")
    side = tester.camera_cache_file(path)
    assert side == str(tmp_path / "imdb_pose_iter2_K.pkl")
    four = [np.zeros((1, 2, 1)), np.ones((1, 2, 1)), [[[np.eye(3, 4)], [np.eye(3, 4)]]], [[[np.eye(3, 4)], [np.eye(3, 4)]]]]
    tester.save_result_cache(path, four)
    assert os.path.exists(path) and not os.path.exists(side)
    got, all_K = tester.load_result_cache(path)
    assert all_K is None and len(got) == 4
    tester.save_result_cache(path, four, all_K=[[K1]])
    assert os.path.exists(side)
    with open(path, "rb") as f:
        assert len(pickle.load(f, encoding="latin1")) == 4          # the cache keeps the reference's four containers
    got, all_K = tester.load_result_cache(path)
    np.testing.assert_array_equal(all_K[0][0], K1)
    np.testing.assert_array_equal(got[2][0][1][0], np.eye(3, 4))
    tester.save_result_cache(path, four)                            # a run without cameras leaves no stale sidecar behind
    assert not os.path.exists(side) and tester.load_result_cache(path)[1] is None


class _Recorder(LM6D_REFINE):
    """pose_metrics with the device call replaced: records (class, n, K) and answers with re = 120° on chosen rows"""

    def __init__(self, classes, flip_rows):
        LM6D_REFINE.__init__(self, classes, {c: np.zeros((4, 3), np.float32) for c in classes}, {c: 0.1 for c in classes})
        self.calls, self.flip_rows = [], flip_rows

    def _device_metrics(self, cls_name, est, gt, K):
        self.calls.append((cls_name, len(est), np.array(K, np.float32)))
        m = np.zeros((len(est), 5))
        if len(est) == 6:                    # the first pass over iterations x poses
            m[self.flip_rows.get(cls_name, []), 0] = 120.0
            m[:, 4] = np.arange(6)
        else:                                # the re-evaluation of the flipped rows
            m[:, 4] = 100 + np.arange(len(est))
        return m


def test_pose_metrics_stacks_the_cameras_over_iterations_and_the_flip_subset():
    cfg = default_config()
    cfg.TEST.test_iter = 2
    classes = ["ape", "eggbox"]
    n = 3
    est = [[[np.eye(3, 4, dtype=np.float32)] * n for _ in range(2)] for _ in classes]
    gt = [[[np.eye(3, 4, dtype=np.float32)] * n for _ in range(2)] for _ in classes]
    all_K = [[K0, K1, K2], [K2, K0, K1]]
    ds = _Recorder(classes, {"eggbox": [1, 5]})                      # iteration 0 pose 1 and iteration 1 pose 2
    res = ds.pose_metrics(cfg, est, gt, all_K)
    assert [(c[0], c[1]) for c in ds.calls] == [("ape", 6), ("eggbox", 6), ("eggbox", 2)]
    np.testing.assert_array_equal(ds.calls[0][2], np.stack([K0, K1, K2, K0, K1, K2]))       # tiled as gt is
    np.testing.assert_array_equal(ds.calls[1][2], np.stack([K2, K0, K1, K2, K0, K1]))
    np.testing.assert_array_equal(ds.calls[2][2], np.stack([K0, K1]))                        # the flipped rows' cameras
    assert res["eggbox"].shape == (2, n, 4)
    np.testing.assert_array_equal(res["eggbox"][:, :, 3], [[0, 100, 2], [3, 4, 101]])       # re-evaluated rows replaced
    # without all_K: the config camera, once, for every call — as before
    ds = _Recorder(classes, {"eggbox": [1, 5]})
    ds.pose_metrics(cfg, est, gt)
    for c in ds.calls:
        np.testing.assert_array_equal(c[2], np.asarray(cfg.dataset.INTRINSIC_MATRIX, np.float32).reshape(3, 3))
    with pytest.raises(ValueError, match="cameras for"):
        _Recorder(classes, {}).pose_metrics(cfg, est, gt, [[K0], [K0, K1, K2]])
