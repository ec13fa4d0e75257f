"""Host checks of the occluded synthetic scenes (no GPU): the properties of the numpy emulation of deepim_sample_occluders
(tests/occluder_emulation.py) and every refusal of lib/utils/synthetic_observed.OccluderSpec."""
import numpy as np
import pytest

import occluder_emulation as occ
import pose_sampler_emulation as emu
from mx_deepim_amd.lib.pair_matching.pose_sampler import MAX_SLOTS
from mx_deepim_amd.lib.utils.synthetic_observed import OccluderSpec

SEED, B = 404, 96
DIAMETERS = np.array([0.10, 0.12], np.float32)


def _targets(n=B):
    rng = np.random.default_rng(8)
    pose = emu.random_poses(rng, n, 0.5, 0.7)
    return (np.arange(n) % 2).astype(np.int32), pose


def _draw(ids, cls, pose, **kw):
    return occ.occluders(SEED, ids, cls, pose, [0, 1], DIAMETERS, **kw)


def test_counts_slots_and_targets():
    cls_t, pose_t = _targets()
    ids = 1000 + np.arange(B, dtype=np.uint64)
    cls, pose, label, n = _draw(ids, cls_t, pose_t, min_occluders=1, max_occluders=3)
    assert cls.shape == (B, 4) and pose.shape == (B, 4, 3, 4) and cls.dtype == np.int32 and pose.dtype == np.float32
    assert n.min() == 1 and n.max() == 3 and set(n.tolist()) == {1, 2, 3}            # uniform over [min, max], all values seen
    np.testing.assert_array_equal(cls[:, 0], cls_t)                                   # slot 0 is the target, copied through
    np.testing.assert_array_equal(pose[:, 0].view(np.uint32), pose_t.view(np.uint32))
    np.testing.assert_array_equal(label, np.tile([1, 2, 3, 4], (B, 1)))
    for b in range(B):
        for s in range(1, 4):
            if s > n[b]:
                assert cls[b, s] == -1 and not pose[b, s].any()                       # slots beyond n are empty
            else:
                assert cls[b, s] in (0, 1)
                R, t = pose[b, s, :, :3].astype(np.float64), pose[b, s, :, 3].astype(np.float64)
                assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
                d = float(DIAMETERS[cls_t[b]])
                off = t - pose_t[b, :, 3]
                rho, tau = np.hypot(off[0], off[1]) / d, -off[2] / d
                assert 0.2 - 1e-5 <= rho <= 0.9 + 1e-5 and 0.5 - 1e-5 <= tau <= 1.5 + 1e-5
    assert ((cls[:, 1:] == 0).any() and (cls[:, 1:] == 1).any())
    assert (cls[:, 1:] == cls[:, :1]).any()                                           # an occluder may be of the target's class


def test_outputs_depend_on_seed_and_draw_id_alone():
    cls_t, pose_t = _targets()
    ids = (1 << 33) + np.arange(B, dtype=np.uint64)          # ids beyond 32 bits: the high counter word is used
    whole = _draw(ids, cls_t, pose_t)
    perm = np.random.default_rng(2).permutation(B)
    permuted = _draw(ids[perm], cls_t[perm], pose_t[perm])
    halves = [_draw(ids[i:i + B // 2], cls_t[i:i + B // 2], pose_t[i:i + B // 2]) for i in (0, B // 2)]
    for k in range(4):
        np.testing.assert_array_equal(permuted[k], whole[k][perm])
        np.testing.assert_array_equal(np.concatenate([halves[0][k], halves[1][k]]), whole[k])
    other = occ.occluders(SEED + 1, ids, cls_t, pose_t, [0, 1], DIAMETERS)
    assert not np.array_equal(other[1], whole[1])
    low = _draw(ids & np.uint64(0xFFFFFFFF), cls_t, pose_t)
    assert not np.array_equal(low[1], whole[1])


def test_an_occluder_behind_the_camera_is_an_empty_slot():
    cls_t, pose_t = _targets(32)
    pose_t[:, 2, 3] = 0.05                                   # 5 cm from the camera: d tau >= 0.05 pushes every occluder behind it
    cls, pose, _label, n = _draw(np.arange(32, dtype=np.uint64), cls_t, pose_t, min_occluders=2, max_occluders=2)
    assert (n == 2).all() and (cls[:, 1:] == -1).all() and not pose[:, 1:].any()


def test_no_occluders_means_one_slot_and_no_draw(monkeypatch):
    calls = []
    real = emu.draw
    monkeypatch.setattr(emu, "draw", lambda seed, ids, attempt, stream: (calls.append((attempt, stream)), real(seed, ids, attempt, stream))[1])
    cls_t, pose_t = _targets(8)
    cls, pose, label, n = _draw(np.arange(8, dtype=np.uint64), cls_t, pose_t, max_occluders=0)
    assert cls.shape == (8, 1) and pose.shape == (8, 1, 3, 4) and label.tolist() == [[1]] * 8 and not n.any()
    assert calls == []
    _draw(np.arange(8, dtype=np.uint64), cls_t, pose_t, min_occluders=1, max_occluders=1)
    assert set(calls) == {(0, 7), (1, 7), (1, 8)}            # the count, then slot 1's placement and rotation blocks


def test_occluder_spec_defaults():
    s = OccluderSpec([0, 1], {0: 0.1, 1: 0.12})
    assert (s.max_occluders, s.min_occluders, s.lateral, s.toward, s.min_visible, s.slots) == (2, 0, (0.2, 0.9), (0.5, 1.5), 0.4, 3)
    np.testing.assert_array_equal(s.diameter_table(3), np.array([0.1, 0.12, 0.0], np.float32))
    assert OccluderSpec([1], [0.1, 0.2]).diameters == {0: 0.1, 1: 0.2}               # a sequence indexed by class id
    assert OccluderSpec([0], {0: 0.1}, max_occluders=MAX_SLOTS - 1).slots == MAX_SLOTS == 8
    assert OccluderSpec([], {}, max_occluders=0).slots == 1                          # nothing to draw from, nothing drawn


@pytest.mark.parametrize("kw,err,match", [
    (dict(max_occluders=8), ValueError, "at most 8"),
    (dict(max_occluders=-1), ValueError, "min_occluders <= max_occluders"),
    (dict(min_occluders=3), ValueError, "min_occluders <= max_occluders"),
    (dict(min_occluders=-1), ValueError, "min_occluders <= max_occluders"),
    (dict(max_occluders=1.5), ValueError, "whole numbers"),
    (dict(classes=[]), ValueError, "classes is empty"),
    (dict(classes=[0, -1]), ValueError, "class ids >= 0"),
    (dict(classes=[0, 2]), KeyError, "no diameter"),
    (dict(diameters={0: 0.1, 1: 0.0}), ValueError, "positive length"),
    (dict(diameters={0: 0.1, 1: float("nan")}), ValueError, "positive length"),
    (dict(lateral=(0.9, 0.2)), ValueError, "lateral"),
    (dict(lateral=(-0.1, 0.2)), ValueError, "lateral"),
    (dict(lateral=0.5), ValueError, "lateral"),
    (dict(toward=(1.5, 0.5)), ValueError, "toward"),
    (dict(toward=(0.5, float("inf"))), ValueError, "toward"),
    (dict(min_visible=1.1), ValueError, "min_visible"),
    (dict(min_visible=-0.1), ValueError, "min_visible"),
    (dict(min_visible=float("nan")), ValueError, "min_visible"),
])
def test_occluder_spec_refusals(kw, err, match):
    args = dict(classes=[0, 1], diameters={0: 0.1, 1: 0.12})
    args.update(kw)
    with pytest.raises(err, match=match):
        OccluderSpec(**args)
