"""Host checks of the device loader's random draws (no GPU): the numpy emulation of csrc/sample.hip
(tests/pose_sampler_emulation.py) against Philox4x32-10's known answers and against the reference-run golden file
(tests/golden/pose_sampler_golden.npz, made by tests/golden/make_pose_sampler_golden.py), the mask-dilate table against
lib/utils/mask_dilate.mask_dilate_draws, and the epoch factoring of core/loader.epoch_plan."""
import os

import numpy as np
import pytest

import pose_sampler_emulation as emu
from mx_deepim_amd.core.loader import epoch_plan
from mx_deepim_amd.lib.pair_matching.pose_sampler import POSE_NOISE_DEFAULTS, noise_array, pose_noise
from mx_deepim_amd.lib.utils import mask_dilate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_sampler_golden.npz")


def test_philox_known_answers():
    for ctr, key, want in emu.KNOWN_ANSWERS:
        got = emu.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert [int(v) for v in got] == list(want), [hex(int(v)) for v in got]
    # vectorised over a batch, and draw() lays the counter out as (id lo, id hi, attempt, stream), the key as (seed lo, seed hi)
    got = emu.philox4x32_10(np.array([k[0] for k in emu.KNOWN_ANSWERS], np.uint64), np.array([k[1] for k in emu.KNOWN_ANSWERS], np.uint64))
    assert got.tolist() == [list(k[2]) for k in emu.KNOWN_ANSWERS]
    pi = emu.KNOWN_ANSWERS[2]
    got = emu.draw(pi[1][0] | (pi[1][1] << 32), [pi[0][0] | (pi[0][1] << 32)], pi[0][2], pi[0][3])
    assert got[0].tolist() == list(pi[2])


def test_uniforms_are_strictly_inside_the_unit_interval():
    u = emu.uniform(np.array([0, 1, 0xFFFFFFFF], np.uint32))
    assert u[0] == 2.0 ** -33 and u[2] == 1.0 - 2.0 ** -33 and 0 < u.min() and u.max() < 1
    z0, z1 = emu.box_muller(np.array([0], np.uint32), np.array([0], np.uint32))
    assert np.isfinite(z0).all() and np.isfinite(z1).all() and abs(z0[0]) < 6.8        # the largest |z| a word pair can give


def test_emulation_matches_the_reference_run_golden():
    g = np.load(GOLDEN)
    n = len(g["src"])
    assert n >= 220 and float(g["rdist_formula_gap"]) <= 1e-6
    tags = set(g["tag"].tolist())
    assert tags == {"random", "gimbal", "identity", "angle_max", "border", "behind"}
    W, H, border = int(g["width"]), int(g["height"]), float(g["border"])
    worst_pose = worst_r = 0.0
    for i in range(n):
        pose, r_dist, cx, cy, ok = emu.perturb(g["src"][i], g["normals"][i], g["K"], g["noise"][g["cfg"][i]], W, H, border)
        worst_pose = max(worst_pose, np.abs(pose - g["pose"][i]).max())
        worst_r = max(worst_r, abs(r_dist - g["r_dist"][i]))
        assert ok == bool(g["accept"][i]), (i, g["tag"][i])
        assert abs(cx - g["cx"][i]) <= 1e-9 * abs(g["cx"][i]) and abs(cy - g["cy"][i]) <= 1e-9 * abs(g["cy"][i]), i
    print("pose %.3e (bar 1e-12), r_dist %.3e deg (bar 1e-5)" % (worst_pose, worst_r))
    assert worst_pose <= 1e-12         # both sides are float64
    assert worst_r <= 1e-5             # ten times the gap the generator asserts between the two angle formulas
    behind = g["tag"] == "behind"
    assert g["accept_toolkit"][behind].all() and not g["accept"][behind].any()       # the z > 0 clause is ours
    assert np.array_equal(g["accept"][~behind], g["accept_toolkit"][~behind])


class _Stub(object):
    """np.random stand-in: the first randint(10) of a call gives the direction, every thickness draw gives max - 1."""

    def __init__(self, direction):
        self.direction, self.calls = direction, 0

    def randint(self, n):
        self.calls += 1
        return self.direction if self.calls == 1 else n - 1


def test_mask_dilate_table_matches_the_host_draws():
    assert emu.SKIPPED == mask_dilate._SKIPPED
    seen = set()
    ids = np.arange(400, dtype=np.uint64)
    thick, direction = emu.mask_dilate(11, ids, 10)
    assert thick.min() >= 0 and thick.max() <= 10
    for d in range(10):
        want = mask_dilate.mask_dilate_draws(1, 10, rng=_Stub(d))[0] > 0
        rows = np.nonzero(direction == d)[0]
        assert rows.size > 0
        for r in rows:
            assert np.array_equal(thick[r] > 0, want), (d, thick[r])
        seen.add(d)
    assert seen == set(range(10))
    # max_thickness = 1: every enabled side is 1
    t1, _ = emu.mask_dilate(11, ids, 1)
    assert set(np.unique(t1)) <= {0, 1} and np.array_equal(t1 > 0, thick > 0)


def test_attempt_loop_bounds():
    rng = np.random.default_rng(5)
    src = emu.random_poses(rng, 8)
    ids = np.arange(8)
    noise = emu.TOOLKIT_NOISE.copy()
    noise[1] = 0.0            # angle_max 0: nothing is accepted
    out, attempts, zs, _ = emu.sample(src, emu.LM_K, noise, 640, 480, 16.0, 3, 1, ids)
    assert (attempts == 0).all() and np.array_equal(out, src) and not zs.any()
    noise[1] = 180.0
    out, attempts, zs, _ = emu.sample(src, emu.LM_K, noise, 640, 480, -1e9, 1, 1, ids)
    assert (attempts == 1).all() and np.array_equal(zs, emu.normals(1, ids, 0))


def test_premises_of_the_gpu_scenarios():
    """What tests/test_gpu_pose_sampler.py takes for granted about its fixed seeds, checked on the emulation alone."""
    s = emu.rejection_scenario()
    a = s["attempts"]
    print("rejection scenario: %.0f %% of pairs retry, mean %.2f attempts, max %d, exhausted %d, borderline %d"
          % (100 * (a > 1).mean(), a.mean(), a.max(), (a == 0).sum(), s["borderline"].sum()))
    assert not s["borderline"].any() and (a >= 1).all() and (a > 1).mean() >= 0.3
    mean, std, rho = emu.normal_statistics(emu.stat_normals())
    print("normals of seed %d: |mean| %.4f, |std - 1| %.4f, |rho| %.4f" % (emu.STAT_SEED, mean, std, rho))
    assert mean <= 5 / np.sqrt(4096) and std <= 5 / np.sqrt(8192) and rho <= 5 / np.sqrt(4096)
    assert np.abs(emu.stat_normals()).max() <= 6.8


def test_pose_noise_defaults_are_the_toolkit_constants():
    assert POSE_NOISE_DEFAULTS == {"angle_std": 15.0, "angle_max": 45.0, "x_std": 0.01, "y_std": 0.01, "z_std": 0.05,
                                   "border": 16.0, "max_attempts": 100}
    assert np.array_equal(noise_array(pose_noise()), emu.TOOLKIT_NOISE)
    assert pose_noise({"angle_max": 20.0})["angle_max"] == 20.0 and POSE_NOISE_DEFAULTS["angle_max"] == 45.0
    with pytest.raises(ValueError, match="unknown"):
        pose_noise({"angle": 1.0})


def test_epoch_plan():
    M, R, bs = 5, 3, 4
    pairs, ids, dropped = epoch_plan(M, R, bs, False, np.random.RandomState(0), 0)
    assert pairs.shape == (3, 4) and dropped == 3 and pairs.reshape(-1).tolist() == list(range(12))
    assert ids.dtype == np.uint64 and np.array_equal(ids, pairs.astype(np.uint64))
    pairs2, ids2, _ = epoch_plan(M, R, bs, False, np.random.RandomState(0), 2)
    assert np.array_equal(pairs2, pairs) and np.array_equal(ids2, pairs.astype(np.uint64) + 2 * 15)
    # shuffle: a permutation's head, the id follows the pair, the same seed gives the same order, successive epochs differ
    a, b = np.random.RandomState(7), np.random.RandomState(7)
    p0, i0, d0 = epoch_plan(M, R, bs, True, a, 0)
    q0, j0, _ = epoch_plan(M, R, bs, True, b, 0)
    assert np.array_equal(p0, q0) and np.array_equal(i0, j0) and d0 == 3
    assert len(set(p0.reshape(-1).tolist())) == 12 and p0.min() >= 0 and p0.max() < 15
    assert np.array_equal(i0, p0.astype(np.uint64))
    p1, i1, _ = epoch_plan(M, R, bs, True, a, 1)
    assert not np.array_equal(p1, p0) and np.array_equal(i1, p1.astype(np.uint64) + 15)
    assert not np.array_equal(p0, np.arange(12).reshape(3, 4))
    # an exact multiple drops nothing; a batch larger than the epoch gives no batch
    assert epoch_plan(4, 2, 4, False, None, 0)[2] == 0 and epoch_plan(4, 2, 4, False, None, 0)[0].shape == (2, 4)
    assert epoch_plan(1, 3, 4, False, None, 0)[0].shape == (0, 4)
    with pytest.raises(ValueError):
        epoch_plan(0, 1, 1, False, None, 0)
