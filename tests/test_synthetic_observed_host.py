"""Host checks of the synthetic observed frames (no GPU): the numpy emulation of the observed-pose rule and the light draws
(tests/observed_pose_emulation.py) against the reference-run golden file (tests/golden/observed_pose_golden.npz, made by
tests/golden/make_observed_pose_golden.py), lib/pair_matching/pose_sampler.observed_pose_stats against the golden stat_poses
values, the premises of the GPU scenario, and core/loader.epoch_plan with synthetic pairs."""
import os

import numpy as np
import pytest

import observed_pose_emulation as oemu
from mx_deepim_amd.core.loader import epoch_plan
from mx_deepim_amd.lib.pair_matching.pose_sampler import (BRIGHTNESS_RATIOS, OBSERVED_TABLE_COLUMNS, observed_pose_stats,
                                                          pack_observed_table)
from mx_deepim_amd.lib.utils.synthetic_observed import runs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observed_pose_golden.npz")


def test_emulation_matches_the_reference_run_golden():
    g = np.load(GOLDEN)
    n = len(g["cls"])
    assert n >= 220 and set(g["tag"].tolist()) == {"random", "angle_max", "border", "behind"}
    W, H, border = int(g["width"]), int(g["height"]), float(g["border"])
    worst_rot = worst_deg = 0.0
    for i in range(n):
        pose, deg, cx, cy, ok = oemu.candidate(g["table"][g["cls"][i]], g["normals"][i], g["K"], W, H, border)
        want = g["pose"][i]
        assert ok == bool(g["accept"][i]), (i, g["tag"][i])
        worst_rot = max(worst_rot, np.abs(pose[:, :3] - want[:, :3]).max())
        assert (np.abs(pose[:, 3] - want[:, 3]) <= 2.4e-7 * np.abs(want[:, 3])).all(), i
        worst_deg = max(worst_deg, abs(deg - g["deg"][i]))
        assert abs(cx - g["cx"][i]) <= 1e-9 * abs(g["cx"][i]) and abs(cy - g["cy"][i]) <= 1e-9 * abs(g["cy"][i]), i
    print("rotation %.3e (2.4e-7), deg %.3e (1e-5)" % (worst_rot, worst_deg))
    assert worst_rot <= 2.4e-7 and worst_deg <= 1e-5           # the bars of test_gpu_pose_sampler.py:72-73
    behind = g["tag"] == "behind"
    assert g["accept_toolkit"][behind].all() and not g["accept"][behind].any()      # the z > 0 clause is ours


def test_observed_pose_stats_equal_the_golden_stat_poses():
    g = np.load(GOLDEN)
    stats = observed_pose_stats({c: g["train_poses"][c] for c in (0, 1)})
    for c in (0, 1):
        s = stats[c]
        for key in ("trans_mean", "trans_std", "pz_mean"):
            assert np.abs(s[key] - g[key][c]).max() <= 1e-12, key
        assert abs(s["angle_max"] - g["angle_max"][c]) <= 1e-12
        np.testing.assert_array_equal(s["fallback"], g["train_poses"][c][g["closest"][c]])
    table = pack_observed_table(stats)
    assert table.shape == (2, OBSERVED_TABLE_COLUMNS) and table.dtype == np.float64
    assert np.abs(table - g["table"]).max() <= 1e-12
    np.testing.assert_array_equal(table[:, 10:], g["table"][:, 10:])
    # np.std is the population's
    assert np.abs(stats[0]["trans_std"] - g["train_poses"][0][:, :, 3].std(0, ddof=0)).max() <= 1e-15
    # a class without statistics: every candidate rejected, a zero fallback
    sparse = pack_observed_table({1: stats[1]}, n_classes=3)
    assert sparse[0, 9] == -1 and sparse[2, 9] == -1 and not sparse[0, 10:].any() and np.array_equal(sparse[1], table[1])
    with pytest.raises(ValueError):
        pack_observed_table({3: stats[1]}, n_classes=3)
    with pytest.raises(ValueError):
        observed_pose_stats({0: np.zeros((0, 3, 4))})
    # the emulation's own statistics agree (summation order apart)
    assert np.abs(oemu.observed_pose_stats(g["train_poses"][0]) - table[0]).max() <= 1e-12


def test_premises_of_the_gpu_scenario():
    s = oemu.block_scenario()
    a = s["attempts"]
    assert len(a) == 257 and set(np.unique(s["cls"])) == {0, 1}
    assert (a > 1).mean() >= 0.3 and (a >= 1).all()            # the rule rejects often, nobody exhausts 100 attempts
    assert s["borderline"].mean() <= 0.01                       # the seed's own share of pairs near a threshold
    first = np.array([oemu.candidate(s["table"][c], z, oemu.K_SMALL, 64, 48, oemu.SCENARIO_BORDER)[4]
                      for c, z in zip(s["cls"], oemu.normals7(oemu.SCENARIO_SEED, s["ids"], 0))])
    for c in (0, 1):
        assert 0.15 <= first[s["cls"] == c].mean() <= 0.45, c   # 20-40 % pass the angle rule; the border takes a little more
    np.testing.assert_array_equal(first, a == 1)
    assert (s["stat"][:, 3] == 1).all() and (s["stat"][:, 0] <= s["table"][s["cls"], 9]).all()
    assert np.abs(np.linalg.det(s["pose"][:, :, :3].astype(np.float64)) - 1).max() <= 1e-6


def test_emulated_bounds():
    table = oemu.class_table(angle_max=(0.0, 0.0))
    cls = np.array([0, 1, -1, 2, 1], np.int32)
    pose, attempts, zs, stat, _b = oemu.sample(cls, table, oemu.K_SMALL, 64, 48, 4.8, 1, 3, np.arange(5))
    assert attempts.tolist() == [0, 0, -1, -1, 0] and not zs.any() and not stat.any()
    np.testing.assert_array_equal(pose[[0, 1, 4]].reshape(3, 12), table[[0, 1, 1], 10:].astype(np.float32))
    assert not pose[[2, 3]].any()


def test_light_draws_cover_every_choice_and_are_a_pure_function_of_seed_and_id():
    ids = (1 << 33) + np.arange(4096, dtype=np.uint64)
    off, inten, ratio, (pos, colour, k) = oemu.lights(7, ids)
    assert off.dtype == inten.dtype == ratio.dtype == np.float32
    assert sorted(set(pos.tolist())) == list(range(6)) and sorted(set(colour.tolist())) == list(range(7))
    assert sorted(set(k.tolist())) == list(range(5))
    assert sorted(set(ratio.tolist())) == sorted(np.asarray(BRIGHTNESS_RATIOS, np.float32).tolist())
    np.testing.assert_array_equal(off, (0.5 * oemu.LIGHT_POSITIONS[(ids % np.uint64(6)).astype(int)]).astype(np.float32))
    on = oemu.LIGHT_COLORS[colour] != 0
    assert (inten[~on] == 0).all() and (inten[on] >= np.float32(0.9)).all() and (inten[on] <= np.float32(1.1)).all()
    assert np.abs(np.bincount(colour, minlength=7) - 4096 / 7).max() <= 5 * np.sqrt(4096 * 6 / 49)
    assert np.abs(np.bincount(k, minlength=5) - 4096 / 5).max() <= 5 * np.sqrt(4096 * 4 / 25)
    # a pure function of (seed, id): any subset, any order, alone
    perm = np.random.default_rng(1).permutation(4096)[:300]
    again = oemu.lights(7, ids[perm])
    for a, b in zip(again[:3], (off, inten, ratio)):
        np.testing.assert_array_equal(a.view(np.uint32), b[perm].view(np.uint32))
    one = oemu.lights(7, ids[17:18])
    np.testing.assert_array_equal(one[1], inten[17:18])
    other = oemu.lights(8, ids)
    assert not np.array_equal(other[1], inten) and np.array_equal(other[0], off)         # the position is the id's alone
    three = oemu.lights(7, ids[:64], ratios=(0.1, 0.5, 0.9))
    assert set(three[2].tolist()) <= set(np.asarray((0.1, 0.5, 0.9), np.float32).tolist())


def test_epoch_plan_with_synthetic_pairs():
    M, R, BS, S = 5, 3, 4, 5
    for shuffle in (False, True):
        for epoch in (0, 1, 4):
            want = epoch_plan(M, R, BS, shuffle, np.random.RandomState(3), epoch)
            for got in (epoch_plan(M, R, BS, shuffle, np.random.RandomState(3), epoch, 0),
                        epoch_plan(M, R, BS, shuffle, np.random.RandomState(3), epoch, num_synthetic=0)):
                assert got[2] == want[2]
                for a, b in zip(got[:2], want[:2]):
                    assert a.dtype == b.dtype and np.array_equal(a, b)
    pairs, ids, dropped = epoch_plan(M, R, BS, False, np.random.RandomState(3), 2, S)
    assert pairs.shape == (5, 4) and dropped == 0 and ids.dtype == np.uint64
    np.testing.assert_array_equal(pairs.reshape(-1), np.arange(20))
    np.testing.assert_array_equal(ids, (pairs + 2 * 20).astype(np.uint64))
    assert (pairs >= M * R).sum() == S                           # pairs 15..19 are the synthetic ones
    pairs, ids, dropped = epoch_plan(M, R, BS, True, np.random.RandomState(3), 1, S + 2)
    assert pairs.shape == (5, 4) and dropped == 2
    flat = pairs.reshape(-1)
    assert len(set(flat.tolist())) == 20 and flat.max() < 22 and sorted(flat.tolist()) != flat.tolist()
    np.testing.assert_array_equal(ids, (pairs + 22).astype(np.uint64))
    assert 3 <= (flat >= M * R).sum() <= 7
    np.testing.assert_array_equal(flat, np.random.RandomState(3).permutation(22)[:20])
    with pytest.raises(ValueError):
        epoch_plan(M, R, BS, False, np.random.RandomState(3), 0, -1)


def test_runs_of_destination_rows():
    assert runs([]) == []
    assert runs([3]) == [(0, 1, 3)]
    assert runs([1, 2, 3, 7, 0, 1]) == [(0, 3, 1), (3, 4, 7), (4, 6, 0)]
