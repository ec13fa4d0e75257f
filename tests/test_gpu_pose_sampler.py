"""csrc/sample.hip on the GPU against its numpy emulation (tests/pose_sampler_emulation.py) and the reference-run golden file
(tests/golden/pose_sampler_golden.npz): the generator bit for bit, the rendered-pose rule, the bounded attempt loop, placement
invariance of a pair's draw, the bounds, the statistics of the normals and the mask-dilate draws."""
import ctypes
import os

import numpy as np
import pytest

import pose_sampler_emulation as emu
from mx_deepim_amd.lib.pair_matching.pose_sampler import sample_rendered_poses
from mx_deepim_amd.lib.utils.mask_dilate import mask_dilate_draws_device
from mx_deepim_amd.runtime import lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_sampler_golden.npz")
W, H = 640, 480
FAR = -1e9          # a border no centre reaches


def _perturb(ctx, src, normals, K, noise, border=16.0, width=W, height=H):
    B = len(src)
    pose, stat = ctx.empty((B, 3, 4)), ctx.empty((B, 4), np.float64)
    lib.deepim_pose_perturb(ctx.handle, pose, stat, ctx.array(src), ctx.array(normals, dtype=np.float64),
                            np.ascontiguousarray(K, np.float32), np.ascontiguousarray(noise, np.float32), width, height,
                            ctypes.c_float(border), B)
    return pose.asnumpy(), stat.asnumpy()


def _sample(ctx, src, noise, max_attempts, seed, draw_base=0, draw_ids=None, border=16.0, K=emu.LM_K):
    """deepim_sample_rendered_poses -> (pose, attempts, normals) on the host."""
    B = len(src)
    pose, attempts, normals = ctx.empty((B, 3, 4)), ctx.empty((B,), np.int32), ctx.empty((B, 6), np.float64)
    ids = None if draw_ids is None else ctx.array(draw_ids, dtype=np.uint64)
    lib.deepim_sample_rendered_poses(ctx.handle, pose, attempts, normals, ctx.array(src), np.ascontiguousarray(K, np.float32),
                                     np.ascontiguousarray(noise, np.float32), W, H, ctypes.c_float(border), max_attempts,
                                     ctypes.c_ulonglong(seed), ctypes.c_ulonglong(draw_base), ids, B)
    return pose.asnumpy(), attempts.asnumpy(), normals.asnumpy()


def _noise(angle_max):
    n = emu.TOOLKIT_NOISE.copy()
    n[1] = angle_max
    return n


def test_philox_is_bit_equal_to_the_emulation(ctx):
    rng = np.random.default_rng(1)
    ctr = np.concatenate([np.array([k[0] for k in emu.KNOWN_ANSWERS], np.uint32), rng.integers(0, 2 ** 32, (1024, 4), dtype=np.uint32)])
    key = np.concatenate([np.array([k[1] for k in emu.KNOWN_ANSWERS], np.uint32), rng.integers(0, 2 ** 32, (1024, 2), dtype=np.uint32)])
    out = ctx.empty((len(ctr), 4), np.uint32)
    lib.deepim_selfcheck_philox(ctx.handle, out, ctx.array(ctr, dtype=np.uint32), ctx.array(key, dtype=np.uint32), len(ctr))
    got = out.asnumpy()
    assert got[:3].tolist() == [list(k[2]) for k in emu.KNOWN_ANSWERS]
    np.testing.assert_array_equal(got, emu.philox4x32_10(ctr, key))


def test_perturb_matches_the_reference_run_golden(ctx):
    g = np.load(GOLDEN)
    for cfg in (0, 1):
        sel = g["cfg"] == cfg
        pose, stat = _perturb(ctx, g["src"][sel], g["normals"][sel], g["K"], g["noise"][cfg], float(g["border"]), int(g["width"]),
                              int(g["height"]))
        want = g["pose"][sel]
        rot = np.abs(pose[:, :, :3] - want[:, :, :3]).max()
        dt, at = np.abs(pose[:, :, 3] - want[:, :, 3]), np.abs(want[:, :, 3])
        tr = (dt[at > 0] / at[at > 0]).max()
        rd = np.abs(stat[:, 0] - g["r_dist"][sel]).max()
        cxy = max((np.abs(stat[:, 1] - g["cx"][sel]) / np.abs(g["cx"][sel])).max(), (np.abs(stat[:, 2] - g["cy"][sel]) / np.abs(g["cy"][sel])).max())
        print("angle_max %g: rotation %.3e (2.4e-7), translation rel %.3e (2.4e-7), r_dist %.3e deg (1e-5), centre rel %.3e (1e-9)"
              % (g["noise"][cfg][1], rot, tr, rd, cxy))
        assert rot <= 2.4e-7 and (dt <= 2.4e-7 * at).all()        # two float32 roundings of a double result; an exact 0 stays 0
        assert rd <= 1e-5 and cxy <= 1e-9
        np.testing.assert_array_equal(stat[:, 3] != 0, g["accept"][sel])
        assert set(np.unique(stat[:, 3])) <= {0.0, 1.0}


def test_sampler_across_a_block_matches_the_emulation(ctx):
    B, seed, base = 257, 91, 5
    src = emu.random_poses(np.random.default_rng(12), B)
    noise = _noise(45.0)
    pose, attempts, normals = _sample(ctx, src, noise, 100, seed, draw_base=base)
    want_pose, want_attempts, want_z, borderline = emu.sample(src, emu.LM_K, noise, W, H, 16.0, 100, seed, base + np.arange(B))
    assert not borderline.any()
    np.testing.assert_array_equal(attempts, want_attempts)
    print("normals: %.3e from the emulation (bar 1e-12)" % np.abs(normals - want_z).max())
    assert np.abs(normals - want_z).max() <= 1e-12
    again, stat = _perturb(ctx, src, normals, emu.LM_K, noise)
    np.testing.assert_array_equal(pose.view(np.uint32), again.view(np.uint32))
    assert (stat[:, 3] == 1).all() and (attempts >= 1).all()
    assert np.abs(pose - want_pose).max() <= 2.4e-7 * max(1.0, np.abs(want_pose).max())


def test_many_rejections_follow_the_emulated_replay(ctx):
    s = emu.rejection_scenario()
    pose, attempts, _z = _sample(ctx, s["src"], s["noise"], s["max_attempts"], s["seed"], draw_ids=s["ids"])
    keep = ~s["borderline"]
    assert (~keep).mean() <= 0.01
    print("%.0f %% of pairs retried, mean %.2f attempts, max %d" % (100 * (attempts > 1).mean(), attempts.mean(), attempts.max()))
    np.testing.assert_array_equal(attempts[keep], s["attempts"][keep])
    assert (attempts > 1).mean() >= 0.3             # a kernel that never retries cannot pass
    assert np.abs(pose[keep] - s["pose"][keep]).max() <= 2.4e-7 * max(1.0, np.abs(s["pose"]).max())


def test_a_pairs_draw_does_not_depend_on_its_placement(ctx):
    src = emu.random_poses(np.random.default_rng(31), 64)
    noise, seed, base = _noise(20.0), 5, 100
    whole = _sample(ctx, src, noise, 64, seed, draw_base=base)
    halves = [_sample(ctx, src[i:i + 32], noise, 64, seed, draw_base=base + i) for i in (0, 32)]
    perm = np.random.default_rng(2).permutation(64)
    permuted = _sample(ctx, src[perm], noise, 64, seed, draw_base=12345, draw_ids=base + perm)      # given ids: draw_base unused
    assert (whole[1] > 1).any()
    for k in range(3):
        np.testing.assert_array_equal(np.concatenate([halves[0][k], halves[1][k]]).view(np.uint8), whole[k].view(np.uint8))
        np.testing.assert_array_equal(permuted[k].view(np.uint8), whole[k][perm].view(np.uint8))


def test_bounds(ctx):
    src = emu.random_poses(np.random.default_rng(8), 70)
    pose, attempts, normals = _sample(ctx, src, _noise(0.0), 3, 1)
    assert (attempts == 0).all() and not normals.any()
    np.testing.assert_array_equal(pose.view(np.uint32), src.view(np.uint32))
    pose, attempts, _z = _sample(ctx, src, _noise(180.0), 1, 1, border=FAR)
    assert (attempts == 1).all() and not np.array_equal(pose, src)
    near = src.copy()
    near[:, :, 3] = [0.0, 0.0, 0.01]
    pose, attempts, _z = _sample(ctx, near, _noise(180.0), 100, 1, border=FAR)
    _p, want, _n, _b = emu.sample(near, emu.LM_K, _noise(180.0), W, H, FAR, 100, 1, np.arange(70))
    assert (pose[:, 2, 3] > 0).all() and (attempts > 1).any()         # only the z > 0 clause can reject here
    np.testing.assert_array_equal(attempts, want)
    with pytest.raises(RuntimeError, match="max_attempts"):
        _sample(ctx, src, _noise(45.0), 0, 1)
    with pytest.raises(RuntimeError, match="max_thickness"):
        mask_dilate_draws_device(ctx, 4, 1, max_thickness=0)
    bad = _noise(45.0)
    bad[4] = -0.05
    with pytest.raises(RuntimeError, match="standard deviations"):
        _sample(ctx, src, bad, 3, 1)
    assert _sample(ctx, src[:0], _noise(45.0), 3, 1)[0].shape == (0, 3, 4)


def test_statistics_of_the_normals(ctx):
    B = emu.STAT_B
    src = emu.random_poses(np.random.default_rng(3), B)
    _pose, attempts, z = _sample(ctx, src, _noise(180.0), 4, emu.STAT_SEED, border=FAR)
    assert (attempts == 1).all()
    assert np.abs(z - emu.stat_normals()).max() <= 1e-12
    mean, std, rho = emu.normal_statistics(z)
    print("|mean| %.4f (0.078), |std - 1| %.4f (0.055), |rho| %.4f (0.078)" % (mean, std, rho))
    assert mean <= 5 / np.sqrt(4096) and std <= 5 / np.sqrt(8192) and rho <= 5 / np.sqrt(4096)


def test_mask_dilate_draws(ctx):
    B, seed, base = 4096, 17, 1 << 33           # ids beyond 32 bits: the high counter word is used
    got = mask_dilate_draws_device(ctx, B, seed, draw_base=base).asnumpy()
    want, direction = emu.mask_dilate(seed, base + np.arange(B, dtype=np.uint64), 10)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32 and got.min() >= 0 and got.max() <= 10
    counts = np.bincount(direction, minlength=10)
    print("directions:", counts.tolist())
    assert len(counts) == 10 and np.abs(counts - 409.6).max() <= 5 * 19.2
    ids = np.random.default_rng(4).permutation(B).astype(np.uint64) + np.uint64(base)
    again = mask_dilate_draws_device(ctx, B, seed, draw_ids=ids).asnumpy()
    np.testing.assert_array_equal(again, want[(ids - np.uint64(base)).astype(np.int64)])
    np.testing.assert_array_equal(mask_dilate_draws_device(ctx, 64, seed, draw_base=base, max_thickness=3).asnumpy(),
                                  emu.mask_dilate(seed, base + np.arange(64, dtype=np.uint64), 3)[0])


def test_python_entry_returns_device_arrays(ctx):
    src = emu.random_poses(np.random.default_rng(12), 9)
    pose, attempts, normals = sample_rendered_poses(ctx.array(src), emu.LM_K, W, H, seed=91, draw_base=5, with_normals=True)
    want = _sample(ctx, src, _noise(45.0), 100, 91, draw_base=5)
    for got, w in zip((pose, attempts, normals), want):
        np.testing.assert_array_equal(got.asnumpy(), w)
    pose2, attempts2 = sample_rendered_poses(ctx.array(src), emu.LM_K, W, H, seed=91, draw_ids=5 + np.arange(9), noise={"angle_max": 45.0})
    np.testing.assert_array_equal(pose2.asnumpy(), want[0])
    with pytest.raises(TypeError):
        sample_rendered_poses(src, emu.LM_K, W, H, seed=1)
