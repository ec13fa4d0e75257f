"""Flow EPE without a GPU: the numpy restatement of deepim_flow_epe (tests/flow_epe_emulation.py) against what the reference's
own par_generate_gt + calc_EPE_one_pair gave (tests/golden/flow_epe_golden.npz, made by tests/golden/make_flow_epe_golden.py);
the C ABI of the entry point.

Bars: `visible` and the three counts exact; the sums within 1e-9 relative — both sides are float64 and differ in operation order
only (BLAS products against left-to-right sums per pixel, pairwise against sequential sums over at most 91 pixels), about
N·2^-53 ≈ 1e-14."""
import ctypes
import os

import numpy as np
import pytest

import flow_epe_emulation as emu
from mx_deepim_amd import runtime

from flow_epe_emulation import CASES, GOLDEN, check_rows, frames_of, ref_name


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def test_fixture_covers_what_it_claims(gold):
    for tag, (B, H, W) in (("a", (2, 6, 12)), ("b", (3, 7, 13))):
        assert gold[tag + "_flow_est"].shape == (B, 2, H, W) and gold[tag + "_flow_est"].dtype == np.float32
        assert gold[tag + "_depth_rendered"].dtype == np.uint16 and gold[tag + "_mask_gt_observed"].dtype == np.uint8
        for rep in (False, True):
            gt, nogt = gold[ref_name(tag, rep, True) + "_rows"], gold[ref_name(tag, rep, False) + "_rows"]
            assert gt.dtype == np.float64 and gt.shape == (B, 6)
            assert (gt[:, 1] == H * W).all() and (0 < gt[:, 3]).all() and (gt[:, 3] < gt[:, 5]).all() and (gt[:, 5] < H * W).all()
            assert (nogt[:, 3] < gt[:, 3]).all()          # the sensor depth hides pixels the ground-truth depth shows
        old, std = gold[ref_name(tag, False, True) + "_flow_gt"], gold[ref_name(tag, True, True) + "_flow_gt"]
        np.testing.assert_array_equal(old[..., ::-1], std)      # the two representations swap the channels
        assert np.abs(old[..., 0] - old[..., 1]).max() > 0.1


@pytest.mark.parametrize("tag,rep,with_gt", CASES)
def test_restated_visibility_and_ground_truth_flow_equal_the_reference(gold, tag, rep, with_gt):
    f = frames_of(gold, tag, with_gt)
    dr, do = emu.par_generate_gt(f)
    K, Kinv = gold[tag + "_K"], emu.inv3(gold[tag + "_K"])
    name = ref_name(tag, rep, with_gt)
    for b in range(len(dr)):
        dw, dh, vis = emu.calc_flow_core(dr[b], do[b], emu.calc_KT(f["pose_rendered"][b], f["pose_observed"][b], K), Kinv, 3e-3)
        np.testing.assert_array_equal(vis, gold[name + "_visible"][b] == 1)
        want = gold[name + "_flow_gt"][b]
        got = np.dstack([dw, dh] if rep else [dh, dw])
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("tag,rep,with_gt", CASES)
def test_restated_epe_equals_the_reference(gold, tag, rep, with_gt):
    f = frames_of(gold, tag, with_gt)
    dr, do = emu.par_generate_gt(f)
    got = emu.flow_epe(gold[tag + "_flow_est"], dr, do, f["pose_rendered"], f["pose_observed"], gold[tag + "_K"],
                       standard_rep=rep)
    check_rows(got, gold[ref_name(tag, rep, with_gt) + "_rows"])


def test_restatement_skips_and_rounds_like_numpy(gold):
    f = frames_of(gold, "b")
    dr, do = emu.par_generate_gt(f)
    args = (gold["b_flow_est"], dr, do, f["pose_rendered"], f["pose_observed"], gold["b_K"])
    full, part = emu.flow_epe(*args), emu.flow_epe(*args, skip=np.array([0, 1, 0]))
    assert (part[1] == 0).all()
    np.testing.assert_array_equal(part[[0, 2]], full[[0, 2]])
    est = gold["b_flow_est"].copy()
    est[0, 0, 3, 3] = 7e4                                   # beyond fp16: inf, as numpy's astype gives
    assert np.isposinf(emu.flow_epe(est, *args[1:])[0, 0])


def test_header_declares_flow_epe_and_the_library_exports_it():
    protos = runtime.parse_header()
    assert "deepim_flow_epe" in protos
    ret, argtypes, names = protos["deepim_flow_epe"]
    assert ret is ctypes.c_int
    assert names == ["ctx", "out", "totals", "flow_est", "depth_rendered", "depth_observed", "pose_rendered", "pose_observed",
                     "K_host", "skip", "thresh", "standard_rep", "B", "H", "W"]
    assert argtypes[:10] == [ctypes.c_void_p] * 10 and argtypes[10] is ctypes.c_float and argtypes[11:] == [ctypes.c_int] * 4
    assert os.path.exists(runtime.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert hasattr(ctypes.CDLL(runtime.LIB_PATH), "deepim_flow_epe")
