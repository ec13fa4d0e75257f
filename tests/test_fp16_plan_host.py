"""CPU: deepim_conv_f16_plan (host arithmetic, ctx = NULL: default options) pins the launch plan of every case of
tests/test_gpu_fp16_plans.py, and every plan the network's nine fp16 encoder layers (conv2 … conv6_1; conv1 has a kernel of its own)
take at 480x640 and B in {1, 4, 8, 32} is one that test runs. A change of the plan model that moves a case off the plan it is there
for, or the network onto a plan without a kernel-level test, fails here."""
import ctypes

import numpy as np
import pytest

import fp16_plan_cases as pc
from mx_deepim_amd.runtime import lib
from mx_deepim_amd.symbols.deepIM_flownet import ENCODER
from oracle import net as onet
from oracle import pipeline as opipe


def _plan(case, x3=0):
    B, cin, H, W, cout, k, s, p = case
    plan = (ctypes.c_int * 8)(*[-7] * 8)
    lib.deepim_conv_f16_plan(None, x3, B, cin if x3 else pc.cin_pad(case), H, W, cout, k, k, s, p, plan)   # no context, no device
    return tuple(plan)


DEFAULT_ROWS = [r for r in pc.ROWS if not r[2]]
OPTION_ROWS = [r for r in pc.ROWS if r[2]]


@pytest.mark.parametrize("row", DEFAULT_ROWS, ids=[r[0] for r in DEFAULT_ROWS])
def test_case_takes_the_plan_it_is_there_for(row):
    _, case, _, want = row
    assert _plan(case) == want


@pytest.mark.parametrize("row", OPTION_ROWS, ids=[r[0] for r in OPTION_ROWS])
def test_option_rows_differ_from_the_default_plan(row):
    """Rows that run under a context option (pinned with the context on the GPU): under the defaults their geometry takes another
    plan — one a default row pins — so the option is what the row is about."""
    _, case, _, want = row
    got = _plan(case)
    assert got != want
    assert got in [r[3] for r in DEFAULT_ROWS if r[1] == case]


def test_rows_cover_what_the_issue_lists():
    plans = {r[0]: r[3] for r in pc.ROWS}
    kinds = {(p[0], p[5] > 1, p[6] > 1) for p in plans.values()}
    assert kinds == {(k, s, t) for k in (pc.REG, pc.DMA, pc.PP) for s, t in ((False, False), (True, False), (False, True))} - \
        {(pc.REG, False, False), (pc.REG, False, True)}            # the register-staged kernel has no tail split; unsliced: test_gpu_fp16
    assert {p[1:3] for p in plans.values() if p[0] == pc.REG and p[5] > 1} == {(64, 256), (128, 256), (256, 256)}
    assert any(p[0] == pc.DMA and c[4] % 128 and p[5] > 1 for _, c, _, p in pc.ROWS)
    assert any(p[0] == pc.DMA and c[4] % 128 and p[5] == 1 for _, c, _, p in pc.ROWS)
    assert any(p[0] == pc.REG and c[1] % 64 == 0 and c[4] < 64 for _, c, _, p in pc.ROWS)
    for _, case, _, p in pc.ROWS:
        assert p[3] == -(-pc.npix(case) // p[2]) * -(-case[4] // p[1])
        if p[6] > 1:
            assert p[7] == p[3] % (512 if p[0] == pc.DMA else 256) and pc.tail_region(case, p)[0] < pc.npix(case)


def _encoder_cases(B):
    cin, H, W = ENCODER[0][1], 240, 320          # conv1's output at 480x640
    for name, cout, k, s, p in ENCODER[1:]:
        yield name, (B, cin, H, W, cout, k, s, p)
        (H, W), cin = pc.out_hw((B, cin, H, W, cout, k, s, p)), cout


def test_every_plan_of_the_network_has_a_kernel_level_case():
    tested = {pc.combination(case, want) for _, case, _, want in DEFAULT_ROWS}
    found = {}
    for B in (1, 4, 8, 32):
        layers = list(_encoder_cases(B))
        assert len(layers) == 9 and layers[-1][1][1:5] == (1024, 8, 10, 1024)
        for name, case in layers:
            found.setdefault(pc.combination(case, _plan(case)), []).append((B, name))
    missing = {c: l for c, l in found.items() if c not in tested}
    assert not missing, missing
    # what the kernel-level cases are there for really occurs: tail splits and split-K of the ping-pong kernel at the real batch sizes
    assert any(c[0] == pc.PP and c[4] for c in found) and any(c[0] == pc.PP and c[3] for c in found)
    assert _plan((32, 256, 60, 80, 256, 3, 1, 1))[5:] == (1, 2, 88) and _plan((8, 64, 240, 320, 128, 5, 2, 2))[5:] == (1, 3, 44)


def test_x3_twin_takes_a_tail_split():
    """The X3 launcher plans 256x128 tiles on the four-wave kernel: 600 tiles, 512 whole + 88 cut into two K slices — the plan
    tests/test_gpu_x3.py::test_conv_x3_is_fp32_grade is there for. The plain fp16 layer of the same shape takes none."""
    assert _plan(pc.X3_TAIL_CASE, x3=1) == (pc.DMA, 256, 128, 600, 9, 1, 2, 88)
    B, cin, H, W, cout, k, s, p = pc.X3_TAIL_CASE
    assert _plan((B, 2 * cin, H, W, cout, k, s, p)) == (pc.PP, 256, 256, 300, 9, 1, 0, 0)


def test_query_refuses_what_the_launchers_refuse():
    plan = (ctypes.c_int * 8)()
    raw = lib.load().deepim_conv_f16_plan
    for args in ((0, 1, 12, 8, 8, 64, 3, 3, 1, 1), (0, 1, 8, 8, 8, 66, 3, 3, 1, 1), (0, 1, 8, 8, 8, 64, 9, 9, 1, 4),
                 (1, 1, 16, 8, 8, 128, 3, 3, 1, 1), (1, 1, 32, 8, 8, 64, 3, 3, 1, 1), (0, 0, 8, 8, 8, 64, 3, 3, 1, 1),
                 (0, 64, 1024, 480, 640, 64, 3, 3, 1, 1)):
        assert raw(None, *args, plan) != 0, args
        assert list(plan) == [-1] * 8
    assert raw(None, 0, 1, 8, 8, 8, 64, 3, 3, 1, 1, None) != 0


SMALLEST_PER_FAMILY = ["reg-ut-32", "dma128-split-whole", "pp128-whole"]


@pytest.mark.parametrize("rid", SMALLEST_PER_FAMILY)
def test_two_percent_cap_has_headroom_for_a_correct_fp32_accumulation(rid):
    """The GPU test's cap — fewer than 2 % of elements differ from float16(lrelu(S)), S the float64 sum — is a condition, not a
    measurement: the oracle's own fp32 accumulation of the same fp16-rounded operands, rounded to fp16 once, differs from it on fewer
    than 1 % of elements."""
    _, case, _, plan = pc.ROWS[pc.ROW_IDS.index(rid)]
    assert case == min((r[1] for r in pc.ROWS if r[3][0] == plan[0]), key=lambda c: pc.npix(c) * c[4] * c[1] * c[5] ** 2)
    x, w, b = pc.random_operands(case, 1)
    S, _ = pc.random_reference(case, x, w, b)
    emu = opipe.q16(onet.conv2d(opipe.q16(x), opipe.q16(w), b, case[6], case[7], 0.1))
    assert np.mean(emu != pc.lrelu16(S, pc.SLOPE_RANDOM)) < 0.01
