"""conv1's Winograd kernel (csrc/wino_c1.hip) keeps its bits: the SHA-256 of deepim_conv1_wino_forward's raw output buffer on seeded
inputs and weights against the digests recorded in tests/golden/conv1_wino_bits.json (tests/golden/make_conv1_wino_bits.py, which
also holds the cases and runs each twice to check that it repeats). The kernel fixes every output's summation order, so a change to
its load order or instruction selection has an exact yardstick: one partly filled tile block, two tile blocks per row with a ragged
second one, odd output sizes on the scalar-load instantiation, and 768 tile blocks on 256 blocks (three per block: both input
prefetch distances and the past-the-end loads), with and without bias."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_conv1_wino_bits", os.path.join(_GOLDEN, "make_conv1_wino_bits.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

with open(os.path.join(_GOLDEN, "conv1_wino_bits.json")) as _f:
    RECORDED = json.load(_f)["sha256"]


@pytest.fixture(scope="module")
def computed(ctx):
    return maker.digests(ctx)   # asserts that each case's two runs agree


def test_every_case_is_recorded():
    assert sorted(RECORDED) == sorted(maker.keys())


@pytest.mark.parametrize("key", maker.keys())
def test_output_bits_match_the_recorded_digest(computed, key):
    assert computed[key] == RECORDED[key]
