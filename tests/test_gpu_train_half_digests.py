"""The half-precision encoder backward (csrc/train_half.hip, fp16 and split-fp16 mode) bit for bit against recorded results: every
case of tests/golden/make_train_half_digests.py recomputed with the tree's own library and compared with the SHA-256 digest in
tests/golden/train_half_digests.json. The recorded digests come from the library of the commit before the two modes' sources were
merged into one (the file's `note`), so equality here means that the merged kernels, launchers and Python wiring compute what the
separate ones did. The entry points are deterministic, so a mismatch is a changed result bit, never noise."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_train_half_digests", os.path.join(_GOLDEN, "make_train_half_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
CASES = gen.cases()
with open(os.path.join(_GOLDEN, "train_half_digests.json")) as _f:
    RECORDED = json.load(_f)["digests"]


def test_the_fixture_lists_exactly_the_generator_s_cases():
    """(a) 7 weight-gradient cases, (b) 12 activation-gradient cases, (c) 6 data-gradient cases, (d) 3 overflow cases, (e) one
    training iteration per mode."""
    assert list(RECORDED) == list(CASES) and len(CASES) == 30


@pytest.mark.parametrize("name", list(CASES))
def test_digest_equals_the_recorded_one(ctx, name):
    assert CASES[name](ctx) == RECORDED[name], name
