"""The graph's launches, pinned on the host: bind, one inference iteration and one training step of every encoder arithmetic run
on a recording stand-in for the library (tests/launch_trace.py) and must reproduce the recorded golden call for call and argument
for argument. Only a run of consecutive weight-pack calls is compared as a multiset (launch_trace.normalise)."""
import json
import os

import numpy as np
import pytest

import launch_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: json.loads(z[k].tobytes().decode()) for k in z.files}


def test_golden_covers_every_configuration(golden):
    assert sorted(golden) == sorted(launch_trace.CONFIGS)


@pytest.mark.parametrize("name", sorted(launch_trace.CONFIGS))
def test_launch_trace_matches_golden(name, golden, monkeypatch):
    got = launch_trace.trace_config(name, monkeypatch.setattr)
    assert sorted(got) == sorted(golden[name])
    for phase, want in golden[name].items():
        a, b = launch_trace.normalise(got[phase]), launch_trace.normalise(want)
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        assert a == b, "%s / %s: call %d of %d (golden %d)\n  got    %s\n  golden %s" % (
            name, phase, first, len(a), len(b), a[first] if first < len(a) else None, b[first] if first < len(b) else None)
