"""Writes launch_trace_golden.npz: per configuration of tests/launch_trace.py the launch trace of every phase, as JSON text.

    python tests/golden/make_launch_trace_golden.py                      (re)write the golden from this checkout
    python tests/golden/make_launch_trace_golden.py CONFIG PHASE         print one trace of this checkout, one call per line

The golden pins what the graph launched when it was written: a change that means to keep every launch leaves it alone and must
reproduce it. To see what moved, print the trace at both commits and diff the two."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import launch_trace  # noqa: E402

PATH = os.path.join(HERE, "launch_trace_golden.npz")


def traces(name):
    with pytest.MonkeyPatch.context() as mp:
        return launch_trace.trace_config(name, mp.setattr)


def main(argv):
    if argv:
        for call in traces(argv[0])[argv[1]]:
            print(json.dumps(call))
        return
    out = {}
    for name in launch_trace.CONFIGS:
        t = traces(name)
        out[name] = np.frombuffer(json.dumps(t, separators=(",", ":")).encode(), np.uint8)
        print(name, {k: len(v) for k, v in t.items()})
    np.savez_compressed(PATH, **out)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
