#!/usr/bin/env python
"""Store what the reference's own flow kernel computes, so that tests/test_gpu_flow_reference.py and tests/test_abi.py pin F1 / B2
in a checkout without the reference.

Needs a GPU and the test-only builds oracle/Makefile makes from the reference's lib/flow_c (oracle/_ref/, present only where the
reference checkout was available at build time):  python tests/golden/make_flow_ref_golden.py [OUT.npz]
(default: tests/golden/flow_ref_kernel_golden.npz).  Records, for each input case of tests/test_gpu_flow_reference.py:
  <case>_inputs_sha256             digest of the case's inputs (depth_src, depth_tgt, KT, Kinv as float32)
  <case>_<nofma|fma>_flow / _valid  the reference kernel's outputs, -ffp-contract=off and -ffp-contract=fast builds
and once:
  header_client_undefined          the symbols a C++ TU including the reference's gpu_flow.hpp leaves for libdeepim_hip.so to
                                   define (`nm -D --undefined-only` of oracle/_ref/libflow_hpp_client.so, strong entries)
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

from mx_deepim_amd import synthetic  # noqa: E402
import test_gpu_flow_reference as T  # noqa: E402


def main(out):
    small_batch = synthetic.make_batch(2, seed=2333, n_frames=2)       # tests/conftest.py: small_batch
    rec = {}
    for name, src, tgt, KT, Kinv in T._cases(small_batch):
        key = T._case_key(name)
        rec[key + "_inputs_sha256"] = np.array(T._inputs_digest(src, tgt, KT, Kinv))
        for which in ("nofma", "fma"):
            got = T._live_ref_flow(which, src, tgt, KT, Kinv)
            assert got is not None, "oracle/_ref/libref_flow_%s.so not built" % which
            rec["%s_%s_flow" % (key, which)], rec["%s_%s_valid" % (key, which)] = got
            print("%s %s: %d valid pixels" % (name, which, int(got[1].sum())))
    client = os.path.join(T.REF_DIR, "libflow_hpp_client.so")
    nm = subprocess.run(["nm", "-D", "--undefined-only", client], capture_output=True, text=True, check=True).stdout
    rec["header_client_undefined"] = np.array([ln.split()[-1] for ln in nm.splitlines() if ln.split()[0] == "U"])
    print("header client leaves undefined:", rec["header_client_undefined"].tolist())
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "flow_ref_kernel_golden.npz"))
