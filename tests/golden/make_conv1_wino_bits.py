"""Writes tests/golden/conv1_wino_bits.json: SHA-256 of the raw output buffer of deepim_conv1_wino_forward (csrc/wino_c1.hip) on seeded
inputs and weights, at the smallest shapes that reach every path of the kernel. The kernel fixes every output's summation order, so a
change to its scheduling must leave these bits alone; tests/test_gpu_wino_c1_bits.py recomputes them.

    python tests/golden/make_conv1_wino_bits.py [note]   # on the GPU, after the library is built; the note goes into the header

Run against a build of the commit whose bits are the yardstick (DEEPIM_LIB selects another library file)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv1_wino_bits.json")
SLOPE = 0.1

# (B, H, W, output modes, bias variants)
#   8 x 12:    one partly filled tile block, TX = 3
#   16 x 136:  TX = 34: two tile blocks per row, the second ragged
#   10 x 14:   odd Ho / Wo (5 x 7) and W % 4 != 0: the scalar-load instantiation
#   128 x 264: 768 tile blocks on 256 blocks: every block walks three, so the one-ahead and two-ahead input prefetches and the
#              past-the-end loads all run
CASES = [
    (1, 8, 12, (1, 3), (True,)),
    (1, 16, 136, (1, 3), (True,)),
    (1, 10, 14, (1,), (True,)),
    (8, 128, 264, (3,), (True, False)),
]


def keys():
    return ["B%d_%dx%d_mode%d_%s" % (B, H, W, m, "bias" if wb else "nobias") for B, H, W, modes, biases in CASES for m in modes
            for wb in biases]


def operands(B, H, W):
    rng = np.random.default_rng(B * 7919 + H * 31 + W + 22)
    x = rng.standard_normal((B, 8, H, W)).astype(np.float32)
    w = (rng.standard_normal((64, 8, 7, 7)) / np.sqrt(8 * 49)).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    return x, w, b


def digests(ctx):
    """{key: sha256 hex of the output buffer}; every case runs twice and must repeat"""
    from mx_deepim_amd.runtime import DeviceArray, lib
    out = {}
    for B, H, W, modes, biases in CASES:
        x, w, b = operands(B, H, W)
        pk = DeviceArray(ctx, (lib.load().deepim_conv1_wino_packed_size() // 4,))
        lib.deepim_conv1_wino_pack_weights(ctx.handle, pk, ctx.array(w))
        xd, bd = ctx.array(x), ctx.array(b)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        for m in modes:
            for wb in biases:
                got = []
                for _ in range(2):
                    y = ctx.zeros((B, 64, Ho, Wo))
                    lib.deepim_conv1_wino_forward(ctx.handle, y, xd, pk, bd if wb else None, B, H, W, ctypes.c_float(SLOPE), m)
                    got.append(hashlib.sha256(y.asnumpy().tobytes()).hexdigest())
                key = "B%d_%dx%d_mode%d_%s" % (B, H, W, m, "bias" if wb else "nobias")
                assert got[0] == got[1], "%s: two runs differ" % key
                out[key] = got[0]
    return out


if __name__ == "__main__":
    from mx_deepim_amd.runtime import Context
    commit = subprocess.check_output(["git", "-C", ROOT, "describe", "--always", "--dirty"]).decode().strip() \
        if os.path.isdir(os.path.join(ROOT, ".git")) else "unknown"
    doc = {"header": "sha256 of deepim_conv1_wino_forward's output buffer, written by tests/golden/make_conv1_wino_bits.py from a build "
                     "of commit %s%s" % (commit, "".join(" (%s)" % a for a in sys.argv[1:])),
           "sha256": digests(Context.get(0))}
    with open(os.environ.get("CONV1_BITS_OUT", OUT), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("%d digests" % len(doc["sha256"]))
