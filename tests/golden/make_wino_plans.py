"""Writes tests/golden/wino_plans.json: deepim_conv_wino_plan and the four deepim_conv_wino_preferred* answers under the DEFAULT options
(ctx = None: host arithmetic, no GPU) for every Winograd geometry the tests use, at B = 1 ... 32.

    python tests/golden/make_wino_plans.py [note]   # after the library is built; the note is appended to the file's header

tests/test_oracle_wino.py::test_default_launch_plans_match_the_recorded_ones recomputes every row. A change that moves a threshold or a
plan on purpose regenerates the file; its diff then shows which layers moved."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "wino_plans.json")
BATCHES = (1, 2, 4, 8, 16, 32)
COLUMNS = ["B", "Cin", "H", "W", "Cout", "out_nc8", "s2d", "rc", "plan0", "plan1", "plan2", "plan3", "plan4", "plan5", "plan6", "plan7",
           "plan8", "preferred", "preferred_s2d", "preferred_s2d3", "preferred_s2d3_wide"]


def _s2d(cases, s2d):
    """(B, Cin, H, W, Cout) of a stride-2 layer -> (Cin, H, W, Cout, s2d) of its space-to-depth problem"""
    return [(4 * cin, H // 2, W // 2, cout, s2d) for _, cin, H, W, cout in cases]


def geometries():
    """(Cin, H, W, Cout, out_nc8, s2d) as deepim_conv_wino_plan takes them"""
    g = [(256, 120, 160, 128, 3, 1), (512, 60, 80, 256, 1, 1), (256, 60, 80, 256, 3, 0), (512, 30, 40, 512, 1, 0),
         (512, 15, 20, 512, 1, 0), (1024, 8, 10, 1024, 0, 0)]                                       # test_oracle_wino._WINO_LAYERS
    g += [(cin, H, W, cout, 1, s2d) for cin, H, W, cout in ((1024, 30, 40, 512), (2048, 15, 20, 512), (2048, 8, 10, 1024))
          for s2d in (2, 3)]                                                                         # test_wino_s2d3_transform._LAYERS
    # the GPU tests' cases, in each output layout they run
    wino = [(256, 12, 16, 256), (512, 30, 40, 512), (64, 15, 20, 64), (1024, 8, 10, 1024), (8, 7, 9, 32), (16, 2, 2, 96), (24, 1, 5, 160),
            (8, 6, 6, 32)]                                                                           # test_gpu_wino.CASES
    g += [c + (o, 0) for c in wino for o in (1, 0)]
    streamk = [(32, 96, 128, 128), (64, 40, 56, 256), (256, 60, 80, 256)]                            # test_gpu_wino.STREAMK_CASES
    g += [c + (o, 0) for c in streamk for o in (1, 3, 0)]
    s2d3 = _s2d([(1, 256, 60, 80, 512), (1, 512, 30, 40, 512), (2, 16, 12, 16, 64), (3, 32, 10, 14, 128), (2, 64, 6, 10, 64)], 2)
    g += [c[:4] + (o, c[4]) for c in s2d3 for o in (1, 3, 0)]                                        # test_gpu_wino_s2d3.CASES
    wide = [(2, 16, 12, 16, 256), (3, 32, 10, 14, 256), (2, 64, 6, 10, 512), (1, 512, 30, 40, 512)]  # test_gpu_wino_s2d3_wide.CASES
    g += [c[:4] + (o, c[4]) for s2d in (2, 3) for c in _s2d(wide, s2d) for o in (1, 3, 0)]
    return g


def layer_of(cin, H, W, s2d):
    """the layer's own input geometry, as the deepim_conv_wino_preferred* functions take it"""
    return (cin // 4, 2 * H, 2 * W) if s2d else (cin, H, W)


def rows(L):
    out = []
    for cin, H, W, cout, out_nc8, s2d in geometries():
        for B in BATCHES:
            plan = (ctypes.c_int * 9)()
            rc = L.deepim_conv_wino_plan(None, B, cin, H, W, cout, out_nc8, s2d, plan)
            lc, lh, lw = layer_of(cin, H, W, s2d)
            pref = [f(None, B, lc, lh, lw, cout) for f in (L.deepim_conv_wino_preferred, L.deepim_conv_wino_preferred_s2d,
                                                           L.deepim_conv_wino_preferred_s2d3, L.deepim_conv_wino_preferred_s2d3_wide)]
            out.append([B, cin, H, W, cout, out_nc8, s2d, rc] + list(plan) + pref)
    return out


if __name__ == "__main__":
    from mx_deepim_amd.runtime import lib
    commit = subprocess.check_output(["git", "-C", ROOT, "describe", "--always", "--dirty"]).decode().strip()
    doc = {"header": "default-option Winograd launch plans, written by tests/golden/make_wino_plans.py from a build of commit %s%s"
                     % (commit, "".join(" (%s)" % a for a in sys.argv[1:])),
           "columns": COLUMNS, "rows": rows(lib.load())}
    with open(OUT, "w") as f:
        f.write('{"header": %s,\n "columns": %s,\n "rows": [\n  ' % (json.dumps(doc["header"]), json.dumps(COLUMNS)))
        f.write(",\n  ".join(json.dumps(r) for r in doc["rows"]))
        f.write("\n ]}\n")
    print("%s: %d rows" % (OUT, len(doc["rows"])))
