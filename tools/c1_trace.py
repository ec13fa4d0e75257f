"""Dev probe: s_memtime sums of one mid-grid block of conv1's Winograd kernel, per wave and step segment (build:
SRC=wino_c1 tools/build_variants_f16.sh c1trace:"-DC1_TRACE=1", run with DEEPIM_LIB=variants/lib_c1trace.so).
usage: c1_trace.py [B [H W]]"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mx_deepim_amd.runtime import Context, DeviceArray, lib
ctx = Context.get(0)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
H, W = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (480, 640)
rng = np.random.default_rng(0)
fn = lib.load().deepim_dev_c1_trace
fn.argtypes = [ctypes.c_void_p]
n = B * 8 * H * W
x = ctx.array(np.resize(rng.standard_normal(min(n, 1 << 22)).astype(np.float32), n).reshape(B, 8, H, W))
wd = ctx.array((rng.standard_normal((64, 8, 7, 7)) / np.sqrt(8 * 49)).astype(np.float32))
pk = DeviceArray(ctx, (lib.load().deepim_conv1_wino_packed_size() // 4,))
lib.deepim_conv1_wino_pack_weights(ctx.handle, pk, wd)
bias = ctx.array(rng.standard_normal(64).astype(np.float32))
out = ctx.empty((B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1))
tr = ctx.zeros((8 * 16,), dtype=np.uint32)
assert fn(ctypes.c_void_p(tr.ptr)) == 0
for _ in range(3):
    lib.deepim_conv1_wino_forward(ctx.handle, out, x, pk, bias, B, H, W, ctypes.c_float(0.1), 3)
ctx.sync()
t = tr.asnumpy().reshape(8, 16).astype(np.int64)
SEG = ["finish", "pairs 1-3", "pair 4", "pairs 5+", "tf1/U/in", "barrier", "tf0", "pairs 1-3", "pair 4", "pairs 5+", "send", "U/in", "barrier"]
print("conv1 B %d %dx%d: ticks per tile block, one mid-grid block (a pair = 4 MFMAs = 256 cycles); step 0 = segments 0-5, step 1 = 6-12" % (B, H, W))
print("wave role half " + " ".join("%9s" % s for s in SEG) + "     total  blocks")
for w in range(8):
    nb = max(int(t[w, 13]), 1)
    print("%4d   R%d    %d " % (w, w >> 1, w & 1) + " ".join("%9.0f" % (t[w, k] / nb) for k in range(13))
          + " %9.0f %7d" % (t[w, 14] / nb, t[w, 13]))
