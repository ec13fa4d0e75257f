// The stride-2 data gradient as four stride-1 convolutions, one per output parity class: the class geometry and the kernel that
// puts a class's result window onto its positions. Shared by the fp16 (train_f16.hip) and the split-fp16 (train_x3.hip) backward;
// a split16 tensor of C channels is stitched as an fp16 tensor of 2C.
#pragma once
#include "common.h"

namespace {

typedef _Float16 s2_h8 __attribute__((ext_vector_type(8)));

// ---- data gradient, stride 2: one parity class's result window onto its positions of dx ------------------------------------
// dx (B,Hd,Wd,C)[.., 2t + py, 2u + px, :] = cls (B,Hs,Ws,C)[.., t + cy, u + cx, :]; one thread per 8-channel octet
__global__ __launch_bounds__(256) void stitch_f16_kernel(_Float16* __restrict__ dx, const _Float16* __restrict__ cls, int C, int Hd,
                                                         int Wd, int Hs, int Ws, int hq, int wq, int cy, int cx, int py, int px,
                                                         long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int no = C >> 3;
  const int o = (int)(i % no);
  long r = i / no;
  const int u = (int)(r % wq);
  r /= wq;
  const int t = (int)(r % hq);
  const long n = r / hq;
  const s2_h8 v = *reinterpret_cast<const s2_h8*>(cls + (((n * Hs + t + cy) * Ws + u + cx) * C + o * 8));
  *reinterpret_cast<s2_h8*>(dx + (((n * Hd + 2 * t + py) * Wd + 2 * u + px) * C + o * 8)) = v;
}

struct S2ClassF16 { int py, px, ky0, kx0, nky, nkx, cy, cx, P; };
// the taps output parity class z of a stride-2 layer meets and where its window lies in the stride-1 result (DESIGN.md "dgrad")
S2ClassF16 s2_class_f16(int z, int k, int pad) {
  S2ClassF16 c;
  c.py = z >> 1; c.px = z & 1;
  c.ky0 = (c.py + pad) % 2; c.kx0 = (c.px + pad) % 2;
  c.nky = (k - c.ky0 + 1) / 2; c.nkx = (k - c.kx0 + 1) / 2;
  c.P = std::max(c.nky, c.nkx) - 1;
  c.cy = (c.py + pad - c.ky0) / 2 + c.P - (c.nky - 1);
  c.cx = (c.px + pad - c.kx0) / 2 + c.P - (c.nkx - 1);
  return c;
}

}  // namespace
