// conv1 (flow_conv1: 7x7 stride 2 pad 3, 8 -> 64 channels, deepIM_flownet.py:63) as fp32 Winograd over its four input phases.
//
// Space-to-depth: output pixel Y (one dimension) reads input 2Y + ky - 3. Input phase p (= input index mod 2) meets the taps
// ky = 2a' + p - 1, a' = 0..3, at phase index Y - 2 + a' — four taps for the odd phase, three (a' = 0 is ky = -1) for the even one.
// So every phase is a 4-tap correlation over phase indices Y - 2 .. Y + 1, and a 2-output tile of it is Winograd F(2,4): 5 points,
// a 5-wide input patch. In 2D per 2x2 output tile and phase: V = B^T d B (5x5), U = G g G^T, M = sum over phases and channels of
// U .* V, Y = A^T M A. Interpolation points 0, 1, -1, 1/2, infinity (rows of B^T / G scaled to small integers in B^T):
//   B^T = [ 1 -2 -1  2  0 ]   G = [ 1    0    0    0   ]   A^T = [ 1 1  1  1   0 ]
//         [ 0 -1  1  2  0 ]       [ 1/2  1/2  1/2  1/2 ]         [ 0 1 -1  1/2 1 ]
//         [ 0 -1  3 -2  0 ]       [ 1/6 -1/6  1/6 -1/6 ]
//         [ 0  1  0 -1  0 ]       [ 8/3  4/3  2/3  1/3 ]
//         [ 0  1 -2 -1  2 ]       [ 0    0    0    1/2 ]
// G's first row picks tap a' = 0 alone, which the even phase does not have: position 0 of that dimension is identically zero there.
// Of the 4 x 25 (phase, position) pairs 16 + 20 + 20 + 25 = 81 remain, each a GEMM over the 8 input channels: 648 multiply-adds
// per output channel and 2x2 tile against 4 x 49 x 8 = 1568 for the direct sum (2.42x fewer). Results differ from the direct sum in
// the last bits (tests: within 1e-5 of the layer's range; tests/test_wino_c1_transform.py restates the transforms in float64).
//
// Kernel (persistent 512-thread blocks, one per CU: two waves per SIMD, 128 + 128 registers each):
//   * a block owns 64 output channels x 32 tiles (a tile block: one tile row, 32 consecutive tile columns) and walks each of its tile
//     blocks in two steps, one per input row phase py: the 36 (py = 0) or 45 (py = 1) pairs of that row phase;
//   * V of a (tile block, row phase) is computed ONCE for all 64 output channels and handed to every wave through LDS,
//     [pair][k half][tile][4 input channels], 1 KB per pair. Each row phase has its own buffer (36 + 45 KB), so the two form a double
//     buffer: a transform lane owns one (tile, input channel) and both column phases — 5 patch rows x 10 input columns, two 16-byte
//     and one 8-byte load per row from one base offset per job — runs B^T d B in registers and stores one float per live pair. The
//     four waves that transform a row phase (one per SIMD) do it during the other row phase's MFMAs; their loads are issued a step
//     and a half before they are used;
//   * v_mfma_f32_32x32x2_f32 on 32 output channels x 32 tiles; k-step s of lane half hh multiplies input channel 4 hh + s, so a pair's
//     8 input channels are 4 MFMAs fed by one ds_read_b128 of V and one 16-byte load of U. U (166 KB) is streamed from global memory,
//     where it stays resident in L2;
//   * wave w multiplies channel half w & 1; its role R = w >> 1 owns whole rows of positions: R0 row xi = 1 and (0, 0..2), R1 row 2
//     and (0, 3..4), R2 row 3, R3 row 4 (8 / 7 / 5 / 5 accumulator tuples). Waves w and w + 4 share a SIMD, so (R0, R2) and (R1, R3)
//     issue 41 and 40 of a tile block's 81 pairs per channel half;
//   * output transform Y = A^T M A: each wave runs the nu-pass over its own rows in registers (S[xi][b], 5 -> 2 per row); the four
//     waves of a channel half exchange 32 floats per lane through LDS (16 KB), and R0 / R1 finish output row 0 / 1 at the start of the
//     next step: bias, LeakyReLU, one 16-byte store per 4 channels and pixel (plain NC8, or space-to-depth NC8 for conv2);
//   * two barriers per tile block. Every output's summation order is fixed: bit-identical from run to run and for any grid size;
//   * block b works on XCD b % 8's contiguous eighth of the tile blocks, so that the input rows the blocks of an XCD share (a patch
//     spans 10 input rows, a tile row 4) are read into its L2 once.
#include "common.h"

// dev switches for measuring the parts alone (SRC=wino_c1 tools/build_variants_f16.sh); the shipped build has one path
#ifndef C1_UDEEP
#define C1_UDEEP 2   // U operands a step requests ahead, see c1_udepth: 0 = C1_D in every step; 1 = all nine only in the step behind the
#endif               // wave's own input loads; 2 = all nine in every nine-pair step
#ifndef C1_PIN
#define C1_PIN 1     // 0: the compiler may move instructions across the two barriers of a tile block
#endif
// dev builds (-DC1_TRACE=1, tools/c1_trace.py): the eight waves of one block in the middle of the grid sum the s_memtime ticks of
// their step segments (C1Tr below). A stamp is subtracted one segment after it was requested, so the scalar wait is free. Stamps
// cost issue slots and make the next LDS wait a full one: for attribution only, timings come from unstamped builds.
#ifndef C1_TRACE
#define C1_TRACE 0
#endif

#if C1_TRACE
__device__ unsigned* g_c1_trace = nullptr;   // [wave][16]: the 13 segment sums, tile blocks walked, total ticks
#endif

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int C1_PAIRS = 81;
constexpr int C1_TB = 32;                                 // tiles per tile block (one tile row)
constexpr int C1_PY1 = 36;                                // pairs of row phase 0; row phase 1 holds pairs 36..80
constexpr int C1_PACKED_FLOATS = 2 * C1_PAIRS * 64 * 4;   // U: [half][pair][lane][k-step]
constexpr int C1_V1 = C1_PY1 * 1024;                      // LDS: V of row phase 0 at 0, of row phase 1 here, ...
constexpr int C1_X = C1_PAIRS * 1024;                     // ... the output exchange here: [half][role][b][g][lane][4 channels]
constexpr int C1_BIAS = C1_X + 2 * 4 * 8192;              // the 64 biases (zeros without bias)
constexpr int C1_LDS = C1_BIAS + 256;                     // 148 736 bytes
constexpr int C1_OOB = (int)0x80000000;                   // an out-of-range buffer offset: the load returns zero

// first pair of phase ph = py*2 + px; positions (xi, nu) from (py == 0, px == 0) to 4 in row-major order
__host__ __device__ constexpr int c1_pair0(int ph) { return ph == 0 ? 0 : ph == 1 ? 16 : ph == 2 ? 36 : 56; }
__host__ __device__ constexpr int c1_pair(int py, int px, int xi, int nu) {
  return c1_pair0(py * 2 + px) + (xi - (py == 0)) * (5 - (px == 0)) + (nu - (px == 0));
}
__host__ __device__ constexpr bool c1_live(int py, int px, int xi, int nu) { return (py || xi) && (px || nu); }

// accumulator q of role R -> position (xi, nu)
__host__ __device__ constexpr int c1_npos(int R) { return R == 0 ? 8 : R == 1 ? 7 : 5; }
__host__ __device__ constexpr int c1_xi(int R, int q) { return q < 5 ? R + 1 : 0; }
__host__ __device__ constexpr int c1_nu(int R, int q) { return q < 5 ? q : R == 0 ? q - 5 : q - 2; }

// the pairs role R multiplies in row phase PY, column phase major; first: the entry starts its accumulator (C = 0)
struct C1Entries {
  int n;
  int pair[16], q[16];
  bool first[16];
};
__host__ __device__ constexpr C1Entries c1_entries(int R, int PY) {
  C1Entries e{0, {}, {}, {}};
  for (int px = 0; px < 2; ++px)
    for (int q = 0; q < c1_npos(R); ++q) {
      const int xi = c1_xi(R, q), nu = c1_nu(R, q);
      if (!c1_live(PY, px, xi, nu)) continue;
      bool first = PY == 0 || !(c1_live(0, 0, xi, nu) || c1_live(0, 1, xi, nu));
      for (int k = 0; k < e.n; ++k)
        if (e.q[k] == q) first = false;
      e.pair[e.n] = c1_pair(PY, px, xi, nu);
      e.q[e.n] = q;
      e.first[e.n] = first;
      ++e.n;
    }
  return e;
}

struct C1Params {
  const float* in;      // (B, 8, H, W) NCHW
  const float* wp;      // packed U: [half][pair][lane][k-step]
  const float* bias;
  float* out;
  int B, H, W, Ho, Wo;
  int TX, TXB;          // tile columns, tile blocks per tile row
  int TY;
  int items;            // B * TY * TXB
  int out_s2d;          // 1: NC8 in space-to-depth order; 0: plain NC8
  float slope;
  unsigned in_bytes;
};

// segment K ends at stamp K; the stamps of a tile block, in order:
//   step 0:  0 finish | 1 the first C1_D pairs | 2 pair C1_D (the first whose U the loop requested, where there is one) | 3 the other
//            pairs | 4 transform of row phase 1, U prefetch, input loads | 5 barrier
//   step 1:  6 transform of row phase 0 | 7, 8, 9 as 1, 2, 3 | 10 nu-pass and exchange | 11 U prefetch, input loads | 12 barrier
struct C1Tr {
#if C1_TRACE
  unsigned seg[13], a, b;
  template <int K>
  __device__ __forceinline__ void stamp() {
    __builtin_amdgcn_sched_barrier(0);
    const unsigned t = (unsigned)__builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
    seg[(K + 12) % 13] += b - a;   // the segment that ended one stamp ago
    a = b;
    b = t;
  }
#else
  template <int K>
  __device__ __forceinline__ void stamp() {}
#endif
};

// one row of B^T applied to a 5-vector; OUT = which output (compile-time)
template <int OUT>
__device__ __forceinline__ float bt_row(float d0, float d1, float d2, float d3, float d4) {
  if constexpr (OUT == 0) return __builtin_fmaf(2.f, d3 - d1, d0 - d2);
  else if constexpr (OUT == 1) return __builtin_fmaf(2.f, d3, d2 - d1);
  else if constexpr (OUT == 2) return __builtin_fmaf(-2.f, d3, __builtin_fmaf(3.f, d2, -d1));
  else if constexpr (OUT == 3) return d1 - d3;
  else return __builtin_fmaf(2.f, d4 - d2, d1 - d3);
}
template <int OUT>
__device__ __forceinline__ float bt5(const float (&d)[5]) { return bt_row<OUT>(d[0], d[1], d[2], d[3], d[4]); }

// raw input of one transform job (row phase PY, input channel c, tile (ty, tx)): patch rows r = input rows 4ty - 4 + 2r + PY, input
// columns 4tx - 4 .. 4tx + 5 (column phase px = column & 1). One base offset per job, a fixed stride per row; out-of-image rows and
// column chunks carry an out-of-range offset, which reads zero = the padding.
// VEC: W % 4 == 0 — every 16-byte (8-byte) load lies wholly inside or wholly outside its image row
template <int VEC, int PY>
__device__ __forceinline__ void c1_load(float (&raw)[5][10], const __amdgpu_buffer_rsrc_t rsrc, const C1Params& p, int n, int c,
                                        int ty, int tx, bool live) {
  const int c0 = 4 * tx - 4, r0 = 4 * ty - 4 + PY;
  const int base = (((n * 8 + c) * p.H + r0) * p.W + c0) * 4;
  const int rs = 8 * p.W;
  if constexpr (VEC) {
    // 4 tx <= W for every tile: chunk 0 is outside only at tx = 0, chunks 1 and 2 only at the right edge
    const bool k0 = c0 >= 0, k1 = c0 + 4 < p.W, k2 = c0 + 8 < p.W;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int row = r0 + 2 * r;
      const int rb = live && (unsigned)row < (unsigned)p.H ? base + r * rs : C1_OOB;
      const f32x4 a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, k0 ? rb : C1_OOB, 0, 0));
      const f32x4 b = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, k1 ? rb + 16 : C1_OOB, 0, 0));
      const f32x2 e = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, k2 ? rb + 32 : C1_OOB, 0, 0));
      raw[r][0] = a.x; raw[r][1] = a.y; raw[r][2] = a.z; raw[r][3] = a.w;
      raw[r][4] = b.x; raw[r][5] = b.y; raw[r][6] = b.z; raw[r][7] = b.w;
      raw[r][8] = e.x; raw[r][9] = e.y;
    }
  } else {
    bool kq[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) kq[q] = (unsigned)(c0 + q) < (unsigned)p.W;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int row = r0 + 2 * r;
      const int rb = live && (unsigned)row < (unsigned)p.H ? base + r * rs : C1_OOB;
#pragma unroll
      for (int q = 0; q < 10; ++q)
        raw[r][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, kq[q] ? rb + 4 * q : C1_OOB, 0, 0));
    }
  }
}

// V = B^T d B of one transform job for both column phases of row phase PY, one float per live pair into the row phase's buffer
template <int PY>
__device__ __forceinline__ void c1_transform(const float (&raw)[5][10], char* smem, unsigned vbase) {
  float* const vb = reinterpret_cast<float*>(smem + (PY ? C1_V1 : 0) + vbase);
#pragma unroll
  for (int px = 0; px < 2; ++px) {
    float T[5][5];   // row pass: T[r][nu] from patch row r (columns 2c + px)
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const float d[5] = {raw[r][px], raw[r][2 + px], raw[r][4 + px], raw[r][6 + px], raw[r][8 + px]};
      if (px) T[r][0] = bt5<0>(d);
      T[r][1] = bt5<1>(d); T[r][2] = bt5<2>(d); T[r][3] = bt5<3>(d); T[r][4] = bt5<4>(d);
    }
#pragma unroll
    for (int nu = (px == 0); nu < 5; ++nu) {
      const float col[5] = {T[0][nu], T[1][nu], T[2][nu], T[3][nu], T[4][nu]};
      float V[5];
      if (PY) V[0] = bt5<0>(col);
      V[1] = bt5<1>(col); V[2] = bt5<2>(col); V[3] = bt5<3>(col); V[4] = bt5<4>(col);
#pragma unroll
      for (int xi = (PY == 0); xi < 5; ++xi) vb[(c1_pair(PY, px, xi, nu) - (PY ? C1_PY1 : 0)) * 256] = V[xi];
    }
  }
}

// U operands requested ahead of their use. vmcnt is in order, so a U load issued behind a transform job's input loads (HBM misses)
// waits for them, and the CU's vector memory path serves its waves in order too: behind ANOTHER wave's input loads a U load waits
// as long (R2 / R3 measured 1 800 cycles on the first U their row phase 0 loop requested, right after R0 / R1's input loads). So a
// step of nine pairs — row phase 0 in every role, row phase 1 in R2 / R3, all on five accumulator tuples — requests all nine
// operands (36 registers) at the end of the step before, ahead of the wave's input loads and, for R2 / R3, of the barrier the others
// reach thousands of cycles later. R0 / R1's row phase 1 (14 / 13 pairs on 8 / 7 tuples) requests C1_D there and the rest inside its
// MFMA loop: its own input loads come after that loop and R2 / R3's were issued a whole transform earlier.
constexpr int C1_D = 3;
constexpr int C1_UMAX = C1_UDEEP ? 9 : C1_D;
__host__ __device__ constexpr int c1_udepth(int R, int PY) {
  return C1_UDEEP == 2 ? (c1_entries(R, PY).n <= C1_UMAX ? C1_UMAX : C1_D) : C1_UDEEP && PY == (R >= 2) ? C1_UMAX : C1_D;
}
template <int R, int PY>
__device__ __forceinline__ void c1_upre(f32x4 (&ua)[C1_UMAX], const __amdgpu_buffer_rsrc_t rsrw, int lane) {
  constexpr C1Entries E = c1_entries(R, PY);
  static_assert(c1_udepth(R, PY) == C1_D || E.n <= C1_UMAX, "a deep step requests every U operand ahead");
#pragma unroll
  for (int e = 0; e < c1_udepth(R, PY); ++e)
    if (e < E.n) ua[e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrw, lane * 16, E.pair[e] * 1024, 0));
}

// the MFMAs of role R in row phase PY: per pair one 16-byte U load (rsrw: this channel half's U) and one ds_read_b128 of V, issued
// c1_udepth and C1_D pairs ahead of their use (ua: the first c1_udepth pairs' U, from c1_upre)
template <int R, int PY>
__device__ __forceinline__ void c1_mfma(f32x16 (&acc)[8], const char* smem, const __amdgpu_buffer_rsrc_t rsrw, int lane,
                                        f32x4 (&ua)[C1_UMAX], C1Tr& tr) {
  constexpr C1Entries E = c1_entries(R, PY);
  constexpr int D = C1_D, DU = c1_udepth(R, PY);
  const char* const vr = smem + (PY ? C1_V1 : 0) + lane * 16;
  f32x4 va[D];
  const f32x16 zero = {};
#pragma unroll
  for (int e = 0; e < D; ++e)
    if (e < E.n) va[e] = *reinterpret_cast<const f32x4*>(vr + (E.pair[e] - (PY ? C1_PY1 : 0)) * 1024);
#pragma unroll
  for (int e = 0; e < E.n; ++e) {
    const int s = e % D, su = e % DU;
    f32x16 c = E.first[e] ? zero : acc[E.q[e]];
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[su].x, va[s].x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[su].y, va[s].y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[su].z, va[s].z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[su].w, va[s].w, c, 0, 0, 0);
    acc[E.q[e]] = c;
    if (e + DU < E.n)
      ua[su] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrw, lane * 16, E.pair[e + DU] * 1024, 0));
    if (e + D < E.n) va[s] = *reinterpret_cast<const f32x4*>(vr + (E.pair[e + D] - (PY ? C1_PY1 : 0)) * 1024);
    if (e == D - 1) tr.template stamp<PY ? 7 : 1>();
    if (e == D) tr.template stamp<PY ? 8 : 2>();
  }
}

// nu-pass over the role's rows: S[xi][b] = sum_nu M[xi][nu] A^T[b][nu]. Y[0][b] = S0 + S1 + S2 + S3, Y[1][b] = S1 - S2 + S3/2 + S4.
// R0 keeps (S0 part) + S1 for row 0 and sends S1; R1 keeps S2 and sends (S0 part) + S2; R2 sends S3, R3 sends S4.
// xw: this wave's 8 KB of the exchange, [b][g][lane][4]
template <int R>
__device__ __forceinline__ void c1_send(const f32x16 (&acc)[8], f32x16 (&keep)[2], char* xw) {
  const f32x16 s0 = ((acc[0] + acc[1]) + acc[2]) + acc[3];
  const f32x16 s1 = ((acc[1] - acc[2]) + 0.5f * acc[3]) + acc[4];
  f32x16 o0 = s0, o1 = s1;
  if constexpr (R == 0) {
    keep[0] = ((acc[5] + acc[6]) + acc[7]) + s0;
    keep[1] = (acc[6] - acc[7]) + s1;
  } else if constexpr (R == 1) {
    keep[0] = s0;
    keep[1] = s1;
    o0 = acc[5] + s0;
    o1 = (0.5f * acc[5] + acc[6]) + s1;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *reinterpret_cast<f32x4*>(xw + g * 1024) = f32x4{o0[4 * g], o0[4 * g + 1], o0[4 * g + 2], o0[4 * g + 3]};
    *reinterpret_cast<f32x4*>(xw + (4 + g) * 1024) = f32x4{o1[4 * g], o1[4 * g + 1], o1[4 * g + 2], o1[4 * g + 3]};
  }
}

// R0 finishes output row 0, R1 row 1 of tile block `item`: the other waves' S from the exchange (xr: the channel half's 32 KB),
// bias, LeakyReLU, one 16-byte store per 4 channels and pixel. Lane: tile lane & 31, channels 8g + 4 (lane >> 5) + 0..3 of the half.
template <int R>
__device__ __forceinline__ void c1_finish(const f32x16 (&keep)[2], const char* xr, const float* bl, const C1Params& p, int item,
                                          int half, int lane) {
  const int txb = item % p.TXB, rr = item / p.TXB;
  const int ty = rr % p.TY, n = rr / p.TY;
  const int tx = txb * C1_TB + (lane & 31), hh = lane >> 5;
  const int yy = 2 * ty + R;
  if (tx >= p.TX || yy >= p.Ho) return;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int xx = 2 * tx + b;
    if (xx >= p.Wo) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int xo = (b * 4 + g) * 1024;
      const f32x4 k = {keep[b][4 * g], keep[b][4 * g + 1], keep[b][4 * g + 2], keep[b][4 * g + 3]};
      f32x4 v;
      if constexpr (R == 0) {
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(xr + 1 * 8192 + xo), x2 = *reinterpret_cast<const f32x4*>(xr + 2 * 8192 + xo);
        v = (k + x1) + x2;
      } else {
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(xr + xo), x2 = *reinterpret_cast<const f32x4*>(xr + 2 * 8192 + xo);
        const f32x4 x3 = *reinterpret_cast<const f32x4*>(xr + 3 * 8192 + xo);
        v = ((x0 - k) + 0.5f * x2) + x3;
      }
      const int o = half * 32 + 8 * g + 4 * hh;
      v += *reinterpret_cast<const f32x4*>(bl + o);   // from LDS: a global load here would wait behind the input loads
      v.x = v.x > 0.f ? v.x : v.x * p.slope; v.y = v.y > 0.f ? v.y : v.y * p.slope;
      v.z = v.z > 0.f ? v.z : v.z * p.slope; v.w = v.w > 0.f ? v.w : v.w * p.slope;
      const int cb = o >> 3, sub = o & 7;
      long off;
      if (p.out_s2d)   // pixel (yy, xx) of channel block cb -> block (phase*8 + cb) at (ty, tx) of (Ho/2, Wo/2)
        off = ((((long)n * 32 + (R * 2 + b) * 8 + cb) * (p.Ho >> 1) + ty) * (p.Wo >> 1) + tx) * 8 + sub;
      else
        off = ((((long)n * 8 + cb) * p.Ho + yy) * p.Wo + xx) * 8 + sub;
      *reinterpret_cast<f32x4*>(p.out + off) = v;
    }
  }
}

// one role's whole walk over the block's tile blocks. Step 0 of a tile block: MFMAs of row phase 0 (R0 / R1 first finish the previous
// tile block's output; R2 / R3 then transform this tile block's row phase 1). Step 1: R0 / R1 transform the next tile block's row
// phase 0; MFMAs of row phase 1; nu-pass and exchange. At the end of a step a wave requests the next step's U operands (c1_udepth of them) and
// then its next transform job's input (one and a half steps ahead), and every wave passes one barrier. No load is conditional: past
// the last tile block the input loads are out of range (zeros, no traffic), so the compiler's vmcnt waits stay counted.
template <int VEC, int R>
__device__ __forceinline__ void c1_body(const C1Params& p, char* smem, const int wave) {
  constexpr int TPY = R >= 2;   // the row phase this wave transforms
  const int lane = threadIdx.x & 63;
  const int half = wave & 1, tg = (wave >> 1) & 1;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
  const int per = (p.items + 7) >> 3;
  const int start = xcd * per, end = min(p.items, start + per);
  int item = start + slot;
  if (item >= end) return;   // block-uniform
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrw =
      __builtin_amdgcn_make_buffer_rsrc((void*)(p.wp + half * (C1_PAIRS * 64 * 4)), 0, C1_PAIRS * 64 * 16, 0x00020000);
  // transform job: tile tg * 16 + lane / 4 of the tile block, input channel 4 half + lane % 4
  const int c = 4 * half + (lane & 3), tl = tg * 16 + (lane >> 2);
  const unsigned vbase = half * 512 + tg * 256 + lane * 4;
  char* const xw = smem + C1_X + (half * 4 + R) * 8192 + lane * 16;
  const char* const xr = smem + C1_X + half * 4 * 8192 + lane * 16;
  const float* const bl = reinterpret_cast<const float*>(smem + C1_BIAS);
  auto load = [&](float (&raw)[5][10], int it) {
    const bool ok = it < end;
    it = ok ? it : end - 1;
    const int txb = it % p.TXB, rr = it / p.TXB;
    const int ty = rr % p.TY, n = rr / p.TY, tx = txb * C1_TB + tl;
    c1_load<VEC, TPY>(raw, rsrc, p, n, c, ty, tx, ok && tx < p.TX);
  };

  if (threadIdx.x < 64) reinterpret_cast<float*>(smem + C1_BIAS)[threadIdx.x] = p.bias ? p.bias[threadIdx.x] : 0.f;
  float raw[5][10];
  f32x16 acc[8], keep[2];
  f32x4 ua[C1_UMAX];
  load(raw, item);
  if constexpr (TPY == 0) {
    c1_transform<0>(raw, smem, vbase);
    c1_upre<R, 0>(ua, rsrw, lane);
    load(raw, item + nslot);
  } else {
    c1_upre<R, 0>(ua, rsrw, lane);
  }
  __syncthreads();
  C1Tr tr;
#if C1_TRACE
  for (int k = 0; k < 13; ++k) tr.seg[k] = 0;
  const unsigned tr_t0 = tr.a = tr.b = (unsigned)__builtin_amdgcn_s_memtime();
  unsigned tr_n = 0;
#endif
  int prev = -1;
  for (;;) {
    const int next = item + nslot;
    if constexpr (R < 2)
      if (prev >= 0) c1_finish<R>(keep, xr, bl, p, prev, half, lane);
    tr.template stamp<0>();
    c1_mfma<R, 0>(acc, smem, rsrw, lane, ua, tr);
    tr.template stamp<3>();
    if constexpr (TPY == 1) c1_transform<1>(raw, smem, vbase);
    c1_upre<R, 1>(ua, rsrw, lane);
    if constexpr (TPY == 1) load(raw, next);
    tr.template stamp<4>();
    __syncthreads();
    // nothing moves up across a barrier: the compiler otherwise starts R0 / R1's transform among the MFMAs of the step before, whose
    // second MFMA then waits for the input loads issued a moment earlier. (VEC = 0 keeps the compiler's order: with its 50 scalar
    // input loads in flight the pinned stream does not fit 256 registers.)
    if (C1_PIN && VEC) __builtin_amdgcn_sched_barrier(0);
    tr.template stamp<5>();
    if constexpr (TPY == 0) c1_transform<0>(raw, smem, vbase);   // past the last tile block: zeros nobody reads
    tr.template stamp<6>();
    c1_mfma<R, 1>(acc, smem, rsrw, lane, ua, tr);
    tr.template stamp<9>();
    c1_send<R>(acc, keep, xw);
    tr.template stamp<10>();
    c1_upre<R, 0>(ua, rsrw, lane);
    if constexpr (TPY == 0) load(raw, next + nslot);
    tr.template stamp<11>();
    __syncthreads();
    if (C1_PIN && VEC) __builtin_amdgcn_sched_barrier(0);
    tr.template stamp<12>();
#if C1_TRACE
    ++tr_n;
#endif
    prev = item;
    if (next >= end) break;
    item = next;
  }
#if C1_TRACE
  if (g_c1_trace && blockIdx.x == gridDim.x / 2 && lane == 0) {
    tr.seg[12] += tr.b - tr.a;
    unsigned* const o = g_c1_trace + wave * 16;
    for (int k = 0; k < 13; ++k) o[k] = tr.seg[k];
    o[13] = tr_n; o[14] = tr.b - tr_t0;
  }
#endif
  if constexpr (R < 2) c1_finish<R>(keep, xr, bl, p, prev, half, lane);
}

template <int VEC>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv1_wino_kernel(C1Params p) {
  __shared__ f32x4 lds4[C1_LDS / 16];
  char* const smem = reinterpret_cast<char*>(lds4);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the role is a compile-time constant of each body: the four roles run different streams
  switch (wave >> 1) {
    case 0: c1_body<VEC, 0>(p, smem, wave); break;
    case 1: c1_body<VEC, 1>(p, smem, wave); break;
    case 2: c1_body<VEC, 2>(p, smem, wave); break;
    default: c1_body<VEC, 3>(p, smem, wave); break;
  }
}

// U = G g G^T in double, rounded once, for every (half, pair, lane, s): output channel half*32 + lane % 32, input channel
// 4 (lane / 32) + s, phase (py, px) and position (xi, nu) of the pair; g = the phase's 4x4 sub-kernel w[2a + py - 1][2b + px - 1]
__global__ void pack_conv1_wino_kernel(float* __restrict__ packed, const float* __restrict__ w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C1_PACKED_FLOATS) return;
  const int s = i & 3, lane = (i >> 2) & 63, pr = (i >> 8) % C1_PAIRS, half = (i >> 8) / C1_PAIRS;
  int ph = 3;
  while (c1_pair0(ph) > pr) --ph;
  const int py = ph >> 1, px = ph & 1;
  const int q = pr - c1_pair0(ph), nnu = 5 - (px == 0);
  const int xi = q / nnu + (py == 0), nu = q % nnu + (px == 0);
  const int o = half * 32 + (lane & 31), c = 4 * (lane >> 5) + s;
  const double G[5][4] = {{1, 0, 0, 0}, {0.5, 0.5, 0.5, 0.5}, {1.0 / 6, -1.0 / 6, 1.0 / 6, -1.0 / 6},
                          {8.0 / 3, 4.0 / 3, 2.0 / 3, 1.0 / 3}, {0, 0, 0, 0.5}};
  double u = 0.0;
  for (int a = 0; a < 4; ++a) {
    const int ky = 2 * a + py - 1;
    if (ky < 0) continue;
    for (int b = 0; b < 4; ++b) {
      const int kx = 2 * b + px - 1;
      if (kx < 0) continue;
      u += G[xi][a] * G[nu][b] * (double)w[((o * 8 + c) * 7 + ky) * 7 + kx];
    }
  }
  packed[i] = (float)u;
}

}  // namespace

#if C1_TRACE
extern "C" int deepim_dev_c1_trace(void* buf) {
  unsigned* b = (unsigned*)buf;
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_c1_trace), &b, sizeof(b));
}
#endif

extern "C" size_t deepim_conv1_wino_packed_size(void) { return (size_t)C1_PACKED_FLOATS * sizeof(float); }

extern "C" int deepim_conv1_wino_preferred(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin != 8 || Cout != 64) return 0;
  if (ctx && ctx->conv_max_split == 1) return 0;      // canonical-order configuration: the direct kernel's fmaf chain
  if ((size_t)B * Cin * H * W * 4 >= (1ull << 31)) return 0;
  return 1;
}

extern "C" int deepim_conv1_wino_pack_weights(deepim_ctx* ctx, float* packed_w, const float* w) {
  DI_DEVICE(ctx);
  hipLaunchKernelGGL(pack_conv1_wino_kernel, dim3((C1_PACKED_FLOATS + 255) / 256), dim3(256), 0, ctx->stream, packed_w, w);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_conv1_wino_forward(deepim_ctx* ctx, float* out, const float* in, const float* packed_w, const float* bias,
                                         int B, int H, int W, float slope, int out_mode) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B > 0 && H > 0 && W > 0, "conv1_wino: empty input");
  DI_REQUIRE(out_mode == 1 || out_mode == 3, "conv1_wino: out_mode 1 (NC8) or 3 (NC8, space-to-depth order)");
  DI_REQUIRE((size_t)B * 8 * H * W * 4 < 0x7fffffffUL, "conv1_wino: input tensor must be < 2 GiB");
  C1Params p;
  p.in = in; p.wp = packed_w; p.bias = bias; p.out = out;
  p.B = B; p.H = H; p.W = W;
  p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1;
  if (out_mode == 3) DI_REQUIRE(((p.Ho | p.Wo) & 1) == 0, "conv1_wino: space-to-depth output needs even output height and width");
  p.TY = (p.Ho + 1) / 2; p.TX = (p.Wo + 1) / 2;
  p.TXB = (p.TX + C1_TB - 1) / C1_TB;
  const long items = (long)B * p.TY * p.TXB;
  DI_REQUIRE(items < (1L << 30), "conv1_wino: too many tiles");
  p.items = (int)items;
  p.out_s2d = out_mode == 3;
  p.slope = slope;
  p.in_bytes = (unsigned)((size_t)B * 8 * H * W * 4);
  // one block per CU (145 KB of LDS, two waves per SIMD): at most 32 per XCD, a multiple of 8
  const long per_xcd = (items + 7) / 8;
  const int grid = 8 * (int)std::min<long>(32, per_xcd);
  if ((W & 3) == 0)
    hipLaunchKernelGGL(conv1_wino_kernel<1>, dim3(grid), dim3(512), 0, ctx->stream, p);
  else
    hipLaunchKernelGGL(conv1_wino_kernel<0>, dim3(grid), dim3(512), 0, ctx->stream, p);
  DI_LAUNCH_CHECK();
  return 0;
}
