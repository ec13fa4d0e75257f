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
// Kernel (one wave per SIMD, persistent, no barrier after the prologue):
//   * a wave owns 32 output channels (a channel half) x 16 tiles (one tile row, consecutive tile columns) x all 25 positions:
//     25 x 2 accumulator tuples of v_mfma_f32_16x16x4_f32 (200 registers); lane (kq = lane / 16, t = lane % 16) is tile t and the
//     k index kq of the MFMA; k-step j multiplies input channel kq + 4j;
//   * the wave computes its own V: per (row phase py, k-step j) a lane loads the 5 x 10 input values its tile's patch needs in both
//     column phases (two 16-byte and one 8-byte load per row, straight from the NCHW net input; out-of-image rows / columns carry an
//     out-of-range buffer offset, which reads zero = the padding), and runs B^T d B in registers; the next unit's loads are issued
//     before the current unit's MFMAs;
//   * U of the block's channel half (81 pairs x 2 k-steps x 64 lanes x 2 floats = 81 KB) is copied into LDS once; a pair's A
//     operands are one ds_read_b64;
//   * output transform, bias and LeakyReLU in the lane: its 4 consecutive channels of each tuple leave as one 16-byte NC8 store per
//     output pixel (plain NC8, or space-to-depth NC8 for the stride-2 Winograd layer conv2).
//   * blocks = 4 waves of one channel half; block b works on XCD b % 8's contiguous eighth of the tile blocks, so that the tile rows
//     the waves of an XCD share (a patch spans 10 input rows, a tile row 4) are read into its L2 once.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int C1_PAIRS = 81;
constexpr int C1_TILES = 16;                                  // tiles per wave (one tile row)
constexpr int C1_HALF_FLOATS = C1_PAIRS * 2 * 64 * 2;         // packed U of one channel half

// first pair of phase ph = py*2 + px; positions (xi, nu) from (py == 0, px == 0) to 4 in row-major order
__host__ __device__ constexpr int c1_pair0(int ph) { return ph == 0 ? 0 : ph == 1 ? 16 : ph == 2 ? 36 : 56; }
__host__ __device__ constexpr int c1_pair(int py, int px, int xi, int nu) {
  return c1_pair0(py * 2 + px) + (xi - (py == 0)) * (5 - (px == 0)) + (nu - (px == 0));
}

struct C1Params {
  const float* in;      // (B, 8, H, W) NCHW
  const float* wp;      // packed U: [half][pair][j][lane][2]
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

// raw input of one unit (row phase, input channel): 5 patch rows x 10 input columns (column phase px = column & 1)
// VEC: W % 4 == 0 — every 16-byte (8-byte) load lies wholly inside or wholly outside its image row
template <int VEC>
__device__ __forceinline__ void c1_load(float (&raw)[5][10], const __amdgpu_buffer_rsrc_t rsrc, const C1Params& p, int n, int c,
                                        int ty, int tx, int py, bool live) {
  const int c0 = 4 * tx - 4;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const int row = 4 * ty - 4 + 2 * r + py;
    const bool rok = live && row >= 0 && row < p.H;
    const int base = ((n * 8 + c) * p.H + row) * p.W + c0;   // element index (row-valid lanes only use it)
    if constexpr (VEC) {
      const int o0 = rok && c0 >= 0 && c0 < p.W ? base * 4 : (int)0x80000000;
      const int o1 = rok && c0 + 4 < p.W ? base * 4 + 16 : (int)0x80000000;
      const int o2 = rok && c0 + 8 < p.W ? base * 4 + 32 : (int)0x80000000;
      const f32x4 a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o0, 0, 0));
      const f32x4 b = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o1, 0, 0));
      const f32x2 e = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, o2, 0, 0));
      raw[r][0] = a.x; raw[r][1] = a.y; raw[r][2] = a.z; raw[r][3] = a.w;
      raw[r][4] = b.x; raw[r][5] = b.y; raw[r][6] = b.z; raw[r][7] = b.w;
      raw[r][8] = e.x; raw[r][9] = e.y;
    } else {
#pragma unroll
      for (int q = 0; q < 10; ++q) {
        const int col = c0 + q;
        const int o = rok && col >= 0 && col < p.W ? (base + q) * 4 : (int)0x80000000;
        raw[r][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, o, 0, 0));
      }
    }
  }
}

// the MFMAs of one unit: both column phases of row phase PY, k-step J, from `raw`
template <int PY, int J>
__device__ __forceinline__ void c1_unit(f32x4 (&acc)[5][5][2], const float (&raw)[5][10], const float* __restrict__ ulds, int lane) {
#pragma unroll
  for (int px = 0; px < 2; ++px) {
    // row pass: T[r][nu] from patch row r (columns 2c + px)
    float T[5][5];
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
      for (int xi = (PY == 0); xi < 5; ++xi) {
        const int pr = c1_pair(PY, px, xi, nu);
        const f32x2 u = *reinterpret_cast<const f32x2*>(ulds + ((pr * 2 + J) * 64 + lane) * 2);
        acc[xi][nu][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(u.x, V[xi], acc[xi][nu][0], 0, 0, 0);
        acc[xi][nu][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(u.y, V[xi], acc[xi][nu][1], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);   // one column's V at a time: hoisted transforms run the register file out
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv1_wino_kernel(C1Params p) {
  __shared__ f32x4 ulds4[C1_HALF_FLOATS / 4];
  const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
  const int half = jb & 1, slot = jb >> 1, nslot = gridDim.x >> 4;
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(p.wp) + (size_t)half * (C1_HALF_FLOATS / 4);
    for (int i = threadIdx.x; i < C1_HALF_FLOATS / 4; i += 256) ulds4[i] = src[i];
  }
  __syncthreads();
  const float* ulds = reinterpret_cast<const float*>(ulds4);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = lane & 15, kq = lane >> 4;
  const int per = (p.items + 7) >> 3;
  const int start = xcd * per, end = min(p.items, start + per);
  const int stride = nslot * 4;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);

  int item = start + slot * 4 + wave;
  if (item >= end) return;
  // item -> (n, ty, tile column of this lane)
  auto decode = [&](int it, int& n, int& ty, int& tx) {
    const int txb = it % p.TXB, r = it / p.TXB;
    ty = r % p.TY; n = r / p.TY;
    tx = txb * C1_TILES + t;
  };
  float raw[2][5][10];
  int n, ty, tx;
  decode(item, n, ty, tx);
  c1_load<VEC>(raw[0], rsrc, p, n, kq, ty, tx, 0, tx < p.TX);
  for (;;) {
    const int next = item + stride;
    const bool more = next < end;
    int nn = 0, nty = 0, ntx = 0;
    if (more) decode(next, nn, nty, ntx);
    f32x4 acc[5][5][2];
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
      for (int b = 0; b < 5; ++b) acc[a][b][0] = acc[a][b][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool live = tx < p.TX;
    // units (py, j) = (0,0) (0,1) (1,0) (1,1); each issues the next unit's loads before its own MFMAs
    c1_load<VEC>(raw[1], rsrc, p, n, kq + 4, ty, tx, 0, live);
    c1_unit<0, 0>(acc, raw[0], ulds, lane);
    c1_load<VEC>(raw[0], rsrc, p, n, kq, ty, tx, 1, live);
    c1_unit<0, 1>(acc, raw[1], ulds, lane);
    c1_load<VEC>(raw[1], rsrc, p, n, kq + 4, ty, tx, 1, live);
    c1_unit<1, 0>(acc, raw[0], ulds, lane);
    if (more) c1_load<VEC>(raw[0], rsrc, p, nn, kq, nty, ntx, 0, ntx < p.TX);
    c1_unit<1, 1>(acc, raw[1], ulds, lane);

    // output transform Y = A^T M A per channel, bias, LeakyReLU, one 16-byte store per pixel and tuple
    if (live) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f32x4 R0[5], R1[5];   // rows of A^T M
#pragma unroll
        for (int nu = 0; nu < 5; ++nu) {
          R0[nu] = acc[0][nu][s] + acc[1][nu][s] + acc[2][nu][s] + acc[3][nu][s];
          R1[nu] = acc[1][nu][s] - acc[2][nu][s] + 0.5f * acc[3][nu][s] + acc[4][nu][s];
        }
        const int o = half * 32 + s * 16 + kq * 4;
        const f32x4 bv = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + o) : f32x4{0.f, 0.f, 0.f, 0.f};
        const int cb = o >> 3, sub = o & 7;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const f32x4* R = a ? R1 : R0;
          f32x4 y[2];
          y[0] = R[0] + R[1] + R[2] + R[3];
          y[1] = R[1] - R[2] + 0.5f * R[3] + R[4];
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int yy = 2 * ty + a, xx = 2 * tx + b;
            if (yy >= p.Ho || xx >= p.Wo) continue;
            f32x4 v = y[b] + bv;
            v.x = v.x > 0.f ? v.x : v.x * p.slope; v.y = v.y > 0.f ? v.y : v.y * p.slope;
            v.z = v.z > 0.f ? v.z : v.z * p.slope; v.w = v.w > 0.f ? v.w : v.w * p.slope;
            long off;
            if (p.out_s2d)   // pixel (yy, xx) of channel block cb -> block (phase*8 + cb) at (ty, tx) of (Ho/2, Wo/2)
              off = ((((long)n * 32 + (a * 2 + b) * 8 + cb) * (p.Ho >> 1) + ty) * (p.Wo >> 1) + tx) * 8 + sub;
            else
              off = ((((long)n * 8 + cb) * p.Ho + yy) * p.Wo + xx) * 8 + sub;
            *reinterpret_cast<f32x4*>(p.out + off) = v;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (!more) break;
    item = next; n = nn; ty = nty; tx = ntx;
  }
}

// U = G g G^T in double, rounded once, for every (half, pair, j, lane, s): output channel half*32 + s*16 + lane % 16, input channel
// lane / 16 + 4j, phase (py, px) and position (xi, nu) of the pair; g = the phase's 4x4 sub-kernel w[2a + py - 1][2b + px - 1]
__global__ void pack_conv1_wino_kernel(float* __restrict__ packed, const float* __restrict__ w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * C1_HALF_FLOATS) return;
  const int s = i & 1, lane = (i >> 1) & 63, j = (i >> 7) & 1, pr = (i >> 8) % C1_PAIRS, half = (i >> 8) / C1_PAIRS;
  int ph = 3;
  while (c1_pair0(ph) > pr) --ph;
  const int py = ph >> 1, px = ph & 1;
  const int q = pr - c1_pair0(ph), nnu = 5 - (px == 0);
  const int xi = q / nnu + (py == 0), nu = q % nnu + (px == 0);
  const int o = half * 32 + s * 16 + (lane & 15), c = (lane >> 4) + 4 * j;
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

extern "C" size_t deepim_conv1_wino_packed_size(void) { return (size_t)2 * C1_HALF_FLOATS * sizeof(float); }

extern "C" int deepim_conv1_wino_preferred(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin != 8 || Cout != 64) return 0;
  if (ctx && ctx->conv_max_split == 1) return 0;      // canonical-order configuration: the direct kernel's fmaf chain
  if ((size_t)B * Cin * H * W * 4 >= (1ull << 31)) return 0;
  return 1;
}

extern "C" int deepim_conv1_wino_pack_weights(deepim_ctx* ctx, float* packed_w, const float* w) {
  DI_DEVICE(ctx);
  hipLaunchKernelGGL(pack_conv1_wino_kernel, dim3((2 * C1_HALF_FLOATS + 255) / 256), dim3(256), 0, ctx->stream, packed_w, w);
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
  p.TXB = (p.TX + C1_TILES - 1) / C1_TILES;
  const long items = (long)B * p.TY * p.TXB;
  DI_REQUIRE(items < (1L << 30), "conv1_wino: too many tiles");
  p.items = (int)items;
  p.out_s2d = out_mode == 3;
  p.slope = slope;
  p.in_bytes = (unsigned)((size_t)B * 8 * H * W * 4);
  // one block per CU at most (81 KB of LDS, one wave per SIMD); a multiple of 16 = 8 XCDs x 2 channel halves
  const long per_xcd_half = (items + 31) / 32;   // 4 waves per block, 8 XCDs
  const int grid = 16 * (int)std::min<long>(16, std::max<long>(1, per_xcd_half));
  if ((W & 3) == 0)
    hipLaunchKernelGGL(conv1_wino_kernel<1>, dim3(grid), dim3(256), 0, ctx->stream, p);
  else
    hipLaunchKernelGGL(conv1_wino_kernel<0>, dim3(grid), dim3(256), 0, ctx->stream, p);
  DI_LAUNCH_CHECK();
  return 0;
}
