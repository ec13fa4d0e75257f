// fp16 Winograd F(2x2, 3x3) for the fp16 conv path's 3x3 stride-1 layers (conv3_1 / conv4_1 / conv5_1 / conv6_1), opt-in through
// network.FP16_WINOGRAD (default off). Same tensors as deepim_conv2d_f16_forward: NHWC fp16 in, NHWC fp16 out, Convolution 3x3
// stride 1 pad 1 + bias + LeakyReLU. A SECOND fp16 arithmetic, not the direct kernel's within one ulp (about 1.5x its per-layer
// error, tests/test_fp16_wino_host.py). G, B^T, A^T are the matrices of csrc/wino.hip (Lavin & Gray, points 0, +-1, inf).
//
// Arithmetic contract (restated in numpy by tests/fp16_wino_emulation.py):
//   weights   g = f16(w) (RNE), then in fp32, in THIS order of operations (no fused multiply-add: -ffp-contract=off), per column j
//               s = g[0][j] + g[2][j];  t[0][j] = g[0][j];  t[1][j] = (s + g[1][j]) * 0.5;  t[2][j] = (s - g[1][j]) * 0.5;  t[3][j] = g[2][j]
//             and per row i of t the same again:
//               s = t[i][0] + t[i][2];  U[i][0] = t[i][0];  U[i][1] = (s + t[i][1]) * 0.5;  U[i][2] = (s - t[i][1]) * 0.5;  U[i][3] = t[i][2]
//             then ONE rounding to fp16 (RNE). Position p = 4 i + nu (i: down the rows).
//   input     the 4x4 patch d of tile (ty, tx) = rows 2ty-1 .. 2ty+2, columns 2tx-1 .. 2tx+2; pixels outside the image are zeros (the
//             buffer load's out-of-range zero). Both passes in fp16 arithmetic, every entry ONE fp16 add or subtract (RNE):
//               T[0][j] = d[0][j] - d[2][j]   T[1][j] = d[1][j] + d[2][j]   T[2][j] = d[2][j] - d[1][j]   T[3][j] = d[1][j] - d[3][j]
//               V[i][0] = T[i][0] - T[i][2]   V[i][1] = T[i][1] + T[i][2]   V[i][2] = T[i][2] - T[i][1]   V[i][3] = T[i][1] - T[i][3]
//             — two fp16 roundings, on purpose: packed fp16 adds on the loaded halves keep the transform cheap beside fp16 MFMAs.
//   product   sixteen GEMMs M[p] = U[p] · V[p] over the input channels on v_mfma_f32_32x32x16_f16, fp32 accumulation, ONE block walks
//             all of Cin in ascending 16-channel steps: no K split, no atomics, bit-identical from run to run.
//   output    fp32: P[0][nu] = (M[0][nu] + M[1][nu]) + M[2][nu], P[1][nu] = (M[1][nu] - M[2][nu]) - M[3][nu], then
//             Y[a][0] = (P[a][0] + P[a][1]) + P[a][2], Y[a][1] = (P[a][1] - P[a][2]) - P[a][3]; + fp32 bias, LeakyReLU in fp32, one RNE
//             rounding to fp16. Odd H or W: the last tile row / column computes and drops its out-of-image outputs.
//   range     |V| <= 4 max|x|: an activation above about 16 000 can become inf here where the direct kernel would not. Not clamped.
//
// conv_wino_f16_kernel: block = 4 waves on 64 output channels x 64 tiles (2 x 2 waves of 32 channels x 32 tiles), every wave holds ALL
// 16 positions of its 32 x 32 (channel, tile) pairs: sixteen 32x32 accumulators = 256 registers, one wave per SIMD — the shape of
// conv_wino_kernel in csrc/wino.hip, so the output transform needs no exchange: a lane holds the 16 positions of its pairs.
//   * K step = 32 input channels. Producer (all 256 threads): thread = (tile t = tid / 4, octet o = tid % 4) loads the 16 patch pixels'
//     8 channels with sixteen 16-byte buffer loads (4 lanes = 64 contiguous bytes of a pixel), transforms them in packed fp16 and writes
//     V to LDS as [position][tile][4 slots][8 halves], slot = octet ^ ((tile >> 2) & 3) — the source-side XOR of csrc/conv_f16.hip: a
//     wave's ds_write_b128 covers 1 KB contiguous, a fragment's ds_read_b128 (32 tiles x one octet per half wave) every bank once.
//   * Consumer: per 16-channel sub-step and position one ds_read_b128 (V fragment) and one 16-byte global load (U fragment, in the
//     pack kernel's operand order: 1 KB contiguous per wave, served by L1 / L2), U loaded four positions ahead of its MFMAs.
//   * two V stages of 64 KB, one barrier per K step; the next step's patch loads are issued before this step's MFMAs.
#include "common.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int WF_BM = 64, WF_BT = 64;                 // block: output channels x tiles
constexpr int WF_STAGE = 16 * WF_BT * 4;              // h8 per V stage: [16 positions][64 tiles][4 slots]
constexpr int WF_LDS = 2 * WF_STAGE * 16;             // bytes: two stages

// a - b on eight halves as four v_pk_add_f16 with the second operand negated by the instruction's modifier — the same value bit for
// bit as the fp16 subtraction. (The compiler splits `a - b` on this vector type into sixteen scalar v_sub_f16 and eight packs;
// the additions it does emit as v_pk_add_f16.)
__device__ __forceinline__ h8 hsub(h8 a, h8 b) {
  const i32x4 x = __builtin_bit_cast(i32x4, a), y = __builtin_bit_cast(i32x4, b);
  i32x4 r;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int z;
    asm("v_pk_add_f16 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(z) : "v"(x[q]), "v"(y[q]));
    r[q] = z;
  }
  return __builtin_bit_cast(h8, r);
}

struct WinoF16Params {
  const void* in;       // NHWC fp16 (B,H,W,Cin)
  const h8* up;         // packed U (deepim_conv_wino_f16_pack_weights)
  const float* bias;
  _Float16* out;        // NHWC fp16 (B,H,W,Cout)
  int Cin, H, W, Cout, TY, TX, ntiles, gx;
  unsigned in_bytes;
  float slope;
};

// one thread per (co, ci): the 16 transformed taps, each to its place in the operand order
__global__ void pack_wino_f16_kernel(_Float16* __restrict__ packed, const float* __restrict__ w, int Cout, int Cin) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Cout * Cin) return;
  const int co = idx / Cin, ci = idx - co * Cin;
  float g[3][3], t[4][3];
#pragma unroll
  for (int a = 0; a < 9; ++a) g[a / 3][a % 3] = (float)(_Float16)w[(size_t)idx * 9 + a];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float s = g[0][j] + g[2][j];
    t[0][j] = g[0][j]; t[1][j] = (s + g[1][j]) * 0.5f; t[2][j] = (s - g[1][j]) * 0.5f; t[3][j] = g[2][j];
  }
  const int mb = co >> 5, k16 = ci >> 4, lane = (co & 31) + 32 * ((ci >> 3) & 1), e = ci & 7;
  _Float16* dst = packed + ((size_t)(mb * (Cin >> 4) + k16) * 16 * 64 + lane) * 8 + e;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float s = t[i][0] + t[i][2];
    const float u[4] = {t[i][0], (s + t[i][1]) * 0.5f, (s - t[i][1]) * 0.5f, t[i][2]};
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) dst[(size_t)(4 * i + nu) * 64 * 8] = (_Float16)u[nu];
  }
}

__global__ __launch_bounds__(256, 1) void conv_wino_f16_kernel(WinoF16Params p) {
  extern __shared__ __attribute__((aligned(16))) h8 smem[];   // [2 stages][16 positions][64 tiles][4 slots]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int bx = blockIdx.x % p.gx, mb = blockIdx.x / p.gx;   // consecutive blocks share a 64-channel slice of U
  const int lrow = lane >> 5, lcol = lane & 31;

  // producer: this thread's tile and octet, the byte offsets of its 16 patch pixels (bit 31 = outside the image or past the last tile)
  const int ptile = tid >> 2, oct = tid & 3;
  unsigned voff[16];
  {
    const int t = bx * WF_BT + ptile;
    const int per = p.TY * p.TX;
    const int n = t / per, r = t - n * per;
    const int ty = r / p.TX, tx = r - ty * p.TX;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int y = 2 * ty - 1 + i, x = 2 * tx - 1 + j;
        const bool ok = t < p.ntiles && y >= 0 && y < p.H && x >= 0 && x < p.W;
        voff[4 * i + j] = ok ? (unsigned)(((n * p.H + y) * p.W + x) * p.Cin * 2 + oct * 16) : 0x80000000u;
      }
  }
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  h8* const vdst = smem + ptile * 4 + (oct ^ ((ptile >> 2) & 3));      // + stage * WF_STAGE + position * (WF_BT * 4)

  h8 d[16];
  auto load_patch = [&](int ks) {
#pragma unroll
    for (int a = 0; a < 16; ++a)
      d[a] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff[a], ks * 64, 0));
  };
  auto transform_store = [&](int stage) {
    h8* dst = vdst + stage * WF_STAGE;
#pragma unroll
    for (int j = 0; j < 4; ++j) {     // row pass, column j of the patch, in place
      const h8 d0 = d[j], d1 = d[4 + j], d2 = d[8 + j], d3 = d[12 + j];
      d[j] = hsub(d0, d2); d[4 + j] = d1 + d2; d[8 + j] = hsub(d2, d1); d[12 + j] = hsub(d1, d3);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {     // column pass, row i of T
      const h8 t0 = d[4 * i], t1 = d[4 * i + 1], t2 = d[4 * i + 2], t3 = d[4 * i + 3];
      dst[(4 * i + 0) * (WF_BT * 4)] = hsub(t0, t2);
      dst[(4 * i + 1) * (WF_BT * 4)] = t1 + t2;
      dst[(4 * i + 2) * (WF_BT * 4)] = hsub(t2, t1);
      dst[(4 * i + 3) * (WF_BT * 4)] = hsub(t1, t3);
    }
  };

  f32x16 acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  const int nk = p.Cin >> 5;           // K steps of 32 channels = 2 sub-steps of 16
  // U fragments of this wave's 32 channels: [k16][position][lane] in h8 units
  const h8* const ubase = p.up + (size_t)(mb * 2 + wm) * (p.Cin >> 4) * (16 * 64) + lane;
  // V fragment of (position, sub-step): tile wn*32 + lcol, octet 2 sub + lrow → slot octet ^ ((tile >> 2) & 3)
  const int vt = wn * 32 + lcol, vsw = (vt >> 2) & 3;
  const h8* const vsrc = smem + vt * 4;

  load_patch(0);
  transform_store(0);
  __syncthreads();

  constexpr int UG = 4, NG = 32 / UG;   // U fragments per group, groups per K step (2 sub-steps x 16 positions)
  h8 uf[2][UG];
#pragma unroll
  for (int q = 0; q < UG; ++q) uf[0][q] = ubase[(size_t)q * 64];
  for (int ks = 0; ks < nk; ++ks) {
    const bool more = ks + 1 < nk;
    if (more) load_patch(ks + 1);
    const h8* vs = vsrc + (ks & 1) * WF_STAGE;
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {   // U of the next group of positions loads while this group multiplies
      const int sub = grp / (NG / 2), p0 = (grp % (NG / 2)) * UG;
      {
        // fragments [k16][position] are consecutive, so the next group follows this one; past the last K step the last group of
        // all once more (in range, unused)
        const int gn = min(ks * NG + grp + 1, nk * NG - 1);
        const h8* un = ubase + (size_t)gn * (UG * 64);
#pragma unroll
        for (int q = 0; q < UG; ++q) uf[(grp + 1) & 1][q] = un[(size_t)q * 64];
      }
#pragma unroll
      for (int q = 0; q < UG; ++q) {
        const h8 vf = vs[(p0 + q) * (WF_BT * 4) + ((sub * 2 + lrow) ^ vsw)];
        acc[p0 + q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(uf[grp & 1][q], vf, acc[p0 + q], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);   // keeps later groups' U loads from being hoisted over this one (register budget)
    }
    if (more) transform_store((ks + 1) & 1);
    __syncthreads();
  }

  // output transform in the lane that holds all 16 positions of (channel 8g + 4 lrow + r, tile lcol), bias + LeakyReLU, NHWC store
  const int t = bx * WF_BT + vt;
  if (t >= p.ntiles) return;
  const int per = p.TY * p.TX;
  const int n = t / per, rr = t - n * per;
  const int ty = rr / p.TX, tx = rr - ty * p.TX;
  const int y0 = 2 * ty, x0 = 2 * tx;
  const bool y1ok = y0 + 1 < p.H, x1ok = x0 + 1 < p.W;
  _Float16* const o00 = p.out + ((size_t)(n * p.H + y0) * p.W + x0) * p.Cout;
  const size_t rowstep = (size_t)p.W * p.Cout;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int co0 = mb * WF_BM + wm * 32 + 8 * g + 4 * lrow;
    const float4 bq = *reinterpret_cast<const float4*>(p.bias + co0);
    const float bias4[4] = {bq.x, bq.y, bq.z, bq.w};
    h4 y00, y01, y10, y11;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = 4 * g + r;
      float P[2][4];
#pragma unroll
      for (int nu = 0; nu < 4; ++nu) {
        P[0][nu] = (acc[nu][e] + acc[4 + nu][e]) + acc[8 + nu][e];
        P[1][nu] = (acc[4 + nu][e] - acc[8 + nu][e]) - acc[12 + nu][e];
      }
      float Y[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        Y[a][0] = (P[a][0] + P[a][1]) + P[a][2];
        Y[a][1] = (P[a][1] - P[a][2]) - P[a][3];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float v = Y[a][b] + bias4[r];
          Y[a][b] = v > 0.f ? v : v * p.slope;
        }
      }
      y00[r] = (_Float16)Y[0][0]; y01[r] = (_Float16)Y[0][1]; y10[r] = (_Float16)Y[1][0]; y11[r] = (_Float16)Y[1][1];
    }
    *reinterpret_cast<h4*>(o00 + co0) = y00;
    if (x1ok) *reinterpret_cast<h4*>(o00 + p.Cout + co0) = y01;
    if (y1ok) *reinterpret_cast<h4*>(o00 + rowstep + co0) = y10;
    if (y1ok && x1ok) *reinterpret_cast<h4*>(o00 + rowstep + p.Cout + co0) = y11;
    __builtin_amdgcn_sched_barrier(0);   // one channel quad at a time: all four quads' arithmetic ahead of the stores spills
  }
}

}  // namespace

extern "C" int deepim_conv_wino_f16_supported(int Cin, int Cout) {
  return Cin > 0 && Cout > 0 && (Cin & 31) == 0 && (Cout & 63) == 0 ? 1 : 0;
}

extern "C" size_t deepim_conv_wino_f16_packed_size(int Cout, int Cin) {
  return deepim_conv_wino_f16_supported(Cin, Cout) ? (size_t)Cout * Cin * 16 * sizeof(_Float16) : 0;
}

extern "C" int deepim_conv_wino_f16_pack_weights(deepim_ctx* ctx, void* packed, const float* w, int Cout, int Cin) {
  DI_DEVICE(ctx);
  DI_REQUIRE(deepim_conv_wino_f16_supported(Cin, Cout), "conv_wino_f16_pack: needs Cin % 32 == 0 and Cout % 64 == 0");
  hipLaunchKernelGGL(pack_wino_f16_kernel, dim3(di_div_up((long)Cout * Cin, 256)), dim3(256), 0, ctx->stream, (_Float16*)packed, w,
                     Cout, Cin);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_conv2d_wino_f16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const void* in_nhwc_f16, const void* packed_w,
                                              const float* bias, int B, int Cin, int H, int W, int Cout, float slope) {
  DI_DEVICE(ctx);
  DI_REQUIRE(deepim_conv_wino_f16_supported(Cin, Cout), "conv2d_wino_f16: needs Cin % 32 == 0 and Cout % 64 == 0");
  DI_REQUIRE(B >= 0 && H > 0 && W > 0 && bias != nullptr, "conv2d_wino_f16: bad shape or no bias");
  if (B == 0) return 0;
  WinoF16Params p;
  p.TY = (H + 1) / 2; p.TX = (W + 1) / 2;
  const long ntiles = (long)B * p.TY * p.TX;
  // bit 31 of a patch pixel's byte offset marks the zero padding, and the output offsets of a tile are ints before the channel scale
  DI_REQUIRE((size_t)B * H * W * Cin * 2 < 0x7fffffffUL && ntiles < (1L << 30), "conv2d_wino_f16: input must be < 2 GiB");
  p.in = in_nhwc_f16; p.up = (const h8*)packed_w; p.bias = bias; p.out = (_Float16*)out_nhwc_f16;
  p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.ntiles = (int)ntiles;
  p.gx = di_div_up(ntiles, WF_BT);
  p.in_bytes = (unsigned)((size_t)B * H * W * Cin * 2);
  p.slope = slope;
  static const char attr_tag = 0;   // function attributes are per DEVICE: remember them per context
  if (di_attr_needed(ctx, &attr_tag))
    DI_CHECK(hipFuncSetAttribute((const void*)conv_wino_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WF_LDS));
  hipLaunchKernelGGL(conv_wino_f16_kernel, dim3((unsigned)p.gx * (Cout / WF_BM)), dim3(256), WF_LDS, ctx->stream, p);
  DI_LAUNCH_CHECK();
  return 0;
}
