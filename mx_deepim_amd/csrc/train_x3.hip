// Split-fp16 ("x3") training of the encoder (TRAIN.X3_CONV): the backward of the x3 conv stack on the fp16 matrix cores at fp32
// grade, with a device-resident gradient scale. Numerics contract (split(v, s) = x3_split: hi = f16(clamp(v·s)),
// lo = f16(clamp(v·s) − hi), clamp at ±60000; S = the gradient scale, a power of two; the stored activations y_l are split16 at
// scale 16; a product of two pairs is hi·hi + hi·lo + lo·hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation):
//   e_l   the scaled gradient reaching the stored output y_l: S·(fc6 data gradient + d_dec61) at conv6_1, d_l [+ S·skip_l] below
//   dz_l  = split(lrelu'(y_l)·e_l, 1)   lrelu' from the sign of y_l's hi half; fp32 on hi + lo     deepim_lrelu_bias_backward_x3
//   db_l  = Σ dz_l / S                  fp32 sums of hi + lo in a fixed order                       deepim_lrelu_bias_backward_x3
//   dW_l  = Σ_pix dz_l ⊗ im2col(y_l-1) / (16·S)                                                    deepim_conv2d_wgrad_x3
//   d_l-1 = split(conv_transpose(dz_l, split(w_l, s_w)) / s_w, 1)                                  deepim_conv2d_dgrad_x3
// A clamp in any of these splits, or a non-finite value, raises word 2 of the scale state {scale, inv_scale, overflow, good_steps}.
// The forward kernels this file reuses (the data gradient is the x3 forward convolution) report a clamp through the context's status
// word; deepim_x3_status_to_state moves that bit into word 2 on the device. Underflow is not detected: a layer whose scaled
// maximum falls below about 2^-4 degrades towards fp16 grade, so S is chosen to keep every layer above it (profiles/r12_x3_train.md).
// No entry point syncs the host. Everything is deterministic: fixed slices, sums in a fixed order.
#include "common.h"
#include "train_s2.h"
#include "x3_split.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- fused activation gradient + bias gradient over split16 records -----------------------------------------------------------
// Block (channel group of 64, pixel slice): thread = 8 channels of a pixel (the hi octet and the lo octet of half a record), 32
// pixels per step. Per-thread fp32 sums, combined over the 32 pixel lanes in a fixed order, one partial per (slice, channel); the
// second pass adds the slices in order.
constexpr int LB_PIX = 32;
__global__ __launch_bounds__(256) void lrelu_bias_backward_x3_kernel(_Float16* dz, float* __restrict__ partial, const _Float16* d,
                                                                     const float* __restrict__ add, const _Float16* __restrict__ y,
                                                                     unsigned* __restrict__ state, float slope, int C, long hw,
                                                                     long npix, long per_slice) {
  const int tid = threadIdx.x, oc = tid & 7, pl = tid >> 3;
  const int c0 = blockIdx.x * 64 + oc * 8;
  const int rec = (c0 >> 4) * 32 + (c0 & 15);      // halves from the pixel's first record to this thread's hi octet; lo at + 16
  const long lo = (long)blockIdx.y * per_slice, hi = min(npix, lo + per_slice);
  const float S = __uint_as_float(state[0]);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool bad = false;
  for (long px = lo + pl; px < hi; px += LB_PIX) {
    const long off = px * (2 * C) + rec;
    const h8 yh = *reinterpret_cast<const h8*>(y + off);
    h8 dh, dl;
    if (d) {
      dh = *reinterpret_cast<const h8*>(d + off);
      dl = *reinterpret_cast<const h8*>(d + off + 16);
    }
    const long n = px / hw, r = px - n * hw;
    h8 oh, ol;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float e = d ? (float)dh[j] + (float)dl[j] : 0.f;
      if (add) e = d ? e + S * add[(n * C + c0 + j) * hw + r] : S * add[(n * C + c0 + j) * hw + r];
      e = (float)yh[j] > 0.f ? e : e * slope;
      bad |= !(fabsf(e) <= 60000.f);               // a clamp in the split, or a NaN
      const X3Pair s2 = x3_split(e, 1.f);
      oh[j] = s2.hi; ol[j] = s2.lo;
      acc[j] += (float)s2.hi + (float)s2.lo;
    }
    *reinterpret_cast<h8*>(dz + off) = oh;
    *reinterpret_cast<h8*>(dz + off + 16) = ol;
  }
  __shared__ float red[LB_PIX][65];
#pragma unroll
  for (int j = 0; j < 8; ++j) red[pl][oc * 8 + j] = acc[j];
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
    for (int i = 0; i < LB_PIX; ++i) s += red[i][tid];
    partial[(long)blockIdx.y * C + blockIdx.x * 64 + tid] = s;
  }
  if (bad) state[2] = 1u;
}

// block = one channel: thread t adds slices t, t + 256, … in order, then a fixed LDS tree
__global__ __launch_bounds__(256) void bias_x3_final_kernel(float* __restrict__ db, const float* __restrict__ partial, int C, int S,
                                                            unsigned* __restrict__ state) {
  const int c = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (int i = tid; i < S; i += 256) s += partial[(long)i * C + c];
  __shared__ float red[256];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const float v = red[0] * __uint_as_float(state[1]);
    db[c] = v;
    if (!__builtin_isfinite(v)) state[2] = 1u;
  }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------
// GEMM D[co][n] = Σ_pix dz[pix][co] · x[pix shifted by tap(n)][ci(n)], n = tap·Cin + ci: M = Cout, N = k²·Cin, K = pixels, each
// product as hi·hi + hi·lo + lo·hi. Both operands are split16 NHWC, so the reduction axis is the strided one. A 256-thread block
// owns a 128 x 128 tile of D. Per stage it stages 32 pixels of both operands in LDS as record-contiguous 512-byte rows: 128 real
// channels = 8 records = 32 chunks of 16 bytes, one coalesced 16-byte load per lane and row chunk, hardware zero fill for padding
// taps, pixels past the end and channels past Cout / N. Each wave owns 64 x 64 of the tile and reads, per 16-pixel k-step, the hi
// and lo fragments of its two 32-channel blocks of either operand with ds_read_b64_tr_b16: eight fragments for twelve MFMAs.
// Conflict-free LDS image: a transposed read of a 32-lane half touches rows k0 … k0 + 3 and, of each row, the four chunks
// {b, b + 1, b + 4, b + 5} (two 16-channel hi — or lo — runs, 32 halves apart because each record carries its lo half behind its
// hi half; b % 8 == 0 for hi, 2 for lo). Bits 0 and 2 of the chunk index vary inside a read, so the swizzle puts the row into bits
// 1 and 3: the 16 accesses land in 16 different 16-byte bank groups. A row chunk write covers 16 consecutive chunks per 16 lanes,
// which any XOR permutes among themselves. Split-K: fixed slices of the pixel range chosen from the geometry alone; slice partials
// are added in slice order by the second pass. The epilogue unscales by inv_scale / x_scale, checks finiteness and writes only the
// real channels.
constexpr int WX_BM = 128, WX_BN = 128, WX_BK = 32;
constexpr int WX_ROW_BYTES = 512;
constexpr int WX_TILE_BYTES = WX_BK * WX_ROW_BYTES;   // one operand, one stage: 32 rows x 256 halves
constexpr int WX_LDS = 4 * WX_TILE_BYTES;

struct WgX3Params {
  const _Float16* x;    // split16 (B,H,W,2·Cin)
  const _Float16* dz;   // split16 (B,Ho,Wo,2·Cout)
  float* dw;            // natural (Cout,Cin,k,k) or tap-major (Cout,k*k,Cin)
  float* partial;       // [S][Cout][N] when S > 1
  unsigned* state;
  int Cin, H, W, Cout, k, stride, pad, Ho, Wo, layout, N;
  long npix;
  int ksteps, S, steps_per_split, tiles_n;
  unsigned x_bytes, dz_bytes;
  float unscale;        // 1 / (scale of x)
};

__device__ __forceinline__ int wx_off(int row, int ch) { return WX_ROW_BYTES * row + 16 * (ch ^ (((row & 1) << 1) | ((row & 2) << 2))); }

// 8 K-consecutive halves (rows k0 + 8h .. k0 + 8h + 7) of the 32 real channels whose first hi (or lo) half is virtual column
// vcol of an image: lanes 0-15 / 32-47 take the record at vcol, lanes 16-31 / 48-63 the next one (32 halves on)
__device__ __forceinline__ h8 wx_frag(const char* img, int k0, int vcol, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3, h = g >> 1;
  const int ch = ((vcol + 32 * (g & 1)) >> 3) + (p >> 1);
  typedef __attribute__((address_space(3))) s4 lds_s4;
  const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(img + wx_off(k0 + 8 * h + q, ch) + 8 * (p & 1)));
  const s4 hi2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(img + wx_off(k0 + 8 * h + 4 + q, ch) + 8 * (p & 1)));
  return __builtin_bit_cast(h8, __builtin_shufflevector(lo, hi2, 0, 1, 2, 3, 4, 5, 6, 7));
}

__device__ __forceinline__ void wx_store(const WgX3Params& p, int co, int n, float v) {
  const int tap = n / p.Cin, ci = n - tap * p.Cin;
  v *= p.unscale * __uint_as_float(p.state[1]);
  if (!__builtin_isfinite(v)) p.state[2] = 1u;
  const int khw = p.k * p.k;
  const long o = p.layout ? ((long)co * khw + tap) * p.Cin + ci : ((long)co * p.Cin + ci) * khw + tap;
  p.dw[o] = v;
}

__global__ __launch_bounds__(256) void wgrad_x3_kernel(WgX3Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x - tm * p.tiles_n;
  const int m0 = tm * WX_BM, n0 = tn * WX_BN;
  const int split = blockIdx.y;
  const int s_begin = split * p.steps_per_split, s_end = min(p.ksteps, s_begin + p.steps_per_split);
  const int ch = tid & 31, r0 = tid >> 5;          // this thread stages chunk ch of rows r0, r0 + 8, r0 + 16, r0 + 24
  // dz chunk: virtual channels 2·m0 + 8ch .. +7 (half a record's hi or lo run)
  const int mv = 2 * m0 + 8 * ch;
  const bool a_ok = mv < 2 * p.Cout;
  // x chunk: virtual GEMM columns 2·n0 + 8ch .. +7 = half a record's hi or lo run of one tap
  const int nv = 2 * n0 + 8 * ch;
  const bool b_ok = nv < 2 * p.N;
  const int tap = b_ok ? nv / (2 * p.Cin) : 0, cv0 = b_ok ? nv - tap * 2 * p.Cin : 0;
  const int ky = tap / p.k, kx = tap - (tap / p.k) * p.k;
  const __amdgpu_buffer_rsrc_t rs_dz = __builtin_amdgcn_make_buffer_rsrc((void*)p.dz, 0, (int)p.dz_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const long hwo = (long)p.Ho * p.Wo;
  i32x4 areg[4], breg[4];
  auto load = [&](int s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long px = (long)s * WX_BK + r0 + 8 * e;
      unsigned oa = 0x80000000u, ob = 0x80000000u;      // out of range: the buffer load returns zeros
      if (px < p.npix) {
        if (a_ok) oa = (unsigned)((px * (2 * p.Cout) + mv) * 2);
        const long n = px / hwo, rr = px - n * hwo;
        const int oy = (int)(rr / p.Wo), ox = (int)(rr - (long)oy * p.Wo);
        const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
        if (b_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
          ob = (unsigned)((((n * p.H + iy) * p.W + ix) * (2 * p.Cin) + cv0) * 2);
      }
      areg[e] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_dz, (int)oa, 0, 0));
      breg[e] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)ob, 0, 0));
    }
  };
  auto stage = [&](int buf) {
    char* A = smem + buf * 2 * WX_TILE_BYTES;
    char* Bm = A + WX_TILE_BYTES;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      *reinterpret_cast<i32x4*>(A + wx_off(r0 + 8 * e, ch)) = areg[e];
      *reinterpret_cast<i32x4*>(Bm + wx_off(r0 + 8 * e, ch)) = breg[e];
    }
  };
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if (s_begin < s_end) {
    load(s_begin);
    stage(0);
    __syncthreads();
    for (int s = s_begin; s < s_end; ++s) {
      const int buf = (s - s_begin) & 1;
      if (s + 1 < s_end) load(s + 1);
      const char* A = smem + buf * 2 * WX_TILE_BYTES;
      const char* Bm = A + WX_TILE_BYTES;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        h8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          ah[i] = wx_frag(A, 16 * kk, 2 * (wm + 32 * i), lane);
          al[i] = wx_frag(A, 16 * kk, 2 * (wm + 32 * i) + 16, lane);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          bh[j] = wx_frag(Bm, 16 * kk, 2 * (wn + 32 * j), lane);
          bl[j] = wx_frag(Bm, 16 * kk, 2 * (wn + 32 * j) + 16, lane);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
          }
      }
      if (s + 1 < s_end) stage(buf ^ 1);
      __syncthreads();
    }
  }
  // C/D map of the 32x32 MFMA: column = lane & 31, row = 8 (r >> 2) + 4 (lane >> 5) + (r & 3)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn + 32 * j + (lane & 31);
      if (n >= p.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = m0 + wm + 32 * i + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        if (co >= p.Cout) continue;
        if (p.S > 1) p.partial[((long)split * p.Cout + co) * p.N + n] = acc[i][j][r];
        else wx_store(p, co, n, acc[i][j][r]);
      }
    }
}

__global__ __launch_bounds__(256) void wgrad_x3_reduce_kernel(WgX3Params p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)p.Cout * p.N;
  if (i >= total) return;
  float s = 0.f;
  for (int sl = 0; sl < p.S; ++sl) s += p.partial[(long)sl * total + i];
  wx_store(p, (int)(i / p.N), (int)(i % p.N), s);
}

// ---- scale state plumbing ---------------------------------------------------------------------------------------------------
// the saturation bit of the context's status word → word 2 of the scale state; the bit is cleared (the state word now carries it)
__global__ void x3_status_to_state_kernel(int* status, unsigned* state) {
  if (*status & DI_STATUS_X3_SATURATED) {
    state[2] = 1u;
    *status &= ~DI_STATUS_X3_SATURATED;
  }
}

// split16 NHWC → NCHW fp32 in real units: (hi + lo) · inv_scale · state[1]; lanes run along pixels of one channel
__global__ __launch_bounds__(256) void split16_to_nchw_unscaled_kernel(float* __restrict__ out, const _Float16* __restrict__ in,
                                                                       const unsigned* __restrict__ state, int C, long hw,
                                                                       float inv_scale, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long r = i % hw;
  const int c = (int)((i / hw) % C);
  const long n = i / (hw * C);
  const _Float16* rec = in + (n * hw + r) * (2 * C) + (c >> 4) * 32 + (c & 15);
  out[i] = ((float)rec[0] + (float)rec[16]) * (inv_scale * __uint_as_float(state[1]));
}

// a weight tensor against the scale its x3 pack was given: |w·s_w| > 60000 (the pack clamps there) or a NaN raises word 2
__global__ __launch_bounds__(256) void x3_weight_range_kernel(const float* __restrict__ w, long n, float w_scale,
                                                              unsigned* __restrict__ state) {
  bool bad = false;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) bad |= !(fabsf(w[i] * w_scale) <= 60000.f);
  if (bad) state[2] = 1u;
}

// bytes of the largest of the four parity-class weight packs of a stride-2 layer (the class buffer follows it in the workspace)
size_t x3_class_pack_bytes(int Ci_l, int Co_l, int k, int pad) {
  size_t pk = 0;
  for (int z = 0; z < 4; ++z) {
    const S2ClassF16 c = s2_class_f16(z, k, pad);
    pk = std::max(pk, deepim_conv_x3_packed_size(Ci_l, Co_l, c.nky, c.nkx));
  }
  return (pk + 255) / 256 * 256;
}

}  // namespace

extern "C" int deepim_lrelu_bias_backward_x3(deepim_ctx* ctx, void* dz_split16, float* db, const void* d_split16, const float* add_nchw,
                                             const void* y_split16, unsigned* state, float slope, int B, int C, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(C > 0 && C % 64 == 0, "lrelu_bias_backward_x3: C % 64 must be 0");
  DI_REQUIRE(d_split16 || add_nchw, "lrelu_bias_backward_x3: no incoming gradient");
  const long hw = (long)H * W, npix = (long)B * hw;
  if (npix == 0) {
    DI_CHECK(hipMemsetAsync(db, 0, (size_t)C * sizeof(float), ctx->stream));
    return 0;
  }
  const int groups = C / 64;
  int S = (int)std::max(1L, std::min((long)di_div_up(1024, groups), (long)di_div_up(npix, 1024)));
  const long per_slice = di_div_up(di_div_up(npix, (long)S), (long)LB_PIX) * LB_PIX;
  S = (int)di_div_up(npix, per_slice);
  void* scratch;
  int rc = deepim_scratch(ctx, (size_t)S * C * sizeof(float), &scratch);
  if (rc) return rc;
  hipLaunchKernelGGL(lrelu_bias_backward_x3_kernel, dim3(groups, S), dim3(256), 0, ctx->stream, (_Float16*)dz_split16, (float*)scratch,
                     (const _Float16*)d_split16, add_nchw, (const _Float16*)y_split16, state, slope, C, hw, npix, per_slice);
  hipLaunchKernelGGL(bias_x3_final_kernel, dim3(C), dim3(256), 0, ctx->stream, db, (const float*)scratch, C, S, state);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_conv2d_wgrad_x3(deepim_ctx* ctx, float* dw, const void* x_split16, const void* dz_split16, unsigned* state, int B,
                                      int Cin, int H, int W, int Cout, int k, int stride, int pad, int layout, float x_scale) {
  DI_DEVICE(ctx);
  DI_REQUIRE(Cin > 0 && Cin % 16 == 0 && Cout > 0 && Cout % 16 == 0 && k >= 1 && k <= 7,
             "conv2d_wgrad_x3: Cin % 16 and Cout % 16 must be 0 (whole split16 records), k <= 7");
  DI_REQUIRE(x_scale > 0.f, "conv2d_wgrad_x3: x_scale must be positive");
  WgX3Params p;
  p.x = (const _Float16*)x_split16; p.dz = (const _Float16*)dz_split16; p.dw = dw; p.state = state;
  p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.k = k; p.stride = stride; p.pad = pad;
  p.Ho = (H + 2 * pad - k) / stride + 1; p.Wo = (W + 2 * pad - k) / stride + 1;
  p.layout = layout ? 1 : 0;
  p.N = k * k * Cin;
  p.npix = (long)B * p.Ho * p.Wo;
  p.unscale = 1.f / x_scale;
  const size_t xb = (size_t)B * H * W * Cin * 4, zb = (size_t)p.npix * Cout * 4;
  DI_REQUIRE(xb < 0x7fffffffUL && zb < 0x7fffffffUL, "conv2d_wgrad_x3: operands must be < 2 GiB");
  p.x_bytes = (unsigned)xb; p.dz_bytes = (unsigned)zb;
  p.ksteps = (int)di_div_up(p.npix, (long)WX_BK);
  p.tiles_n = di_div_up(p.N, WX_BN);
  const int tiles = di_div_up(Cout, WX_BM) * p.tiles_n;
  // fixed slices from the geometry alone: about 512 blocks, never an empty slice
  int S = std::max(1, std::min(p.ksteps, di_div_up(512, tiles)));
  p.steps_per_split = di_div_up(std::max(p.ksteps, 1), S);
  p.S = di_div_up(std::max(p.ksteps, 1), p.steps_per_split);
  p.partial = nullptr;
  if (p.S > 1) {
    void* scratch;
    int rc = deepim_scratch(ctx, (size_t)p.S * Cout * p.N * sizeof(float), &scratch);
    if (rc) return rc;
    p.partial = (float*)scratch;
  }
  static const char attr_tag = 0;   // function attributes are per DEVICE: remember them per context
  if (di_attr_needed(ctx, &attr_tag))
    DI_CHECK(hipFuncSetAttribute((const void*)wgrad_x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WX_LDS));
  hipLaunchKernelGGL(wgrad_x3_kernel, dim3(tiles, p.S), dim3(256), WX_LDS, ctx->stream, p);
  if (p.S > 1)
    hipLaunchKernelGGL(wgrad_x3_reduce_kernel, dim3(di_div_up((long)Cout * p.N, 256L)), dim3(256), 0, ctx->stream, p);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t deepim_conv_dgrad_x3_workspace_size(int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad) {
  if (stride == 1) return deepim_conv_x3_packed_size(Ci_l, Co_l, k, k);
  const int Ho = (Hd + 2 * pad - k) / 2 + 1, Wo = (Wd + 2 * pad - k) / 2 + 1;
  size_t cls = 0;
  for (int z = 0; z < 4; ++z) {
    const S2ClassF16 c = s2_class_f16(z, k, pad);
    cls = std::max(cls, (size_t)B * (Ho + 2 * c.P - c.nky + 1) * (Wo + 2 * c.P - c.nkx + 1) * Ci_l * 4);
  }
  return x3_class_pack_bytes(Ci_l, Co_l, k, pad) + cls;
}

extern "C" int deepim_conv2d_dgrad_x3(deepim_ctx* ctx, void* dx_split16, const void* dz_split16, const float* w_layer, void* ws,
                                      unsigned* state, int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad,
                                      float w_scale) {
  DI_DEVICE(ctx);
  DI_REQUIRE(stride == 1 || stride == 2, "conv2d_dgrad_x3: stride 1 or 2");
  DI_REQUIRE(Co_l % 32 == 0 && Ci_l % 128 == 0, "conv2d_dgrad_x3: needs Co_l % 32 == 0 and Ci_l % 128 == 0");
  DI_REQUIRE(w_scale > 0.f, "conv2d_dgrad_x3: w_scale must be positive");
  if (B == 0) return 0;
  const float acc_scale = 1.f / w_scale;      // dz carries scale 1 (in units of S), and so does dx
  int rc;
  if (stride == 1) {
    const int P = k - 1 - pad;
    DI_REQUIRE(P >= 0 && Hd + 2 * pad - k + 1 > 0, "conv2d_dgrad_x3: pad > k - 1");
    const int Ho = Hd + 2 * pad - k + 1, Wo = Wd + 2 * pad - k + 1;
    rc = deepim_conv_x3_pack_dgrad(ctx, ws, w_layer, state, Co_l, Ci_l, k, 0, 0, 1, k, k, w_scale);
    if (rc) return rc;
    rc = deepim_conv2d_x3_forward(ctx, dx_split16, dz_split16, ws, nullptr, B, Co_l, Ho, Wo, Ci_l, k, k, 1, P, 1.f, acc_scale, 1.f);
    if (rc) return rc;
    return deepim_x3_status_to_state(ctx, state);
  }
  const int Ho = (Hd + 2 * pad - k) / 2 + 1, Wo = (Wd + 2 * pad - k) / 2 + 1;
  _Float16* cls = (_Float16*)((char*)ws + x3_class_pack_bytes(Ci_l, Co_l, k, pad));
  for (int z = 0; z < 4; ++z) {
    const S2ClassF16 c = s2_class_f16(z, k, pad);
    const int hq = (Hd - c.py + 1) / 2, wq = (Wd - c.px + 1) / 2;
    if (hq <= 0 || wq <= 0) continue;
    const int Hs = Ho + 2 * c.P - c.nky + 1, Ws = Wo + 2 * c.P - c.nkx + 1;
    DI_REQUIRE(c.cy + hq <= Hs && c.cx + wq <= Ws, "conv2d_dgrad_x3: class window outside the convolution result");
    rc = deepim_conv_x3_pack_dgrad(ctx, ws, w_layer, state, Co_l, Ci_l, k, c.ky0, c.kx0, 2, c.nky, c.nkx, w_scale);
    if (rc) return rc;
    rc = deepim_conv2d_x3_forward(ctx, cls, dz_split16, ws, nullptr, B, Co_l, Ho, Wo, Ci_l, c.nky, c.nkx, 1, c.P, 1.f, acc_scale, 1.f);
    if (rc) return rc;
    const long total = (long)B * hq * wq * (2 * Ci_l / 8);
    hipLaunchKernelGGL(stitch_f16_kernel, dim3(di_div_up(total, 256L)), dim3(256), 0, ctx->stream, (_Float16*)dx_split16, cls, 2 * Ci_l,
                       Hd, Wd, Hs, Ws, hq, wq, c.cy, c.cx, c.py, c.px, total);
    DI_LAUNCH_CHECK();
  }
  return deepim_x3_status_to_state(ctx, state);
}

extern "C" int deepim_x3_status_to_state(deepim_ctx* ctx, unsigned* state) {
  DI_DEVICE(ctx);
  hipLaunchKernelGGL(x3_status_to_state_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->status, state);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_split16_to_nchw_f32_unscaled(deepim_ctx* ctx, float* out, const void* in_split16, const unsigned* state, int B,
                                                   int C, int H, int W, float inv_scale) {
  DI_DEVICE(ctx);
  DI_REQUIRE((C & 15) == 0, "split16_to_nchw_unscaled: C must be a multiple of 16");
  const long total = (long)B * C * H * W;
  if (total == 0) return 0;
  hipLaunchKernelGGL(split16_to_nchw_unscaled_kernel, dim3(di_div_up(total, 256)), dim3(256), 0, ctx->stream, out,
                     (const _Float16*)in_split16, state, C, (long)H * W, inv_scale, total);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_x3_weight_range_check(deepim_ctx* ctx, const float* w, long n, float w_scale, unsigned* state) {
  DI_DEVICE(ctx);
  if (n <= 0) return 0;
  hipLaunchKernelGGL(x3_weight_range_kernel, dim3((unsigned)std::min(1024L, (n + 255) / 256)), dim3(256), 0, ctx->stream, w, n, w_scale,
                     state);
  DI_LAUNCH_CHECK();
  return 0;
}
