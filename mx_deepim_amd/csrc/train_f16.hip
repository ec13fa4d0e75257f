// Mixed-precision training of the encoder (network.FP16_CONV in the training graph): the backward of the fp16 conv stack on the
// fp16 matrix cores, with a device-resident loss scale. Numerics contract (q = round to fp16 (RNE) and back,
// S = the loss scale, a power of two):
//   e_l   the scaled gradient reaching the stored output y_l: S·(fc6 data gradient + d_dec61) at conv6_1, d_l [+ S·skip_l] below
//   dz_l  = q(lrelu'(y_l)·e_l)                                      NHWC fp16            deepim_lrelu_bias_backward_f16
//   db_l  = Σ dz_l / S                                              fp32 sums            deepim_lrelu_bias_backward_f16
//   dW_l  = Σ_pix dz_l ⊗ im2col(y_{l-1}) / S                         exact fp16 products, fp32 sums   deepim_conv2d_wgrad_f16
//   d_l-1 = q(conv_transpose(dz_l, q(w_l)))                          NHWC fp16            deepim_conv2d_dgrad_f16
// A non-finite dz / dW / db raises word 2 of the loss-scale state. Every d feeds the next layer's dz, so a non-finite d shows up
// there (lrelu' is 1 or 0.1, never 0). The state {scale, inv_scale, overflow, good_steps} is read by the kernels on the device:
// no step syncs the host.
#include "common.h"
#include "train_s2.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef _Float16 hf8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- fused activation gradient + bias gradient ----------------------------------------------------------------------------
// Block (channel group of 64, pixel slice): thread = one 8-channel octet of a pixel, 32 pixels per step. Per-thread fp32 sums,
// combined over the 32 pixel lanes in a fixed order, one partial per (slice, channel); the second pass adds the slices in order.
constexpr int LB_PIX = 32;
__global__ __launch_bounds__(256) void lrelu_bias_backward_f16_kernel(_Float16* dz, float* __restrict__ partial, const _Float16* d,
                                                                      const float* __restrict__ add, const _Float16* __restrict__ y,
                                                                      unsigned* __restrict__ state, float slope, int C, long hw,
                                                                      long npix, long per_slice) {
  const int tid = threadIdx.x, oc = tid & 7, pl = tid >> 3;
  const int c0 = blockIdx.x * 64 + oc * 8;
  const long lo = (long)blockIdx.y * per_slice, hi = min(npix, lo + per_slice);
  const float S = __uint_as_float(state[0]);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool bad = false;
  for (long px = lo + pl; px < hi; px += LB_PIX) {
    const long off = px * C + c0;
    const hf8 yv = *reinterpret_cast<const hf8*>(y + off);
    hf8 dv;
    if (d) dv = *reinterpret_cast<const hf8*>(d + off);
    const long n = px / hw, r = px - n * hw;
    hf8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float e = d ? (float)dv[j] : 0.f;
      if (add) e = d ? e + S * add[(n * C + c0 + j) * hw + r] : S * add[(n * C + c0 + j) * hw + r];
      e = (float)yv[j] > 0.f ? e : e * slope;
      out[j] = (_Float16)e;
      const float q = (float)out[j];
      bad |= !__builtin_isfinite(q);
      acc[j] += q;
    }
    *reinterpret_cast<hf8*>(dz + off) = out;
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

// block = one channel: thread t adds slices t, t + 256, … in order, then a fixed LDS tree (a serial walk over up to 1024 slices
// per channel was latency-bound: 35 us per layer)
__global__ __launch_bounds__(256) void bias_f16_final_kernel(float* __restrict__ db, const float* __restrict__ partial, int C, int S,
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
// GEMM D[co][n] = Σ_pix dz[pix][co] · x[pix shifted by tap(n)][ci(n)], n = tap·Cin_pad + ci: M = Cout, N = k²·Cin_pad, K = pixels.
// Both operands are NHWC fp16, so the reduction axis is the strided one. A 256-thread block owns a 128 x 128 tile of D; per stage
// it stages 32 pixels of both operands in LDS as channel-contiguous 256-byte rows (one coalesced 16-byte load per lane and row
// chunk, hardware zero fill for padding taps, pixels past the end and channels past Cout / N), and each wave reads its
// K-contiguous 32x32x16 fragments with ds_read_b64_tr_b16. Every lane takes part in every read (the tile is padded, not masked).
// Split-K: fixed slices of the pixel range chosen from the geometry alone; slice partials are added in slice order by the second
// pass. The epilogue unscales by inv_scale, checks finiteness and writes only the real channels.
constexpr int WG_BM = 128, WG_BN = 128, WG_BK = 32;
constexpr int WG_TILE_BYTES = WG_BK * 256;   // one operand, one stage: 32 rows x 128 halves

struct WgF16Params {
  const _Float16* x;    // (B,H,W,Cin_pad)
  const _Float16* dz;   // (B,Ho,Wo,Cout)
  float* dw;            // natural (Cout,Cin,k,k) or tap-major (Cout,k*k,Cin)
  float* partial;       // [S][Cout][N] when S > 1
  unsigned* state;
  int Cin, Cin_pad, H, W, Cout, k, stride, pad, Ho, Wo, layout, N;
  long npix;
  int ksteps, S, steps_per_split, tiles_n;
  unsigned x_bytes, dz_bytes;
};

// byte offset of 16-byte chunk ch of row `row` in a [32][128 halves] image: XOR swizzle that keeps both the row-chunk writes
// and the 32x32x16 transposed reads free of bank conflicts
__device__ __forceinline__ int wg_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// 8 K-consecutive halves (rows k0 + 8h .. k0 + 8h + 7) of column col_base + (lane & 31) of an image: two transposed reads
__device__ __forceinline__ h8 wg_frag(const char* img, int k0, int col_base, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3, h = g >> 1;
  const int ch = ((col_base + 16 * (g & 1)) >> 3) + (p >> 1);
  typedef __attribute__((address_space(3))) s4 lds_s4;
  const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(img + wg_off(k0 + 8 * h + q, ch) + 8 * (p & 1)));
  const s4 hi2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(img + wg_off(k0 + 8 * h + 4 + q, ch) + 8 * (p & 1)));
  return __builtin_bit_cast(h8, __builtin_shufflevector(lo, hi2, 0, 1, 2, 3, 4, 5, 6, 7));
}

__device__ __forceinline__ void wg_store(const WgF16Params& p, int co, int n, float v) {
  const int tap = n / p.Cin_pad, ci = n - tap * p.Cin_pad;
  if (ci >= p.Cin) return;
  v *= __uint_as_float(p.state[1]);
  if (!__builtin_isfinite(v)) p.state[2] = 1u;
  const int khw = p.k * p.k;
  const long o = p.layout ? ((long)co * khw + tap) * p.Cin + ci : ((long)co * p.Cin + ci) * khw + tap;
  p.dw[o] = v;
}

__global__ __launch_bounds__(256) void wgrad_f16_kernel(WgF16Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x - tm * p.tiles_n;
  const int m0 = tm * WG_BM, n0 = tn * WG_BN;
  const int split = blockIdx.y;
  const int s_begin = split * p.steps_per_split, s_end = min(p.ksteps, s_begin + p.steps_per_split);
  const int ch = tid & 15, r0 = tid >> 4;          // this thread stages chunk ch of rows r0 and r0 + 16
  // dz chunk: channels m0 + 8ch .. +7
  const bool a_ok = m0 + 8 * ch < p.Cout;
  // x chunk: GEMM columns n0 + 8ch .. +7 = one octet of one tap
  const int nn = n0 + 8 * ch;
  const bool b_ok = nn < p.N;
  const int tap = b_ok ? nn / p.Cin_pad : 0, ci0 = b_ok ? nn - tap * p.Cin_pad : 0;
  const int ky = tap / p.k, kx = tap - (tap / p.k) * p.k;
  const __amdgpu_buffer_rsrc_t rs_dz = __builtin_amdgcn_make_buffer_rsrc((void*)p.dz, 0, (int)p.dz_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const long hwo = (long)p.Ho * p.Wo;
  i32x4 areg[2], breg[2];
  auto load = [&](int s) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const long px = (long)s * WG_BK + r0 + 16 * e;
      unsigned oa = 0x80000000u, ob = 0x80000000u;      // out of range: the buffer load returns zeros
      if (px < p.npix) {
        if (a_ok) oa = (unsigned)((px * p.Cout + m0 + 8 * ch) * 2);
        const long n = px / hwo, rr = px - n * hwo;
        const int oy = (int)(rr / p.Wo), ox = (int)(rr - (long)oy * p.Wo);
        const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
        if (b_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
          ob = (unsigned)((((n * p.H + iy) * p.W + ix) * p.Cin_pad + ci0) * 2);
      }
      areg[e] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_dz, (int)oa, 0, 0));
      breg[e] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)ob, 0, 0));
    }
  };
  auto stage = [&](int buf) {
    char* A = smem + buf * 2 * WG_TILE_BYTES;
    char* Bm = A + WG_TILE_BYTES;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      *reinterpret_cast<i32x4*>(A + wg_off(r0 + 16 * e, ch)) = areg[e];
      *reinterpret_cast<i32x4*>(Bm + wg_off(r0 + 16 * e, ch)) = breg[e];
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
      const char* A = smem + buf * 2 * WG_TILE_BYTES;
      const char* Bm = A + WG_TILE_BYTES;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        h8 af[2], bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = wg_frag(A, 16 * kk, wm + 32 * i, lane);
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = wg_frag(Bm, 16 * kk, wn + 32 * j, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
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
        else wg_store(p, co, n, acc[i][j][r]);
      }
    }
}

__global__ __launch_bounds__(256) void wgrad_f16_reduce_kernel(WgF16Params p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)p.Cout * p.N;
  if (i >= total) return;
  float s = 0.f;
  for (int sl = 0; sl < p.S; ++sl) s += p.partial[(long)sl * total + i];
  wg_store(p, (int)(i / p.N), (int)(i % p.N), s);
}

__global__ void amp_scale_update_kernel(unsigned* state, int window) {
  float s = __uint_as_float(state[0]);
  unsigned good = state[3];
  if (state[2]) {
    s = fmaxf(1.f, 0.5f * s);
    good = 0;
  } else if (++good >= (unsigned)window) {
    s = fminf(16777216.f, 2.f * s);
    good = 0;
  }
  state[0] = __float_as_uint(s);
  state[1] = __float_as_uint(1.f / s);
  state[2] = 0u;
  state[3] = good;
}

}  // namespace

extern "C" int deepim_lrelu_bias_backward_f16(deepim_ctx* ctx, void* dz_nhwc_f16, float* db, const void* d_nhwc_f16, const float* add_nchw,
                                              const void* y_nhwc_f16, unsigned* state, float slope, int B, int C, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(C > 0 && C % 64 == 0, "lrelu_bias_backward_f16: C % 64 must be 0");
  DI_REQUIRE(d_nhwc_f16 || add_nchw, "lrelu_bias_backward_f16: no incoming gradient");
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
  hipLaunchKernelGGL(lrelu_bias_backward_f16_kernel, dim3(groups, S), dim3(256), 0, ctx->stream, (_Float16*)dz_nhwc_f16, (float*)scratch,
                     (const _Float16*)d_nhwc_f16, add_nchw, (const _Float16*)y_nhwc_f16, state, slope, C, hw, npix, per_slice);
  hipLaunchKernelGGL(bias_f16_final_kernel, dim3(C), dim3(256), 0, ctx->stream, db, (const float*)scratch, C, S, state);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_conv2d_wgrad_f16(deepim_ctx* ctx, float* dw, const void* x_nhwc_f16, const void* dz_nhwc_f16, unsigned* state,
                                       int B, int Cin, int Cin_pad, int H, int W, int Cout, int k, int stride, int pad, int layout) {
  DI_DEVICE(ctx);
  DI_REQUIRE(Cin_pad % 8 == 0 && Cin <= Cin_pad && Cin > 0 && Cout % 8 == 0 && Cout > 0 && k >= 1 && k <= 7,
             "conv2d_wgrad_f16: Cin_pad % 8, Cout % 8 must be 0, Cin <= Cin_pad, k <= 7");
  WgF16Params p;
  p.x = (const _Float16*)x_nhwc_f16; p.dz = (const _Float16*)dz_nhwc_f16; p.dw = dw; p.state = state;
  p.Cin = Cin; p.Cin_pad = Cin_pad; p.H = H; p.W = W; p.Cout = Cout; p.k = k; p.stride = stride; p.pad = pad;
  p.Ho = (H + 2 * pad - k) / stride + 1; p.Wo = (W + 2 * pad - k) / stride + 1;
  p.layout = layout ? 1 : 0;
  p.N = k * k * Cin_pad;
  p.npix = (long)B * p.Ho * p.Wo;
  const size_t xb = (size_t)B * H * W * Cin_pad * 2, zb = (size_t)p.npix * Cout * 2;
  DI_REQUIRE(xb < 0x7fffffffUL && zb < 0x7fffffffUL, "conv2d_wgrad_f16: operands must be < 2 GiB");
  p.x_bytes = (unsigned)xb; p.dz_bytes = (unsigned)zb;
  p.ksteps = (int)di_div_up(p.npix, (long)WG_BK);
  p.tiles_n = di_div_up(p.N, WG_BN);
  const int tiles = di_div_up(Cout, WG_BM) * p.tiles_n;
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
  hipLaunchKernelGGL(wgrad_f16_kernel, dim3(tiles, p.S), dim3(256), 4 * WG_TILE_BYTES, ctx->stream, p);
  if (p.S > 1)
    hipLaunchKernelGGL(wgrad_f16_reduce_kernel, dim3(di_div_up((long)Cout * p.N, 256L)), dim3(256), 0, ctx->stream, p);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t deepim_conv_dgrad_f16_workspace_size(int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad) {
  if (stride == 1) return deepim_conv_f16_packed_size(Ci_l, Co_l, k, k);
  const int Ho = (Hd + 2 * pad - k) / 2 + 1, Wo = (Wd + 2 * pad - k) / 2 + 1;
  size_t pk = 0, cls = 0;
  for (int z = 0; z < 4; ++z) {
    const S2ClassF16 c = s2_class_f16(z, k, pad);
    pk = std::max(pk, deepim_conv_f16_packed_size(Ci_l, Co_l, c.nky, c.nkx));
    cls = std::max(cls, (size_t)B * (Ho + 2 * c.P - c.nky + 1) * (Wo + 2 * c.P - c.nkx + 1) * Ci_l * 2);
  }
  return (pk + 255) / 256 * 256 + cls;
}

extern "C" int deepim_conv2d_dgrad_f16(deepim_ctx* ctx, void* dx_nhwc_f16, const void* dz_nhwc_f16, const float* w_layer, void* ws,
                                       int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad) {
  DI_DEVICE(ctx);
  DI_REQUIRE(stride == 1 || stride == 2, "conv2d_dgrad_f16: stride 1 or 2");
  DI_REQUIRE(Co_l % 8 == 0 && Ci_l % 8 == 0, "conv2d_dgrad_f16: channel counts must be multiples of 8");
  if (B == 0) return 0;
  if (stride == 1) {
    const int P = k - 1 - pad;
    DI_REQUIRE(P >= 0 && Hd + 2 * pad - k + 1 > 0, "conv2d_dgrad_f16: pad > k - 1");
    const int Ho = Hd + 2 * pad - k + 1, Wo = Wd + 2 * pad - k + 1;
    int rc = deepim_conv_f16_pack_dgrad(ctx, ws, w_layer, Co_l, Ci_l, k, 0, 0, 1, k, k);
    if (rc) return rc;
    return deepim_conv2d_f16_forward(ctx, dx_nhwc_f16, dz_nhwc_f16, ws, nullptr, B, Co_l, Ho, Wo, Ci_l, k, k, 1, P, 1.f);
  }
  const int Ho = (Hd + 2 * pad - k) / 2 + 1, Wo = (Wd + 2 * pad - k) / 2 + 1;
  size_t pk = 0;
  for (int z = 0; z < 4; ++z) {
    const S2ClassF16 c = s2_class_f16(z, k, pad);
    pk = std::max(pk, deepim_conv_f16_packed_size(Ci_l, Co_l, c.nky, c.nkx));
  }
  _Float16* cls = (_Float16*)((char*)ws + (pk + 255) / 256 * 256);
  for (int z = 0; z < 4; ++z) {
    const S2ClassF16 c = s2_class_f16(z, k, pad);
    const int hq = (Hd - c.py + 1) / 2, wq = (Wd - c.px + 1) / 2;
    if (hq <= 0 || wq <= 0) continue;
    const int Hs = Ho + 2 * c.P - c.nky + 1, Ws = Wo + 2 * c.P - c.nkx + 1;
    DI_REQUIRE(c.cy + hq <= Hs && c.cx + wq <= Ws, "conv2d_dgrad_f16: class window outside the convolution result");
    int rc = deepim_conv_f16_pack_dgrad(ctx, ws, w_layer, Co_l, Ci_l, k, c.ky0, c.kx0, 2, c.nky, c.nkx);
    if (rc) return rc;
    rc = deepim_conv2d_f16_forward(ctx, cls, dz_nhwc_f16, ws, nullptr, B, Co_l, Ho, Wo, Ci_l, c.nky, c.nkx, 1, c.P, 1.f);
    if (rc) return rc;
    const long total = (long)B * hq * wq * (Ci_l / 8);
    hipLaunchKernelGGL(stitch_f16_kernel, dim3(di_div_up(total, 256L)), dim3(256), 0, ctx->stream, (_Float16*)dx_nhwc_f16, cls, Ci_l,
                       Hd, Wd, Hs, Ws, hq, wq, c.cy, c.cx, c.py, c.px, total);
    DI_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int deepim_amp_scale_update(deepim_ctx* ctx, unsigned* state, int window) {
  DI_DEVICE(ctx);
  DI_REQUIRE(window >= 1, "amp_scale_update: window must be >= 1");
  hipLaunchKernelGGL(amp_scale_update_kernel, dim3(1), dim3(1), 0, ctx->stream, state, window);
  DI_LAUNCH_CHECK();
  return 0;
}
