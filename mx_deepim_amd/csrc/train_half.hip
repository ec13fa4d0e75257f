// Half-precision training of the encoder: the backward of the conv stack on the fp16 matrix cores with a device-resident scale, in
// two representations served by one body each, `bool X3` being the compile-time switch (as conv_f16.hip does for the forward):
//   fp16 (X3 = false)  network.FP16_CONV in the training graph, DESIGN.md §8f-4c. Tensors are NHWC fp16; q = round to fp16 (RNE)
//                      and back; S = the loss scale.
//   x3   (X3 = true)   TRAIN.X3_CONV, split-fp16 at fp32 grade, DESIGN.md §8f-4e. Tensors are split16 NHWC (records of 16 hi halves
//                      followed by their 16 lo halves); split(v, s) = x3_split: hi = f16(clamp(v·s)), lo = f16(clamp(v·s) − hi),
//                      clamp at ±60000; the stored activations y_l are split16 at scale 16; a product of two pairs is hi·hi + hi·lo +
//                      lo·hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation; S = the gradient scale.
// Numerics contract, S a power of two in either mode:
//   e_l   the scaled gradient reaching the stored output y_l: S·(fc6 data gradient + d_dec61) at conv6_1, d_l [+ S·skip_l] below
//   dz_l  fp16: q(lrelu'(y_l)·e_l)                                                              deepim_lrelu_bias_backward_{f16,x3}
//         x3:   split(lrelu'(y_l)·e_l, 1), lrelu' from the sign of y_l's hi half, fp32 on hi + lo
//   db_l  = Σ dz_l / S              fp32 sums in a fixed order (x3: of hi + lo)                  deepim_lrelu_bias_backward_{f16,x3}
//   dW_l  fp16: Σ_pix dz_l ⊗ im2col(y_l-1) / S, exact fp16 products, fp32 sums                  deepim_conv2d_wgrad_{f16,x3}
//         x3:   Σ_pix dz_l ⊗ im2col(y_l-1) / (16·S)
//   d_l-1 fp16: q(conv_transpose(dz_l, q(w_l)))                                                 deepim_conv2d_dgrad_{f16,x3}
//         x3:   split(conv_transpose(dz_l, split(w_l, s_w)) / s_w, 1)
// The state {scale, inv_scale, overflow, good_steps} is read by the kernels on the device: no entry point syncs the host, and
// everything is deterministic (fixed slices, sums in a fixed order). What raises word 2 of it:
//   fp16: a non-finite dz / dW / db. Every d feeds the next layer's dz, so a non-finite d shows up there (lrelu' is 1 or 0.1,
//         never 0).
//   x3:   a clamp in any of the splits above, or a non-finite value. The forward kernels this file reuses (the data gradient is the
//         x3 forward convolution) report a clamp through the context's status word; deepim_x3_status_to_state moves that bit into
//         word 2 on the device. Underflow is not detected: a layer whose scaled maximum falls below about 2^-4 degrades towards
//         fp16 grade, so S is chosen to keep every layer above it (profiles/r12_x3_train.md).
#include "common.h"
#include "x3_split.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// one text for the checks both modes make: the entry point's own name goes in front
#define HALF_MSG(fn, text) (X3 ? fn "_x3: " text : fn "_f16: " text)

// ---- fused activation gradient + bias gradient ----------------------------------------------------------------------------
// Block (channel group of 64, pixel slice): thread = 8 channels of a pixel (fp16: one octet; x3: the hi octet and the lo octet of
// half a record), 32 pixels per step. Per-thread fp32 sums, combined over the 32 pixel lanes in a fixed order, one partial per
// (slice, channel); the second pass adds the slices in order.
constexpr int LB_PIX = 32;
template <bool X3>
__global__ __launch_bounds__(256) void lrelu_bias_backward_half_kernel(_Float16* dz, float* __restrict__ partial, const _Float16* d,
                                                                       const float* __restrict__ add, const _Float16* __restrict__ y,
                                                                       unsigned* __restrict__ state, float slope, int C, long hw,
                                                                       long npix, long per_slice) {
  const int tid = threadIdx.x, oc = tid & 7, pl = tid >> 3;
  const int c0 = blockIdx.x * 64 + oc * 8;
  // halves from the pixel's first channel to this thread's octet; x3: to its hi octet, lo at + 16
  const int rec = X3 ? (c0 >> 4) * 32 + (c0 & 15) : c0;
  const int pitch = X3 ? 2 * C : C;
  const long lo = (long)blockIdx.y * per_slice, hi = min(npix, lo + per_slice);
  const float S = __uint_as_float(state[0]);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool bad = false;
  for (long px = lo + pl; px < hi; px += LB_PIX) {
    const long off = px * pitch + rec;
    const h8 yh = *reinterpret_cast<const h8*>(y + off);
    h8 dh, dl;
    if (d) {
      dh = *reinterpret_cast<const h8*>(d + off);
      if constexpr (X3) dl = *reinterpret_cast<const h8*>(d + off + 16);
    }
    const long n = px / hw, r = px - n * hw;
    h8 oh, ol;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float e = 0.f;
      if (d) {
        if constexpr (X3) e = (float)dh[j] + (float)dl[j];
        else e = (float)dh[j];
      }
      if (add) e = d ? e + S * add[(n * C + c0 + j) * hw + r] : S * add[(n * C + c0 + j) * hw + r];
      e = (float)yh[j] > 0.f ? e : e * slope;
      if constexpr (X3) {
        bad |= !(fabsf(e) <= 60000.f);               // a clamp in the split, or a NaN
        const X3Pair s2 = x3_split(e, 1.f);
        oh[j] = s2.hi; ol[j] = s2.lo;
        acc[j] += (float)s2.hi + (float)s2.lo;
      } else {
        oh[j] = (_Float16)e;
        const float q = (float)oh[j];
        bad |= !__builtin_isfinite(q);
        acc[j] += q;
      }
    }
    *reinterpret_cast<h8*>(dz + off) = oh;
    if constexpr (X3) *reinterpret_cast<h8*>(dz + off + 16) = ol;
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
__global__ __launch_bounds__(256) void bias_final_kernel(float* __restrict__ db, const float* __restrict__ partial, int C, int S,
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

template <bool X3>
int launch_lrelu_bias_backward(deepim_ctx* ctx, void* dz, float* db, const void* d, const float* add_nchw, const void* y, unsigned* state,
                               float slope, int B, int C, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(C > 0 && C % 64 == 0, HALF_MSG("lrelu_bias_backward", "C % 64 must be 0"));
  DI_REQUIRE(d || add_nchw, HALF_MSG("lrelu_bias_backward", "no incoming gradient"));
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
  hipLaunchKernelGGL(lrelu_bias_backward_half_kernel<X3>, dim3(groups, S), dim3(256), 0, ctx->stream, (_Float16*)dz, (float*)scratch,
                     (const _Float16*)d, add_nchw, (const _Float16*)y, state, slope, C, hw, npix, per_slice);
  hipLaunchKernelGGL(bias_final_kernel, dim3(C), dim3(256), 0, ctx->stream, db, (const float*)scratch, C, S, state);
  DI_LAUNCH_CHECK();
  return 0;
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------
// GEMM D[co][n] = Σ_pix dz[pix][co] · x[pix shifted by tap(n)][ci(n)], n = tap·Cin_pad + ci: M = Cout, N = k²·Cin_pad, K = pixels
// (x3: Cin_pad = Cin, each product as hi·hi + hi·lo + lo·hi). Both operands are NHWC, so the reduction axis is the strided one. A
// 256-thread block owns a 128 x 128 tile of D; per stage it stages 32 pixels of both operands in LDS as channel-contiguous rows of
// the tile's 128 channels (one coalesced 16-byte load per lane and row chunk, hardware zero fill for padding taps, pixels past the
// end and channels past Cout / N). Each wave owns 64 x 64 of the tile and reads, per 16-pixel k-step, its K-contiguous 32x32x16
// fragments with ds_read_b64_tr_b16. Every lane takes part in every read (the tile is padded, not masked).
//   fp16: a row is 256 bytes = 16 chunks of 16 bytes; four fragments for four MFMAs per k-step.
//   x3:   a row is 512 bytes: 128 real channels = 8 records = 32 chunks; a "virtual" channel index counts halves, hi and lo alike
//         (2·Cout, 2·N of them); the hi and the lo fragments of each 32-channel block, eight fragments for twelve MFMAs.
// Split-K: fixed slices of the pixel range chosen from the geometry alone; slice partials are added in slice order by the second
// pass. The epilogue unscales by inv_scale (x3: inv_scale / x_scale), checks finiteness and writes only the real channels.
//
// Conflict-free LDS images. A row chunk write covers 16 consecutive chunks per 16 lanes, which any XOR permutes among themselves;
// the swizzle is chosen for the transposed reads.
//   fp16: a transposed read of a 32-lane half touches four rows and, of each, the chunks of 32 consecutive channels; the swizzle
//         XORs the chunk index with ((row & 3) << 2) | ((row >> 2) & 3), which keeps both the row-chunk writes and the 32x32x16
//         transposed reads free of bank conflicts.
//   x3:   a transposed read of a 32-lane half touches rows k0 … k0 + 3 and, of each row, the four chunks {b, b + 1, b + 4, b + 5}
//         (two 16-channel hi — or lo — runs, 32 halves apart because each record carries its lo half behind its hi half; b % 8 == 0
//         for hi, 2 for lo). Bits 0 and 2 of the chunk index vary inside a read, so the swizzle puts the row into bits 1 and 3: the
//         16 accesses land in 16 different 16-byte bank groups.
constexpr int WG_BM = 128, WG_BN = 128, WG_BK = 32;

template <bool X3> struct WgImage {
  static constexpr int HALVES = X3 ? 2 : 1;                 // halves per real channel
  static constexpr int ROW_BYTES = 256 * HALVES;            // 128 real channels
  static constexpr int CHUNKS = ROW_BYTES / 16;             // 16-byte chunks of a row: one thread stages one chunk of ...
  static constexpr int ROW_STEP = 256 / CHUNKS;             // ... every ROW_STEP-th row,
  static constexpr int ROWS = WG_BK / ROW_STEP;             // ROWS rows in all
  static constexpr int TILE_BYTES = WG_BK * ROW_BYTES;      // one operand, one stage
  static constexpr int LDS = 4 * TILE_BYTES;                // two operands, two stages: 32 KB / 64 KB
  // byte offset of 16-byte chunk ch of row `row`
  static __device__ __forceinline__ int off(int row, int ch) {
    if constexpr (X3) return ROW_BYTES * row + 16 * (ch ^ (((row & 1) << 1) | ((row & 2) << 2)));
    else return ROW_BYTES * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  }
  // 8 K-consecutive halves (rows k0 + 8h .. k0 + 8h + 7) of 32 channels of an image: two transposed reads. col = the column (in
  // halves) of the first one; lanes 0-15 / 32-47 take the 16 channels there, lanes 16-31 / 48-63 the next 16 (x3: the next record's,
  // 32 halves on).
  static __device__ __forceinline__ h8 frag(const char* img, int k0, int col, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3, h = g >> 1;
    const int ch = ((col + 16 * HALVES * (g & 1)) >> 3) + (p >> 1);
    typedef __attribute__((address_space(3))) s4 lds_s4;
    const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(img + off(k0 + 8 * h + q, ch) + 8 * (p & 1)));
    const s4 hi2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(img + off(k0 + 8 * h + 4 + q, ch) + 8 * (p & 1)));
    return __builtin_bit_cast(h8, __builtin_shufflevector(lo, hi2, 0, 1, 2, 3, 4, 5, 6, 7));
  }
};

struct WgradParams {
  const _Float16* x;    // (B,H,W,Cin_pad) fp16, or split16 (B,H,W,2·Cin)
  const _Float16* dz;   // (B,Ho,Wo,Cout) fp16, or split16 (B,Ho,Wo,2·Cout)
  float* dw;            // natural (Cout,Cin,k,k) or tap-major (Cout,k*k,Cin)
  float* partial;       // [S][Cout][N] when S > 1
  unsigned* state;
  int Cin, Cin_pad, H, W, Cout, k, stride, pad, Ho, Wo, layout, N;   // x3: Cin_pad = Cin
  long npix;
  int ksteps, S, steps_per_split, tiles_n;
  unsigned x_bytes, dz_bytes;
  float unscale;        // 1 / (scale of x); fp16: 1, and not applied
};

template <bool X3> __device__ __forceinline__ void wgrad_store(const WgradParams& p, int co, int n, float v) {
  const int cp = X3 ? p.Cin : p.Cin_pad;      // (equal for x3: one field read, not two)
  const int tap = n / cp, ci = n - tap * cp;
  if constexpr (X3) {
    v *= p.unscale * __uint_as_float(p.state[1]);
  } else {
    if (ci >= p.Cin) return;
    v *= __uint_as_float(p.state[1]);
  }
  if (!__builtin_isfinite(v)) p.state[2] = 1u;
  const int khw = p.k * p.k;
  const long o = p.layout ? ((long)co * khw + tap) * p.Cin + ci : ((long)co * p.Cin + ci) * khw + tap;
  p.dw[o] = v;
}

template <bool X3> __global__ __launch_bounds__(256) void wgrad_half_kernel(WgradParams p) {
  typedef WgImage<X3> Img;
  constexpr int HV = Img::HALVES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x - tm * p.tiles_n;
  const int m0 = tm * WG_BM, n0 = tn * WG_BN;
  const int split = blockIdx.y;
  const int s_begin = split * p.steps_per_split, s_end = min(p.ksteps, s_begin + p.steps_per_split);
  const int ch = tid & (Img::CHUNKS - 1), r0 = tid / Img::CHUNKS;   // this thread stages chunk ch of rows r0, r0 + ROW_STEP, …
  // dz chunk: (virtual) channels HV·m0 + 8ch .. +7
  const int mv = HV * m0 + 8 * ch;
  const bool a_ok = mv < HV * p.Cout;
  // x chunk: (virtual) GEMM columns HV·n0 + 8ch .. +7 = one octet of one tap
  const int nv = HV * n0 + 8 * ch;
  const bool b_ok = nv < HV * p.N;
  const int cp = X3 ? p.Cin : p.Cin_pad;      // (equal for x3: one field read, not two)
  const int tap = b_ok ? nv / (HV * cp) : 0, cv0 = b_ok ? nv - tap * HV * cp : 0;
  const int ky = tap / p.k, kx = tap - (tap / p.k) * p.k;
  const __amdgpu_buffer_rsrc_t rs_dz = __builtin_amdgcn_make_buffer_rsrc((void*)p.dz, 0, (int)p.dz_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const long hwo = (long)p.Ho * p.Wo;
  i32x4 areg[Img::ROWS], breg[Img::ROWS];
  auto load = [&](int s) {
#pragma unroll
    for (int e = 0; e < Img::ROWS; ++e) {
      const long px = (long)s * WG_BK + r0 + Img::ROW_STEP * e;
      unsigned oa = 0x80000000u, ob = 0x80000000u;      // out of range: the buffer load returns zeros
      if (px < p.npix) {
        // (one number; each mode keeps the order of the sum it was built with, which the compiler's address code follows)
        if constexpr (X3) { if (a_ok) oa = (unsigned)((px * (2 * p.Cout) + mv) * 2); }
        else { if (a_ok) oa = (unsigned)((px * p.Cout + m0 + 8 * ch) * 2); }
        const long n = px / hwo, rr = px - n * hwo;
        const int oy = (int)(rr / p.Wo), ox = (int)(rr - (long)oy * p.Wo);
        const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
        if (b_ok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
          ob = (unsigned)((((n * p.H + iy) * p.W + ix) * (HV * cp) + cv0) * 2);
      }
      areg[e] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_dz, (int)oa, 0, 0));
      breg[e] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)ob, 0, 0));
    }
  };
  auto stage = [&](int buf) {
    char* A = smem + buf * 2 * Img::TILE_BYTES;
    char* Bm = A + Img::TILE_BYTES;
#pragma unroll
    for (int e = 0; e < Img::ROWS; ++e) {
      *reinterpret_cast<i32x4*>(A + Img::off(r0 + Img::ROW_STEP * e, ch)) = areg[e];
      *reinterpret_cast<i32x4*>(Bm + Img::off(r0 + Img::ROW_STEP * e, ch)) = breg[e];
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
      const char* A = smem + buf * 2 * Img::TILE_BYTES;
      const char* Bm = A + Img::TILE_BYTES;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        h8 af[2][HV], bf[2][HV];       // [block][0] the fp16 (x3: hi) fragment, [block][1] x3's lo fragment
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          af[i][0] = Img::frag(A, 16 * kk, HV * (wm + 32 * i), lane);
          if constexpr (X3) af[i][1] = Img::frag(A, 16 * kk, HV * (wm + 32 * i) + 16, lane);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          bf[j][0] = Img::frag(Bm, 16 * kk, HV * (wn + 32 * j), lane);
          if constexpr (X3) bf[j][1] = Img::frag(Bm, 16 * kk, HV * (wn + 32 * j) + 16, lane);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][0], bf[j][0], acc[i][j], 0, 0, 0);
            if constexpr (X3) {        // hh, hl, lh in this order: each accumulator is one dependent chain
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][0], bf[j][1], acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i][1], bf[j][0], acc[i][j], 0, 0, 0);
            }
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
        else wgrad_store<X3>(p, co, n, acc[i][j][r]);
      }
    }
}

template <bool X3> __global__ __launch_bounds__(256) void wgrad_reduce_kernel(WgradParams p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)p.Cout * p.N;
  if (i >= total) return;
  float s = 0.f;
  for (int sl = 0; sl < p.S; ++sl) s += p.partial[(long)sl * total + i];
  wgrad_store<X3>(p, (int)(i / p.N), (int)(i % p.N), s);
}

// The launch plan of a weight gradient, from the geometry alone (the same in both modes: N counts real channels, x3's Cin_pad = Cin).
// launch_wgrad and deepim_conv_wgrad_half_plan read it here.
struct WgPlan { int Ho, Wo, N, tiles_m, tiles_n, ksteps, S, steps_per_split; long npix; };
WgPlan wgrad_plan(int B, int Cin_pad, int H, int W, int Cout, int k, int stride, int pad) {
  WgPlan q;
  q.Ho = (H + 2 * pad - k) / stride + 1; q.Wo = (W + 2 * pad - k) / stride + 1;
  q.N = k * k * Cin_pad;
  q.npix = (long)B * q.Ho * q.Wo;
  q.ksteps = (int)di_div_up(q.npix, (long)WG_BK);
  q.tiles_m = di_div_up(Cout, WG_BM);
  q.tiles_n = di_div_up(q.N, WG_BN);
  // fixed slices from the geometry alone: about 512 blocks, never an empty slice
  const int S = std::max(1, std::min(q.ksteps, di_div_up(512, q.tiles_m * q.tiles_n)));
  q.steps_per_split = di_div_up(std::max(q.ksteps, 1), S);
  q.S = di_div_up(std::max(q.ksteps, 1), q.steps_per_split);
  return q;
}

// what both modes ask of a weight gradient's geometry beyond their channel rules: WG_OK, or the reason it is refused
enum { WG_OK = 0, WG_EMPTY, WG_TOO_LARGE };
int wgrad_refusal(bool x3, int B, int Cin_pad, int H, int W, int Cout, int k, int stride, int pad) {
  if (!(B >= 0 && H >= 1 && W >= 1 && stride >= 1 && pad >= 0 && H + 2 * pad >= k && W + 2 * pad >= k)) return WG_EMPTY;
  const size_t ebytes = x3 ? 4 : 2;
  const size_t Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const size_t xb = (size_t)B * H * W * Cin_pad * ebytes, zb = (size_t)B * Ho * Wo * Cout * ebytes;
  return xb < 0x7fffffffUL && zb < 0x7fffffffUL ? WG_OK : WG_TOO_LARGE;
}

// the caller has checked the channel counts of its mode; x_scale: the scale x was stored at (fp16: 1)
template <bool X3>
int launch_wgrad(deepim_ctx* ctx, float* dw, const void* x, const void* dz, unsigned* state, int B, int Cin, int Cin_pad, int H, int W,
                 int Cout, int k, int stride, int pad, int layout, float x_scale) {
  const int why = wgrad_refusal(X3, B, Cin_pad, H, W, Cout, k, stride, pad);
  DI_REQUIRE(why != WG_EMPTY, HALF_MSG("conv2d_wgrad", "no output pixel: H + 2 pad < k, or stride < 1"));
  DI_REQUIRE(why != WG_TOO_LARGE, HALF_MSG("conv2d_wgrad", "operands must be < 2 GiB"));
  const WgPlan q = wgrad_plan(B, Cin_pad, H, W, Cout, k, stride, pad);
  WgradParams p;
  p.x = (const _Float16*)x; p.dz = (const _Float16*)dz; p.dw = dw; p.state = state;
  p.Cin = Cin; p.Cin_pad = Cin_pad; p.H = H; p.W = W; p.Cout = Cout; p.k = k; p.stride = stride; p.pad = pad;
  p.Ho = q.Ho; p.Wo = q.Wo;
  p.layout = layout ? 1 : 0;
  p.N = q.N;
  p.npix = q.npix;
  p.unscale = 1.f / x_scale;
  constexpr size_t ebytes = 2 * WgImage<X3>::HALVES;
  p.x_bytes = (unsigned)((size_t)B * H * W * Cin_pad * ebytes); p.dz_bytes = (unsigned)((size_t)p.npix * Cout * ebytes);
  p.ksteps = q.ksteps;
  p.tiles_n = q.tiles_n;
  const int tiles = q.tiles_m * q.tiles_n;
  p.steps_per_split = q.steps_per_split;
  p.S = q.S;
  p.partial = nullptr;
  if (p.S > 1) {
    void* scratch;
    int rc = deepim_scratch(ctx, (size_t)p.S * Cout * p.N * sizeof(float), &scratch);
    if (rc) return rc;
    p.partial = (float*)scratch;
  }
  constexpr int lds = WgImage<X3>::LDS;
  if constexpr (lds > 48 * 1024) {    // x3's 64 KB of dynamic LDS has to be asked for; fp16's 32 KB does not
    static const char attr_tag = 0;   // function attributes are per DEVICE: remember them per context
    if (di_attr_needed(ctx, &attr_tag))
      DI_CHECK(hipFuncSetAttribute((const void*)wgrad_half_kernel<X3>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL(wgrad_half_kernel<X3>, dim3(tiles, p.S), dim3(256), lds, ctx->stream, p);
  if (p.S > 1)
    hipLaunchKernelGGL(wgrad_reduce_kernel<X3>, dim3(di_div_up((long)Cout * p.N, 256L)), dim3(256), 0, ctx->stream, p);
  DI_LAUNCH_CHECK();
  return 0;
}

// ---- data gradient ----------------------------------------------------------------------------------------------------------
// The data gradient is the mode's own forward convolution over re-packed weights. Stride 1: pack (transposed, flipped) plus one
// forward. Stride 2: four stride-1 convolutions, one per output parity class of the un-dilated dz, each into a class buffer whose
// result window is stitched onto its positions of dx. A split16 tensor of C channels is stitched as an fp16 tensor of 2C.

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
  const h8 v = *reinterpret_cast<const h8*>(cls + (((n * Hs + t + cy) * Ws + u + cx) * C + o * 8));
  *reinterpret_cast<h8*>(dx + (((n * Hd + 2 * t + py) * Wd + 2 * u + px) * C + o * 8)) = v;
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

// the pack / forward pair of a mode; state and w_scale are x3's (dz carries scale 1 in units of S, and so does dx)
template <bool X3> size_t dgrad_packed_size(int Ci_l, int Co_l, int nky, int nkx) {
  return X3 ? deepim_conv_x3_packed_size(Ci_l, Co_l, nky, nkx) : deepim_conv_f16_packed_size(Ci_l, Co_l, nky, nkx);
}
template <bool X3>
int dgrad_class_conv(deepim_ctx* ctx, void* out, const void* dz, const float* w_layer, void* ws, unsigned* state, int B, int Ci_l,
                     int Ho, int Wo, int Co_l, int k, int ky0, int kx0, int st, int nky, int nkx, int P, float w_scale) {
  if constexpr (X3) {
    int rc = deepim_conv_x3_pack_dgrad(ctx, ws, w_layer, state, Co_l, Ci_l, k, ky0, kx0, st, nky, nkx, w_scale);
    if (rc) return rc;
    return deepim_conv2d_x3_forward(ctx, out, dz, ws, nullptr, B, Co_l, Ho, Wo, Ci_l, nky, nkx, 1, P, 1.f, 1.f / w_scale, 1.f);
  } else {
    int rc = deepim_conv_f16_pack_dgrad(ctx, ws, w_layer, Co_l, Ci_l, k, ky0, kx0, st, nky, nkx);
    if (rc) return rc;
    return deepim_conv2d_f16_forward(ctx, out, dz, ws, nullptr, B, Co_l, Ho, Wo, Ci_l, nky, nkx, 1, P, 1.f);
  }
}

// bytes of the largest of the four parity-class weight packs of a stride-2 layer (the class buffer follows it in the workspace)
template <bool X3> size_t class_pack_bytes(int Ci_l, int Co_l, int k, int pad) {
  size_t pk = 0;
  for (int z = 0; z < 4; ++z) {
    const S2ClassF16 c = s2_class_f16(z, k, pad);
    pk = std::max(pk, dgrad_packed_size<X3>(Ci_l, Co_l, c.nky, c.nkx));
  }
  return (pk + 255) / 256 * 256;
}

template <bool X3> size_t dgrad_workspace_size(int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad) {
  if (stride == 1) return dgrad_packed_size<X3>(Ci_l, Co_l, k, k);
  const int Ho = (Hd + 2 * pad - k) / 2 + 1, Wo = (Wd + 2 * pad - k) / 2 + 1;
  size_t cls = 0;
  for (int z = 0; z < 4; ++z) {
    const S2ClassF16 c = s2_class_f16(z, k, pad);
    cls = std::max(cls, (size_t)B * (Ho + 2 * c.P - c.nky + 1) * (Wo + 2 * c.P - c.nkx + 1) * Ci_l * (X3 ? 4 : 2));
  }
  return class_pack_bytes<X3>(Ci_l, Co_l, k, pad) + cls;
}

// the caller has checked the channel counts (and w_scale) of its mode
template <bool X3>
int dgrad_half(deepim_ctx* ctx, void* dx, const void* dz, const float* w_layer, void* ws, unsigned* state, int B, int Ci_l, int Hd, int Wd,
               int Co_l, int k, int stride, int pad, float w_scale) {
  if (B == 0) return 0;
  int rc;
  if (stride == 1) {
    const int P = k - 1 - pad;
    DI_REQUIRE(P >= 0 && Hd + 2 * pad - k + 1 > 0, HALF_MSG("conv2d_dgrad", "pad > k - 1"));
    const int Ho = Hd + 2 * pad - k + 1, Wo = Wd + 2 * pad - k + 1;
    rc = dgrad_class_conv<X3>(ctx, dx, dz, w_layer, ws, state, B, Ci_l, Ho, Wo, Co_l, k, 0, 0, 1, k, k, P, w_scale);
    if (rc) return rc;
  } else {
    const int Ho = (Hd + 2 * pad - k) / 2 + 1, Wo = (Wd + 2 * pad - k) / 2 + 1;
    const int Cs = X3 ? 2 * Ci_l : Ci_l;      // halves per pixel of dx
    _Float16* cls = (_Float16*)((char*)ws + class_pack_bytes<X3>(Ci_l, Co_l, k, pad));
    for (int z = 0; z < 4; ++z) {
      const S2ClassF16 c = s2_class_f16(z, k, pad);
      const int hq = (Hd - c.py + 1) / 2, wq = (Wd - c.px + 1) / 2;
      if (hq <= 0 || wq <= 0) continue;
      const int Hs = Ho + 2 * c.P - c.nky + 1, Ws = Wo + 2 * c.P - c.nkx + 1;
      DI_REQUIRE(c.cy + hq <= Hs && c.cx + wq <= Ws, HALF_MSG("conv2d_dgrad", "class window outside the convolution result"));
      rc = dgrad_class_conv<X3>(ctx, cls, dz, w_layer, ws, state, B, Ci_l, Ho, Wo, Co_l, k, c.ky0, c.kx0, 2, c.nky, c.nkx, c.P, w_scale);
      if (rc) return rc;
      const long total = (long)B * hq * wq * (Cs / 8);
      hipLaunchKernelGGL(stitch_f16_kernel, dim3(di_div_up(total, 256L)), dim3(256), 0, ctx->stream, (_Float16*)dx, cls, Cs, Hd, Wd, Hs,
                         Ws, hq, wq, c.cy, c.cx, c.py, c.px, total);
      DI_LAUNCH_CHECK();
    }
  }
  if constexpr (X3) return deepim_x3_status_to_state(ctx, state);      // a clamp of dx, reported by the forward kernel
  return 0;
}

// ---- scale state plumbing ---------------------------------------------------------------------------------------------------
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

}  // namespace

// ---- C ABI: thin wrappers, each with the argument checks of its own mode ------------------------------------------------------
extern "C" int deepim_lrelu_bias_backward_f16(deepim_ctx* ctx, void* dz_nhwc_f16, float* db, const void* d_nhwc_f16, const float* add_nchw,
                                              const void* y_nhwc_f16, unsigned* state, float slope, int B, int C, int H, int W) {
  return launch_lrelu_bias_backward<false>(ctx, dz_nhwc_f16, db, d_nhwc_f16, add_nchw, y_nhwc_f16, state, slope, B, C, H, W);
}

extern "C" int deepim_lrelu_bias_backward_x3(deepim_ctx* ctx, void* dz_split16, float* db, const void* d_split16, const float* add_nchw,
                                             const void* y_split16, unsigned* state, float slope, int B, int C, int H, int W) {
  return launch_lrelu_bias_backward<true>(ctx, dz_split16, db, d_split16, add_nchw, y_split16, state, slope, B, C, H, W);
}

extern "C" int deepim_conv2d_wgrad_f16(deepim_ctx* ctx, float* dw, const void* x_nhwc_f16, const void* dz_nhwc_f16, unsigned* state,
                                       int B, int Cin, int Cin_pad, int H, int W, int Cout, int k, int stride, int pad, int layout) {
  DI_DEVICE(ctx);
  DI_REQUIRE(Cin_pad % 8 == 0 && Cin <= Cin_pad && Cin > 0 && Cout % 8 == 0 && Cout > 0 && k >= 1 && k <= 7,
             "conv2d_wgrad_f16: Cin_pad % 8, Cout % 8 must be 0, Cin <= Cin_pad, k <= 7");
  return launch_wgrad<false>(ctx, dw, x_nhwc_f16, dz_nhwc_f16, state, B, Cin, Cin_pad, H, W, Cout, k, stride, pad, layout, 1.f);
}

extern "C" int deepim_conv2d_wgrad_x3(deepim_ctx* ctx, float* dw, const void* x_split16, const void* dz_split16, unsigned* state, int B,
                                      int Cin, int H, int W, int Cout, int k, int stride, int pad, int layout, float x_scale) {
  DI_DEVICE(ctx);
  DI_REQUIRE(Cin > 0 && Cin % 16 == 0 && Cout > 0 && Cout % 16 == 0 && k >= 1 && k <= 7,
             "conv2d_wgrad_x3: Cin % 16 and Cout % 16 must be 0 (whole split16 records), k <= 7");
  DI_REQUIRE(x_scale > 0.f, "conv2d_wgrad_x3: x_scale must be positive");
  return launch_wgrad<true>(ctx, dw, x_split16, dz_split16, state, B, Cin, Cin, H, W, Cout, k, stride, pad, layout, x_scale);
}

extern "C" int deepim_conv_wgrad_half_plan(int x3, int B, int Cin_pad, int H, int W, int Cout, int k, int stride, int pad, int* plan) {
  DI_REQUIRE(plan != nullptr, "conv_wgrad_half_plan: null plan");
  for (int i = 0; i < 6; ++i) plan[i] = -1;
  if (x3)
    DI_REQUIRE(Cin_pad > 0 && Cin_pad % 16 == 0 && Cout > 0 && Cout % 16 == 0 && k >= 1 && k <= 7,
               "conv_wgrad_half_plan: x3 needs Cin % 16 and Cout % 16 == 0 (whole split16 records), k <= 7");
  else
    DI_REQUIRE(Cin_pad > 0 && Cin_pad % 8 == 0 && Cout > 0 && Cout % 8 == 0 && k >= 1 && k <= 7,
               "conv_wgrad_half_plan: Cin_pad % 8, Cout % 8 must be 0, k <= 7");
  const int why = wgrad_refusal(x3 != 0, B, Cin_pad, H, W, Cout, k, stride, pad);
  DI_REQUIRE(why != WG_EMPTY, "conv_wgrad_half_plan: no output pixel: H + 2 pad < k, or stride < 1");
  DI_REQUIRE(why != WG_TOO_LARGE, "conv_wgrad_half_plan: operands must be < 2 GiB");
  const WgPlan q = wgrad_plan(B, Cin_pad, H, W, Cout, k, stride, pad);
  const int out[6] = {q.tiles_m, q.tiles_n, q.ksteps, q.S, q.steps_per_split, q.npix % WG_BK != 0 ? 1 : 0};
  for (int i = 0; i < 6; ++i) plan[i] = out[i];
  return 0;
}

extern "C" size_t deepim_conv_dgrad_f16_workspace_size(int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad) {
  return dgrad_workspace_size<false>(B, Ci_l, Hd, Wd, Co_l, k, stride, pad);
}

extern "C" size_t deepim_conv_dgrad_x3_workspace_size(int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad) {
  return dgrad_workspace_size<true>(B, Ci_l, Hd, Wd, Co_l, k, stride, pad);
}

extern "C" int deepim_conv2d_dgrad_f16(deepim_ctx* ctx, void* dx_nhwc_f16, const void* dz_nhwc_f16, const float* w_layer, void* ws,
                                       int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad) {
  DI_DEVICE(ctx);
  DI_REQUIRE(stride == 1 || stride == 2, "conv2d_dgrad_f16: stride 1 or 2");
  DI_REQUIRE(Co_l % 8 == 0 && Ci_l % 8 == 0, "conv2d_dgrad_f16: channel counts must be multiples of 8");
  return dgrad_half<false>(ctx, dx_nhwc_f16, dz_nhwc_f16, w_layer, ws, nullptr, B, Ci_l, Hd, Wd, Co_l, k, stride, pad, 1.f);
}

extern "C" int deepim_conv2d_dgrad_x3(deepim_ctx* ctx, void* dx_split16, const void* dz_split16, const float* w_layer, void* ws,
                                      unsigned* state, int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad,
                                      float w_scale) {
  DI_DEVICE(ctx);
  DI_REQUIRE(stride == 1 || stride == 2, "conv2d_dgrad_x3: stride 1 or 2");
  DI_REQUIRE(Co_l % 32 == 0 && Ci_l % 128 == 0, "conv2d_dgrad_x3: needs Co_l % 32 == 0 and Ci_l % 128 == 0");
  DI_REQUIRE(w_scale > 0.f, "conv2d_dgrad_x3: w_scale must be positive");
  return dgrad_half<true>(ctx, dx_split16, dz_split16, w_layer, ws, state, B, Ci_l, Hd, Wd, Co_l, k, stride, pad, w_scale);
}

extern "C" int deepim_amp_scale_update(deepim_ctx* ctx, unsigned* state, int window) {
  DI_DEVICE(ctx);
  DI_REQUIRE(window >= 1, "amp_scale_update: window must be >= 1");
  hipLaunchKernelGGL(amp_scale_update_kernel, dim3(1), dim3(1), 0, ctx->stream, state, window);
  DI_LAUNCH_CHECK();
  return 0;
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
