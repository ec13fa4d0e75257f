// fp16 FlowNetS decoder and flow / mask heads (deepIM_flownet.py:120-167, :627-713) for the fp16 conv path (BASELINE config 5
// arithmetic with the test graph of config 4). Activations stay NHWC fp16 from the encoder through Concat2 / Concat3; the three
// few-filter predictors write fp32 NCHW low-resolution maps that the fp32 upsampling / inverse-zoom kernels of the heads read.
//
//   deconv5 / deconv4   MXNet Deconvolution k4 s2 p0 + Crop(1,1) + LeakyReLU as four parity-class GEMMs in ONE launch on
//                       v_mfma_f32_32x32x16_f16: output (2r+py, 2c+px) sees kernel rows ky in {1,3} (py = 0, input rows r, r-1)
//                       or {0,2} (py = 1, rows r+1, r), columns alike. Per class M = Cout, N = B·(pixels of the class), K = 4·Cin_pad
//                       running (tap, ci) with ci fastest, so a lane's 8 k-values are 8 channels of one tap = one 16-byte NHWC load.
//                       Fragments come straight from global memory (weights pre-packed in fragment order: 1 KB contiguous per
//                       wave and k-step); a 128x128 block tile of four 64x64 wave tiles; a split-K plan (fixed by geometry) fills
//                       the chip where the tiles alone do not, its fp32 slices reduced in order by a second pass.
//   few-filter 3x3      Convolution1 / Convolution2 / Convolution3 + mask_conv3: one lane per 8-channel octet holds its weights of
//                       all 9 taps and up to 3 filters in registers; a block sweeps a row segment with a 3x3 window of 16-byte loads,
//                       v_dot2_f32_f16 (exact products, fp32 sums), a fixed-order wave + block reduction. Concat3 feeds mask_conv3
//                       and Convolution3 in the same pass (read once).
//   upsample_flow       2→2 deconvolution of the fp32 flow into fp16 concat channels (VALU, fp32 throughout, one rounding).
//   slice copy          encoder activation → concat channels [0, C), 16 bytes per thread.
#include "common.h"

namespace {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// parity class tap a (0, 1) of output parity p: kernel index and input offset (input index = r + offset)
__host__ __device__ inline int dc_k(int p, int a) { return p == 0 ? (a == 0 ? 1 : 3) : (a == 0 ? 0 : 2); }
__host__ __device__ inline int dc_d(int p, int a) { return p == 0 ? (a == 0 ? 0 : -1) : (a == 0 ? 1 : 0); }

constexpr int DC_BM = 128, DC_BN = 128;

struct DeconvF16Params {
  const _Float16* in;
  const h8* wp;
  const float* bias;
  _Float16* out;
  float* partial;          // split-K slices [split][Ho·Wo·B][Cout] (ksplit > 1)
  int B, H, W, Cin_pad, in_ctotal, Cout, Ho, Wo, out_ctotal, out_coff;
  float slope;
  int nsteps, ksplit, steps_per_split;
  int rows[2], cols[2];    // rows of parity py, columns of parity px
  int npix[4];             // pixels of class c = 2·py + px (all images)
  int tile_base[5];        // prefix of (Cout/128 rounded up) x (pixel tiles) over the classes
};

// packed[((cls·Cout/32 + mt)·nsteps + s)·64 + lane][j] = f16(w[ci][co][ky][kx]), co = 32·mt + (lane & 31),
// k = 8·(2s + (lane >> 5)) + j = tap·Cin_pad + ci, tap = 2a + b → (ky, kx) of the class; zero for ci >= Cin
__global__ void pack_deconv_f16_kernel(h8* __restrict__ packed, const float* __restrict__ w, int Cin, int Cin_pad, int Cout,
                                       int nsteps, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63);
  long r = i >> 6;
  const int s = (int)(r % nsteps); r /= nsteps;
  const int mt = (int)(r % (Cout / 32));
  const int cls = (int)(r / (Cout / 32));
  const int co = mt * 32 + (lane & 31);
  const int k0 = 8 * (2 * s + (lane >> 5));
  const int tap = k0 / Cin_pad, ci0 = k0 - tap * Cin_pad;
  const int ky = dc_k(cls >> 1, tap >> 1), kx = dc_k(cls & 1, tap & 1);
  h8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = ci0 + j;
    v[j] = ci < Cin ? (_Float16)w[(((long)ci * Cout + co) * 4 + ky) * 4 + kx] : (_Float16)0.f;
  }
  packed[i] = v;
}

// 256 threads = 2 x 2 waves, each a 64 x 64 tile (2 x 2 MFMA tiles of 32 x 32) of a 128 (channels) x 128 (pixels) block tile
__global__ __launch_bounds__(256) void deconv_f16_kernel(DeconvF16Params p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int ntile_all = p.tile_base[4];
  const int split = blockIdx.x / ntile_all;
  int t = blockIdx.x - split * ntile_all;
  int cls = 0;
  while (cls < 3 && t >= p.tile_base[cls + 1]) ++cls;
  t -= p.tile_base[cls];
  const int MT = (p.Cout + DC_BM - 1) / DC_BM;
  const int mblk = t % MT, nblk = t / MT;
  const int co_w = mblk * DC_BM + wm * 64;
  if (co_w >= p.Cout) return;    // Cout % 64 == 0: a wave's 64 channels are all inside or all outside
  const int py = cls >> 1, px = cls & 1;
  const int R = p.rows[py], C = p.cols[px], npix = p.npix[cls];
  const int h = lane >> 5, col = lane & 31;

  // this lane's two pixels (one per N sub-tile) and the input offsets of their four taps (-1: outside the frame)
  int off[2][4], pimg[2], poy[2], pox[2];
  bool pvalid[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = nblk * DC_BN + wn * 64 + j * 32 + col;
    pvalid[j] = n < npix;
    const int nn = pvalid[j] ? n : 0;
    const int b = nn / (R * C), rem = nn - b * (R * C);
    const int r = rem / C, c = rem - r * C;
    pimg[j] = b; poy[j] = 2 * r + py; pox[j] = 2 * c + px;
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
      const int iy = r + dc_d(py, tap >> 1), ix = c + dc_d(px, tap & 1);
      const bool v = pvalid[j] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      off[j][tap] = v ? ((b * p.H + iy) * p.W + ix) * p.in_ctotal : -1;
    }
  }

  const int s0 = split * p.steps_per_split;
  const int s1 = min(p.nsteps, s0 + p.steps_per_split);
  const int noct = p.Cin_pad >> 3;
  int q = 2 * s0 + h;                    // this lane's k-octet: tap = q / noct, channels 8·(q % noct) …
  int tap = q / noct, oc = q - tap * noct;
  const h8* wp0 = p.wp + ((long)(cls * (p.Cout / 32) + co_w / 32) * p.nsteps) * 64 + lane;
  const long wstride_m = (long)p.nsteps * 64;   // next 32-channel M tile

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // register selects, not runtime-indexed private arrays (those would live in scratch)
#define DC_LOAD(S, TP, O, A, BF)                                                                                        \
  {                                                                                                                     \
    A[0] = wp0[(long)(S) * 64];                                                                                         \
    A[1] = wp0[wstride_m + (long)(S) * 64];                                                                             \
    const int b0 = (TP) == 0 ? off00 : (TP) == 1 ? off01 : (TP) == 2 ? off02 : off03;                                 \
    const int b1 = (TP) == 0 ? off10 : (TP) == 1 ? off11 : (TP) == 2 ? off12 : off13;                                 \
    BF[0] = b0 >= 0 ? *reinterpret_cast<const h8*>(p.in + b0 + 8 * (O)) : zero8;                                        \
    BF[1] = b1 >= 0 ? *reinterpret_cast<const h8*>(p.in + b1 + 8 * (O)) : zero8;                                        \
  }
  const int off00 = off[0][0], off01 = off[0][1], off02 = off[0][2], off03 = off[0][3];
  const int off10 = off[1][0], off11 = off[1][1], off12 = off[1][2], off13 = off[1][3];
  if (s0 < s1) {
    h8 a_cur[2], b_cur[2], a_nxt[2] = {zero8, zero8}, b_nxt[2] = {zero8, zero8};
    DC_LOAD(s0, tap, oc, a_cur, b_cur);
    for (int s = s0; s < s1; ++s) {
      oc += 2;
      while (oc >= noct) { oc -= noct; ++tap; }
      if (s + 1 < s1) DC_LOAD(s + 1, tap, oc, a_nxt, b_nxt);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_cur[i], b_cur[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i) { a_cur[i] = a_nxt[i]; b_cur[i] = b_nxt[i]; }
    }
  }
#undef DC_LOAD

  // epilogue: lane = one pixel, registers 4g … 4g+3 = channels 8g + 4h … +3 of the 32-channel sub-tile
  const long npix_out = (long)p.B * p.Ho * p.Wo;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!pvalid[j]) continue;
    const long opix = ((long)pimg[j] * p.Ho + poy[j]) * p.Wo + pox[j];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int co = co_w + 32 * i + 8 * g + 4 * h;
        if (p.ksplit == 1) {
          h4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float x = acc[i][j][4 * g + e] + p.bias[co + e];
            x = x > 0.f ? x : x * p.slope;
            o[e] = (_Float16)x;
          }
          *reinterpret_cast<h4*>(p.out + opix * p.out_ctotal + p.out_coff + co) = o;
        } else {
          float4 v = make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
          *reinterpret_cast<float4*>(p.partial + ((long)split * npix_out + opix) * p.Cout + co) = v;
        }
      }
    }
  }
}

// split-K second pass: out[pix][coff + c] = f16(lrelu(Σ_s partial[s][pix][c] + bias[c])), slices in order, 4 channels per thread
__global__ __launch_bounds__(256) void deconv_f16_reduce_kernel(_Float16* __restrict__ out, const float* __restrict__ partial,
                                                                const float* __restrict__ bias, long total4, int S, int Cout,
                                                                int out_ctotal, int out_coff, float slope) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const float4* p4 = reinterpret_cast<const float4*>(partial);
  float4 v = p4[i];
  for (int s = 1; s < S; ++s) {
    const float4 u = p4[(long)s * total4 + i];
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  const long pix = (i * 4) / Cout;
  const int c0 = (int)(i * 4 - pix * Cout);
  const float r[4] = {v.x, v.y, v.z, v.w};
  h4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float x = r[k] + bias[c0 + k];
    x = x > 0.f ? x : x * slope;
    o[k] = (_Float16)x;
  }
  *reinterpret_cast<h4*>(out + pix * out_ctotal + out_coff + c0) = o;
}

// ----------------------------------------------------------------------------------------------------------------------
// few-filter 3x3 stride-1 pad-1 convolution, NHWC fp16 in → up to 3 fp32 NCHW output channels (two tensors)
constexpr int FO_MAXOUT = 3;
constexpr int FO_MAXSEG = 64;   // output columns per block
constexpr int FO_MAXWAVES = 4;  // 4 x 64 octets = 2048 input channels

struct FewoutParams {
  const _Float16* in;
  const h8* wp;            // [octet][tap 9][filter 3] x 8 halves
  const float* bias0;
  const float* bias1;
  float* out0;
  float* out1;
  int n0, n1;              // filters of out0 / out1 (n0 + n1 = NOUT)
  int B, H, W, in_ctotal, noct, seg, nseg;
};

// packed[(o·9 + tap)·3 + f][j] = f16(w_f[o·8 + j][ky][kx]) with w_f = filter f of (w0 | w1); zero beyond Cin and beyond n0 + n1
__global__ void pack_fewout_f16_kernel(h8* __restrict__ packed, const float* __restrict__ w0, int n0, const float* __restrict__ w1,
                                       int n1, int Cin, int noct) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= noct * 9 * FO_MAXOUT) return;
  const int f = i % FO_MAXOUT, tap = (i / FO_MAXOUT) % 9, o = i / (9 * FO_MAXOUT);
  const float* w = f < n0 ? w0 : (f < n0 + n1 ? w1 : nullptr);
  const int fl = f < n0 ? f : f - n0;
  h8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = o * 8 + j;
    v[j] = (w && ci < Cin) ? (_Float16)w[((long)fl * Cin + ci) * 9 + tap] : (_Float16)0.f;
  }
  packed[i] = v;
}

__device__ __forceinline__ float dot8(h8 x, h8 w, float acc) {
  acc = __builtin_amdgcn_fdot2(h2{x[0], x[1]}, h2{w[0], w[1]}, acc, false);
  acc = __builtin_amdgcn_fdot2(h2{x[2], x[3]}, h2{w[2], w[3]}, acc, false);
  acc = __builtin_amdgcn_fdot2(h2{x[4], x[5]}, h2{w[4], w[5]}, acc, false);
  acc = __builtin_amdgcn_fdot2(h2{x[6], x[7]}, h2{w[6], w[7]}, acc, false);
  return acc;
}

// block = (image, output row, column segment); thread = input octet. Each lane keeps a 3x3 window of its octet's 16-byte records
// and slides it along the row: three new loads per output pixel.
template <int NOUT>
__global__ __launch_bounds__(256) void fewout_f16_kernel(FewoutParams p) {
  __shared__ float red[FO_MAXSEG * FO_MAXWAVES * FO_MAXOUT];
  const int o = threadIdx.x, lane = o & 63, wave = o >> 6, nw = blockDim.x >> 6;
  const int seg = blockIdx.x % p.nseg, row = blockIdx.x / p.nseg;
  const int b = row / p.H, oy = row - b * p.H;
  const int x0 = seg * p.seg, x1 = min(p.W, x0 + p.seg);
  const bool active = o < p.noct;
  const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  h8 w[9][NOUT];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int f = 0; f < NOUT; ++f) w[tap][f] = active ? p.wp[((long)o * 9 + tap) * FO_MAXOUT + f] : zero8;
  const _Float16* base = p.in + (long)b * p.H * p.W * p.in_ctotal + 8 * o;
  auto ld = [&](int iy, int ix) -> h8 {
    if (!active || iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) return zero8;
    return *reinterpret_cast<const h8*>(base + ((long)iy * p.W + ix) * p.in_ctotal);
  };
  h8 x[3][3];   // [ky][kx] = input (oy + ky − 1, ox + kx − 1)
  if (x0 < x1) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      x[ky][0] = zero8;
      x[ky][1] = ld(oy + ky - 1, x0 - 1);
      x[ky][2] = ld(oy + ky - 1, x0);
    }
  }
  for (int ox = x0; ox < x1; ++ox) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      x[ky][0] = x[ky][1];
      x[ky][1] = x[ky][2];
      x[ky][2] = ld(oy + ky - 1, ox + 1);
    }
    float s[NOUT];
#pragma unroll
    for (int f = 0; f < NOUT; ++f) {
      float a = 0.f;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) a = dot8(x[tap / 3][tap % 3], w[tap][f], a);
      s[f] = a;
    }
#pragma unroll
    for (int f = 0; f < NOUT; ++f)
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s[f] += __shfl_xor(s[f], m, 64);
    if (lane == 0)
#pragma unroll
      for (int f = 0; f < NOUT; ++f) red[((ox - x0) * FO_MAXWAVES + wave) * FO_MAXOUT + f] = s[f];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (x1 - x0) * NOUT; i += blockDim.x) {
    const int px = i / NOUT, f = i - px * NOUT;
    float v = 0.f;
    for (int k = 0; k < nw; ++k) v += red[(px * FO_MAXWAVES + k) * FO_MAXOUT + f];
    const long hw = (long)p.H * p.W, pix = (long)oy * p.W + x0 + px;
    if (f < p.n0) p.out0[((long)b * p.n0 + f) * hw + pix] = v + p.bias0[f];
    else p.out1[((long)b * p.n1 + (f - p.n0)) * hw + pix] = v + p.bias1[f - p.n0];
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// upsample_flow: Deconvolution k4 s2 (2 → 2 channels) + Crop(1,1), fp32 NCHW in, fp16 into channels [coff, coff + 2) of NHWC
__global__ __launch_bounds__(256) void upsample_flow_f16_kernel(_Float16* __restrict__ out, const float* __restrict__ in,
                                                                const float* __restrict__ w, const float* __restrict__ bias,
                                                                int B, int H, int W, int Ho, int Wo, int out_ctotal, int out_coff) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Ho * Wo) return;
  const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho), b = (int)(i / ((long)Wo * Ho));
  const int py = oy & 1, px = ox & 1, r = oy >> 1, c = ox >> 1;
  float acc[2] = {0.f, 0.f};
  for (int ci = 0; ci < 2; ++ci)
    for (int a = 0; a < 2; ++a) {
      const int iy = r + dc_d(py, a), ky = dc_k(py, a);
      if (iy < 0 || iy >= H) continue;
      for (int bb = 0; bb < 2; ++bb) {
        const int ix = c + dc_d(px, bb), kx = dc_k(px, bb);
        if (ix < 0 || ix >= W) continue;
        const float v = in[(((long)b * 2 + ci) * H + iy) * W + ix];
        for (int co = 0; co < 2; ++co) acc[co] += v * w[((ci * 2 + co) * 4 + ky) * 4 + kx];
      }
    }
  h2 o = {(_Float16)(acc[0] + bias[0]), (_Float16)(acc[1] + bias[1])};
  *reinterpret_cast<h2*>(out + i * out_ctotal + out_coff) = o;
}

// NHWC fp16 channel-slice copy, 8 channels (16 bytes) per thread
__global__ __launch_bounds__(256) void copy_channels_nhwc_f16_kernel(_Float16* __restrict__ dst, int dst_ctotal, int dst_coff,
                                                                     const _Float16* __restrict__ src, int src_ctotal, int src_coff,
                                                                     int noct, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long pix = i / noct;
  const int o = (int)(i - pix * noct);
  *reinterpret_cast<h8*>(dst + pix * dst_ctotal + dst_coff + 8 * o) =
      *reinterpret_cast<const h8*>(src + pix * src_ctotal + src_coff + 8 * o);
}

// split-K plan of the deconvolution: with fewer than 512 block tiles (two per CU), split K so that ~1024 blocks run (four per
// CU: one per SIMD), at least 16 k-steps per slice. Fixed by the geometry.
int deconv_f16_split(int tiles, int nsteps) {
  if (tiles >= 512) return 1;
  int s = std::min(8, (1024 + tiles - 1) / tiles);
  while (s > 1 && nsteps / s < 16) --s;
  return std::max(1, s);
}

// The launch plan of the deconvolution, from the geometry alone: the launcher and deepim_deconv_f16_plan both read it here.
struct DeconvF16Plan {
  int rows[2], cols[2], npix[4], tile_base[5];
  int nsteps, ksplit, steps_per_split;
};

int deconv_f16_plan(int B, int Cin_pad, int H, int W, int Cout, int Ho, int Wo, DeconvF16Plan& q) {
  DI_REQUIRE(B > 0, "deconv_f16: empty batch");
  DI_REQUIRE((Cout & 63) == 0 && Cout > 0 && (Cin_pad & 7) == 0 && Cin_pad > 0,
             "deconv_f16: needs Cout % 64 == 0 and Cin_pad % 8 == 0");
  DI_REQUIRE(Ho <= 2 * H && Wo <= 2 * W && Ho > 0 && Wo > 0, "deconv_f16: Ho <= 2H, Wo <= 2W (crop 1,1 of the 2H+2 x 2W+2 output)");
  q.nsteps = Cin_pad / 4;
  for (int k = 0; k < 2; ++k) { q.rows[k] = (Ho - k + 1) / 2; q.cols[k] = (Wo - k + 1) / 2; }
  const int MT = di_div_up(Cout, DC_BM);
  q.tile_base[0] = 0;
  for (int c = 0; c < 4; ++c) {
    q.npix[c] = B * q.rows[c >> 1] * q.cols[c & 1];
    q.tile_base[c + 1] = q.tile_base[c] + MT * di_div_up(q.npix[c], DC_BN);
  }
  q.ksplit = deconv_f16_split(q.tile_base[4], q.nsteps);
  q.steps_per_split = di_div_up(q.nsteps, q.ksplit);
  q.ksplit = di_div_up(q.nsteps, q.steps_per_split);
  return 0;
}

// The launch plan of the few-filter kernel: one thread per input octet in whole waves; row segments of up to 64 columns, rows split
// further (up to 4 segments) until ~1024 blocks run. The launcher and deepim_fewout_f16_plan both read it here.
struct FewoutF16Plan { int threads, seg, nseg, waves; };

int fewout_f16_plan(int B, int H, int W, int Cin_pad, FewoutF16Plan& q) {
  DI_REQUIRE(B > 0 && H > 0 && W > 0, "conv3x3_fewout_f16: empty input (B, H, W > 0)");
  DI_REQUIRE((Cin_pad & 7) == 0 && Cin_pad > 0 && Cin_pad <= 8 * 64 * FO_MAXWAVES,
             "conv3x3_fewout_f16: Cin_pad % 8 == 0, 0 < Cin_pad <= 2048");
  const int rows = B * H;
  int nseg = std::max(di_div_up(W, FO_MAXSEG), std::min(4, di_div_up(1024, rows)));
  nseg = std::min(nseg, W);
  q.seg = di_div_up(W, nseg);
  q.nseg = di_div_up(W, q.seg);
  q.waves = di_div_up(Cin_pad / 8, 64);
  q.threads = 64 * q.waves;
  return 0;
}

}  // namespace

extern "C" size_t deepim_deconv_f16_packed_size(int Cin_pad, int Cout) {
  return (size_t)4 * Cout * 4 * Cin_pad * sizeof(_Float16);
}

extern "C" int deepim_deconv_f16_pack_weights(deepim_ctx* ctx, void* packed, const float* w, int Cin, int Cin_pad, int Cout) {
  DI_DEVICE(ctx);
  DI_REQUIRE((Cout & 63) == 0 && (Cin_pad & 7) == 0 && Cin_pad >= Cin && Cin > 0,
             "deconv_f16_pack: needs Cout % 64 == 0, Cin_pad % 8 == 0, Cin_pad >= Cin");
  const int nsteps = Cin_pad / 4;
  const long total = (long)4 * (Cout / 32) * nsteps * 64;
  hipLaunchKernelGGL(pack_deconv_f16_kernel, dim3(di_div_up(total, 256)), dim3(256), 0, ctx->stream, (h8*)packed, w, Cin, Cin_pad,
                     Cout, nsteps, total);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_deconv4x4s2_crop_f16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const void* in_nhwc_f16,
                                                   const void* packed_w, const float* bias, int B, int Cin_pad, int in_ctotal,
                                                   int H, int W, int Cout, int Ho, int Wo, float slope, int out_ctotal,
                                                   int out_coff) {
  DI_DEVICE(ctx);
  if (B == 0) return 0;
  DeconvF16Plan q;
  if (int rc = deconv_f16_plan(B, Cin_pad, H, W, Cout, Ho, Wo, q)) return rc;
  DI_REQUIRE((in_ctotal & 7) == 0 && Cin_pad <= in_ctotal, "deconv_f16: in_ctotal % 8 == 0 and Cin_pad <= in_ctotal");
  DI_REQUIRE((out_ctotal & 3) == 0 && (out_coff & 3) == 0 && out_coff >= 0 && out_coff + Cout <= out_ctotal,
             "deconv_f16: out_ctotal, out_coff % 4 == 0 and the slice inside the output record");
  DI_REQUIRE((long)B * H * W * in_ctotal < (1L << 31), "deconv_f16: input must hold < 2^31 halves");
  DeconvF16Params p;
  p.in = (const _Float16*)in_nhwc_f16; p.wp = (const h8*)packed_w; p.bias = bias; p.out = (_Float16*)out_nhwc_f16;
  p.partial = nullptr;
  p.B = B; p.H = H; p.W = W; p.Cin_pad = Cin_pad; p.in_ctotal = in_ctotal; p.Cout = Cout; p.Ho = Ho; p.Wo = Wo;
  p.out_ctotal = out_ctotal; p.out_coff = out_coff; p.slope = slope;
  p.nsteps = q.nsteps; p.ksplit = q.ksplit; p.steps_per_split = q.steps_per_split;
  for (int k = 0; k < 2; ++k) { p.rows[k] = q.rows[k]; p.cols[k] = q.cols[k]; }
  for (int c = 0; c < 4; ++c) p.npix[c] = q.npix[c];
  for (int c = 0; c < 5; ++c) p.tile_base[c] = q.tile_base[c];
  const int tiles = p.tile_base[4];
  const long npix_out = (long)B * Ho * Wo;
  if (p.ksplit > 1) {
    void* scratch;
    int rc = deepim_scratch(ctx, (size_t)p.ksplit * npix_out * Cout * sizeof(float), &scratch);
    if (rc) return rc;
    p.partial = (float*)scratch;
  }
  hipLaunchKernelGGL(deconv_f16_kernel, dim3(tiles * p.ksplit), dim3(256), 0, ctx->stream, p);
  DI_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    const long total4 = npix_out * Cout / 4;
    hipLaunchKernelGGL(deconv_f16_reduce_kernel, dim3(di_div_up(total4, 256)), dim3(256), 0, ctx->stream, p.out, p.partial, bias,
                       total4, p.ksplit, Cout, out_ctotal, out_coff, slope);
    DI_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int deepim_deconv_f16_plan(int B, int Cin_pad, int H, int W, int Cout, int Ho, int Wo, int* plan) {
  DI_REQUIRE(plan != nullptr, "deconv_f16_plan: null plan");
  for (int i = 0; i < 8; ++i) plan[i] = -1;
  DeconvF16Plan q;
  if (int rc = deconv_f16_plan(B, Cin_pad, H, W, Cout, Ho, Wo, q)) return rc;
  const int out[8] = {q.tile_base[4], q.npix[0], q.npix[1], q.npix[2], q.npix[3], q.nsteps, q.ksplit, q.steps_per_split};
  for (int i = 0; i < 8; ++i) plan[i] = out[i];
  return 0;
}

extern "C" size_t deepim_fewout_f16_packed_size(int Cin_pad) { return (size_t)(Cin_pad / 8) * 9 * FO_MAXOUT * 16; }

extern "C" int deepim_fewout_f16_pack_weights(deepim_ctx* ctx, void* packed, const float* w0, int n0, const float* w1, int n1,
                                              int Cin, int Cin_pad) {
  DI_DEVICE(ctx);
  DI_REQUIRE(n0 >= 1 && n1 >= 0 && n0 + n1 <= FO_MAXOUT && (n1 == 0 || w1 != nullptr),
             "fewout_f16_pack: 1 to 3 filters in all, n0 >= 1");
  DI_REQUIRE((Cin_pad & 7) == 0 && Cin_pad > 0 && Cin_pad >= Cin && Cin_pad <= 8 * 64 * FO_MAXWAVES,
             "fewout_f16_pack: Cin_pad % 8 == 0, Cin <= Cin_pad <= 2048, Cin_pad > 0");
  const int noct = Cin_pad / 8, total = noct * 9 * FO_MAXOUT;
  hipLaunchKernelGGL(pack_fewout_f16_kernel, dim3(di_div_up(total, 256)), dim3(256), 0, ctx->stream, (h8*)packed, w0, n0, w1, n1,
                     Cin, noct);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_conv3x3_fewout_f16_forward(deepim_ctx* ctx, float* out0, int n0, float* out1, int n1, const void* in_nhwc_f16,
                                                 const void* packed_w, const float* bias0, const float* bias1, int B, int H, int W,
                                                 int in_ctotal, int Cin_pad) {
  DI_DEVICE(ctx);
  if (B == 0) return 0;
  DI_REQUIRE(n0 >= 1 && n1 >= 0 && n0 + n1 <= FO_MAXOUT && out0 && bias0 && (n1 == 0 || (out1 && bias1)),
             "conv3x3_fewout_f16: 1 to 3 filters in all, n0 >= 1, an output and a bias per tensor");
  FewoutF16Plan q;
  if (int rc = fewout_f16_plan(B, H, W, Cin_pad, q)) return rc;
  DI_REQUIRE(Cin_pad <= in_ctotal && (in_ctotal & 7) == 0, "conv3x3_fewout_f16: in_ctotal % 8 == 0, Cin_pad <= in_ctotal");
  FewoutParams p;
  p.in = (const _Float16*)in_nhwc_f16; p.wp = (const h8*)packed_w; p.bias0 = bias0; p.bias1 = bias1; p.out0 = out0; p.out1 = out1;
  p.n0 = n0; p.n1 = n1; p.B = B; p.H = H; p.W = W; p.in_ctotal = in_ctotal; p.noct = Cin_pad / 8;
  p.seg = q.seg; p.nseg = q.nseg;
  const int threads = q.threads;
  const dim3 grid(B * H * p.nseg);
  switch (n0 + n1) {
    case 1: hipLaunchKernelGGL(fewout_f16_kernel<1>, grid, dim3(threads), 0, ctx->stream, p); break;
    case 2: hipLaunchKernelGGL(fewout_f16_kernel<2>, grid, dim3(threads), 0, ctx->stream, p); break;
    default: hipLaunchKernelGGL(fewout_f16_kernel<3>, grid, dim3(threads), 0, ctx->stream, p); break;
  }
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_fewout_f16_plan(int B, int H, int W, int Cin_pad, int* plan) {
  DI_REQUIRE(plan != nullptr, "fewout_f16_plan: null plan");
  for (int i = 0; i < 4; ++i) plan[i] = -1;
  FewoutF16Plan q;
  if (int rc = fewout_f16_plan(B, H, W, Cin_pad, q)) return rc;
  plan[0] = q.threads; plan[1] = q.seg; plan[2] = q.nseg; plan[3] = q.waves;
  return 0;
}

extern "C" int deepim_upsample_flow_f16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const float* in, const float* w,
                                                const float* bias, int B, int H, int W, int Ho, int Wo, int out_ctotal,
                                                int out_coff) {
  DI_DEVICE(ctx);
  const long total = (long)B * Ho * Wo;
  if (total == 0) return 0;
  DI_REQUIRE((out_coff & 1) == 0 && (out_ctotal & 1) == 0 && out_coff + 2 <= out_ctotal,
             "upsample_flow_f16: even out_ctotal / out_coff, the 2 channels inside the output record");
  DI_REQUIRE(Ho <= 2 * H && Wo <= 2 * W, "upsample_flow_f16: Ho <= 2H, Wo <= 2W");
  hipLaunchKernelGGL(upsample_flow_f16_kernel, dim3(di_div_up(total, 256)), dim3(256), 0, ctx->stream, (_Float16*)out_nhwc_f16, in,
                     w, bias, B, H, W, Ho, Wo, out_ctotal, out_coff);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_copy_channels_nhwc_f16(deepim_ctx* ctx, void* dst, int dst_ctotal, int dst_coff, const void* src,
                                             int src_ctotal, int src_coff, int C, long npix) {
  DI_DEVICE(ctx);
  DI_REQUIRE(((dst_ctotal | dst_coff | src_ctotal | src_coff | C) & 7) == 0,
             "copy_channels_nhwc_f16: channel counts and offsets must be multiples of 8");
  DI_REQUIRE(dst_coff + C <= dst_ctotal && src_coff + C <= src_ctotal, "copy_channels_nhwc_f16: slice outside the record");
  const long total = npix * (C / 8);
  if (total == 0) return 0;
  hipLaunchKernelGGL(copy_channels_nhwc_f16_kernel, dim3(di_div_up(total, 256)), dim3(256), 0, ctx->stream, (_Float16*)dst, dst_ctotal,
                     dst_coff, (const _Float16*)src, src_ctotal, src_coff, C / 8, total);
  DI_LAUNCH_CHECK();
  return 0;
}
