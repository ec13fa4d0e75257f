// I-group: decoded camera frames -> the fp32 NCHW tensors the graph reads (lib/utils/image.py `transform` :583-594, the
// depth / DEPTH_FACTOR of :178-181 / :203-219, `label == mask_idx` of :255-260 / :308-312) and the loader's mask dilation
// (lib/utils/mask_dilate.py:19-47). Four HBM streams: no LDS, no reductions, nothing allocated, per-sample ids and draws read
// from device arrays — legal inside a graph capture, and a replay follows whatever the buffers hold then.
//
// The first three are per-pixel maps, so they walk the batch as ONE flat run of B·H·W pixels, four pixels per lane: a lane
// reads 12 contiguous bytes of an interleaved BGR frame (8 of a uint16 depth map, 4 of a label map) and writes one float4 per
// plane. Four pixels of a frame start at byte 12·g of the batch, so the loads are dword-aligned whatever W is; the float4
// stores need H·W % 4 == 0 (else the planes of one sample start at odd offsets) and fall back to scalar stores. The last
// B·H·W % 4 pixels are a scalar tail.
#include "common.h"

namespace {

struct alignas(4) Bytes12 { uint32_t w[3]; };

__device__ __forceinline__ uint32_t byte_of(const Bytes12& v, int i) { return (v.w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }

// sample b and in-sample pixel q of flat pixel p: ONE division per lane (32-bit where the batch allows), the lane's next pixels
// follow by next_pixel
__device__ __forceinline__ void locate_pixel(long p, long hw, long n, long& b, long& q) {
  b = n <= 0x7fffffffL ? (long)((uint32_t)p / (uint32_t)hw) : p / hw;
  q = p - b * hw;
}
__device__ __forceinline__ void next_pixel(long hw, long& b, long& q) {
  if (++q == hw) { q = 0; ++b; }
}

// the tail of the BGR kernels: px[tensor channel][pixel] less the channel's mean, to the three planes of each pixel's sample
template <bool VEC_OUT>
__device__ __forceinline__ void store_planes(float* __restrict__ out, float (&px)[3][4], const Vec3& means, const long (&bs)[4],
                                             const long (&qs)[4], long hw, int cnt) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) px[c][j] -= means.v[c];
  if (VEC_OUT) {   // hw % 4 == 0: the four pixels share a sample and cnt == 4
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float4*>(out + (bs[0] * 3 + c) * hw + qs[0]) = make_float4(px[c][0], px[c][1], px[c][2], px[c][3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(bs[j] * 3 + c) * hw + qs[j]] = px[c][j];
      }
  }
}

// Frames through an index (the *_frames entries): the input of pair b is frame frame_index[b] of N, not sample b. The ids live
// on the device: one outside [0, N) reads nothing (the pair's output is that of an empty frame) and is reported through
// DI_STATUS_FRAME_RANGE by the lane that owns the pair's first pixel. Unused (and never read) by the per-sample entries.
// N may be a whole resident dataset: every offset into the frames is 64-bit (frame 2 331 of a 480x640 BGR set starts past 2^31).
struct FrameSel {
  const int32_t* frame_index;   // (B)
  int* status;
  int N;
};
// input offset, in pixels, of in-sample pixel q of pair b (flat pixel p of the batch), or -1 for a pair without a frame
template <bool FRAMES>
__device__ __forceinline__ long source_pixel(const FrameSel& fs, long p, long b, long q, long hw) {
  if (!FRAMES) return p;
  const int id = fs.frame_index[b];
  if (id < 0 || id >= fs.N) {
    if (q == 0) atomicOr(fs.status, DI_STATUS_FRAME_RANGE);
    return -1;
  }
  return (long)id * hw + q;
}

// VEC_IN: every input pointer is dword-aligned (12-byte loads); VEC_OUT: hw % 4 == 0 and `out` 16-byte aligned (float4 stores).
// FRAMES (deepim_ingest_bgr8_frames): `frames` and `fg` are (N,H,W[,3]) and pair b reads frame frame_index[b]; `bg` stays per
// pair. Per sample the 12-byte loads are dword-aligned for any W because the batch is one flat run; through an index frame f
// starts at byte 3·hw·f and a lane's four pixels must share a frame, so VEC_IN then also needs hw % 4 == 0 (the launcher's
// rule) — otherwise the scalar path, where a lane's four pixels may belong to two pairs naming different frames and each
// pixel takes its own pair's frame. A pair without a frame is (0 - mean) and composites no background.
template <bool VEC_IN, bool VEC_OUT, bool FRAMES>
__global__ __launch_bounds__(256) void ingest_bgr8_kernel(float* __restrict__ out, const uint8_t* __restrict__ frames,
                                                          const uint8_t* __restrict__ bg, const uint8_t* __restrict__ fg,
                                                          const int32_t* __restrict__ use_bg, Vec3 means, long hw, long n,
                                                          FrameSel fs) {
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= n) return;
  const int cnt = (int)min(4L, n - p0);
  float px[3][4];   // [tensor channel][pixel]
  long bs[4], qs[4];
  locate_pixel(p0, hw, n, bs[0], qs[0]);
#pragma unroll
  for (int j = 1; j < 4; ++j) { bs[j] = bs[j - 1]; qs[j] = qs[j - 1]; next_pixel(hw, bs[j], qs[j]); }
  if (VEC_IN && cnt == 4) {
    const long s0 = source_pixel<FRAMES>(fs, p0, bs[0], qs[0], hw);
    const bool have = !FRAMES || s0 >= 0;
    Bytes12 v = {{0u, 0u, 0u}};
    if (have) v = *reinterpret_cast<const Bytes12*>(frames + s0 * 3);
    if (bg && have) {
      const Bytes12 g = *reinterpret_cast<const Bytes12*>(bg + p0 * 3);
      const uint32_t l = *reinterpret_cast<const uint32_t*>(fg + s0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool take_bg = ((l >> (8 * j)) & 0xffu) == 0 && (!use_bg || use_bg[bs[j]] != 0);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c][j] = (float)(take_bg ? byte_of(g, j * 3 + 2 - c) : byte_of(v, j * 3 + 2 - c));
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c][j] = (float)byte_of(v, j * 3 + 2 - c);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c][j] = 0.f;
      if (j < cnt) {
        const long p = p0 + j;
        const long sp = source_pixel<FRAMES>(fs, p, bs[j], qs[j], hw);
        if (!FRAMES || sp >= 0) {
          const bool take_bg = bg && fg[sp] == 0 && (!use_bg || use_bg[bs[j]] != 0);
          const uint8_t* s = take_bg ? bg + p * 3 : frames + sp * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) px[c][j] = (float)s[2 - c];
        }
      }
    }
  }
  store_planes<VEC_OUT>(out, px, means, bs, qs, hw, cnt);
}

// The background pool of deepim_ingest_bgr8_pool (lib/utils/background.py builds it once): P decoded BGR images back to back,
// and per image everything image.py:108-145 derives from its size and the frame's — the crop, cv2.resize's INTER_LINEAR taps
// and 11-bit weights, the size of the resized image — so that the kernel is integer arithmetic on four gathered taps.
struct BgPool {
  const uint8_t* pixels;     // dword-aligned, every image's start too, 12 readable bytes behind the last image
  const int64_t* desc;       // (P,4): byte offset of the image, its row stride in bytes, oh, ow (the resized image's size)
  const uint32_t* xtab;      // (P,W): output column x as x0 << 13 | (x1 != x0) << 12 | a1, with a0 = 2048 - a1; zeros from ow on
  const uint32_t* ytab;      // (P,H): output row y the same way: y0, y1 = y0 or y0 + 1, b1, b0 = 2048 - b1; zeros from oh on
  const int32_t* bg_index;   // (B)
  int* status;
  int P, H, W;
};
// what pair b draws from: on = it composites a pool image (use_bg[b] != 0), live = that image exists (bg_index[b] in [0, P)).
// Without a live image the pointers are the pool's own with an empty oh x ow: every pixel is outside it, and the loads a lane
// issues for such a pixel (entry 0 of the first tables, the pool's first bytes) stay inside the pool.
struct BgImage {
  const uint8_t* px;
  const uint32_t *xt, *yt;
  int stride, oh, ow;
  bool on, live;
};
__device__ __forceinline__ BgImage bg_image_of(const BgPool& pool, const int32_t* __restrict__ use_bg, long b) {
  BgImage im;
  im.on = !use_bg || use_bg[b] != 0;
  const int id = im.on ? pool.bg_index[b] : -1;
  im.live = id >= 0 && id < pool.P;
  const int k = im.live ? id : 0;
  const int64_t* d = pool.desc + (long)k * 4;
  im.px = pool.pixels + d[0];
  im.stride = (int)d[1];
  im.oh = im.live ? (int)d[2] : 0;
  im.ow = im.live ? (int)d[3] : 0;
  im.xt = pool.xtab + (long)k * pool.W;
  im.yt = pool.ytab + (long)k * pool.H;
  return im;
}
// ONE aligned 12-byte window covers the six bytes from byte address a on whatever a's alignment, so the two taps of a row
// cost one load instead of six
__device__ __forceinline__ Bytes12 load_window(const uint8_t* a) {
  return *reinterpret_cast<const Bytes12*>((uintptr_t)a & ~(uintptr_t)3);
}
// the BGR pixel at byte `at` (0..3) of the window (t0) and, with `next`, the one three bytes on (t1, else t0 again), as 0x00RRGGBB
__device__ __forceinline__ void taps_of(const Bytes12& w, int at, bool next, uint32_t& t0, uint32_t& t1) {
  const uint32_t d0 = (uint32_t)((((uint64_t)w.w[1] << 32) | w.w[0]) >> (8 * at));   // bytes 0..3 from a
  const uint32_t d1 = (uint32_t)((((uint64_t)w.w[2] << 32) | w.w[1]) >> (8 * at));   // bytes 4..7
  t0 = d0 & 0xffffffu;
  t1 = next ? (d0 >> 24) | ((d1 & 0xffffu) << 8) : t0;
}
// cv2.resize INTER_LINEAR on 8-bit pixels (the generic path: 11-bit weights, a horizontal pass kept at 15 bits, a rounded
// vertical pass) from the windows of the two source rows and the column's and the row's table entries, as 0x00RRGGBB
__device__ __forceinline__ uint32_t bg_resample(const Bytes12& w0, const Bytes12& w1, int at0, int at1, uint32_t ex, uint32_t ey) {
  const int a1 = (int)(ex & 0xfffu), a0 = 2048 - a1, b1 = (int)(ey & 0xfffu), b0 = 2048 - b1;
  uint32_t p00, p01, p10, p11;
  taps_of(w0, at0, (ex & 0x1000u) != 0, p00, p01);
  taps_of(w1, at1, (ex & 0x1000u) != 0, p10, p11);
  uint32_t r = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int r0 = (int)((p00 >> (8 * c)) & 0xffu) * a0 + (int)((p01 >> (8 * c)) & 0xffu) * a1;
    const int r1 = (int)((p10 >> (8 * c)) & 0xffu) * a0 + (int)((p11 >> (8 * c)) & 0xffu) * a1;
    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    r |= (uint32_t)min(max(v, 0), 255) << (8 * c);
  }
  return r;
}

// ingest_bgr8_kernel with the background made on the fly: same flat walk, same loads of the frame and its labels, same
// stores. A pixel whose label is 0, in a pair with use_bg != 0, is the pool image's resampled pixel inside oh x ow and black
// outside (image.py:118,145: the resized crop is pasted at the top-left of a black frame); a pair whose bg_index is outside
// [0, P) is black everywhere and reported through DI_STATUS_BG_RANGE by the lane that owns the pair's first pixel.
// Lanes without a label-0 pixel read nothing of the pool. The others work in stages without a branch in between, so that
// the loads of a stage are in flight together: the descriptor (once per lane; once per pixel only where H·W % 4 != 0 lets a
// lane's pixels cross into the next pair), the four pixels' table entries, their eight windows, the arithmetic. A pixel that
// takes no background rides along on entry 0 and the image's first bytes, and its result is dropped.
// FRAMES (deepim_ingest_bgr8_pool_frames): `frames` and `fg` are (N,H,W[,3]) and pair b reads frame frame_index[b] of both,
// under ingest_bgr8_kernel's alignment rule; use_bg and bg_index stay per pair. A pair without a frame is black with a
// non-zero label everywhere: (0 - mean), no background.
template <bool VEC_IN, bool VEC_OUT, bool FRAMES>
__global__ __launch_bounds__(256) void ingest_bgr8_pool_kernel(float* __restrict__ out, const uint8_t* __restrict__ frames,
                                                               const uint8_t* __restrict__ fg,
                                                               const int32_t* __restrict__ use_bg, BgPool pool, Vec3 means,
                                                               long hw, long n, FrameSel fs) {
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= n) return;
  const int cnt = (int)min(4L, n - p0);
  long bs[4], qs[4];
  locate_pixel(p0, hw, n, bs[0], qs[0]);
#pragma unroll
  for (int j = 1; j < 4; ++j) { bs[j] = bs[j - 1]; qs[j] = qs[j - 1]; next_pixel(hw, bs[j], qs[j]); }
  uint32_t pix[4], lab[4];   // 0x00RRGGBB of the frame; the label
  if (VEC_IN && cnt == 4) {
    const long s0 = source_pixel<FRAMES>(fs, p0, bs[0], qs[0], hw);
    Bytes12 v = {{0u, 0u, 0u}};
    uint32_t l = 0x01010101u;
    if (!FRAMES || s0 >= 0) {
      v = *reinterpret_cast<const Bytes12*>(frames + s0 * 3);
      l = *reinterpret_cast<const uint32_t*>(fg + s0);
    }
    pix[0] = v.w[0] & 0xffffffu;
    pix[1] = (v.w[0] >> 24) | ((v.w[1] & 0xffffu) << 8);
    pix[2] = (v.w[1] >> 16) | ((v.w[2] & 0xffu) << 16);
    pix[3] = v.w[2] >> 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) lab[j] = (l >> (8 * j)) & 0xffu;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pix[j] = 0; lab[j] = 1;
      if (j < cnt) {
        const long sp = source_pixel<FRAMES>(fs, p0 + j, bs[j], qs[j], hw);
        if (!FRAMES || sp >= 0) {
          const uint8_t* s = frames + sp * 3;
          pix[j] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
          lab[j] = fg[sp];
        }
      }
    }
  }
  bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) any |= j < cnt && (lab[j] == 0 || qs[j] == 0);
  if (any) {
    int ys[4], xs[4];
    ys[0] = (int)((uint32_t)qs[0] / (uint32_t)pool.W);   // hw < 2^31 (checked by the launcher)
    xs[0] = (int)qs[0] - ys[0] * pool.W;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      xs[j] = xs[j - 1] + 1; ys[j] = ys[j - 1];
      if (xs[j] == pool.W) { xs[j] = 0; if (++ys[j] == pool.H) ys[j] = 0; }
    }
    BgImage im[4];
    im[0] = bg_image_of(pool, use_bg, bs[0]);
#pragma unroll
    for (int j = 1; j < 4; ++j) im[j] = VEC_OUT || j >= cnt ? im[0] : bg_image_of(pool, use_bg, bs[j]);
    bool take[4], in[4];   // the pixel is background; it lies inside the resized image
    uint32_t ex[4], ey[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt && qs[j] == 0 && im[j].on && !im[j].live) atomicOr(pool.status, DI_STATUS_BG_RANGE);
      take[j] = j < cnt && lab[j] == 0 && im[j].on;
      in[j] = take[j] && ys[j] < im[j].oh && xs[j] < im[j].ow;
      ex[j] = im[j].xt[in[j] ? xs[j] : 0];
      ey[j] = im[j].yt[in[j] ? ys[j] : 0];
    }
    Bytes12 win[4][2];
    int at[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint8_t* r0 = im[j].px + (long)(ey[j] >> 13) * im[j].stride + (ex[j] >> 13) * 3;
      const uint8_t* r1 = (ey[j] & 0x1000u) ? r0 + im[j].stride : r0;
      win[j][0] = load_window(r0); at[j][0] = (int)((uintptr_t)r0 & 3);
      win[j][1] = load_window(r1); at[j][1] = (int)((uintptr_t)r1 & 3);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t v = bg_resample(win[j][0], win[j][1], at[j][0], at[j][1], ex[j], ey[j]);
      if (take[j]) pix[j] = in[j] ? v : 0u;
    }
  }
  float px[3][4];   // [tensor channel][pixel]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c][j] = (float)((pix[j] >> (8 * (2 - c))) & 0xffu);
  store_planes<VEC_OUT>(out, px, means, bs, qs, hw, cnt);
}

// out (B,1,H,W) is as flat as the inputs: pixel p of the batch goes to out[p]. VEC with FRAMES: hw % 4 == 0 as well, so that
// a lane's four pixels share a pair and a frame
template <bool VEC, bool FRAMES>
__global__ __launch_bounds__(256) void ingest_depth16_kernel(float* __restrict__ out, const uint16_t* __restrict__ depth,
                                                             const uint8_t* __restrict__ labels,
                                                             const int32_t* __restrict__ mask_idx, float depth_factor,
                                                             long hw, long n, FrameSel fs) {
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= n) return;
  const int cnt = (int)min(4L, n - p0);
  long b, q;
  locate_pixel(p0, hw, n, b, q);
  if (VEC && cnt == 4) {
    const long s0 = source_pixel<FRAMES>(fs, p0, b, q, hw);
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    if (s0 >= 0) {
      const uint2 d = *reinterpret_cast<const uint2*>(depth + s0);
      r[0] = (float)(d.x & 0xffffu); r[1] = (float)(d.x >> 16); r[2] = (float)(d.y & 0xffffu); r[3] = (float)(d.y >> 16);
      // a correctly rounded fp32 division, as numpy's: a reciprocal multiply gives other bits
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = __fdiv_rn(r[j], depth_factor);
      if (labels) {
        const uint32_t l = *reinterpret_cast<const uint32_t*>(labels + s0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if ((int)((l >> (8 * j)) & 0xffu) != mask_idx[b]) r[j] = 0.f;
          next_pixel(hw, b, q);
        }
      }
    }
    *reinterpret_cast<float4*>(out + p0) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
    for (int j = 0; j < cnt; ++j) {
      const long p = p0 + j;
      const long s = source_pixel<FRAMES>(fs, p, b, q, hw);
      float r = 0.f;
      if (s >= 0) {
        r = __fdiv_rn((float)depth[s], depth_factor);
        if (labels && (int)labels[s] != mask_idx[b]) r = 0.f;
      }
      out[p] = r;
      next_pixel(hw, b, q);
    }
  }
}

template <bool VEC, bool FRAMES>
__global__ __launch_bounds__(256) void ingest_label_mask_kernel(float* __restrict__ out, const uint8_t* __restrict__ labels,
                                                                const int32_t* __restrict__ mask_idx, long hw, long n,
                                                                FrameSel fs) {
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= n) return;
  const int cnt = (int)min(4L, n - p0);
  long b, q;
  locate_pixel(p0, hw, n, b, q);
  if (VEC && cnt == 4) {
    const long s0 = source_pixel<FRAMES>(fs, p0, b, q, hw);
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    if (s0 >= 0) {
      const uint32_t l = *reinterpret_cast<const uint32_t*>(labels + s0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = (int)((l >> (8 * j)) & 0xffu) == mask_idx[b] ? 1.f : 0.f;
        next_pixel(hw, b, q);
      }
    }
    *reinterpret_cast<float4*>(out + p0) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
    for (int j = 0; j < cnt; ++j) {
      const long s = source_pixel<FRAMES>(fs, p0 + j, b, q, hw);
      out[p0 + j] = s >= 0 && (int)labels[s] == mask_idx[b] ? 1.f : 0.f;
      next_pixel(hw, b, q);
    }
  }
}

// mask_dilate.py:19-47 as a gather. Block k of the file ORs the origin mask, shifted by its thickness t_k, into the pixels the
// origin leaves empty: :24 reads origin[y - t], :30 origin[y + t], :36 origin[:, x - t], :42 origin[:, x + t]. A source row
// or column outside the frame is outside the reference's slices too, which also covers t >= H (or W): empty slices. Where the
// origin is non-zero the sum keeps it, and :46 clamps what exceeds 1.
__device__ __forceinline__ float dilate_pixel(const float* __restrict__ m, float c, int y, int x, int H, int W, int td, int tu,
                                              int tr, int tl) {
  if (c != 0.f) return c > 1.f ? 1.f : c;
  bool hit = false;
  if (td > 0 && y >= td) hit = m[(long)(y - td) * W + x] != 0.f;
  if (!hit && tu > 0 && y + (long)tu < H) hit = m[(long)(y + tu) * W + x] != 0.f;
  if (!hit && tr > 0 && x >= tr) hit = m[(long)y * W + (x - tr)] != 0.f;
  if (!hit && tl > 0 && x + (long)tl < W) hit = m[(long)y * W + (x + tl)] != 0.f;
  return hit ? 1.f : 0.f;
}

struct alignas(4) Floats4 { float v[4]; };   // four floats at a dword-aligned address: one 16-byte load

// grid (pixel blocks, B). VEC: W % 4 == 0 and both pointers 16-byte aligned — a lane owns four pixels of one row and gathers each
// enabled side with ONE 16-byte load (rows above / below are float4-aligned, the shifted run of its own row is dword-aligned);
// only the lanes whose run crosses the row's end fall back to per-pixel loads. Lanes without an empty pixel load nothing more.
template <bool VEC>
__global__ __launch_bounds__(256) void mask_dilate_kernel(float* __restrict__ out, const float* __restrict__ mask,
                                                          const int32_t* __restrict__ thickness, int H, int W) {
  const int b = blockIdx.y;
  const long hw = (long)H * W;
  const float* m = mask + b * hw;
  float* o = out + b * hw;
  const int td = thickness[b * 4 + 0], tu = thickness[b * 4 + 1], tr = thickness[b * 4 + 2], tl = thickness[b * 4 + 3];
  if (VEC) {
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= hw) return;
    const int y = (int)((uint32_t)p0 / (uint32_t)W), x = (int)(p0 - (long)y * W);   // hw < 2^31 (checked by the launcher)
    const float4 c4 = *reinterpret_cast<const float4*>(m + p0);
    const float c[4] = {c4.x, c4.y, c4.z, c4.w};
    bool hit[4] = {false, false, false, false};
    if (c[0] == 0.f || c[1] == 0.f || c[2] == 0.f || c[3] == 0.f) {
      if (td > 0 && y >= td) {                                                    // :24 origin[y - t]
        const float4 v = *reinterpret_cast<const float4*>(m + p0 - (long)td * W);
        hit[0] |= v.x != 0.f; hit[1] |= v.y != 0.f; hit[2] |= v.z != 0.f; hit[3] |= v.w != 0.f;
      }
      if (tu > 0 && y + (long)tu < H) {                                           // :30 origin[y + t]
        const float4 v = *reinterpret_cast<const float4*>(m + p0 + (long)tu * W);
        hit[0] |= v.x != 0.f; hit[1] |= v.y != 0.f; hit[2] |= v.z != 0.f; hit[3] |= v.w != 0.f;
      }
      if (tr > 0) {                                                               // :36 origin[:, x - t]
        if (x >= tr) {
          const Floats4 v = *reinterpret_cast<const Floats4*>(m + p0 - tr);
#pragma unroll
          for (int i = 0; i < 4; ++i) hit[i] |= v.v[i] != 0.f;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (x + i >= tr) hit[i] |= m[p0 + i - tr] != 0.f;
        }
      }
      if (tl > 0) {                                                               // :42 origin[:, x + t]
        if (x + 3 + (long)tl < W) {
          const Floats4 v = *reinterpret_cast<const Floats4*>(m + p0 + tl);
#pragma unroll
          for (int i = 0; i < 4; ++i) hit[i] |= v.v[i] != 0.f;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (x + i + (long)tl < W) hit[i] |= m[p0 + i + tl] != 0.f;
        }
      }
    }
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = c[i] != 0.f ? (c[i] > 1.f ? 1.f : c[i]) : (hit[i] ? 1.f : 0.f);
    *reinterpret_cast<float4*>(o + p0) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int y = (int)((uint32_t)p / (uint32_t)W), x = (int)(p - (long)y * W);
    o[p] = dilate_pixel(m, m[p], y, x, H, W, td, tu, tr, tl);
  }
}

// image.py:301-303 for a batch: the planes of the samples whose initial render covered no pixel become zero, the others are
// not touched (no load, no store). covered[b] depends on blockIdx.y only: a scalar load and a uniform exit.
template <bool VEC>
__global__ __launch_bounds__(256) void mask_gate_kernel(float* __restrict__ mask, const int32_t* __restrict__ covered, long hw) {
  const int b = blockIdx.y;
  if (covered[b] != 0) return;
  float* o = mask + b * hw;
  if (VEC) {
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 < hw) *reinterpret_cast<float4*>(o + p0) = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < hw) o[p] = 0.f;
  }
}

// deepim_gather_rows: out[b] = table[index[b]] for rows of `row_units` units T (uint4 where the row length and the three
// pointers allow 16-byte accesses, else one 4-byte word), one lane per unit of the B·row_units flat run. An index outside
// [0, n_rows) reads nothing: the row is zeros, reported through DI_STATUS_FRAME_RANGE by the lane that owns its first unit.
// Rows may be whole frames of a resident set: the table offset is 64-bit.
template <class T>
__global__ __launch_bounds__(256) void gather_rows_kernel(T* __restrict__ out, const T* __restrict__ table,
                                                          const int32_t* __restrict__ index, int n_rows, long row_units, long n,
                                                          int* status) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= n) return;
  long b, r;
  locate_pixel(u, row_units, n, b, r);
  const int id = index[b];
  T v = T();
  if (id >= 0 && id < n_rows) v = table[(long)id * row_units + r];
  else if (r == 0) atomicOr(status, DI_STATUS_FRAME_RANGE);
  out[u] = v;
}

// deepim_occlusion_gate: the fallback of lib/utils/mask_augment.py:91-93 for the synthetic scenes of deepim_render_scene_forward. Pair
// b (blockIdx.y: visible, full, the row and the verdict are scalar loads and uniform exits) is kept iff full[b] > 0 and
// visible[b,0] >= min_visible full[b], in double. Its depth_gt row always becomes the alone depth; a kept pair's blocks stop
// there, the others copy the alone image and label (and depth_observed) over the scene's. A byte copy: four pixels per lane
// (three dwords, two, one) or single pixels. Block (0,0) also adds the batch's counts to the running totals: integer sums over
// visible / full / slot_class, which no block writes, by one block per launch, so plain adds as in sample_stats_kernel.
struct OcclusionGate {
  uint8_t* image; uint16_t* depth_gt; uint8_t* label; uint16_t* depth_observed;       // (N,H,W[,3]); depth_observed or NULL
  const uint8_t* alone_image; const uint16_t* alone_depth; const uint8_t* alone_label;  // (B,H,W[,3])
  const int32_t* visible; const int32_t* full; const int32_t* slot_class; const int32_t* rows;
  int32_t* kept;
  unsigned long long* totals;
  float min_visible;
  int N, B, S;
  long hw;
  __device__ __forceinline__ bool keep(int b) const {
    const int f = full[b];
    return f > 0 && (double)visible[(long)b * S] >= (double)min_visible * (double)f;
  }
};

template <bool VEC>
__global__ __launch_bounds__(256) void occlusion_gate_kernel(OcclusionGate a) {
  const int b = blockIdx.y;
  const bool keep = a.keep(b);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.kept[b] = keep ? 1 : 0;
  if (a.totals != nullptr && blockIdx.x == 0 && b == 0) {      // uniform per block: the barrier below is reached by all 256 threads
    __shared__ unsigned long long red[4][2];
    unsigned long long nk = 0, ns = 0;
    for (int i = threadIdx.x; i < a.B; i += 256) {
      nk += a.keep(i) ? 1ull : 0ull;
      if (a.slot_class != nullptr)
        for (int s = 1; s < a.S; ++s) ns += a.slot_class[(long)i * a.S + s] >= 0 ? 1ull : 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      nk += __shfl_xor(nk, off, 64);
      ns += __shfl_xor(ns, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = nk; red[threadIdx.x >> 6][1] = ns; }
    __syncthreads();
    if (threadIdx.x == 0) {
      a.totals[0] += (unsigned long long)a.B;
      a.totals[1] += (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
      a.totals[2] += (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
  }
  const int row = a.rows ? a.rows[b] : b;
  if ((unsigned)row >= (unsigned)a.N) return;
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
  if (p0 >= a.hw) return;
  const long src = (long)b * a.hw + p0, dst = (long)row * a.hw + p0;
  if (VEC) {
    const uint2 d = *reinterpret_cast<const uint2*>(a.alone_depth + src);
    *reinterpret_cast<uint2*>(a.depth_gt + dst) = d;
    if (keep) return;
    const uint32_t* si = reinterpret_cast<const uint32_t*>(a.alone_image + src * 3);
    uint32_t* di = reinterpret_cast<uint32_t*>(a.image + dst * 3);
    const uint32_t w0 = si[0], w1 = si[1], w2 = si[2];
    di[0] = w0; di[1] = w1; di[2] = w2;
    *reinterpret_cast<uint32_t*>(a.label + dst) = *reinterpret_cast<const uint32_t*>(a.alone_label + src);
    if (a.depth_observed != nullptr) *reinterpret_cast<uint2*>(a.depth_observed + dst) = d;
  } else {
    const uint16_t d = a.alone_depth[src];
    a.depth_gt[dst] = d;
    if (keep) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.image[dst * 3 + c] = a.alone_image[src * 3 + c];
    a.label[dst] = a.alone_label[src];
    if (a.depth_observed != nullptr) a.depth_observed[dst] = d;
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the launch of both BGR entries: fs = NULL reads sample b (deepim_ingest_bgr8), else frame fs->frame_index[b]
int launch_ingest_bgr8(deepim_ctx* ctx, float* out, const uint8_t* frames, const uint8_t* bg_frames, const uint8_t* fg_labels,
                       const int32_t* use_bg, const float* means_rgb, long hw, long n, const FrameSel* fs) {
  Vec3 means = {{0.f, 0.f, 0.f}};
  if (means_rgb) for (int i = 0; i < 3; ++i) means.v[i] = means_rgb[i];
  const bool vin = aligned_to(frames, 4) && (!bg_frames || (aligned_to(bg_frames, 4) && aligned_to(fg_labels, 4))) &&
                   (!fs || hw % 4 == 0);
  const bool vout = hw % 4 == 0 && aligned_to(out, 16);
  const dim3 grid(di_div_up(di_div_up(n, 4), 256)), block(256);
  const FrameSel sel = fs ? *fs : FrameSel{NULL, NULL, 0};
#define DI_INGEST_BGR(VI, VO)                                                                                              \
  do {                                                                                                                     \
    if (fs) hipLaunchKernelGGL((ingest_bgr8_kernel<VI, VO, true>), grid, block, 0, ctx->stream, out, frames, bg_frames,    \
                               fg_labels, use_bg, means, hw, n, sel);                                                      \
    else hipLaunchKernelGGL((ingest_bgr8_kernel<VI, VO, false>), grid, block, 0, ctx->stream, out, frames, bg_frames,      \
                            fg_labels, use_bg, means, hw, n, sel);                                                         \
  } while (0)
  if (vin && vout) DI_INGEST_BGR(true, true);
  else if (vin) DI_INGEST_BGR(true, false);
  else if (vout) DI_INGEST_BGR(false, true);
  else DI_INGEST_BGR(false, false);
#undef DI_INGEST_BGR
  DI_LAUNCH_CHECK();
  return 0;
}

// the launch of both pool entries, after their argument checks
int launch_ingest_bgr8_pool(deepim_ctx* ctx, float* out, const uint8_t* frames, const uint8_t* fg_labels, const int32_t* use_bg,
                            const int32_t* bg_index, const uint8_t* pool_pixels, const int64_t* pool_desc, const int32_t* xtab,
                            const int32_t* ytab, int P, const float* means_rgb, int B, int H, int W, const FrameSel* fs) {
  const long hw = (long)H * W, n = (long)B * hw;
  DI_REQUIRE(hw <= 0x7fffffffL, "ingest_bgr8_pool: frame too large");
  if (n == 0) return 0;
  DI_REQUIRE(out && frames && fg_labels && bg_index, "ingest_bgr8_pool: out, frames, fg_labels and bg_index are required");
  DI_REQUIRE(P >= 1 && pool_pixels && pool_desc && xtab && ytab, "ingest_bgr8_pool: the pool, its tables and P >= 1 are required");
  DI_REQUIRE(aligned_to(pool_pixels, 4) && aligned_to(pool_desc, 8) && aligned_to(xtab, 4) && aligned_to(ytab, 4) &&
                 aligned_to(bg_index, 4) && (!use_bg || aligned_to(use_bg, 4)),
             "ingest_bgr8_pool: pool_desc must be 8-byte aligned, pool_pixels, the tables and the draws 4-byte aligned");
  Vec3 means = {{0.f, 0.f, 0.f}};
  if (means_rgb) for (int i = 0; i < 3; ++i) means.v[i] = means_rgb[i];
  const BgPool pool = {pool_pixels, pool_desc, reinterpret_cast<const uint32_t*>(xtab), reinterpret_cast<const uint32_t*>(ytab),
                       bg_index, ctx->status, P, H, W};
  const bool vin = aligned_to(frames, 4) && aligned_to(fg_labels, 4) && (!fs || hw % 4 == 0);
  const bool vout = hw % 4 == 0 && aligned_to(out, 16);
  const dim3 grid(di_div_up(di_div_up(n, 4), 256)), block(256);
  const FrameSel sel = fs ? *fs : FrameSel{NULL, NULL, 0};
#define DI_INGEST_POOL(VI, VO)                                                                                               \
  do {                                                                                                                       \
    if (fs) hipLaunchKernelGGL((ingest_bgr8_pool_kernel<VI, VO, true>), grid, block, 0, ctx->stream, out, frames, fg_labels, \
                               use_bg, pool, means, hw, n, sel);                                                             \
    else hipLaunchKernelGGL((ingest_bgr8_pool_kernel<VI, VO, false>), grid, block, 0, ctx->stream, out, frames, fg_labels,   \
                            use_bg, pool, means, hw, n, sel);                                                                \
  } while (0)
  if (vin && vout) DI_INGEST_POOL(true, true);
  else if (vin) DI_INGEST_POOL(true, false);
  else if (vout) DI_INGEST_POOL(false, true);
  else DI_INGEST_POOL(false, false);
#undef DI_INGEST_POOL
  DI_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int deepim_ingest_bgr8(deepim_ctx* ctx, float* out, const uint8_t* frames, const uint8_t* bg_frames,
                                  const uint8_t* fg_labels, const int32_t* use_bg, const float* means_rgb, int B, int H,
                                  int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ingest_bgr8: negative size");
  DI_REQUIRE((bg_frames == NULL) == (fg_labels == NULL), "ingest_bgr8: bg_frames and fg_labels come together or not at all");
  DI_REQUIRE(bg_frames != NULL || use_bg == NULL, "ingest_bgr8: use_bg without bg_frames");
  const long hw = (long)H * W, n = (long)B * hw;
  if (n == 0) return 0;
  return launch_ingest_bgr8(ctx, out, frames, bg_frames, fg_labels, use_bg, means_rgb, hw, n, NULL);
}

extern "C" int deepim_ingest_bgr8_frames(deepim_ctx* ctx, float* out, const uint8_t* frames, const int32_t* frame_index, int N,
                                         const float* means_rgb, int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ingest_bgr8_frames: negative size");
  const long hw = (long)H * W, n = (long)B * hw;
  if (n == 0) return 0;
  DI_REQUIRE(N >= 1 && out && frames && frame_index, "ingest_bgr8_frames: out, frames, frame_index and N >= 1 are required");
  DI_REQUIRE(aligned_to(frame_index, 4), "ingest_bgr8_frames: frame_index must be 4-byte aligned");
  const FrameSel fs = {frame_index, ctx->status, N};
  return launch_ingest_bgr8(ctx, out, frames, NULL, NULL, NULL, means_rgb, hw, n, &fs);
}

extern "C" int deepim_ingest_bgr8_pool(deepim_ctx* ctx, float* out, const uint8_t* frames, const uint8_t* fg_labels,
                                       const int32_t* use_bg, const int32_t* bg_index, const uint8_t* pool_pixels,
                                       const int64_t* pool_desc, const int32_t* xtab, const int32_t* ytab, int P,
                                       const float* means_rgb, int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ingest_bgr8_pool: negative size");
  return launch_ingest_bgr8_pool(ctx, out, frames, fg_labels, use_bg, bg_index, pool_pixels, pool_desc, xtab, ytab, P, means_rgb,
                                 B, H, W, NULL);
}

extern "C" int deepim_ingest_bgr8_pool_frames(deepim_ctx* ctx, float* out, const uint8_t* frames, const uint8_t* fg_labels,
                                              const int32_t* frame_index, int N, const int32_t* use_bg, const int32_t* bg_index,
                                              const uint8_t* pool_pixels, const int64_t* pool_desc, const int32_t* xtab,
                                              const int32_t* ytab, int P, const float* means_rgb, int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ingest_bgr8_pool_frames: negative size");
  if ((long)B * H * W == 0) return 0;
  DI_REQUIRE(N >= 1 && frame_index && aligned_to(frame_index, 4),
             "ingest_bgr8_pool_frames: a 4-byte aligned frame_index and N >= 1 are required");
  const FrameSel fs = {frame_index, ctx->status, N};
  return launch_ingest_bgr8_pool(ctx, out, frames, fg_labels, use_bg, bg_index, pool_pixels, pool_desc, xtab, ytab, P, means_rgb,
                                 B, H, W, &fs);
}

extern "C" int deepim_gather_rows(deepim_ctx* ctx, void* out, const void* table, const int32_t* index, int n_rows,
                                  long row_words, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && row_words >= 0 && n_rows >= 0, "gather_rows: negative size");
  if (B == 0 || row_words == 0) return 0;
  DI_REQUIRE(out && table && index && n_rows >= 1, "gather_rows: out, table, index and n_rows >= 1 are required");
  DI_REQUIRE(aligned_to(out, 4) && aligned_to(table, 4) && aligned_to(index, 4), "gather_rows: every pointer must be 4-byte aligned");
  DI_REQUIRE(out != table, "gather_rows: out == table (a gather cannot run in place)");
  if (row_words % 4 == 0 && aligned_to(out, 16) && aligned_to(table, 16)) {
    const long units = row_words / 4, n = (long)B * units;
    DI_REQUIRE(n <= 0x7fffffffL * 256L, "gather_rows: batch too large");
    hipLaunchKernelGGL(gather_rows_kernel<uint4>, dim3(di_div_up(n, 256)), dim3(256), 0, ctx->stream, static_cast<uint4*>(out),
                       static_cast<const uint4*>(table), index, n_rows, units, n, ctx->status);
  } else {
    const long n = (long)B * row_words;
    DI_REQUIRE(n <= 0x7fffffffL * 256L, "gather_rows: batch too large");
    hipLaunchKernelGGL(gather_rows_kernel<uint32_t>, dim3(di_div_up(n, 256)), dim3(256), 0, ctx->stream,
                       static_cast<uint32_t*>(out), static_cast<const uint32_t*>(table), index, n_rows, row_words, n, ctx->status);
  }
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_ingest_depth16(deepim_ctx* ctx, float* out, const uint16_t* depth, const uint8_t* labels,
                                     const int32_t* mask_idx, float depth_factor, int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ingest_depth16: negative size");
  DI_REQUIRE((labels == NULL) == (mask_idx == NULL), "ingest_depth16: labels and mask_idx come together or not at all");
  const long hw = (long)H * W, n = (long)B * hw;
  if (n == 0) return 0;
  const bool vec = aligned_to(out, 16) && aligned_to(depth, 8) && (!labels || aligned_to(labels, 4));
  const dim3 grid(di_div_up(di_div_up(n, 4), 256)), block(256);
  const FrameSel none = {NULL, NULL, 0};
  if (vec)
    hipLaunchKernelGGL((ingest_depth16_kernel<true, false>), grid, block, 0, ctx->stream, out, depth, labels, mask_idx,
                       depth_factor, hw, n, none);
  else
    hipLaunchKernelGGL((ingest_depth16_kernel<false, false>), grid, block, 0, ctx->stream, out, depth, labels, mask_idx,
                       depth_factor, hw, n, none);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_ingest_depth16_frames(deepim_ctx* ctx, float* out, const uint16_t* depth, const uint8_t* labels,
                                            const int32_t* frame_index, const int32_t* mask_idx, float depth_factor, int N,
                                            int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ingest_depth16_frames: negative size");
  DI_REQUIRE((labels == NULL) == (mask_idx == NULL), "ingest_depth16_frames: labels and mask_idx come together or not at all");
  const long hw = (long)H * W, n = (long)B * hw;
  if (n == 0) return 0;
  DI_REQUIRE(N >= 1 && depth && frame_index, "ingest_depth16_frames: depth, frame_index and N >= 1 are required");
  DI_REQUIRE(aligned_to(depth, 2), "ingest_depth16_frames: depth must be 2-byte aligned");
  const bool vec = hw % 4 == 0 && aligned_to(out, 16) && aligned_to(depth, 8) && (!labels || aligned_to(labels, 4));
  const dim3 grid(di_div_up(di_div_up(n, 4), 256)), block(256);
  const FrameSel fs = {frame_index, ctx->status, N};
  if (vec)
    hipLaunchKernelGGL((ingest_depth16_kernel<true, true>), grid, block, 0, ctx->stream, out, depth, labels, mask_idx,
                       depth_factor, hw, n, fs);
  else
    hipLaunchKernelGGL((ingest_depth16_kernel<false, true>), grid, block, 0, ctx->stream, out, depth, labels, mask_idx,
                       depth_factor, hw, n, fs);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_ingest_label_mask(deepim_ctx* ctx, float* out, const uint8_t* labels, const int32_t* mask_idx, int B,
                                        int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ingest_label_mask: negative size");
  const long hw = (long)H * W, n = (long)B * hw;
  if (n == 0) return 0;
  const bool vec = aligned_to(out, 16) && aligned_to(labels, 4);
  const dim3 grid(di_div_up(di_div_up(n, 4), 256)), block(256);
  const FrameSel none = {NULL, NULL, 0};
  if (vec) hipLaunchKernelGGL((ingest_label_mask_kernel<true, false>), grid, block, 0, ctx->stream, out, labels, mask_idx, hw, n, none);
  else hipLaunchKernelGGL((ingest_label_mask_kernel<false, false>), grid, block, 0, ctx->stream, out, labels, mask_idx, hw, n, none);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_ingest_label_mask_frames(deepim_ctx* ctx, float* out, const uint8_t* labels, const int32_t* frame_index,
                                               const int32_t* mask_idx, int N, int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "ingest_label_mask_frames: negative size");
  const long hw = (long)H * W, n = (long)B * hw;
  if (n == 0) return 0;
  DI_REQUIRE(N >= 1 && labels && frame_index && mask_idx, "ingest_label_mask_frames: labels, frame_index, mask_idx and N >= 1 are required");
  const bool vec = hw % 4 == 0 && aligned_to(out, 16) && aligned_to(labels, 4);
  const dim3 grid(di_div_up(di_div_up(n, 4), 256)), block(256);
  const FrameSel fs = {frame_index, ctx->status, N};
  if (vec) hipLaunchKernelGGL((ingest_label_mask_kernel<true, true>), grid, block, 0, ctx->stream, out, labels, mask_idx, hw, n, fs);
  else hipLaunchKernelGGL((ingest_label_mask_kernel<false, true>), grid, block, 0, ctx->stream, out, labels, mask_idx, hw, n, fs);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_mask_dilate(deepim_ctx* ctx, float* out, const float* mask, const int32_t* thickness, int B, int H,
                                  int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "mask_dilate: negative size");
  DI_REQUIRE(out != mask, "mask_dilate: out == mask (the dilation gathers from its input and cannot run in place)");
  DI_REQUIRE(B <= 65535, "mask_dilate: batch too large");
  const long hw = (long)H * W;
  DI_REQUIRE(hw <= 0x7fffffffL, "mask_dilate: frame too large");
  if (B == 0 || hw == 0) return 0;
  const bool vec = W % 4 == 0 && aligned_to(out, 16) && aligned_to(mask, 16);
  if (vec)
    hipLaunchKernelGGL(mask_dilate_kernel<true>, dim3(di_div_up(hw / 4, 256), B), dim3(256), 0, ctx->stream, out, mask,
                       thickness, H, W);
  else
    hipLaunchKernelGGL(mask_dilate_kernel<false>, dim3(di_div_up(hw, 256), B), dim3(256), 0, ctx->stream, out, mask,
                       thickness, H, W);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_mask_gate(deepim_ctx* ctx, float* mask, const int32_t* covered, int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H >= 0 && W >= 0, "mask_gate: negative size");
  DI_REQUIRE(B <= 65535, "mask_gate: batch too large");
  const long hw = (long)H * W;
  if (B == 0 || hw == 0) return 0;
  DI_REQUIRE(mask && covered, "mask_gate: NULL argument");
  const bool vec = hw % 4 == 0 && aligned_to(mask, 16);
  if (vec) hipLaunchKernelGGL(mask_gate_kernel<true>, dim3(di_div_up(hw / 4, 256), B), dim3(256), 0, ctx->stream, mask, covered, hw);
  else hipLaunchKernelGGL(mask_gate_kernel<false>, dim3(di_div_up(hw, 256), B), dim3(256), 0, ctx->stream, mask, covered, hw);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_occlusion_gate(deepim_ctx* ctx, uint8_t* image, uint16_t* depth_gt, uint8_t* label, uint16_t* depth_observed,
                                     int32_t* kept, unsigned long long* totals, const int32_t* rows, int N, const uint8_t* alone_image,
                                     const uint16_t* alone_depth, const uint8_t* alone_label, const int32_t* visible,
                                     const int32_t* full, const int32_t* slot_class, float min_visible, int B, int S, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && N >= B && H >= 0 && W >= 0, "occlusion_gate: the batch arrays need N >= B >= 0 rows");
  DI_REQUIRE(B <= 65535 && S >= 1 && S <= 8, "occlusion_gate: B <= 65535 and S in 1..8");
  DI_REQUIRE(min_visible >= 0.f && min_visible <= 1.f, "occlusion_gate: min_visible in [0, 1]");
  const long hw = (long)H * W;
  DI_REQUIRE(hw <= 0x7fffffffL, "occlusion_gate: frame too large");
  if (B == 0 || hw == 0) return 0;
  DI_REQUIRE(image && depth_gt && label && kept && alone_image && alone_depth && alone_label && visible && full,
             "occlusion_gate: NULL argument");
  DI_REQUIRE(image != alone_image && depth_gt != alone_depth && label != alone_label, "occlusion_gate: the alone frames are the batch's own arrays");
  const OcclusionGate a = {image, depth_gt, label, depth_observed, alone_image, alone_depth, alone_label, visible, full, slot_class,
                           rows, kept, totals, min_visible, N, B, S, hw};
  const bool vec = hw % 4 == 0 && aligned_to(image, 4) && aligned_to(alone_image, 4) && aligned_to(label, 4) && aligned_to(alone_label, 4) &&
                   aligned_to(depth_gt, 8) && aligned_to(alone_depth, 8) && (!depth_observed || aligned_to(depth_observed, 8));
  if (vec) hipLaunchKernelGGL(occlusion_gate_kernel<true>, dim3(di_div_up(hw / 4, 256), B), dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL(occlusion_gate_kernel<false>, dim3(di_div_up(hw, 256), B), dim3(256), 0, ctx->stream, a);
  DI_LAUNCH_CHECK();
  return 0;
}
