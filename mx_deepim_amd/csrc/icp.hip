// Depth ICP on the device: a projective point-to-plane refiner between a rendered (source) and an observed (target) depth map —
// the device counterpart of the `*-pose_icp.txt` poses the reference's evaluation reads from files (deepim/core/tester.py:193-279).
//   deepim_depth_normals   camera-facing normals of a depth map from central differences of its vertices
//   deepim_icp_step        one Gauss-Newton step per pair: per-pixel association → 29 double sums → 6x6 Cholesky → T ← exp(ξ̂)·T
//   deepim_icp_apply       [R_T·R | R_T·t + t_T]
// All arithmetic is double from the float32 inputs (the Makefile's -ffp-contract=off keeps products and sums apart, so that
// tests/depth_icp_emulation.py can restate every decision operation for operation). The step is a streaming reduction shaped
// like the flow EPE (csrc/flow.hip) and the training metrics (csrc/metric.hip): a lane owns four consecutive source pixels (one
// 16-byte load), a block of 256 lanes owns ICP_BLOCK_PIX consecutive pixels of one pair whatever the batch, lane → wave (xor
// shuffles) → block (waves in order, LDS) → one 30-double partial per block; the finish adds a pair's partials in a fixed order
// and solves. No atomics: the same inputs give the same bytes. Two launches per step, one per normal pass, one per apply.
#include "common.h"

namespace {

constexpr int ICP_TERMS = 29;          // 21 upper entries of ΣJJᵀ, 6 of −ΣJr, the pair count, Σr²
constexpr int ICP_SLOTS = 30;          // one spare: a partial is 240 bytes
constexpr int ICP_BLOCK_PIX = 1024;    // 256 lanes x 4 pixels; fixed, so a pair's block partition depends on H·W alone
constexpr int ICP_FIN_PARTS = 32;      // the finish adds a pair's partials in 32 interleaved chains, then the chains in order

struct alignas(4) Floats4u { float v[4]; };      // four floats at a dword-aligned address: one 16-byte load

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// depth · K⁻¹ · (x, y, 1)
__device__ __forceinline__ void vertex(double (&o)[3], const double* kinv, double x, double y, double d) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = ((kinv[3 * r] * x + kinv[3 * r + 1] * y) + kinv[3 * r + 2]) * d;
}

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void cross3(double (&o)[3], const double (&a)[3], const double (&b)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// grid (ceil(H·W / 256), B), 256 threads: one pixel per lane, five depth reads (four of them neighbours' lines in cache), three stores
template <class Cam>
__global__ __launch_bounds__(256) void depth_normals_kernel(float* __restrict__ normals, const float* __restrict__ depth, Cam cam,
                                                            double max_step, int H, int W) {
  __shared__ double kinv[9];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    const Mat3 K = cam.at(b);
    inv3d(K.v, kinv);
  }
  __syncthreads();
  const long plane = (long)H * W;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= plane) return;
  const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
  const float* __restrict__ d = depth + (long)b * plane;
  float n[3] = {0.f, 0.f, 0.f};
  if (x > 0 && x < W - 1 && y > 0 && y < H - 1) {
    const double dc = d[idx], dl = d[idx - 1], dr = d[idx + 1], du = d[idx - W], dd = d[idx + W];
    const bool pos = dc > 0.0 && dl > 0.0 && dr > 0.0 && du > 0.0 && dd > 0.0;
    const bool jump = fabs(dl - dc) > max_step || fabs(dr - dc) > max_step || fabs(du - dc) > max_step || fabs(dd - dc) > max_step;
    if (pos && !jump) {
      double vc[3], vl[3], vr[3], vu[3], vd[3], ex[3], ey[3], c[3];
      vertex(vc, kinv, (double)x, (double)y, dc);
      vertex(vl, kinv, (double)(x - 1), (double)y, dl);
      vertex(vr, kinv, (double)(x + 1), (double)y, dr);
      vertex(vu, kinv, (double)x, (double)(y - 1), du);
      vertex(vd, kinv, (double)x, (double)(y + 1), dd);
#pragma unroll
      for (int i = 0; i < 3; ++i) { ex[i] = vr[i] - vl[i]; ey[i] = vd[i] - vu[i]; }
      cross3(c, ex, ey);
      const double n2 = dot3(c, c);
      if (n2 > 0.0) {
        const double len = sqrt(n2);
        double nn[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) nn[i] = c[i] / len;
        const bool flip = dot3(nn, vc) > 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) n[i] = (float)(flip ? -nn[i] : nn[i]);
      }
    }
  }
  float* __restrict__ o = normals + (long)b * 3 * plane + idx;
  o[0] = n[0];
  o[plane] = n[1];
  o[2 * plane] = n[2];
}

// grid (ceil(H·W / ICP_BLOCK_PIX), B), 256 threads. Block x of pair b owns the source pixels [x·1024, (x + 1)·1024) of the plane
// and writes partials[(b·gridDim.x + x)·30 …]. A block without a source depth writes zeros at once; a wave none of whose pixels
// was accepted skips its shuffles (its sums are zeros).
template <class Cam>
__global__ __launch_bounds__(256) void icp_pixel_kernel(double* __restrict__ partials, const float* __restrict__ T,
                                                        const float* __restrict__ depth_src, const float* __restrict__ depth_tgt,
                                                        const float* __restrict__ normals, Cam cam, double dist_max2, int H, int W) {
  __shared__ double Kd[9], kinv[9], Td[12];
  __shared__ double sh[4][ICP_SLOTS];
  const int b = blockIdx.y;
  const long plane = (long)H * W;
  const long p0 = (long)blockIdx.x * ICP_BLOCK_PIX + (long)threadIdx.x * 4;
  const int cnt = p0 >= plane ? 0 : (plane - p0 < 4 ? (int)(plane - p0) : 4);
  const float* __restrict__ src = depth_src + (long)b * plane;
  const float* __restrict__ tgt = depth_tgt + (long)b * plane;
  const float* __restrict__ nrm = normals + (long)b * 3 * plane;
  float ds4[4] = {0.f, 0.f, 0.f, 0.f};
  if (cnt == 4) {
    const Floats4u a = *reinterpret_cast<const Floats4u*>(src + p0);
#pragma unroll
    for (int j = 0; j < 4; ++j) ds4[j] = a.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) ds4[j] = j < cnt ? src[p0 + j] : 0.f;      // the padding of a tail is "no measurement"
  }
  // a block of background (most of a frame) writes its zeros and leaves before the camera is inverted: the same sums, bit for bit
  if (!__syncthreads_or(ds4[0] > 0.f || ds4[1] > 0.f || ds4[2] > 0.f || ds4[3] > 0.f)) {
    if (threadIdx.x < ICP_SLOTS) partials[((long)b * gridDim.x + blockIdx.x) * ICP_SLOTS + threadIdx.x] = 0.0;
    return;
  }
  if (threadIdx.x == 0) {
    const Mat3 K = cam.at(b);
#pragma unroll
    for (int i = 0; i < 9; ++i) Kd[i] = (double)K.v[i];
    inv3d(K.v, kinv);
  }
  if (threadIdx.x >= 64 && threadIdx.x < 76) Td[threadIdx.x - 64] = (double)T[(long)b * 12 + threadIdx.x - 64];
  __syncthreads();
  double acc[ICP_TERMS];
#pragma unroll
  for (int k = 0; k < ICP_TERMS; ++k) acc[k] = 0.0;
  const double wmax = (double)(W - 1), hmax = (double)(H - 1);
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    const double ds = (double)(j == 0 ? ds4[0] : j == 1 ? ds4[1] : j == 2 ? ds4[2] : ds4[3]);     // no indexed register file
    if (!(ds > 0.0)) continue;
    const long idx = p0 + j;
    const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
    double p[3], pp[3];
    vertex(p, kinv, (double)x, (double)y, ds);
#pragma unroll
    for (int i = 0; i < 3; ++i) pp[i] = ((Td[4 * i] * p[0] + Td[4 * i + 1] * p[1]) + Td[4 * i + 2] * p[2]) + Td[4 * i + 3];
    if (!(pp[2] > 0.0)) continue;
    const double uz = (Kd[6] * pp[0] + Kd[7] * pp[1]) + Kd[8] * pp[2];
    const double px = rint(((Kd[0] * pp[0] + Kd[1] * pp[1]) + Kd[2] * pp[2]) / uz);
    const double py = rint(((Kd[3] * pp[0] + Kd[4] * pp[1]) + Kd[5] * pp[2]) / uz);
    if (!(px >= 0.0 && px <= wmax && py >= 0.0 && py <= hmax)) continue;       // NaN fails too: no address depends on bad data
    const long it = (long)(int)py * W + (int)px;
    const double dt = (double)tgt[it];
    double n[3] = {(double)nrm[it], (double)nrm[plane + it], (double)nrm[2 * plane + it]};
    if (!(dt > 0.0) || (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0)) continue;
    double q[3], e[3], J[6];
    vertex(q, kinv, px, py, dt);
#pragma unroll
    for (int i = 0; i < 3; ++i) e[i] = pp[i] - q[i];
    if (dot3(e, e) > dist_max2) continue;
    const double r = dot3(n, e);
    double cr[3];
    cross3(cr, pp, n);
#pragma unroll
    for (int i = 0; i < 3; ++i) { J[i] = cr[i]; J[3 + i] = n[i]; }
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int jj = i; jj < 6; ++jj) acc[k++] += J[i] * J[jj];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += -(J[i] * r);
    acc[27] += 1.0;
    acc[28] += r * r;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (__any(acc[27] > 0.0)) {           // wave-uniform
#pragma unroll
    for (int k = 0; k < ICP_TERMS; ++k) acc[k] = wave_sum(acc[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < ICP_TERMS; ++k) sh[wave][k] = acc[k];
    sh[wave][ICP_TERMS] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < ICP_SLOTS)
    partials[((long)b * gridDim.x + blockIdx.x) * ICP_SLOTS + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// entry (i, j), i <= j, of the packed upper triangle
__device__ __forceinline__ int upper(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

// grid (B), 1024 threads: chain c (32 lanes, one per slot) adds the partials c, c + 32, … of the pair in order (a 480x640 pair has
// 300: short chains, their loads in flight together); lane s < 30 adds the 32 chains in order → sys; thread 0 factors and solves
// (a 6x6 system: nothing to share out) and updates T.
__global__ __launch_bounds__(32 * ICP_FIN_PARTS) void icp_finish_kernel(float* __restrict__ T, double* __restrict__ sys, int32_t* __restrict__ status,
                                                         const double* __restrict__ partials, const int32_t* __restrict__ skip,
                                                         int nblk, int min_pairs, double rcond) {
  __shared__ double part[ICP_FIN_PARTS][32];
  __shared__ double s[32];
  __shared__ double L[36];
  const int b = blockIdx.x, c = threadIdx.x >> 5, slot = threadIdx.x & 31;
  double acc = 0.0;
  if (slot < ICP_SLOTS)
#pragma unroll 4
    for (int i = c; i < nblk; i += ICP_FIN_PARTS) acc += partials[((long)b * nblk + i) * ICP_SLOTS + slot];
  part[c][slot] = acc;
  __syncthreads();
  if (threadIdx.x < ICP_SLOTS) {
    double v = part[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < ICP_FIN_PARTS; ++q) v += part[q][threadIdx.x];
    s[threadIdx.x] = v;
    if (sys) sys[(long)b * ICP_SLOTS + threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;

  int st = 0;
  if (s[27] < (double)min_pairs) {
    st = 1;
  } else {
    double maxdiag = s[upper(0, 0)];
    for (int i = 1; i < 6; ++i) maxdiag = fmax(maxdiag, s[upper(i, i)]);
    const double lim = rcond * maxdiag;
    for (int j = 0; j < 6 && st == 0; ++j) {
      double v = s[upper(j, j)];
      for (int k = 0; k < j; ++k) v = v - L[j * 6 + k] * L[j * 6 + k];
      if (!(v > lim)) { st = 2; break; }
      const double piv = sqrt(v);
      L[j * 6 + j] = piv;
      for (int i = j + 1; i < 6; ++i) {
        v = s[upper(j, i)];
        for (int k = 0; k < j; ++k) v = v - L[i * 6 + k] * L[j * 6 + k];
        L[i * 6 + j] = v / piv;
      }
    }
  }
  status[b] = st;
  if (st != 0 || (skip != nullptr && skip[b] != 0)) return;

  double* yv = part[0];             // the chains are spent: 12 doubles of them hold the two triangular solves
  double* xi = part[1];
  for (int i = 0; i < 6; ++i) {
    double v = s[21 + i];
    for (int k = 0; k < i; ++k) v = v - L[i * 6 + k] * yv[k];
    yv[i] = v / L[i * 6 + i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = yv[i];
    for (int k = i + 1; k < 6; ++k) v = v - L[k * 6 + i] * xi[k];
    xi[i] = v / L[i * 6 + i];
  }
  // exp of the twist (ω, v): Rodrigues and its V matrix; the series below θ² = 1e-8
  const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
  const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
  double ca, cb, cc;
  if (th2 < 1e-8) {
    ca = 1.0 - th2 / 6.0;
    cb = 0.5 - th2 / 24.0;
    cc = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double th = sqrt(th2), sh_ = sin(0.5 * th), sn = sin(th);
    ca = sn / th;
    cb = 2.0 * sh_ * sh_ / th2;
    cc = (th - sn) / (th2 * th);
  }
  const double Wm[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
  const double W2[9] = {-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2, w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2,
                        w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)};
  double Re[9], V[9], te[3], Td[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) Td[i] = (double)T[(long)b * 12 + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double eye = i % 4 == 0 ? 1.0 : 0.0;
    Re[i] = (eye + ca * Wm[i]) + cb * W2[i];
    V[i] = (eye + cb * Wm[i]) + cc * W2[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) te[i] = (V[3 * i] * xi[3] + V[3 * i + 1] * xi[4]) + V[3 * i + 2] * xi[5];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      T[(long)b * 12 + 4 * i + j] = (float)((Re[3 * i] * Td[j] + Re[3 * i + 1] * Td[4 + j]) + Re[3 * i + 2] * Td[8 + j]);
    T[(long)b * 12 + 4 * i + 3] = (float)(((Re[3 * i] * Td[3] + Re[3 * i + 1] * Td[7]) + Re[3 * i + 2] * Td[11]) + te[i]);
  }
}

__global__ __launch_bounds__(64) void icp_apply_kernel(float* pose_out, const float* __restrict__ T, const float* pose_in,
                                                       int B) {   // pose_out may be pose_in: all of a pose is read first
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double Td[12], P[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { Td[i] = (double)T[(long)b * 12 + i]; P[i] = (double)pose_in[(long)b * 12 + i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      pose_out[(long)b * 12 + 4 * i + j] = (float)((Td[4 * i] * P[j] + Td[4 * i + 1] * P[4 + j]) + Td[4 * i + 2] * P[8 + j]);
    pose_out[(long)b * 12 + 4 * i + 3] =
        (float)(((Td[4 * i] * P[3] + Td[4 * i + 1] * P[7]) + Td[4 * i + 2] * P[11]) + Td[4 * i + 3]);
  }
}

}  // namespace

extern "C" int deepim_depth_normals(deepim_ctx* ctx, float* normals, const float* depth, const float* K_host, float max_step,
                                    int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H > 0 && W > 0, "depth_normals: bad shape");
  DI_REQUIRE(B <= 65535, "depth_normals: batch too large");
  DI_REQUIRE((long)H * W <= (1L << 30), "depth_normals: frame too large");
  if (B == 0) return 0;
  DI_CAMERA(ctx, K_host, B, "deepim_depth_normals");
  const dim3 grid(di_div_up((long)H * W, 256), B);
  if (K_host)
    hipLaunchKernelGGL(depth_normals_kernel<CamOne>, grid, dim3(256), 0, ctx->stream, normals, depth, cam_one(K_host),
                       (double)max_step, H, W);
  else
    hipLaunchKernelGGL(depth_normals_kernel<CamTable>, grid, dim3(256), 0, ctx->stream, normals, depth, CamTable{ctx->cam_table},
                       (double)max_step, H, W);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_icp_step(deepim_ctx* ctx, float* T, double* sys, int32_t* status, const float* depth_src,
                               const float* depth_tgt, const float* normals_tgt, const float* K_host, const int32_t* skip,
                               float dist_max, int min_pairs, double rcond, int B, int H, int W) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0 && H > 0 && W > 0, "icp_step: bad shape");
  DI_REQUIRE(B <= 65535, "icp_step: batch too large");
  DI_REQUIRE((long)H * W <= (1L << 30), "icp_step: frame too large");
  DI_REQUIRE(dist_max >= 0.f && rcond >= 0.0, "icp_step: dist_max and rcond must not be negative");
  if (B == 0) return 0;
  DI_CAMERA(ctx, K_host, B, "deepim_icp_step");
  const int nblk = di_div_up((long)H * W, ICP_BLOCK_PIX);
  // scratch: one partial per block (grows on a first call only, outside a capture)
  void* scratch;
  int rc = deepim_scratch(ctx, (size_t)B * nblk * ICP_SLOTS * sizeof(double), &scratch);
  if (rc) return rc;
  double* partials = (double*)scratch;
  const double dist_max2 = (double)dist_max * (double)dist_max;
  if (K_host)
    hipLaunchKernelGGL(icp_pixel_kernel<CamOne>, dim3(nblk, B), dim3(256), 0, ctx->stream, partials, T, depth_src, depth_tgt,
                       normals_tgt, cam_one(K_host), dist_max2, H, W);
  else
    hipLaunchKernelGGL(icp_pixel_kernel<CamTable>, dim3(nblk, B), dim3(256), 0, ctx->stream, partials, T, depth_src, depth_tgt,
                       normals_tgt, CamTable{ctx->cam_table}, dist_max2, H, W);
  hipLaunchKernelGGL(icp_finish_kernel, dim3(B), dim3(32 * ICP_FIN_PARTS), 0, ctx->stream, T, sys, status, partials, skip, nblk, min_pairs, rcond);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_icp_apply(deepim_ctx* ctx, float* pose_out, const float* T, const float* pose_in, int B) {
  DI_DEVICE(ctx);
  DI_REQUIRE(B >= 0, "icp_apply: bad batch");
  if (B == 0) return 0;
  hipLaunchKernelGGL(icp_apply_kernel, dim3(di_div_up(B, 64)), dim3(64), 0, ctx->stream, pose_out, T, pose_in, B);
  DI_LAUNCH_CHECK();
  return 0;
}
