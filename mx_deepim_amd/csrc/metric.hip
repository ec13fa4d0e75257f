// Training metrics reduced on the device (deepim/core/metric.py:51-137 and the weight-norm line of deepim/core/module.py:1113-1122).
//   deepim_train_metrics   one call per batch: the sums of flow_loss, rot_loss, trans_loss and point_matching_loss and the mask
//                          cross-entropy, added into five device doubles (and written, per batch, into five more)
//   deepim_l2_norms_multi  the 2-norm of every row of a {pointer, count} table
// Both are streaming reductions shaped like the flow EPE (csrc/flow.hip): a lane owns four consecutive floats (one 16-byte load at
// a dword-aligned address; the last n % 4 elements are a scalar tail), elements are added in double; lane → wave (xor shuffles) →
// block (waves in order, LDS) → one partial per block; a finish kernel adds the partials in a fixed order. No atomics: the same
// inputs give the same bytes. Two launches per call whatever the sizes.
#include "common.h"

#include <algorithm>

namespace {

struct alignas(4) Floats4u { float v[4]; };      // four floats at a dword-aligned address: one 16-byte load

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// a block's four wave sums → thread 0's return value, waves in order
__device__ __forceinline__ double block_sum(double v, double* sh /*4*/) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// up to four floats of x[p0 …] (cnt = 4: one 16-byte load; fewer: the scalar tail), the rest zero
__device__ __forceinline__ void load_quad(float (&out)[4], const float* __restrict__ x, long p0, int cnt) {
  if (cnt == 4) {
    const Floats4u a = *reinterpret_cast<const Floats4u*>(x + p0);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = a.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = j < cnt ? x[p0 + j] : 0.f;
  }
}

constexpr int NSLOT = 5;                 // flow, rot, trans, pm, mask
constexpr int METRIC_MAX_ITERS = 8;      // quads per lane before a slot's grid reaches METRIC_MAX_BLOCKS
constexpr int METRIC_MAX_BLOCKS = 2048;  // per slot: 8 blocks of 256 threads on each of the 256 CUs; beyond it the lanes walk further

struct MetricSlots {
  const float* x[NSLOT];   // the tensor of the slot (mask: mask_prob), NULL = absent
  const float* gt;         // mask_gt
  long n[NSLOT];
  int first[NSLOT + 1];    // blocks [first[s], first[s + 1]) belong to slot s
  int iters[NSLOT];        // quads per lane, 256 quads apart
};

// metric.py:135 on float32 inputs, every operation in float32 as numpy evaluates it (the Makefile's -ffp-contract=off keeps the
// products and the sum apart): p == 1 gives log(1e-19f), never log(0)
__device__ __forceinline__ float mask_term(float p, float g) {
  const float a = logf(p + 1e-19f);
  const float b = logf((1.f - p) + 1e-19f);
  return -(g * a + (1.f - g) * b);
}

// grid (first[NSLOT]), 256 threads. Block `local` of a slot owns its quads [local·256·iters, (local + 1)·256·iters).
__global__ __launch_bounds__(256) void train_metrics_partial_kernel(double* __restrict__ partials, MetricSlots t) {
  __shared__ double sh[4];
  int s = 0;
  while (s < NSLOT - 1 && (int)blockIdx.x >= t.first[s + 1]) ++s;       // block-uniform
  const long local = (int)blockIdx.x - t.first[s];
  const long n = t.n[s];
  const long quads = (n + 3) >> 2;
  const int iters = t.iters[s];
  const float* __restrict__ x = t.x[s];
  const float* __restrict__ gt = t.gt;
  double acc = 0.0;
  for (int it = 0; it < iters; ++it) {
    const long q = (local * iters + it) * 256 + threadIdx.x;
    if (q >= quads) break;
    const long p0 = q * 4;
    const int cnt = n - p0 < 4 ? (int)(n - p0) : 4;
    float v[4];
    load_quad(v, x, p0, cnt);
    if (s == NSLOT - 1) {
      float g[4];
      load_quad(g, gt, p0, cnt);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) acc += (double)mask_term(v[j], g[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += (double)v[j];                  // the padding of a tail is +0
    }
  }
  const double r = block_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// one block of NSLOT waves: wave s adds the partials of slot s — lane l takes l, l + 64, … in order, then the xor tree — and its
// lane 0 writes step[s] and adds into totals[s]. An absent slot writes step[s] = 0 and leaves totals[s] alone.
__global__ __launch_bounds__(64 * NSLOT) void train_metrics_finish_kernel(double* __restrict__ totals, double* __restrict__ step,
                                                                         const double* __restrict__ partials, MetricSlots t) {
  const int s = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b0 = t.first[s], b1 = t.first[s + 1];
  double acc = 0.0;
  for (int i = b0 + lane; i < b1; i += 64) acc += partials[i];
  acc = wave_sum(acc);
  if (lane == 0) {
    const bool present = t.x[s] != nullptr;
    if (step) step[s] = present ? acc : 0.0;
    if (totals && present) totals[s] += acc;
  }
}

constexpr int NORM_BLOCKS = 256;         // blocks per row: the largest parameter (fc6, 84 MB) still fills the chip

// grid (NORM_BLOCKS, rows), 256 threads. Block x of a row owns the quads [x·per, (x + 1)·per), per = ceil(quads / NORM_BLOCKS).
__global__ __launch_bounds__(256) void l2_norms_partial_kernel(double* __restrict__ partials, const uint64_t* __restrict__ table) {
  __shared__ double sh[4];
  const int row = blockIdx.y;
  const float* __restrict__ x = reinterpret_cast<const float*>(table[2 * row]);
  const long n = (long)table[2 * row + 1];
  const long quads = (n + 3) >> 2;
  const long per = (quads + NORM_BLOCKS - 1) / NORM_BLOCKS;
  const long q1 = ((long)blockIdx.x + 1) * per < quads ? ((long)blockIdx.x + 1) * per : quads;
  double acc = 0.0;
  for (long q = (long)blockIdx.x * per + threadIdx.x; q < q1; q += 256) {
    const long p0 = q * 4;
    float v[4];
    load_quad(v, x, p0, n - p0 < 4 ? (int)(n - p0) : 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += (double)v[j] * (double)v[j];
  }
  const double r = block_sum(acc, sh);
  if (threadIdx.x == 0) partials[(size_t)row * NORM_BLOCKS + blockIdx.x] = r;
}

// grid (rows), one wave: lane l adds the partials l, l + 64, … of its row in order, then the xor tree; out = sqrtf of the rounded sum
__global__ __launch_bounds__(64) void l2_norms_finish_kernel(float* __restrict__ out, const double* __restrict__ partials) {
  const int row = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < NORM_BLOCKS; i += 64) acc += partials[(size_t)row * NORM_BLOCKS + i];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) out[row] = sqrtf((float)acc);
}

}  // namespace

extern "C" int deepim_train_metrics(deepim_ctx* ctx, double* totals, double* step, const float* flow_loss, long n_flow,
                                    const float* rot_loss, long n_rot, const float* trans_loss, long n_trans,
                                    const float* pm_loss, long n_pm, const float* mask_prob, const float* mask_gt,
                                    long n_mask) {
  DI_DEVICE(ctx);
  DI_REQUIRE(n_flow >= 0 && n_rot >= 0 && n_trans >= 0 && n_pm >= 0 && n_mask >= 0, "train_metrics: negative length");
  DI_REQUIRE(std::max({n_flow, n_rot, n_trans, n_pm, n_mask}) <= (1L << 40), "train_metrics: tensor too large");
  DI_REQUIRE((mask_prob == nullptr) == (mask_gt == nullptr), "train_metrics: mask_prob and mask_gt come together");
  if (!totals && !step) return 0;
  MetricSlots t;
  const float* xs[NSLOT] = {flow_loss, rot_loss, trans_loss, pm_loss, mask_prob};
  const long ns[NSLOT] = {n_flow, n_rot, n_trans, n_pm, n_mask};
  t.gt = mask_gt;
  t.first[0] = 0;
  for (int s = 0; s < NSLOT; ++s) {
    t.x[s] = xs[s];
    t.n[s] = xs[s] ? ns[s] : 0;
    const long quads = (t.n[s] + 3) / 4;
    const long nblk = std::min<long>(METRIC_MAX_BLOCKS, (quads + 256L * METRIC_MAX_ITERS - 1) / (256L * METRIC_MAX_ITERS));
    t.iters[s] = nblk ? (int)((quads + nblk * 256 - 1) / (nblk * 256)) : 0;
    t.first[s + 1] = t.first[s] + (int)nblk;
  }
  // scratch: one partial per block, at its largest whatever the lengths (grows on a first call only, outside a capture)
  void* scratch;
  int rc = deepim_scratch(ctx, (size_t)NSLOT * METRIC_MAX_BLOCKS * sizeof(double), &scratch);
  if (rc) return rc;
  double* partials = (double*)scratch;
  if (t.first[NSLOT] > 0)
    hipLaunchKernelGGL(train_metrics_partial_kernel, dim3(t.first[NSLOT]), dim3(256), 0, ctx->stream, partials, t);
  hipLaunchKernelGGL(train_metrics_finish_kernel, dim3(1), dim3(64 * NSLOT), 0, ctx->stream, totals, step, partials, t);
  DI_LAUNCH_CHECK();
  return 0;
}

extern "C" int deepim_l2_norms_multi(deepim_ctx* ctx, float* out, const uint64_t* table, int rows) {
  DI_DEVICE(ctx);
  DI_REQUIRE(rows >= 0 && rows <= 65535, "l2_norms_multi: bad row count");
  if (rows == 0) return 0;
  void* scratch;
  int rc = deepim_scratch(ctx, (size_t)rows * NORM_BLOCKS * sizeof(double), &scratch);
  if (rc) return rc;
  double* partials = (double*)scratch;
  hipLaunchKernelGGL(l2_norms_partial_kernel, dim3(NORM_BLOCKS, rows), dim3(256), 0, ctx->stream, partials, table);
  hipLaunchKernelGGL(l2_norms_finish_kernel, dim3(rows), dim3(64), 0, ctx->stream, out, partials);
  DI_LAUNCH_CHECK();
  return 0;
}
