// Shared internals of libdeepim_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <map>
#include <mutex>
#include <type_traits>
#include <algorithm>
#include "../../include/deepim_hip.h"
#include "wino_plan.h"

constexpr int DI_MAX_BOX_SAMPLES = 4096;
// bits of the sticky status word (deepim_zoom_status)
constexpr int DI_STATUS_ZOOM_EMPTY = 1;       // observed mask/image empty in a zoom-factor computation (zoom_mask.py:55 raises)
constexpr int DI_STATUS_GROUP_RANGE = 2;      // GroupPicker index out of range
constexpr int DI_STATUS_X3_SATURATED = 8;     // split-fp16 conv: a value left fp16's range after scaling and was clamped (results invalid)
constexpr int DI_STATUS_MASK_BOX_EMPTY = 4;   // mask_box / fused re-render: empty mask (data_pair.py:98 np.min raises)
constexpr int DI_STATUS_FRAME_RANGE = 16;     // shared-frame entries: a device-resident frame_index outside [0, N) (that pair sees an empty frame)
constexpr int DI_STATUS_BG_RANGE = 32;        // deepim_ingest_bgr8_pool: a device-resident bg_index outside [0, P) (that pair gets a black background)

// deepim_set_option(ctx, "f16_dev_flags", 0 or DI_F16_NO_PP): the 4-wave kernel of csrc/conv_f16.hip is the ping-pong kernel's
// bit-exact reference in the tests
constexpr int DI_F16_NO_PP = 16;   // no ping-pong kernel (round 4): every LDS-DMA layer on the 4-wave kernel, as in round 3
#ifndef DI_PP_MIN_TILES
#define DI_PP_MIN_TILES 64
#endif
constexpr int DI_F16_PP_MIN_TILES = DI_PP_MIN_TILES;   // ping-pong kernel from 64 tiles of 256x256 (128x512) on (measured, profiles/r04_fp16_pingpong.md): with fewer the 4-wave kernel on 256x128 tiles, two blocks per CU

struct ConvTab { int mode, Cin, kh, kw, H, W; void* tab; };  // im2col tap table of one conv geometry

struct ConvPlanKey { int mode, B, Cin, H, W, Cout, Ho, Wo, stride, pad, nchunk, below, target; };
struct ConvPlan { ConvPlanKey key; int ksplit; };  // autotuned split-K factor of one conv geometry

struct deepim_ctx {
  int device;
  hipStream_t stream;
  // small device scratch shared by the ops (bbox words, zoom factors, split-K partials)
  void* scratch;
  size_t scratch_bytes;
  std::vector<void*> retired_scratch;  // outgrown scratch buffers still referenced by captured graphs
  int* status;  // persistent device status word, bits DI_STATUS_*
  void* comm;        // ncclComm_t of this rank (csrc/comm.hip), NULL in a single-GPU process
  int comm_rank, comm_world;
  int* box_words;   // DI_MAX_BOX_SAMPLES x {xmin,xmax,ymin,ymax}: bbox accumulators of mask_box, armed inside every call
  int* zoom_box;    // DI_MAX_BOX_SAMPLES x 2 maps x {xmin,xmax,ymin,ymax}: bbox accumulators of the zoom-factor computation; armed at
                    // creation and RE-ARMED BY THEIR CONSUMER (zoom_factor_kernel resets what it read), so a call needs no init launch
  unsigned long long* zbuf;   // rasteriser z-buffer (key = depth bits << 32 | triangle): all-ones between calls — the resolve pass
  size_t zbuf_bytes;          // puts every entry back after reading it, so a draw needs no clearing pass (grow-only, cleared on growth)
  // host-side guards of the two self-re-arming buffers: set before the PRODUCER launches (raster / bbox), cleared once the CONSUMER
  // (resolve / zoom_factor) has been launched without error. Found set on entry — an aborted sequence, a launch error in between —
  // the buffer is re-initialised before it is used again instead of handing stale depth keys / boxes to the next call.
  int zbuf_dirty, zoom_box_dirty;
  // pinned host staging for small per-call attribute uploads (K, means, ...)
  std::vector<hipEvent_t> timer_start, timer_stop;
  hipEvent_t sync_event;   // deepim_stream_wait: "everything queued on this stream so far" (created on first use)
  std::vector<hipGraphExec_t> graphs;
  bool capturing;
  std::vector<ConvTab> conv_tabs;
  std::vector<ConvPlan> conv_plans;
  int conv_direct;    // LDS-free register-fed kernel for 128x128-tiled convs: 0 off, 1 (default) unless conv_max_split == 1, 2 always
  int conv_tail_split;  // 1: let the autotuner consider tail splits (default 0, see launch_conv)
  int conv_force_plan;  // dev: 0 = off, n > 0 = uniform split-K n, n < 0 = tail split with -n slices
  int conv_tail_slots;  // resident 128x128 blocks of the LDS-free kernel on the whole chip (256 CUs x 4): round size for the tail split
  int conv_autotune;  // 1: time split-K candidates on the first call of a geometry (default 0: deterministic cost-model plan)
  int conv_max_split;  // 0 auto, 1 off, n cap
  int conv_xcd_swizzle;  // 1: XCD-aware tile order (default), 0: plain
  int dgrad_group;       // 1 (default): the four parity classes of a stride-2 data gradient share one launch; 0: class by class
  WinoOptions wino;      // the "wino_*" options of the fp32 Winograd kernels (csrc/wino_plan.h: fields and defaults)
  int wgrad_lds;         // 1 (default): LDS-staged weight-gradient kernel; 0: the round-2 register-fed kernel (A/B measurements)
  int conv_fewout_blocks, conv_fewout_minc;   // few-filter heads: channel slices so that the grid has about this many blocks (0 = default: 1024 where the pixels alone give >= 32 blocks, else 512), of at least this many channels each (32)
  int conv_fewout_quad;  // 1 (default): the 3x3 stride-1 heads with W % 4 == 0 on the four-pixels-per-lane kernel; 0: one pixel per lane
  std::map<uintptr_t, size_t> allocs;   // deepim_malloc's live allocations (base -> bytes): deepim_d2d's residency test without a driver query
  std::mutex allocs_mu;  // guards `allocs`: a DeviceArray finalizer on another Python thread may free while the main thread copies (ctypes drops the GIL)
  void* wino_counters;   // arrival counters of the Winograd kernels' in-kernel finish, one per tile block (deepim_create; zero between launches)
  int f16_dev_flags;     // 0 (default) or DI_F16_NO_PP: fp16 layers stay off the ping-pong kernel
  std::vector<const void*> attr_done;  // hipFuncSetAttribute groups already applied on THIS context's device (di_attr_needed)
  const float* cam_table;   // deepim_bind_cameras: device (cam_n,3,3) intrinsics read by the entries called with K_host == NULL
  int cam_n;                // (the caller's memory: only the pointer is kept, so a captured graph sees the table's later contents)
  // The closed loop's two zoom boxes, handed from the render pass to the front end through a caller-owned (B,2,4) int32 array.
  // Both are one-shot requests: taken and cleared by the next render entry / the next zoom-factor computation, also when it fails.
  int* export_boxes;        // deepim_render_export_boxes: the next draw with mask_box also writes the boxes of its two masks here
  const int* seed_boxes;    // deepim_zoom_seed_boxes: the next zoom-factor computation reads its boxes here and runs no bbox pass
  unsigned long long bbox_launches;   // bbox_kernel launches this context has queued (deepim_bbox_launches)
  int render_quad;          // 1 (default): resolve and box fill own four pixels per lane where the plane allows; 0: one pixel per lane
};

// true the first time `tag` is seen on this context: guards one-off hipFuncSetAttribute calls (per device, hence per context)
static inline bool di_attr_needed(deepim_ctx* ctx, const void* tag) {
  for (const void* t : ctx->attr_done) if (t == tag) return false;
  ctx->attr_done.push_back(tag);
  return true;
}

void deepim_set_error(const char* where, hipError_t e);
void deepim_set_error_msg(const char* msg);

#define DI_CHECK(expr)                                   \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) {                              \
      deepim_set_error(#expr, _e);                       \
      return (int)_e;                                    \
    }                                                    \
  } while (0)

// Every extern "C" entry that takes a context starts with this: allocations, events and launches follow the CURRENT
// device, not the stream's, and the reference drives several GPUs from one process (gpu_flow_wrapper(device_id),
// one executor per context) — so each call makes its context's device current first.
#define DI_DEVICE(ctx)                                   \
  do {                                                   \
    hipError_t _e = hipSetDevice((ctx)->device);         \
    if (_e != hipSuccess) {                              \
      deepim_set_error("hipSetDevice", _e);              \
      return (int)_e;                                    \
    }                                                    \
  } while (0)

#define DI_LAUNCH_CHECK()                                \
  do {                                                   \
    hipError_t _e = hipGetLastError();                   \
    if (_e != hipSuccess) {                              \
      deepim_set_error("kernel launch", _e);             \
      return (int)_e;                                    \
    }                                                    \
  } while (0)

#define DI_REQUIRE(cond, msg)                            \
  do {                                                   \
    if (!(cond)) {                                       \
      deepim_set_error_msg(msg);                         \
      return -1;                                         \
    }                                                    \
  } while (0)

// fill pass of the box_rendered rectangle from accumulated bbox words (csrc/flow.hip); export_boxes: NULL, or (B,2,4) int32 that
// receives, per sample, the zoom front end's observed box (that of the rectangle drawn) and rendered box (the words)
int deepim_mask_box_fill(deepim_ctx* ctx, float* box, const int* words, int* export_boxes, int B, int H, int W);

void deepim_ctx_default_options(deepim_ctx* c);
// Grow-only scratch; never reallocated while a graph capture is open.
int deepim_scratch(deepim_ctx* ctx, size_t bytes, void** out);

static inline int di_div_up(long a, long b) { return (int)((a + b - 1) / b); }

// small by-value attribute blocks passed as kernel arguments (live in SGPRs)
struct Mat3 { float v[9]; };
struct Vec3 { float v[3]; };

// Where a kernel's camera comes from (the K_host rule of include/deepim_hip.h): one matrix by value for the whole launch, or
// row b of the table bound with deepim_bind_cameras. Kernels that read K are templated on it; both sources hand the same
// operations the same values, so a sample computed from table row b has the bits of a call with K_host = that row.
struct CamOne {
  Mat3 K;
  __device__ __forceinline__ const Mat3& at(int) const { return K; }
};
struct CamTable {
  const float* rows;
  __device__ __forceinline__ Mat3 at(int b) const {
    Mat3 m;
#pragma unroll
    for (int i = 0; i < 9; ++i) m.v[i] = rows[(long)b * 9 + i];
    return m;
  }
};
static inline CamOne cam_one(const float* K_host) {
  CamOne c;
  for (int i = 0; i < 9; ++i) c.K.v[i] = K_host[i];
  return c;
}

// 3x3 inverse in double (adjugate) — for intrinsics this matches numpy's LU result to f64 ulps. Host and device run the same
// IEEE double operations in the same order (no contraction), so both give the same bits.
__host__ __device__ inline void inv3d(const float* K, double* o) {
  double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
  double A = e * i - f * h, Bc = -(d * i - f * g), C = d * h - e * g;
  double det = a * A + b * Bc + c * C;
  o[0] = A / det; o[1] = -(b * i - c * h) / det; o[2] = (b * f - c * e) / det;
  o[3] = Bc / det; o[4] = (a * i - c * g) / det; o[5] = -(a * f - c * d) / det;
  o[6] = C / det; o[7] = -(a * h - b * g) / det; o[8] = (a * e - b * d) / det;
}
// np.linalg.inv(np.matrix(K)) of a float32 K: the double inverse rounded to float32
__host__ __device__ inline Mat3 inv3_f32(const float* K) {
  double kinv[9];
  inv3d(K, kinv);
  Mat3 m;
  for (int i = 0; i < 9; ++i) m.v[i] = (float)kinv[i];
  return m;
}
// The inverse intrinsics of the flow kernels: computed once on the host, or by each block from its pair's table row
struct KinvOne {
  Mat3 Kinv;
  __device__ __forceinline__ const Mat3& at(int) const { return Kinv; }
};
struct KinvTable {
  const float* rows;
  __device__ __forceinline__ Mat3 at(int b) const { return inv3_f32(rows + (long)b * 9); }
};

// The K_host rule on the host, before any launch: K_host, else the bound table with at least B rows, else an error naming `entry`
int deepim_camera_check(deepim_ctx* ctx, const float* K_host, int B, const char* entry);
#define DI_CAMERA(ctx, K_host, B, entry)                                   \
  do {                                                                     \
    if (deepim_camera_check((ctx), (K_host), (B), (entry)) != 0) return -1; \
  } while (0)
