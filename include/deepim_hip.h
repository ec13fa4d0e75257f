/*
 * deepim_hip.h — C ABI of libdeepim_hip.so, the MI355X (gfx950) implementation of
 * mx-DeepIM's render-and-compare inner loop.
 *
 * Boundary rules
 *   - plain C linkage, plain pointers and sizes, no torch / MXNet types;
 *   - every `deepim_*` entry returns 0 on success, non-zero on failure
 *     (`deepim_last_error()` gives the HIP error text); nothing prints-and-continues
 *     the way the reference's CUDA wrapper does (lib/flow_c/gpu_flow_kernel.cu:18-25);
 *   - "d_" / unprefixed tensor pointers are DEVICE pointers obtained from
 *     deepim_malloc(); tensors are dense NCHW float32 unless stated;
 *   - all work is enqueued on the context's HIP stream and is asynchronous;
 *     deepim_sync() / the d2h copy are the synchronisation points.
 *
 * Each entry cites the reference interface it replaces (path:line under the
 * reference checkout).
 */
#ifndef DEEPIM_HIP_H_
#define DEEPIM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct deepim_ctx deepim_ctx;

/* ---------------------------------------------------------------- runtime -- */
/* replaces `mx.gpu(i)` contexts + MXNet NDArray storage (deepim/core/tester.py:27-47) */
int deepim_create(int device_id, deepim_ctx** out);
int deepim_destroy(deepim_ctx* ctx);
const char* deepim_last_error(void);
int deepim_device_count(int* n);
int deepim_malloc(deepim_ctx* ctx, size_t bytes, void** dptr);
int deepim_free(deepim_ctx* ctx, void* dptr);
int deepim_memset(deepim_ctx* ctx, void* dptr, int value, size_t bytes);
int deepim_h2d(deepim_ctx* ctx, void* dst, const void* src, size_t bytes);   /* sync */
int deepim_d2h(deepim_ctx* ctx, void* dst, const void* src, size_t bytes);   /* sync */
int deepim_d2d(deepim_ctx* ctx, void* dst, const void* src, size_t bytes);   /* async */
int deepim_sync(deepim_ctx* ctx);
/* y[i] += alpha * x[i] — CustomOp.assign(dst, 'add', src) (mx.operator.CustomOp.assign) */
int deepim_axpy(deepim_ctx* ctx, float* y, const float* x, float alpha, size_t n);
/* strided channel-slice copy: dst[b, dst_coff:dst_coff+C, :] = src[b, :, :] (MXNet Concat, async) */
int deepim_copy_channels(deepim_ctx* ctx, float* dst, int dst_ctotal, int dst_coff,
                         const float* src, int C, int B, size_t hw);
void* deepim_stream(deepim_ctx* ctx);           /* hipStream_t, for interop */
/* integer tuning knobs. "conv_max_split": 0 = auto split-K (default), 1 = never split AND canonical order
 * (conv/deconv results are then a single (ci,ky,kx)-ordered fmaf chain, bit-identical to the oracle; with NC8 input —
 * deepim_conv2d_forward_ex — still a single chain, in that kernel's own (c/8,ky,kx,s,h) order), n = cap.
 * "conv_direct": 1 (default) = 128x128-tiled convs with even Cin run on the LDS-free register-fed kernel, whose
 * fmaf chain runs over (ci/2,ky,kx,ci%2) (differs from the canonical order in the last bits; the oracle has the
 * matching order switch); it steps aside when conv_max_split == 1; 2 = use it even then; 0 = never.
 * "conv_tail_split": 1 = the autotuner may cut only the tiles of the under-filled last round of a launch into K
 * slices (default 0: a pair's summation order would depend on its position in the batch); "conv_tail_slots": round
 * size in 128x128 blocks (default 1024 = 256 CUs x 4); "conv_force_plan": dev knob, n > 0 uniform split-K,
 * n < 0 tail split with -n slices, 0 = heuristic/autotuner.
 * "conv_xcd_swizzle": 1 (default) = XCD-aware tile order, 0 = plain block order.
 * "conv_autotune": 0 (default) = the split-K factor of an under-filled conv grid comes from a deterministic cost
 * model (same geometry → same summation order in every run, process and rank); 1 = on the first call of a conv
 * geometry, time a few split-K factors and keep the fastest (plans then depend on timing noise). "wgrad_lds": 1 (default) = LDS-staged weight-gradient kernel
 * (and the few-filter stream kernel for Cout <= 4), 0 = the round-2 register-fed kernel; "dgrad_group": 1 (default) = the four
 * parity classes of deepim_conv2d_dgrad_s2 share one launch, 0 = class by class (A/B measurements). "wino_two_wave": 0 (default) =
 * the Winograd layers on the one-wave-per-SIMD kernel (16 positions per wave), 1 = the two-wave form (8 positions per wave, LDS
 * hand-over; measured slower on the big layers); "wino_s2d_skip": 1 (default) = deepim_conv2d_wino_forward_s2d skips the positions
 * whose transformed weights are identically zero, 0 = runs all 16 (A/B measurements). "wino_shared": 1 (default) = Winograd layers with
 * Cout % 64 == 0 run on the shared-transform kernel (8- or 4-wave blocks, the input transform computed once per block and handed over
 * through LDS), 0 = the round-4 one-wave kernel. "wino_wide": block shape of that kernel — 1 (default) = per layer by the work per CU,
 * 0 = 64 channels x 64 tiles, 3 = 128 x 32 (Cout % 128 == 0), 2 = 64 x 32 on four waves, two blocks per CU, 4 = 256 x 32 on nine
 * accumulator tuples per wave where that shape exists (deepim_conv2d_wino_forward_s2d3 with "wino_s2d_skip" on, Cin % 16 == 0 and
 * Cout % 256 == 0: the same bits as 3 for the same K slicing), anywhere else as 3. "wino_split": its split
 * over the input channels where the grid does not fill the chip — 0 (default) = the deterministic plan of the geometry, 1 = never
 * (one block walks all of Cin: the 3x3 layers are then bit-identical to the one-wave kernel), n = at most n slices. "wino_persistent": 1
 * (default) = its grid is one block per resident slot (256 of 8 waves, 512 of 4), each walking its share of the tile blocks, 0 = one
 * block per tile block (same results). "wino_streamk": 1 (default) = where that walk would end in a partly filled round the persistent
 * blocks share that round granule by granule, a cut tile block is finished by whichever of its pieces arrives last (a fixed order of adds:
 * deterministic; rounding as for a K split; like "conv_tail_split" it makes the last bits of a pair's result depend on the pair's place in
 * the batch — which tile blocks are cut does —, never its 1e-5-of-range bound; on by default since it is worth +1 % of the loop where the
 * direct kernels' tail split was not; off with wino_split = 1 or wino_persistent = 0; 2 = wherever it applies, whatever the cost model
 * says; 0 = never: permuting the pairs of a batch then permutes the results bit for bit). "wino_fin": 1 = a layer split over
 * the input channels is finished inside the kernel — the block whose slice of a tile block arrives last adds the raw copies in slice order,
 * the bias and the activation: the second pass's sums bit for bit, without its launch —, 0 (default) = wino_reduce_kernel as a second pass
 * (measured on MI355X, profiles/r06_b4_share.md: the lone finishing block's read-back is a serial tail that costs more than the parallel
 * pass it replaces — conv6_1 at B = 4: 48 -> 129 us). The arrival counters of both in-kernel finishes (64 KB) are allocated by
 * deepim_create: a layer's plan depends on geometry and options only, under graph capture as in eager runs. "conv_fewout_quad": 1 (default) = the 3x3
 * stride-1 pad-1 convolutions with Cout <= 4 and W % 4 == 0 (flow / mask predictors) compute four pixels per lane, 0 = one;
 * "conv_fewout_blocks": the grid those few-filter convolutions slice their input channels for — 0 (default) = ~1024 blocks where the pixels
 * alone give >= 32 blocks, ~512 below (measured, profiles/r06_heads.md), n = about n blocks; "conv_fewout_minc": the smallest channel slice
 * (default 32). "f16_dev_flags": 0 (default), or 16 = the fp16 convolutions never take the ping-pong kernel, all LDS-DMA layers run on
 * the 4-wave kernel (same products in the same order: the tests' bit-exact reference); other values fail. Unknown names fail. */
int deepim_set_option(deepim_ctx* ctx, const char* name, int value);
/* *value = the current setting of an option deepim_set_option knows (host code that has to follow the context's kernel selection —
 * e.g. which weight-gradient layout the training graph registers — reads it here). Unknown names fail. */
int deepim_get_option(deepim_ctx* ctx, const char* name, int* value);
/* Device-side ordering between two contexts (two streams) of ONE GPU: work queued on `waiter` after this call starts only after
 * everything queued on `ctx` before it has finished; the host does not block. Lets independent kernels of one graph (the weight
 * and the data gradient of a layer) share the chip: each context has its own stream and scratch. */
int deepim_stream_wait(deepim_ctx* waiter, deepim_ctx* ctx);
/* HIP-event stopwatch on the context stream (bench.py's per-kernel timing) */
int deepim_timer_create(deepim_ctx* ctx, int* timer_id);
int deepim_timer_start(deepim_ctx* ctx, int timer_id);
int deepim_timer_stop(deepim_ctx* ctx, int timer_id);
int deepim_timer_elapsed_ms(deepim_ctx* ctx, int timer_id, float* ms);  /* syncs on stop event */
/* hipGraph capture of a launch sequence on the context stream */
int deepim_graph_begin(deepim_ctx* ctx);
int deepim_graph_end(deepim_ctx* ctx, int* graph_id);
int deepim_graph_launch(deepim_ctx* ctx, int graph_id);

/* Per-pair cameras. K_table: device (n,3,3) float32 row-major intrinsics, or NULL to unbind. The context stores (pointer, n) and
 * nothing else: no copy, no launch, no derived table, no allocation — the memory stays the caller's and must outlive its use. The
 * kernels read the rows when they run, so a captured graph of an iteration replays for any later batch's cameras, as it does for
 * any batch's class ids.
 * THE K_host RULE. In every entry whose K_host is marked "or NULL: camera table" — the zoom front ends, the five draws,
 * deepim_pose_error, deepim_calc_KT, deepim_flow_epe, deepim_pair_flow_labels, the two depth-ICP passes — K_host == NULL means "sample b of this call reads
 * row b of the bound table". With K_host != NULL the entry does what it always did, whatever is bound. NULL with nothing bound, or
 * with n < B, fails on the host before any launch with a message naming the entry. A call on the slice [b0, b1) of a batch binds
 * K_table + 9*b0 with n = b1 - b0 first. A sample computed from row b has the bits of the same call with K_host = that row (the
 * inverse intrinsics of the flow entries included: the device inverts in double as the host does). A row is data, not an index:
 * a non-finite or singular one gives its sample the NaN zoom factor or empty draw of a bad pose, and no address depends on it.
 * Every other entry that takes a K (deepim_flow_updater_forward, deepim_pose_perturb, the pose samplers) requires it: NULL is an
 * error code, not a table read. */
int deepim_bind_cameras(deepim_ctx* ctx, const float* K_table /*device (n,3,3) row-major, or NULL = unbind*/, int n);

/* ------------------------------------------------ multi-GPU: pose all-gather over RCCL/xGMI -- */
/* pairs shard across GPUs with no data-path collective except ONE all-gather of the refined poses per
 * refinement iteration, so that every rank/host holds all poses for the next render/update — the role of the per-device
 * executor group's merged outputs in the reference (deepim/core/DataParallelExecutorGroup.py:364-388, deepim/test.py:135).
 * One process per GPU; librccl.so is dlopen'ed on first use; no PyTorch. Bootstrap: rank 0 makes the id, ships the bytes
 * out of band (mx_deepim_amd/parallel.py does it over a TCP rendezvous), every rank calls deepim_comm_init. */
#define DEEPIM_COMM_ID_BYTES 128
int deepim_comm_unique_id(void* id_bytes /* DEEPIM_COMM_ID_BYTES, host */);
int deepim_comm_init(deepim_ctx* ctx, int rank, int world, const void* id_bytes);
int deepim_comm_destroy(deepim_ctx* ctx);
/* all_poses (world*B,3,4) device <- poses (B,3,4) device of every rank, rank-major; one asynchronous enqueue on the
 * context stream (a plain copy when no communicator is set) */
int deepim_allgather_poses(deepim_ctx* ctx, float* all_poses, const float* poses, int B);
/* in-place all-reduce of n device doubles on the context stream: op 0 = max, 1 = sum (bench.py's max-over-ranks time) */
int deepim_comm_allreduce_f64(deepim_ctx* ctx, double* buf, int n, int op);
/* What this process bound, as text: "backend=rccl|none;rccl_ranks=N;rccl_version=V;librccl_path=…;libamdhip64_path=…" — the
 * rank count is ncclCommCount of the context's communicator (0 without one), the paths are the files the ncclAllGather / hipMalloc
 * symbols in use live in (dladdr). Reporting only (bench.py's `comm` block); no reference counterpart. */
int deepim_comm_info(deepim_ctx* ctx, char* buf, int n);

/* ------------------------------------------------ F-group: depth warp / flow -- */
/* B2 drop-in. Same symbol, argument list and host-pointer contract as
 * lib/flow_c/gpu_flow.hpp:1-3 (`_flow`, defined gpu_flow_kernel.cu:82-148):
 * all pointers are HOST float32, caller-owned, synchronous. Unlike the
 * reference it aborts via deepim_last_error + stderr + nonzero `deepim_flow_status()`
 * when HIP fails. */
void _flow(float* flow, float* valid, float* depth_src, float* depth_tgt,
           float* KT, float* Kinv, int batch_size, int height, int width,
           int device_id);
/* The one body behind `_flow`.  gpu_flow.hpp:1-3 has C++ linkage (no extern "C") and the reference's Cython
 * extension is built language="c++" (gpu_flow.pyx:13-16, setup_linux.py:116-125), so it links the mangled
 * _Z5_flowPfS_S_S_S_S_iiii: the library exports that symbol too (csrc/flow_cxx.cpp; not declarable in this C header),
 * forwarding here like the C-linkage `_flow` above. */
void deepim_flow_host(float* flow, float* valid, float* depth_src, float* depth_tgt,
                      float* KT, float* Kinv, int batch_size, int height, int width,
                      int device_id);
int deepim_flow_status(void);
/* device-pointer variant of the same kernel (gpu_flow_kernel.cu:32-69) */
int deepim_flow_forward(deepim_ctx* ctx, float* flow, float* valid,
                        const float* depth_src, const float* depth_tgt,
                        const float* KT /*B,3,4 device*/, const float* Kinv_host /*3,3 HOST*/,
                        int B, int H, int W);
/* lib/pair_matching/flow.py:12-63 `calc_flow` semantics (un-rounded bounds test
 * is on rounded coords, valid needs depth_src != 0 and |d_tgt| > 1e-10);
 * KT = K·se3 (B,3,4), Kinv (3,3); flow channel order [dh,dw] unless standard_rep */
int deepim_calc_flow_forward(deepim_ctx* ctx, float* flow /*B,H,W,2*/, float* visible /*B,H,W*/,
                             const float* depth_src, const float* depth_tgt,
                             const float* KT, const float* Kinv_host, float thresh,
                             int standard_rep, int B, int H, int W);
/* Loader-side flow labels (lib/utils/image.py:402-450 get_pair_flow, called from get_data_pair_train_batch,
 * lib/pair_matching/data_pair.py:170-176): calc_flow(depth_rendered, pose_rendered, pose_observed, K, depth_observed)
 * per pair, laid out (B,2,H,W) as the loader hands it to the network, with flow_weights by TRAIN.FLOW_WEIGHT_TYPE:
 * weight_type 0 'all', 1 'viz', 2 'valid', tiled over the two channels. Poses (B,3,4) device, K host. */
int deepim_pair_flow_labels(deepim_ctx* ctx, float* flow /*B,2,H,W*/, float* flow_weights /*B,2,H,W*/,
                            const float* depth_rendered, const float* depth_observed, const float* pose_rendered,
                            const float* pose_observed, const float* K_host /*or NULL: camera table*/, float thresh, int standard_rep,
                            int weight_type, int B, int H, int W);
/* Flow EPE of the test loop, fused (deepim/core/tester.py:366-378: par_generate_gt :530-569 + calc_EPE_one_pair :572-589):
 * per pixel of pair b the float64 ground truth of calc_flow(depth_rendered, pose_rendered, pose_observed, K, depth_observed,
 * thresh, standard_rep) — un-rounded pw − w, ph − h, zero where not visible — against flow_est rounded to fp16 (nearest even,
 * |x| > 65504 → ±inf, as tester.py:350-352's astype) and widened to double; point_diff = sqrt(dx² + dy²); channel 0 of the
 * prediction meets channel 0 of the ground truth under both standard_rep settings. No flow tensor is written.
 * out[b] = { epe_all, num_all, epe_viz, num_viz, epe_vizbg, num_vizbg } (:581-588), vizbg = visible or (not visible and
 * depth_rendered == 0); the counts are integer counts stored as doubles. totals (6 doubles, caller-owned, or NULL) receives
 * totals[k] += out[b][k] for b = 0 … B-1 in that order, so a loop reads it once at its end. skip: device int32 (B) the host
 * never reads, or NULL: a pair with skip[b] != 0 contributes nothing and its row is zeros. Partials are combined in a fixed
 * order without atomics: the same inputs give the same bytes. Asynchronous on the context's stream; scratch grows on a first
 * call only, outside a capture; legal inside deepim_graph_begin/end (K_host, thresh and standard_rep are baked in). */
int deepim_flow_epe(deepim_ctx* ctx, double* out /*B,6*/, double* totals /*6, accumulated; or NULL*/,
                    const float* flow_est /*B,2,H,W*/, const float* depth_rendered, const float* depth_observed,
                    const float* pose_rendered, const float* pose_observed /*B,3,4*/, const float* K_host /*or NULL: camera table*/,
                    const int32_t* skip /*device (B) or NULL*/, float thresh, int standard_rep, int B, int H, int W);
/* image.py:381-387: mask_rendered = depth_rendered with values > thresh set to 1 (others kept) */
int deepim_depth_clip_mask(deepim_ctx* ctx, float* mask, const float* depth, float thresh, size_t n);
/* deepim/operator_py/flow_updater.py:42-102 `FlowUpdater` forward: integer flow
 * from rounded+clamped coords; pose_src/pose_tgt (B,3,4); K, Kinv host 3x3 */
int deepim_flow_updater_forward(deepim_ctx* ctx, float* flow /*B,2,H,W*/, float* flow_weights /*B,2,H,W*/,
                                const float* depth_src, const float* depth_tgt,
                                const float* pose_src, const float* pose_tgt,
                                const float* K_host /*required*/, float thresh, int wh_rep,
                                int B, int H, int W);
/* batch_updater_py_multi.py:255-265: KT = K·(pose_tgt ∘ pose_src⁻¹) and
 * mask_rendered = depth_rendered > 0.2 */
int deepim_calc_KT(deepim_ctx* ctx, float* KT /*B,3,4*/, const float* pose_src,
                   const float* pose_tgt, const float* K_host /*or NULL: camera table*/, int B);
int deepim_depth_to_mask(deepim_ctx* ctx, float* mask, const float* depth, float thresh, size_t n);
/* "box_rendered" / "box_observed" rectangle of a mask (lib/pair_matching/data_pair.py:94-116, the INIT_MASK twin at
 * lib/utils/image.py:355-374): 1 inside [y_start:y_end, x_start:x_end] with start/end = first/last row and column holding a
 * non-zero — numpy slices, so the last row and column stay 0. An empty mask gives zeros and sets bit 2 (value 4) of the status word
 * (deepim_zoom_status) where the reference raises. mask, box: (B,1,H,W) device. */
int deepim_mask_box_forward(deepim_ctx* ctx, float* box, const float* mask, int B, int H, int W);

/* --------------------------------------------------- Z-group: zoom / warp -- */
/* zoom_mask.py:29-112 `ZoomMaskOperator.forward`.
 * K_host: 3x3 float32 (host). Outputs are rounded resampled masks + zoom_factor (B,4). */
int deepim_zoom_mask_forward(deepim_ctx* ctx,
                             const float* mask_observed, const float* mask_gt_observed,
                             const float* mask_rendered, const float* src_pose /*B,3,4*/,
                             const float* K_host /*or NULL: camera table*/,
                             float* zoom_mask_observed, float* zoom_mask_gt_observed,
                             float* zoom_mask_rendered, float* zoom_factor /*B,4*/,
                             int B, int H, int W);
/* zoom_image.py:26-107 `ZoomImageOperator.forward` (no-mask variant). pixel_means_host: 3 floats
 * in the channel order of the image tensor. */
int deepim_zoom_image_forward(deepim_ctx* ctx,
                              const float* image_observed, const float* image_rendered,
                              const float* src_pose, const float* K_host /*or NULL: camera table*/,
                              const float* pixel_means_host,
                              float* zoom_image_observed, float* zoom_image_rendered,
                              float* zoom_factor, int B, int H, int W);
/* zoom_image_with_factor.py:31-65 */
int deepim_zoom_image_with_factor_forward(deepim_ctx* ctx, const float* zoom_factor,
                                          const float* image_observed, const float* image_rendered,
                                          const float* pixel_means_host, int high_light_center,
                                          float* zoom_image_observed, float* zoom_image_rendered,
                                          int B, int H, int W);
/* zoom_depth.py:24-44 */
int deepim_zoom_depth_forward(deepim_ctx* ctx, const float* zoom_factor,
                              const float* depth_observed, const float* depth_rendered,
                              float* zoom_depth_observed, float* zoom_depth_rendered,
                              int B, int H, int W);
/* zoom_flow.py:28-71; flow_weights/zoom_flow_weights may be NULL when b_inv_zoom */
int deepim_zoom_flow_forward(deepim_ctx* ctx, const float* zoom_factor, const float* flow,
                             const float* flow_weights, float* zoom_flow, float* zoom_flow_weights,
                             int b_inv_zoom, int B, int H, int W);
/* zoom_mask_with_factor.py:29-64 */
int deepim_zoom_mask_with_factor_forward(deepim_ctx* ctx, const float* zoom_factor, const float* mask,
                                         float* zoom_mask, int b_inv_zoom, int B, int H, int W);
/* zoom_trans.py:22-46 forward, :48-74 backward */
int deepim_zoom_trans_forward(deepim_ctx* ctx, const float* zoom_factor, const float* trans_delta,
                              float* zoom_trans_delta, int b_inv_zoom, int B);
int deepim_zoom_trans_backward(deepim_ctx* ctx, const float* zoom_factor, const float* out_grad,
                               float* in_grad, int b_inv_zoom, int b_zoom_grad, int B);
/* The fused zoom front end: six entries over ONE channel list (csrc/zoom.hip zoom_concat4_body) and ONE launcher
 * (launch_front_end), which differ along two independent axes only:
 *   observed source  per-pair fp32 tensors (image_observed, depth_observed)   | N shared decoded frames + frame_index (_frames_)
 *   output form      (B,C,H,W) fp32 planes | (B,H,W,8) fp32 NC8 records (_nc8, per-pair tensors only) | fp16 records (_h16)
 * Channels, in order, each with the same operations in every entry: observed and rendered image (un-mean, /255), observed
 * and rendered depth (/255, when given), observed mask (round) and rendered mask (>0.2, round) (when given). Every form
 * carries the bits of the planes form; W % 4 != 0 or a misaligned output is served by the planes form from per-pair tensors
 * only (generic resampler), the other entries refuse it.
 *
 * Fused front end of the test graph (deepIM_flownet.py:33-62 + :563-622): ZoomMask +
 * ZoomImageWithFactor [+ ZoomDepth] + `/255` + Concat written straight into the
 * conv1 input (B,C,H,W), C = 8 (+2 with depth). Also returns zoom_factor. depth_* may be NULL.
 * With both masks NULL (INPUT_MASK=False, deepIM_flownet.py:594-605) the factor comes from ZoomImage's
 * non-black-pixel boxes and C = 6 (+2 with depth). */
int deepim_zoom_concat_forward(deepim_ctx* ctx,
                               const float* image_observed, const float* image_rendered,
                               const float* mask_observed, const float* mask_rendered,
                               const float* depth_observed, const float* depth_rendered,
                               const float* src_pose, const float* K_host /*or NULL: camera table*/,
                               const float* pixel_means_host,
                               float* net_input, float* zoom_factor,
                               int B, int H, int W);
/* the same front end for the shipped 8-channel input (masks, no depth) writing channel-blocked records: net_input_nc8 is
 * (B,H,W,8) = the "NC8" layout [n][C/8][h][w][8] with C = 8, which deepim_conv2d_forward_ex(in_nc8 = 1) reads for conv1;
 * element values identical to deepim_zoom_concat_forward's (B,8,H,W) */
int deepim_zoom_concat_forward_nc8(deepim_ctx* ctx, const float* image_observed, const float* image_rendered,
                                   const float* mask_observed, const float* mask_rendered, const float* src_pose,
                                   const float* K_host /*or NULL: camera table*/, const float* pixel_means_host, float* net_input_nc8,
                                   float* zoom_factor, int B, int H, int W);
/* the front end of the fp16 conv path (config 5): the same values rounded once to fp16 and written as the pixel records
 * deepim_conv1_f16_h16_forward reads — main8 (B,H,W,8 halves) = net-input channels 0-7; with depth_* set (INPUT_DEPTH, C = 10)
 * extra2 (B,H,W,2 halves) = channels 8-9 (the masks). depth_observed, depth_rendered and extra2 are all NULL or all set. */
int deepim_zoom_concat_forward_h16(deepim_ctx* ctx, const float* image_observed, const float* image_rendered,
                                   const float* mask_observed, const float* mask_rendered, const float* depth_observed,
                                   const float* depth_rendered, const float* src_pose, const float* K_host /*or NULL: camera table*/,
                                   const float* pixel_means_host, void* main8, void* extra2, float* zoom_factor, int B,
                                   int H, int W);
/* deepim_zoom_concat_forward for a batch whose pairs look at SHARED camera frames (several objects in one frame): the observed
 * channels are gathered from N decoded frames that stay as the decoder left them, so no fp32 copy of an observed image or
 * depth map exists. frame_index: device int32 (B), the frame pair b looks at; the host never reads it, so a captured graph
 * follows what it holds at replay.
 *   frames_bgr8     (N,H,W,3) uint8, BGR interleaved, any byte alignment. Tensor channel c of pair b is byte 2-c of frame
 *                   frame_index[b]; a tap is float(byte) - pixel_means_host[c], the fp32 subtraction of deepim_ingest_bgr8
 *   depth_frames16  (N,H,W) uint16, 2-byte aligned, or NULL. A tap is float(d) / depth_factor, correctly rounded as in
 *                   deepim_ingest_depth16. depth_frames16 and depth_rendered are both NULL (C = 8) or both set (C = 10)
 *   depth_labels    (N,H,W) uint8 and mask_idx device int32 (B), both or neither, only with depth_frames16: the depth tap is 0
 *                   where depth_labels[frame][pixel] != mask_idx[b] (network.MASK_INPUTS)
 * image_rendered, mask_observed, mask_rendered and depth_rendered are per pair, (B,·,H,W) fp32, as in deepim_zoom_concat_forward.
 * net_input and zoom_factor come out with the bits deepim_zoom_concat_forward gives when it is fed deepim_ingest_bgr8 /
 * deepim_ingest_depth16 of frames[frame_index]. Needs W % 4 == 0, a 16-byte aligned net_input and N >= 1. Both masks are
 * required: the mask-less ZoomImage box search reads fp32 images and is refused.
 * Since the host never sees the ids a bad one cannot be reported: a pair whose frame_index is outside [0, N) reads no memory
 * outside the frames, its observed image and depth come out as if every tap fell outside the frame (image = (0 - mean) / 255,
 * depth = 0), and bit 4 (16) of the status word (deepim_zoom_status) is set. The other pairs are unaffected. */
int deepim_zoom_concat_frames_forward(deepim_ctx* ctx, const uint8_t* frames_bgr8 /*N,H,W,3*/,
                                      const int32_t* frame_index /*device (B)*/, int N, const float* image_rendered,
                                      const float* mask_observed, const float* mask_rendered,
                                      const uint16_t* depth_frames16 /*N,H,W or NULL*/,
                                      const uint8_t* depth_labels /*N,H,W or NULL*/,
                                      const int32_t* mask_idx /*device (B) or NULL*/, float depth_factor,
                                      const float* depth_rendered /*or NULL*/, const float* src_pose, const float* K_host /*or NULL: camera table*/,
                                      const float* pixel_means_host, float* net_input, float* zoom_factor, int B, int H,
                                      int W);
/* the shared-frame front end of the fp16 conv path: the observed channels as in deepim_zoom_concat_frames_forward, the outputs
 * as in deepim_zoom_concat_forward_h16 (main8, extra2: 16-byte aligned; extra2 is set exactly when depth_frames16 is). Same
 * bad-index rule and status bit. */
int deepim_zoom_concat_frames_forward_h16(deepim_ctx* ctx, const uint8_t* frames_bgr8 /*N,H,W,3*/,
                                          const int32_t* frame_index /*device (B)*/, int N, const float* image_rendered,
                                          const float* mask_observed, const float* mask_rendered,
                                          const uint16_t* depth_frames16 /*N,H,W or NULL*/,
                                          const uint8_t* depth_labels /*N,H,W or NULL*/,
                                          const int32_t* mask_idx /*device (B) or NULL*/, float depth_factor,
                                          const float* depth_rendered /*or NULL*/, const float* src_pose,
                                          const float* K_host /*or NULL: camera table*/, const float* pixel_means_host, void* main8, void* extra2,
                                          float* zoom_factor, int B, int H, int W);
/* the same front end in the TRAINING graph (deepIM_flownet.py:392-412): the zoom region comes from mask_gt_observed
 * (B,1,H,W; NULL = mask_observed, i.e. the test graph) */
int deepim_zoom_concat_train_forward(deepim_ctx* ctx, const float* image_observed, const float* image_rendered,
                                     const float* mask_observed, const float* mask_gt_observed, const float* mask_rendered,
                                     const float* depth_observed, const float* depth_rendered, const float* src_pose,
                                     const float* K_host /*or NULL: camera table*/, const float* pixel_means_host, float* net_input,
                                     float* zoom_factor, int B, int H, int W);
/* parity hook: runs all 2^32 float bit patterns through the kernel's 5-op replacement of `v / 255.0f`
 * (deepIM_flownet.py:35-36 divides the zoomed images by 255) against the IEEE division on the device and returns the
 * number of patterns whose results differ in any bit (NaN results compare equal). Must be 0. */
int deepim_selfcheck_div255(deepim_ctx* ctx, unsigned long long* mismatches_host);
/* debug/parity hook: the int32 source indices (x0,y0 = floor of the sampling
 * position) the resampler uses for every output pixel: idx (B,2,H,W) int32 */
int deepim_zoom_indices(deepim_ctx* ctx, const float* zoom_factor, int32_t* idx, int B, int H, int W);
/* debug/parity hook: the affine (wx,wy,tx,ty) the b_inv_zoom ops sample with, i.e. zoom_flow.py:36-44 /
 * zoom_mask_with_factor.py:43-52 applied to a stored factor (NumPy-1.x promotion: float64 chain, rounded once).
 * zoom_factor, inv_factor: (B,4) device */
int deepim_zoom_inverse_factor(deepim_ctx* ctx, const float* zoom_factor, float* inv_factor, int B, int H, int W);
/* sticky status word since the last read (reading clears it):
 * bit0 (1) = a zoom-factor computation saw an observed mask/image with no valid pixel — the reference raises ValueError
 *            there (np.min of an empty array, zoom_mask.py:55); the zoom factor is NaN for that sample
 * bit1 (2) = GroupPicker index out of range
 * bit2 (4) = deepim_mask_box_forward / deepim_render_update_forward saw an empty mask (data_pair.py:98 raises)
 * bit3 (8) = split-fp16 conv path: a value left fp16's range after scaling (|v·scale| > 60000 or NaN) and was clamped — the
 *            results of that call are not fp32-grade; lower the activation scale or use the fp32 path
 * bit4 (16) = a shared-frame entry (deepim_zoom_concat_frames_forward[_h16], deepim_ingest_*_frames) met a frame_index outside
 *            [0, N): that pair's observed channels / output plane are those of an empty frame; or deepim_gather_rows met an
 *            index outside [0, n_rows): that row is zeros
 * bit5 (32) = deepim_ingest_bgr8_pool met a bg_index outside [0, P) in a pair that composites a background: that pair's
 *            background is black */
int deepim_zoom_status(deepim_ctx* ctx, int* status);

/* The closed loop's shortcut from the render pass to the zoom front end. Between two refinement iterations the render pass
 * already knows the boxes the front end's bbox pass would search both full-frame masks for: the box of mask_rendered is the one
 * it reduces for the box_rendered rectangle, and the box of that rectangle (mask_box, the next mask_observed) follows from it.
 * Both calls are ONE-SHOT requests kept on the context; neither launches anything, synchronises or allocates, and both are
 * legal inside a graph capture (the kernels they steer are captured with the array's address).
 *   boxes   caller-owned device int32 (B,2,4), {minx, maxx, miny, maxy}: row 0 the box of the rectangle (values > 0.3 of
 *           mask_box), row 1 the box of mask_rendered (values > 0.2); an empty map has {INT_MAX, -1, INT_MAX, -1}. The
 *           rectangle is half-open, so row 0 is {xs, xe-1, ys, ye-1} of row 1's {xs, xe, ys, ye}, and empty where the rendered
 *           box is one pixel wide or high, or empty itself.
 * deepim_render_export_boxes: the NEXT render entry on the context — which must draw mask_box (deepim_render_update_forward,
 *   deepim_render_lit_forward, deepim_render_classes_forward; any other entry refuses) — writes `boxes` from its box-fill pass.
 * deepim_zoom_seed_boxes: the NEXT deepim_zoom_concat_* call on the context, in any of its forms and given both masks, reads the
 *   two boxes from `boxes` and launches no bbox pass; zoom_factor, the network input and the status bits are those of the
 *   bbox pass on the masks the boxes were exported for. The array is read, not re-armed; the context's own accumulators stay
 *   as the next unseeded call expects them. deepim_zoom_mask_forward / deepim_zoom_image_forward and the training front end's
 *   mask_gt_observed refuse a seed.
 * Either request is cleared by the call that takes it, also when that call fails; boxes == NULL withdraws it.
 * deepim_bbox_launches: the number of bbox passes the context has queued since it was created (a seeded call adds none). */
int deepim_render_export_boxes(deepim_ctx* ctx, int32_t* boxes /*device (B,2,4)*/);
int deepim_zoom_seed_boxes(deepim_ctx* ctx, const int32_t* boxes /*device (B,2,4)*/);
int deepim_bbox_launches(deepim_ctx* ctx, unsigned long long* count);

/* ------------------------------------------ N-group: matching network ops -- */
/* MXNet Convolution (+bias) [+LeakyReLU slope] (deepIM_flownet.py:63-107,123,145,176,317).
 * `packed_w` comes from deepim_conv_pack_weights (one-time re-layout of the
 * (Cout,Cin,kh,kw) tensor into MFMA tile order; size from deepim_conv_packed_size).
 * slope == 1.0f means "no activation". out may have more channels than Cout
 * (out_ctotal, written at channel offset out_coff) so Concat is free. */
size_t deepim_conv_packed_size(int Cout, int Cin, int kh, int kw);
int deepim_conv_pack_weights(deepim_ctx* ctx, float* packed_w, const float* w /*Cout,Cin,kh,kw dev*/,
                             int Cout, int Cin, int kh, int kw);
/* the same with a choice of operand orders: bits 1 = LDS-kernel order, 2 = NCHW register-fed order, 4 = NC8 order. A caller
 * that runs NCHW activations only (the training graph and its data gradients) passes 3 and saves a third of the re-pack
 * after every SGD step; a left-out order must not be used by the forward call (NC8 input needs bit 4). */
int deepim_conv_pack_weights_ex(deepim_ctx* ctx, float* packed_w, const float* w, int Cout, int Cin, int kh, int kw, int orders);
/* packed weights of a DATA GRADIENT straight from the layer's raw tensor w_layer (Co_l,Ci_l,kh_l,kw_l): the packed convolution has
 * Cout = Ci_l, Cin = Co_l, an nky x nkx kernel with tap (a,b) = layer tap (ky0 + st·(nky-1-a), kx0 + st·(nkx-1-b)). st = 1 with
 * the whole kernel = transposed + flipped weights (replaces deepim_conv_flip_weights + pack); st = 2 = one output parity class of
 * a stride-2 layer (replaces deepim_conv_subkernel_flip + pack). orders: bits 1 | 2. */
int deepim_conv_pack_dgrad(deepim_ctx* ctx, float* packed_w, const float* w_layer, int Co_l, int Ci_l, int kh_l, int kw_l, int ky0,
                           int kx0, int st, int nky, int nkx, int orders);
/* the one order (1 or 2) deepim_conv2d_forward will read for this geometry under the context's current options */
int deepim_conv_weight_order(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad);
int deepim_conv2d_forward(deepim_ctx* ctx, float* out, const float* in, const float* packed_w,
                          const float* bias, int B, int Cin, int H, int W, int Cout,
                          int kh, int kw, int stride, int pad, float slope,
                          int out_ctotal, int out_coff);
/* Same convolution with channel-blocked ("NC8") activations between layers: a tensor (B,C,H,W) stored as
 * [n][C/8][h][w][8] (C % 8 == 0). in_nc8 / out_nc8 select the layout of `in` / `out` (0 = NCHW). NC8 input runs on the
 * LDS-free kernel whose fmaf chain per output runs over (c/8, ky, kx, s, h) with channel 8(c/8) + s + 4h — one 16-byte
 * load per lane feeds four MFMA k-steps; it needs Cout > 64. The encoder uses NCHW -> NC8 for conv1, NC8 -> NC8 up to
 * conv6, NC8 -> NCHW for conv6_1 (fc6 wants MXNet's flatten order). deepim_relayout_nc8 converts a tensor either way. */
int deepim_conv2d_forward_ex(deepim_ctx* ctx, float* out, const float* in, const float* packed_w,
                             const float* bias, int B, int Cin, int H, int W, int Cout, int kh, int kw,
                             int stride, int pad, float slope, int out_ctotal, int out_coff, int in_nc8, int out_nc8);
int deepim_relayout_nc8(deepim_ctx* ctx, float* dst, const float* src, int B, int C, size_t hw, int to_nc8);
/* The same conversion (NC8 -> NCHW) written into channels [dst_coff, dst_coff + C) of a dst_ctotal-channel NCHW tensor: the encoder
 * skip connections of the refinement decoder (Concat, deepim/symbols/deepIM_flownet.py:128-131, :143-146) in one pass. */
int deepim_relayout_nc8_slice(deepim_ctx* ctx, float* dst, int dst_ctotal, int dst_coff, const float* src_nc8, int B, int C, size_t hw);
/* the same from an NC8 tensor in space-to-depth order ((B, C, H, W), even H and W; see deepim_relayout_nc8_s2d) */
int deepim_relayout_nc8_s2d_slice(deepim_ctx* ctx, float* dst, int dst_ctotal, int dst_coff, const float* src_s2d, int B, int C, int H, int W);
/* The encoder's 3x3 stride-1 pad-1 layers (conv3_1 / conv4_1 / conv5_1 / conv6_1, deepIM_flownet.py:69-101) as fp32 Winograd
 * F(2x2,3x3): the same fp32 arithmetic with 2.25x fewer multiplies, a different summation (NOT the direct kernels' fmaf chain:
 * within 1e-5 of the layer's range, tests/test_gpu_wino.py). `in` is NC8; `out` NC8 (out_nc8 = 1) or channels [out_coff,
 * out_coff + Cout) of an NCHW tensor with out_ctotal channels (0 = Cout). Cout % 32 == 0, Cin % 8 == 0. packed_w: U = G g G^T
 * from deepim_conv_wino_pack_weights (16 floats per weight tap set: Cout*Cin*64 bytes). */
size_t deepim_conv_wino_packed_size(int Cout, int Cin);
/* 1 when the layer should take the Winograd path: Cout % 64 == 0 (shared-transform kernel, splits the input channels on small grids)
 * from 64 tiles on; other channel counts (one-wave kernel, no split) from 128 blocks of 32 channels x 128 tiles on; always 0 on a
 * context in the canonical-summation-order configuration ("conv_max_split" = 1). ctx may be NULL (the defaults). Which layers
 * qualify — and the split plan — depend on B: so does the rounding of a sample's output, never its 1e-5-of-range bound. */
int deepim_conv_wino_preferred(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout);
/* the same for a 5x5 stride-2 pad-2 layer (B, Cin, H, W) run over its space-to-depth form (one-wave kernel: from 256 blocks on) */
int deepim_conv_wino_preferred_s2d(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout);
/* The launch plan the shared-transform kernel would use for a layer under the context's options (no launch; tests and docs read it):
 * arguments as deepim_conv2d_wino_forward sees them (s2d != 0: Cin, H, W of the space-to-depth problem; 1 = a 5x5 stride-2 layer, 2 = a
 * 3x3 stride-2 one, 3 = that one through deepim_conv2d_wino_forward_s2d3_wide). The nine ints are fields of the planner's WinoPlan
 * (csrc/wino_plan.h, documented there): plan[0] = shape, counted from the first shared-transform shape (0 = 64 channels x 64 tiles,
 * 1 = 128 x 32, 2 = 64 x 32 on four waves, 3 = 256 x 32 on nine accumulator tuples), [1] = grid (blocks launched), [2] = S (K slices),
 * [3] = ks (K steps per slice), [4] = sk_G (stream-K granules per tile block, 0 = off: whole tile blocks per block), [5] = sk_q (granules
 * of the last round per persistent block), [6] = sk_F (whole tile blocks per persistent block before them), [7] = grid0 (tile blocks of
 * the layer, incl. the padding of the XCD deal), [8] = sk_rem (the first so many blocks of an XCD take one granule more). All -1 (and
 * return 0) where another kernel runs the layer, and for an empty batch. Host arithmetic only: ctx = NULL asks for the plan under the
 * default options (no device needed). */
int deepim_conv_wino_plan(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout, int out_nc8, int s2d, int* plan /*9, host*/);
int deepim_conv_wino_pack_weights(deepim_ctx* ctx, float* packed_w, const float* w /*Cout,Cin,3,3 dev*/, int Cout, int Cin);
/* The 5x5 stride-2 pad-2 layers (conv2 / conv3, deepIM_flownet.py:65-68) on the same kernel: a stride-2 convolution is a stride-1
 * convolution over the four input phases (x[2m + py][2l + px] as channel (py*2+px)*Cin + c of a (4 Cin, H/2, W/2) tensor) with the
 * taps w[2a+py][2b+px] — a 3x3 kernel, zero where the index reaches 5. The producer writes that "space-to-depth" NC8 tensor itself
 * (out_nc8 = 3 of deepim_conv2d_forward_ex / deepim_conv2d_wino_forward; deepim_relayout_nc8_s2d converts for tests), this packs
 * the layer's own (Cout, Cin, 5, 5) weights for it (size: deepim_conv_wino_packed_size(Cout, 4*Cin)), and the layer runs as
 * deepim_conv2d_wino_forward(ctx, out, in_s2d, packed, bias, B, 4*Cin, H/2, W/2, Cout, ...). 1.56x fewer multiplies than direct. */
int deepim_conv_wino_pack_weights_s2d(deepim_ctx* ctx, float* packed_w, const float* w /*Cout,Cin,5,5 dev*/, int Cout, int Cin);
/* the stride-2 layer in one call: (B, Cin, H, W) input given in its space-to-depth NC8 form, output (B, Cout, H/2, W/2); the positions
 * whose transformed weights are identically zero (third kernel row / column of the odd input phases) are skipped: 49 of 64 MFMAs.
 * The shared-transform kernel (Cout % 64 == 0, 4 Cin % 64 == 0) walks the four input phases interleaved — two 8-channel blocks of each
 * per loop body — so that the skipped positions are a compile-time property of every step: the same products, the channel sum in
 * that order (2e-6 of range from the one-wave kernel's natural order). */
int deepim_conv2d_wino_forward_s2d(deepim_ctx* ctx, float* out, const float* in_s2d, const float* packed_w, const float* bias,
                                   int B, int Cin, int H, int W, int Cout, float slope, int out_nc8, int out_ctotal, int out_coff);
/* The 3x3 stride-2 pad-1 layers (conv4 / conv5) over the same space-to-depth input: the 3x3 kernel is taps 1..3 of a 5x5 stride-2
 * pad-2 one, so phase (py, px) carries tap (a, b) = w[2a+py-1][2b+px-1] (zero where an index leaves 0..2). An even phase keeps only
 * the middle tap along that axis (live positions 1, 2), an odd one taps 0 and 2 (positions 0, 1, 2); position 3 is dead everywhere:
 * 25 of the 64 (phase, position) GEMMs remain, 1.44x fewer multiplies than the direct sum, dropped at compile time by the
 * shared-transform kernel's phase walk. _pack_weights_s2d3 takes the layer's own (Cout, Cin, 3, 3) weights (size
 * deepim_conv_wino_packed_size(Cout, 4*Cin)); _forward_s2d3 the (B, Cin, H, W) input's space-to-depth NC8 form (even H and W), output
 * (B, Cout, H/2, W/2). _preferred_s2d3 is 0 under "conv_max_split" = 1, without the shared-transform kernel (Cout % 64, Cin % 16,
 * "wino_shared" / "wino_two_wave"), for odd H or W, and below the measured batch threshold. deepim_conv_wino_plan takes s2d = 2.
 * _forward_s2d3_wide is the same layer on blocks of 256 channels x 32 tiles with nine accumulator tuples per wave, where that shape
 * exists ("wino_wide" at its default, "wino_s2d_skip" on, Cin % 16 == 0, Cout % 256 == 0; anywhere else it is _forward_s2d3): the same
 * bits for the same K slicing. _preferred_s2d3_wide says where it measured faster (and _preferred_s2d3 holds): from two whole rounds of
 * such blocks on the chip's 256 CUs, or one round of 80 to 256. deepim_conv_wino_plan takes s2d = 3 for it and reports block shape 3. */
int deepim_conv_wino_preferred_s2d3(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout);
int deepim_conv_wino_preferred_s2d3_wide(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout);
int deepim_conv_wino_pack_weights_s2d3(deepim_ctx* ctx, float* packed_w, const float* w /*Cout,Cin,3,3 dev*/, int Cout, int Cin);
int deepim_conv2d_wino_forward_s2d3(deepim_ctx* ctx, float* out, const float* in_s2d, const float* packed_w, const float* bias,
                                    int B, int Cin, int H, int W, int Cout, float slope, int out_nc8, int out_ctotal, int out_coff);
int deepim_conv2d_wino_forward_s2d3_wide(deepim_ctx* ctx, float* out, const float* in_s2d, const float* packed_w, const float* bias,
                                         int B, int Cin, int H, int W, int Cout, float slope, int out_nc8, int out_ctotal, int out_coff);
int deepim_relayout_nc8_s2d(deepim_ctx* ctx, float* dst, const float* src, int B, int C, int H, int W, int to_s2d);
/* The DATA GRADIENT of a 3x3 stride-1 pad-1 layer on the same kernels: it is the same kind of convolution from the layer's Cout to its
 * Cin channels on the transposed, flipped weights. _pack_weights_dgrad writes U' of that Cin <- Cout problem straight from the layer's
 * raw (Cout, Cin, 3, 3) tensor (size deepim_conv_wino_packed_size(Cin, Cout); needs Cin % 32 == 0, Cout % 8 == 0) — bit-identical to
 * deepim_conv_wino_pack_weights on deepim_conv_flip_weights of it, without the flip buffer. deepim_conv2d_wino_dgrad: dx (B, Cin, H, W)
 * NCHW from the channel-blocked dz (B, Cout/8, H, W, 8), no bias, no activation; <= 1e-5 of the range from the direct sum. Worth it
 * where deepim_conv_wino_preferred(ctx, B, Cout, H, W, Cin) says so. */
int deepim_conv_wino_pack_weights_dgrad(deepim_ctx* ctx, float* packed_w, const float* w /*Cout,Cin,3,3 dev*/, int Cout, int Cin);
int deepim_conv2d_wino_dgrad(deepim_ctx* ctx, float* dx, const float* dz_nc8, const float* packed_w, int B, int Cin, int H, int W,
                             int Cout);
int deepim_conv2d_wino_forward(deepim_ctx* ctx, float* out, const float* in, const float* packed_w, const float* bias,
                               int B, int Cin, int H, int W, int Cout, float slope, int out_nc8, int out_ctotal, int out_coff);
/* conv1 (7x7 stride 2 pad 3, Cin 8, Cout 64, deepIM_flownet.py:63) as fp32 Winograd F(2x2,4x4) over its four input phases
 * (csrc/wino_c1.hip): 81 (phase, position) GEMMs over the 8 channels per 2x2 tile, 2.42x fewer multiplies than the direct sum,
 * within 1e-5 of the layer's range from it. `in` is the NCHW (B, 8, H, W) net input; `out` is NC8 (out_mode 1) or NC8 in
 * space-to-depth order (out_mode 3, even output height and width: what the stride-2 Winograd layer conv2 reads). packed_w from
 * deepim_conv1_wino_pack_weights (the layer's (64, 8, 7, 7) weights; size deepim_conv1_wino_packed_size() bytes, laid out for the
 * shared-transform kernel's 32x32x2 MFMAs: [channel half][pair][lane][4 k-steps]; query the size, the layout may change). _preferred is 0
 * for any other geometry and on a context in the canonical-summation-order configuration ("conv_max_split" = 1). */
size_t deepim_conv1_wino_packed_size(void);
int deepim_conv1_wino_preferred(deepim_ctx* ctx, int B, int Cin, int H, int W, int Cout);
int deepim_conv1_wino_pack_weights(deepim_ctx* ctx, float* packed_w, const float* w /*64,8,7,7 dev*/);
int deepim_conv1_wino_forward(deepim_ctx* ctx, float* out, const float* in, const float* packed_w, const float* bias,
                              int B, int H, int W, float slope, int out_mode);
/* The same 3x3 stride-1 pad-1 Convolution + bias + LeakyReLU layers (deepIM_flownet.py:77-101) as fp32 Winograd F(4,3) x F(2,3): 4-row x
 * 2-column output tiles, 24 positions, 3 multiply-adds per output, input and output channel instead of 4 (csrc/wino42.hip; Cout % 64 == 0,
 * Cin % 8 == 0; channel-blocked input, channel-blocked (out_nc8 = 1) or NCHW-slice (0) output). ~3e-6 of the layer's range from the direct
 * sum (bar 1e-5). Packed size: 24 floats per (output, input channel) pair. Measurements and the reason for this tile: profiles/r06_wino44.md. */
size_t deepim_conv_wino42_packed_size(int Cout, int Cin);
int deepim_conv_wino42_pack_weights(deepim_ctx* ctx, float* packed_w, const float* w, int Cout, int Cin);
int deepim_conv2d_wino42_forward(deepim_ctx* ctx, float* out, const float* in, const float* packed_w, const float* bias,
                                 int B, int Cin, int H, int W, int Cout, float slope, int out_nc8, int out_ctotal, int out_coff);
/* fp16 conv path (BASELINE config 5): NHWC fp16 activations, fp16 weights (packed once), fp16 matrix cores
 * with fp32 accumulation, bias + LeakyReLU in fp32, NHWC fp16 output. Same layer semantics as
 * deepim_conv2d_forward (deepIM_flownet.py:63-107); tolerance documented in DESIGN.md (fp16 cannot meet 1e-4).
 * Cin_pad = Cin rounded up to a multiple of 8 (zero channels); Cout % 4 == 0. */
int deepim_nchw_f32_to_nhwc_f16(deepim_ctx* ctx, void* out_f16, const float* in, int B, int C, int H, int W, int Cpad);
int deepim_nhwc_f16_to_nchw_f32(deepim_ctx* ctx, float* out, const void* in_f16, int B, int C, int H, int W);
size_t deepim_conv_f16_packed_size(int Cout, int Cin_pad, int kh, int kw);
int deepim_conv_f16_pack_weights(deepim_ctx* ctx, void* packed, const float* w /*Cout,Cin,kh,kw dev f32*/,
                                 int Cout, int Cin, int Cin_pad, int kh, int kw);
int deepim_conv2d_f16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const void* in_nhwc_f16, const void* packed_w,
                              const float* bias, int B, int Cin_pad, int H, int W, int Cout, int kh, int kw,
                              int stride, int pad, float slope);
/* The launch plan deepim_conv2d_f16_forward (x3 = 0) or deepim_conv2d_x3_forward (x3 = 1, Cin_pad = Cin there) gives a geometry under
 * the context's options (ctx == NULL: the defaults). Host arithmetic, no device work; the launchers read the same plan. plan[0..7] =
 * kernel (0 register-staged, 1 four-wave LDS-DMA, 2 eight-wave ping-pong), BM (output channels per tile), BN (pixels per tile), tiles,
 * K chunks of 64, ksplit (uniform split-K slices, 1 = none), tail_s (K slices of each tile of the last, partly filled round, 0 = no
 * tail split), R (tiles of that round, 0 without a tail split). Geometries a launch refuses return non-zero here too, and leave
 * plan at -1 (an X3 batch of 2 GiB or more runs as consecutive sub-batches, each a launch of its own: ask for a sub-batch). */
int deepim_conv_f16_plan(deepim_ctx* ctx, int x3, int B, int Cin_pad, int H, int W, int Cout, int kh, int kw, int stride, int pad,
                         int* plan /*8, host*/);
/* fp16 Winograd F(2x2,3x3) for the fp16 path's 3x3 stride-1 pad-1 layers (csrc/wino_f16.hip; network.FP16_WINOGRAD, default off):
 * the tensors of deepim_conv2d_f16_forward (NHWC fp16 in and out, fp32 bias, LeakyReLU), 2.25x fewer MFMAs. Its own arithmetic
 * contract, stated operation by operation at the top of csrc/wino_f16.hip and restated in numpy by tests/fp16_wino_emulation.py:
 * U = f16(G f16(w) G^T) from fp32 products, the input transform V = B^T d B in fp16 arithmetic (one fp16 add per entry and pass: two
 * roundings), sixteen GEMMs on v_mfma_f32_32x32x16_f16 with fp32 accumulation, A^T M A + bias + LeakyReLU in fp32, one rounding.
 * Not the direct fp16 kernel within one ulp: about 1.5x its per-layer error (<= 2^-9 of the layer's range from it). No K split and
 * no atomics: bit-identical from run to run. RANGE: |V| <= 4 max|x|, so an activation above about 16 000 can become inf here where the
 * direct kernel would not; nothing is clamped. Odd H or W are fine; the input must be smaller than 2 GiB.
 * deepim_conv_wino_f16_supported: 1 for Cin % 32 == 0 and Cout % 64 == 0 (a pure shape predicate), else 0; pack and forward refuse the
 * rest (-1, nothing launched), deepim_conv_wino_f16_packed_size returns 0 for them and Cout*Cin*32 bytes otherwise.
 * Packed layout (fp16, MFMA A-operand order): the half at index ((((co / 32) * (Cin / 16) + ci / 16) * 16 + p) * 64 + lane) * 8 + ci % 8
 * with lane = co % 32 + 32 * ((ci / 8) % 2) is U[p][co][ci], position p = 4 i + nu of U = G g G^T (i down the rows, nu along them). */
int deepim_conv_wino_f16_supported(int Cin, int Cout);
size_t deepim_conv_wino_f16_packed_size(int Cout, int Cin);
int deepim_conv_wino_f16_pack_weights(deepim_ctx* ctx, void* packed, const float* w /*Cout,Cin,3,3 dev f32*/, int Cout, int Cin);
int deepim_conv2d_wino_f16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const void* in_nhwc_f16, const void* packed_w,
                                   const float* bias, int B, int Cin, int H, int W, int Cout, float slope);
/* Split-fp16 ("x3") convolution: the same Convolution + bias + LeakyReLU (deepIM_flownet.py:63-107) at fp32-grade accuracy on
 * the fp16 matrix cores. A value v travels as the fp16 pair hi = f16(v·s), lo = f16(v·s − hi) (22 significand bits, s a power
 * of two), a product is hi·hi + hi·lo + lo·hi (v_mfma_f32_32x32x16_f16, fp32 accumulation; the dropped lo·lo term is 2^-22
 * relative). Tensors are "split16" NHWC: per pixel, per 16 channels, 32 halves [hi 0..15 | lo 0..15].
 * acc_scale = 1 / (s_in · s_w) returns the accumulator to real units before bias; out_scale = s of the stored output.
 * Needs Cin % 32 == 0, Cout % 128 == 0 (conv2 … conv6_1 of the encoder; conv1: deepim_conv1_x3_forward, or the fp32 conv with a
 * split16 epilogue for other channel counts). Inputs beyond 2 GiB run as sub-batches. A value that leaves fp16's range after
 * scaling is clamped and reported through bit 3 of the status word (deepim_zoom_status). Not bit-exact against the fp32 path:
 * every layer within 1e-5 of the float64-accumulating oracle (tests/test_gpu_x3.py). */
int deepim_nchw_f32_to_split16(deepim_ctx* ctx, void* out_split16, const float* in, int B, int C, int H, int W, float scale);
int deepim_split16_to_nchw_f32(deepim_ctx* ctx, float* out, const void* in_split16, int B, int C, int H, int W, float inv_scale);
size_t deepim_conv_x3_packed_size(int Cout, int Cin, int kh, int kw);
int deepim_conv_x3_pack_weights(deepim_ctx* ctx, void* packed, const float* w /*Cout,Cin,kh,kw dev f32*/, int Cout, int Cin,
                                int kh, int kw, float w_scale);
/* conv1 of that encoder for channel counts other than 8: the fp32 MFMA convolution (NCHW fp32 in, exact products) writing
 * split16 from its epilogue; Cout % 16 == 0, even Cin */
int deepim_conv2d_forward_split16(deepim_ctx* ctx, void* out_split16, const float* in, const float* packed_w, const float* bias,
                                  int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, float slope,
                                  float out_scale);
/* conv1 (Cin 8, 7x7, stride 2, pad 3, Cout 64; deepIM_flownet.py:63-67) in split fp16 straight from the NCHW fp32 net input:
 * persistent LDS-patch kernel, two taps per 16-wide MFMA k-step. in_scale: scale applied to the input before the split;
 * acc_scale = 1 / (in_scale · w_scale). Output split16 (B,Ho,Wo,64 ch). */
size_t deepim_conv1_x3_packed_size(void);
int deepim_conv1_x3_pack_weights(deepim_ctx* ctx, void* packed, const float* w /*64,8,7,7*/, float w_scale);
int deepim_conv1_x3_forward(deepim_ctx* ctx, void* out_split16, const float* in /*B,8,H,W*/, const void* packed_w,
                            const float* bias, int B, int H, int W, float slope, float in_scale, float acc_scale,
                            float out_scale);
/* the same kernel with plain fp16 operands = conv1 of the fp16 path (config 5): NCHW fp32 in → NHWC fp16 (B,Ho,Wo,64) out;
 * packed_w = the first half (hi parts) of deepim_conv1_x3_pack_weights(..., w_scale = 1) */
int deepim_conv1_f16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const float* in /*B,8,H,W*/, const void* packed_w,
                             const float* bias, int B, int H, int W, float slope);
/* conv1 of the fp16 path for BASELINE config 5's RGB-D net input (INPUT_DEPTH: Cin = 10, deepIM_flownet.py:33-62): channels
 * 0-7 as above, channels 8-9 as 14 pseudo taps of 4 consecutive columns x 2 channels (7 extra k-steps instead of the 24 of a
 * 16-channel padding).  w (64,10,7,7) fp32 → packed (deepim_conv1_f16_c10_packed_size bytes). */
size_t deepim_conv1_f16_c10_packed_size(void);
int deepim_conv1_f16_c10_pack_weights(deepim_ctx* ctx, void* packed, const float* w /*64,10,7,7*/);
int deepim_conv1_f16_c10_forward(deepim_ctx* ctx, void* out_nhwc_f16, const float* in /*B,10,H,W*/, const void* packed_w,
                                 const float* bias, int B, int H, int W, float slope);
/* conv1 of the fp16 path from fp16 pixel records (deepim_zoom_concat_forward_h16): extra2 == NULL → 8-channel input, packed_w as
 * for deepim_conv1_f16_forward; extra2 set → the 10-channel RGB-D input, packed_w from deepim_conv1_f16_c10_pack_weights */
int deepim_conv1_f16_h16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const void* main8, const void* extra2,
                                 const void* packed_w, const float* bias, int B, int H, int W, float slope);
int deepim_conv2d_x3_forward(deepim_ctx* ctx, void* out_split16, const void* in_split16, const void* packed_w, const float* bias,
                             int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, float slope,
                             float acc_scale, float out_scale);
/* MXNet Deconvolution k4 s2 p0 (+bias) + Crop(offset 1,1 → Ho,Wo) [+LeakyReLU]
 * (deepIM_flownet.py:127-143,149-165). w layout (Cin,Cout,4,4). */
size_t deepim_deconv_packed_size(int Cin, int Cout);
int deepim_deconv_pack_weights(deepim_ctx* ctx, float* packed_w, const float* w, int Cin, int Cout);
int deepim_deconv4x4s2_crop_forward(deepim_ctx* ctx, float* out, const float* in, const float* packed_w,
                                    const float* bias, int B, int Cin, int H, int W, int Cout,
                                    int Ho, int Wo, int crop_y, int crop_x, float slope,
                                    int out_ctotal, int out_coff);
/* fp16 FlowNetS decoder (the fp16 conv path with the decoder in the graph; csrc/decoder_f16.hip). Tensors are NHWC fp16 records
 * of `ctotal` channels; a layer reads channels [0, Cin_pad) of its input and writes a channel slice of its output.
 * deconv5 / deconv4: Deconvolution k4 s2 p0 + bias + Crop(1,1) + LeakyReLU (deepIM_flownet.py:127-143,149-165) as four parity-class
 * GEMMs on v_mfma_f32_32x32x16_f16 (fp16 weights x fp16 activations, fp32 accumulation, bias + LeakyReLU in fp32, one rounding at
 * the store) into channels [out_coff, out_coff + Cout). Cout % 64 == 0, Cin_pad % 8 == 0 (input channels [Cin, Cin_pad) zero or
 * finite: their packed weights are zero), out_coff % 4 == 0. w (Cin,Cout,4,4) fp32 → packed (deepim_deconv_f16_packed_size bytes). */
size_t deepim_deconv_f16_packed_size(int Cin_pad, int Cout);
int deepim_deconv_f16_pack_weights(deepim_ctx* ctx, void* packed, const float* w, int Cin, int Cin_pad, int Cout);
int deepim_deconv4x4s2_crop_f16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const void* in_nhwc_f16, const void* packed_w,
                                        const float* bias, int B, int Cin_pad, int in_ctotal, int H, int W, int Cout, int Ho,
                                        int Wo, float slope, int out_ctotal, int out_coff);
/* The launch plan deepim_deconv4x4s2_crop_f16_forward gives a geometry: host arithmetic, no context, no device; the launcher reads the
 * same plan. plan[0..7] = block tiles of all four parity classes, pixels (all images) of class 0..3 (class = 2·(oy % 2) + ox % 2),
 * k-steps of 16 (= Cin_pad / 4), ksplit (K slices, 1 = none), k-steps per slice (the last slice may hold fewer). Geometries the
 * launcher refuses for B, Cin_pad, H, W, Cout, Ho or Wo (an empty batch included) return non-zero and leave plan at -1. */
int deepim_deconv_f16_plan(int B, int Cin_pad, int H, int W, int Cout, int Ho, int Wo, int* plan /*8, host*/);
/* Few-filter 3x3 stride-1 pad-1 Convolution + bias (Convolution1 / 2 / 3, mask_conv3) from an NHWC fp16 input into fp32 NCHW: up to
 * 3 filters in one pass over the input, n0 of them into out0 (B,n0,H,W), n1 into out1 (B,n1,H,W) (n1 = 0, out1 = NULL: one tensor).
 * fp16 weights x fp16 activations (products exact), fp32 sums, fp32 bias. w0 (n0,Cin,3,3), w1 (n1,Cin,3,3) fp32 → packed
 * (deepim_fewout_f16_packed_size bytes); Cin_pad % 8 == 0, above 0 and at most 2048; H, W > 0 (B = 0: nothing to do). */
size_t deepim_fewout_f16_packed_size(int Cin_pad);
int deepim_fewout_f16_pack_weights(deepim_ctx* ctx, void* packed, const float* w0, int n0, const float* w1, int n1, int Cin,
                                   int Cin_pad);
int deepim_conv3x3_fewout_f16_forward(deepim_ctx* ctx, float* out0, int n0, float* out1, int n1, const void* in_nhwc_f16,
                                      const void* packed_w, const float* bias0, const float* bias1, int B, int H, int W,
                                      int in_ctotal, int Cin_pad);
/* The launch plan deepim_conv3x3_fewout_f16_forward gives a geometry (host arithmetic; the launcher reads the same plan): plan[0..3] =
 * threads per block (one per input octet, in whole waves), columns per row segment, segments per row, waves per block. B, H, W or
 * Cin_pad of 0, Cin_pad % 8 != 0 and Cin_pad > 2048 return non-zero, as in the launcher, and leave plan at -1. */
int deepim_fewout_f16_plan(int B, int H, int W, int Cin_pad, int* plan /*4, host*/);
/* upsample_flow6to5 / 5to4: Deconvolution k4 s2 (2 → 2 channels) + bias + Crop(1,1) of an fp32 NCHW flow (B,2,H,W) in fp32,
 * rounded once into channels [out_coff, out_coff + 2) of an NHWC fp16 output (Ho,Wo); w (2,2,4,4) fp32 as stored */
int deepim_upsample_flow_f16_forward(deepim_ctx* ctx, void* out_nhwc_f16, const float* in, const float* w, const float* bias,
                                     int B, int H, int W, int Ho, int Wo, int out_ctotal, int out_coff);
/* NHWC fp16 channel-slice copy: dst[pix][dst_coff + c] = src[pix][src_coff + c], c < C, for npix pixels; all counts % 8 == 0 */
int deepim_copy_channels_nhwc_f16(deepim_ctx* ctx, void* dst, int dst_ctotal, int dst_coff, const void* src, int src_ctotal,
                                  int src_coff, int C, long npix);
/* grouped (depthwise) Deconvolution k32 s16 no-bias + Crop(offset) to (Ho,Wo), times `scale`
 * (deepIM_flownet.py:185-200,326-340,636-648,687-702). w (C,1,32,32). */
int deepim_upsample16_crop_forward(deepim_ctx* ctx, float* out, const float* in, const float* w,
                                   int B, int C, int H, int W, int Ho, int Wo,
                                   int crop_y, int crop_x, float scale);
/* FullyConnected y = x·Wᵀ + b [+LeakyReLU] (deepIM_flownet.py:112-116,211-215) */
int deepim_fc_forward(deepim_ctx* ctx, float* out, const float* in, const float* w /*O,I*/,
                      const float* bias, int B, int I, int O, float slope);
/* fc6 on the fp32 matrix cores, one pass over the weights for up to 32 batch rows (v_mfma_f32_32x32x2_f32 split-K GEMM
 * with a fixed-order reduction): the (O,I) MXNet weight is re-packed once into MFMA operand order, then
 * out (B,O) = lrelu(in (B,I) · wᵀ + bias). Built for O == 256 (fc6, fc7), I % 8 == 0. */
size_t deepim_fc_packed_size(int O, int I);
int deepim_fc_pack_weights(deepim_ctx* ctx, float* packed_w, const float* w, int O, int I);
int deepim_fc_forward_packed(deepim_ctx* ctx, float* out, const float* in, const float* packed_w, const float* bias,
                             int B, int I, int O, float slope);
/* fc7-input → rot(4), trans(3) FCs + ZoomTrans(inverse) + Concat → se3 (B,7)
 * (deepIM_flownet.py:715-726) */
int deepim_pose_head_forward(deepim_ctx* ctx, float* se3 /*B,7*/, const float* feat /*B,F*/,
                             const float* w_rot, const float* b_rot,
                             const float* w_trans, const float* b_trans,
                             const float* zoom_factor, int B, int F);

/* --------------------------------------------- S-group: SE(3) pose update -- */
/* RT_transform (lib/pair_matching/RT_transform.py:127-151) batched: pose_est (B,3,4) f32 from
 * pose_src (B,3,4), se3 (B,7) = [quat(4) | trans(3)]. Computed in float64 like the reference,
 * stored float32. rot_coord: 0 MODEL, 1 CAMERA, 2 CAMERA_NEW, 3 NAIVE. pose_est64 optional (B,3,4) f64. */
int deepim_rt_transform(deepim_ctx* ctx, float* pose_est, double* pose_est64, const float* pose_src,
                        const float* se3, const float* T_means_host, const float* T_stds_host,
                        int rot_coord, int B);
/* calc_RT_delta (lib/pair_matching/RT_transform.py:16-44, rot_type QUAT) batched: the ground-truth
 * (rot (B,4) w>=0, trans (B,3)) labels between a source and a target pose — R_inv_transform (:64-71),
 * T_inv_transform (:105-124), mat2quat (:432-509, largest eigenvector of the 4x4 K matrix; Jacobi sweeps in
 * float64 here). Used by the loader (data_pair.py:188-195) and the batch updater (:239-246). */
int deepim_calc_rt_delta(deepim_ctx* ctx, float* rot /*B,4*/, float* trans /*B,3*/, const float* pose_src,
                         const float* pose_tgt, const float* T_means_host, const float* T_stds_host,
                         int rot_coord, int B);
/* The tail of one test-graph refinement iteration in ONE launch: fc7 (FullyConnected 256 → 256 + LeakyReLU,
 * deepIM_flownet.py:114-116) → rot / trans FullyConnected + inverse ZoomTrans → se3 (:715-726, zoom_trans.py:22-46) →
 * RT_transform (lib/pair_matching/RT_transform.py:127-151, quaternion form) — the same sums in the same order as
 * deepim_fc_forward + deepim_pose_head_forward + deepim_rt_transform, hence bit-identical to them. fc7_out (B,256), se3 (B,7),
 * pose_est (B,3,4; may be pose_src: in-place update), fc6 (B,256); feat must be 256. */
int deepim_pose_tail_forward(deepim_ctx* ctx, float* fc7_out, float* se3, float* pose_est, const float* fc6,
                             const float* w_fc7, const float* b_fc7, const float* w_rot, const float* b_rot,
                             const float* w_trans, const float* b_trans, const float* zoom_factor,
                             const float* pose_src, const float* T_means_host, const float* T_stds_host, int rot_coord,
                             int B, int feat, float slope);
/* RT_transform with an Euler-angle rotation (ROT_TYPE EULER: r.shape[0] == 3 → euler2mat(r0, r1, r2), static xyz axes,
 * RT_transform.py:130-131, :240-307): euler_trans (B,6) = [euler(3) | trans(3)]. */
int deepim_rt_transform_euler(deepim_ctx* ctx, float* pose_est, double* pose_est64, const float* pose_src,
                              const float* euler_trans, const float* T_means_host, const float* T_stds_host,
                              int rot_coord, int B);
/* calc_RT_delta with the reference's rot_type switch (RT_transform.py:34-41): 0 QUAT → rot (B,4), 1 EULER (mat2euler
 * sxyz, :310-373) → rot (B,3), 2 MATRIX → rot (B,9). */
int deepim_calc_rt_delta_ex(deepim_ctx* ctx, float* rot, float* trans, const float* pose_src, const float* pose_tgt,
                            const float* T_means_host, const float* T_stds_host, int rot_coord, int rot_type, int B);
/* the rotation converters of RT_transform.py as batched ops, float64 results like the reference's:
 * op 0 quat2mat (:383-429; in (B,4) → out (B,9)), 1 mat2quat (:432-509; (B,9) → (B,4), w >= 0),
 * 2 euler2mat sxyz (:240-307; (B,3) → (B,9)), 3 mat2euler sxyz (:310-373; (B,9) → (B,3)) */
int deepim_rot_convert(deepim_ctx* ctx, double* out, const float* in, int op, int B);
/* get_point_cloud_observed (lib/pair_matching/data_pair.py): out (B,3,N) = R·points + T for pose (B,3,4) */
int deepim_points_transform(deepim_ctx* ctx, float* out, const float* points, const float* pose, int B, int N);
/* calc_se3 (RT_transform.py:176-187): se3_mul(pose_tgt, se3_inverse(pose_src)) in float32 (lib/utils/projection.py:12-43)
 * → rotm (B,3,3), t (B,3) */
int deepim_calc_se3(deepim_ctx* ctx, float* rotm, float* t, const float* pose_src, const float* pose_tgt, int B);
/* Pose-error metrics of lib/utils/pose_error.py (used by the evaluate_pose functions of LM6D_REFINE.py:278-512 and by
 * tester.py:401): per pair out[b] = { re (:118-124, geodesic angle in degrees; == calc_rt_dist_m's rd_deg),
 * te (:127-145, ||t_gt - t_est||), add (:55-69), adi (:72-88, nearest-neighbour mean, brute force instead of a
 * KD-tree), arp_2d (:36-52, mean reprojection distance in pixels) }. points: (B,3,N) model points or, with
 * points_shared != 0, one (3,N) set for all pairs. float64 accumulation, float32 results (B,5). */
int deepim_pose_error(deepim_ctx* ctx, float* out /*B,5*/, const float* pose_est, const float* pose_gt,
                      const float* points, int points_shared, const float* K_host /*or NULL: camera table*/, int B, int N);
/* Depth ICP (csrc/icp.hip): a projective point-to-plane refiner between a rendered ("source") and an observed ("target") depth
 * map, the device counterpart of the `*-pose_icp.txt` poses the reference reads from files (deepim/core/tester.py:193-279).
 * Every entry is asynchronous on the context stream, legal inside a graph capture once its scratch has grown (a first eager
 * call), free of atomics (fixed-order reductions: the same inputs give the same bytes) and computes in double from the float32
 * inputs, K⁻¹ included (inv3d, as the flow entries). Depths are (B,1,H,W) float32 metres, 0 = no measurement.
 * deepim_depth_normals: vertex v(x,y) = depth · K⁻¹ · (x,y,1); n = normalize((v(x+1,y) − v(x−1,y)) × (v(x,y+1) − v(x,y−1))),
 * negated where n·v > 0 (it faces the camera), rounded to float32. n = 0 on the one-pixel border, where one of the five depths
 * is <= 0, where a neighbour's depth differs from the centre's by more than max_step, and where the cross product is zero. */
int deepim_depth_normals(deepim_ctx* ctx, float* normals /*B,3,H,W*/, const float* depth /*B,1,H,W*/,
                         const float* K_host /*or NULL: camera table*/, float max_step, int B, int H, int W);
/* One Gauss-Newton step of every pair. A source pixel with depth_src > 0 is back-projected to p, moved to p' = R_T·p + t_T,
 * dropped where p'_z <= 0, projected with K and rounded to the nearest pixel (ties to even), dropped outside the frame; with
 * the target vertex q and normal n of that pixel it is dropped where the target depth is <= 0, n = 0 or |p' − q|² > dist_max²;
 * else r = n·(p' − q), J = [p' × n ; n] — the twist (ω, v) of the left update T ← exp(ξ̂)·T. sys[b] (30 doubles, may be NULL):
 * the 21 upper entries of ΣJJᵀ row by row, the 6 of −ΣJr, the pair count, Σr², one spare. Then, in the same call, Cholesky in
 * double: status[b] = 1 when the count is below min_pairs, 2 when a pivot is <= rcond · max diag; either, or skip[b] != 0
 * (skip may be NULL), leaves T[b] untouched; else status[b] = 0 and T[b] ← exp(ξ̂)·T[b] (Rodrigues with its V matrix), float32.
 * The pixels of a pair are cut into blocks of 1024 whatever B is, so a pair's result does not depend on the batch around it. */
int deepim_icp_step(deepim_ctx* ctx, float* T /*B,3,4 in and out*/, double* sys /*B,30 or NULL*/, int32_t* status /*B*/,
                    const float* depth_src, const float* depth_tgt, const float* normals_tgt /*B,3,H,W*/,
                    const float* K_host /*or NULL: camera table*/, const int32_t* skip /*B or NULL*/, float dist_max,
                    int min_pairs, double rcond, int B, int H, int W);
/* pose_out (B,3,4) = [R_T·R | R_T·t + t_T]: the increment applied to the object pose in camera coordinates (may alias pose_in) */
int deepim_icp_apply(deepim_ctx* ctx, float* pose_out, const float* T, const float* pose_in, int B);
/* Transform3D forward/backward (deepim/operator_py/transform3d.py:34-151) */
int deepim_transform3d_forward(deepim_ctx* ctx, float* out /*B,3,N*/, const float* points /*B,3,N*/,
                               const float* rotation /*B,4*/, const float* translation /*B,3*/,
                               const float* pose_src, const float* T_means_host,
                               const float* T_stds_host, int rot_coord, int B, int N);
int deepim_transform3d_backward(deepim_ctx* ctx, float* d_rotation /*B,4*/, float* d_translation /*B,3*/,
                                const float* out_grad /*B,3,N*/, const float* points,
                                const float* rotation, const float* translation,
                                const float* pose_src, const float* T_means_host,
                                const float* T_stds_host, int rot_coord, int B, int N);

/* ---------------------------------------------------- H-group: heads/losses -- */
/* point-matching loss (deepIM_flownet.py:265-312): per-element
 * loss = weights · f((est − gt)/normalize), f ∈ {0: L1 |x|, 1: L2 x², 2: smooth-L1(σ)};
 * writes loss elements (B,3,N), the batch sum and d loss/d est (scaled by grad_scale) */
int deepim_point_matching_loss(deepim_ctx* ctx, float* loss /*B,3,N*/, float* loss_sum /*1*/,
                               float* d_est /*B,3,N or NULL*/, const float* est, const float* gt,
                               const float* weights /*B,3,N or NULL*/, float normalize,
                               int loss_type, float sigma, float grad_scale, int B, int N);
/* flow loss (deepIM_flownet.py:201-207): loss = w·(est − gt/normalize_flow)² */
int deepim_flow_loss(deepim_ctx* ctx, float* loss /*n*/, float* loss_sum, float* d_est,
                     const float* est, const float* gt, const float* weights,
                     float normalize_flow, float grad_scale, size_t n);
/* MXNet L2Normalization, instance mode (deepIM_flownet.py:217 `normalize_quat`): out = x / sqrt(Σx² + eps) */
int deepim_l2_normalize_forward(deepim_ctx* ctx, float* out, const float* in, int B, int D, float eps);
int deepim_l2_normalize_backward(deepim_ctx* ctx, float* d_in, const float* d_out, const float* in, int B, int D,
                                 float eps);
/* rotation distance loss (deepIM_flownet.py:238-248): loss_b = 1 − (q_gt·q_est)², d_q_est = −2(q_gt·q_est)·q_gt·grad_scale.
 * The translation distance loss (:250-262) is deepim_point_matching_loss with N = 1, normalize = 1, no weights. */
int deepim_rot_dist_loss(deepim_ctx* ctx, float* loss /*B*/, float* d_q_est /*B,4 or NULL*/, const float* q_gt,
                         const float* q_est, float grad_scale, int B);
/* mask head test path (deepIM_flownet.py:647-666): sigmoid → ZoomMaskWithFactor(inverse)
 * → round. `logits` is the cropped upsampled mask_conv3 output (B,1,H,W). prob optional. */
int deepim_mask_head_forward(deepim_ctx* ctx, float* mask_pred /*B,1,H,W*/, float* prob /*or NULL*/,
                             const float* logits, const float* zoom_factor, int B, int H, int W);
/* mask loss (deepIM_flownet.py:342-361): LogisticRegressionOutput forward = sigmoid,
 * backward = (p − y)·grad_scale */
int deepim_mask_logistic(deepim_ctx* ctx, float* prob, float* d_logits /*or NULL*/,
                         const float* logits, const float* label, float grad_scale, size_t n);
/* GroupPicker (deepim/operator_py/group_picker.py:22-56) */
int deepim_group_picker_forward(deepim_ctx* ctx, float* out /*B,C/G*/, const float* in /*B,C*/,
                                const float* group_idx /*B*/, int group_num, int B, int C);
int deepim_group_picker_backward(deepim_ctx* ctx, float* in_grad /*B,C*/, const float* out_grad,
                                 const float* group_idx, int group_num, int B, int C);

/* ------------------------------------ T-group: backward of the network + SGD -- */
/* what module.backward and the "sgd" optimizer do for the conv stack and the FC head in the reference's
 * training loop (deepim/core/module.py:1131-1137, deepim/train.py:295-338; layers at deepIM_flownet.py:63-116,211-215).
 * All tensors NCHW fp32 device. Reductions are deterministic (fixed order, no float atomics). */
/* LeakyReLU gradient from the saved OUTPUT y: dz = y > 0 ? dy : slope*dy */
int deepim_lrelu_backward(deepim_ctx* ctx, float* dz, const float* dy, const float* y, float slope, size_t n);
/* db[c] = sum over n, pixels of dz (B,C,hw) */
int deepim_bias_grad(deepim_ctx* ctx, float* db, const float* dz, int B, int C, size_t hw);
/* the two in one walk, with the gradient arriving over a skip connection folded in: dz = lrelu'(y)*(dy [+ add]) (B,C,hw; dz may
 * be dy; add may be NULL), db[c] = sum of dz — what the training graph needs per encoder layer */
int deepim_lrelu_bias_backward(deepim_ctx* ctx, float* dz, float* db, const float* dy, const float* add, const float* y,
                               float slope, int B, int C, size_t hw);
/* the same walk where the saved output lies channel-blocked: y_mode 1 = NC8 (B, C/8, H, W, 8), 3 = NC8 in space-to-depth order (even H
 * and W), 0 = NCHW like the gradients (the last encoder layer: taken for its dz_nc8 output); C % 8 == 0. dy / add / dz stay NCHW and dz holds the same bits as above on the NCHW copy of y; dz_nc8 (may be NULL) receives
 * the same dz values once more as plain NC8 records — the input of deepim_conv2d_wino_dgrad */
int deepim_lrelu_bias_backward_nc8(deepim_ctx* ctx, float* dz, float* dz_nc8, float* db, const float* dy, const float* add,
                                   const float* y_nc8, int y_mode, float slope, int B, int C, int H, int W);
/* wt (Cin,Cout,kh,kw) = w (Cout,Cin,kh,kw) transposed and flipped: the weights with which the data gradient of a
 * convolution is itself a stride-1 convolution (pad kh-1-p) — run on deepim_conv2d_forward after deepim_conv_pack_weights */
int deepim_conv_flip_weights(deepim_ctx* ctx, float* wt, const float* w, int Cout, int Cin, int kh, int kw);
/* Data gradient of a stride-2 convolution as four stride-1 convolutions of the UN-dilated gradient, one per output parity
 * class (py, px): the class only meets the taps ky = ky0 + 2a, kx = kx0 + 2b with ky0 = (py + pad) % 2, kx0 = (px + pad) % 2.
 * wt (Cin,Cout,nky,nkx) = that sub-kernel of w (Cout,Cin,kh,kw), transposed and flipped → deepim_conv_pack_weights →
 * deepim_conv2d_forward(stride 1, pad P) → deepim_interleave2d puts the window [cy, cy + hq) x [cx, cx + wq) of the result on
 * dx[.., 2i + py, 2j + px] (the training loop's module.backward, deepim/core/module.py:1131-1137, for conv2/3/4/5/6). */
int deepim_conv_subkernel_flip(deepim_ctx* ctx, float* wt, const float* w, int Cout, int Cin, int kh, int kw, int ky0, int kx0,
                               int nky, int nkx);
int deepim_interleave2d(deepim_ctx* ctx, float* dx /*BC,H,W*/, const float* src /*BC,Hs,Ws*/, int BC, int Hs, int Ws, int cy,
                        int cx, int H, int W, int py, int px);
/* the class convolution and the interleave in one: the final stores of the conv kernels (and of their split-K second pass)
 * put the window of the result on out (B,Cout,Hd,Wd)[.., 2i + py, 2j + px] — no class buffer */
int deepim_conv2d_forward_remap(deepim_ctx* ctx, float* out, const float* in, const float* packed_w, int B, int Cin, int H, int W,
                                int Cout, int kh, int kw, int pad, int cy, int cx, int Hd, int Wd, int py, int px);
/* The whole data gradient of a stride-2 convolution (kernel k x k, pad): dx (B,Ci_l,Hd,Wd) from dz (B,Co_l,Ho,Wo), Ho = (Hd + 2 pad
 * - k)/2 + 1, and the layer's RAW weights w_layer (Co_l,Ci_l,k,k). The four parity classes above are packed, convolved and
 * reduced TOGETHER — one launch each, the blocks of the convolution launch shared out over the classes — when the register-fed
 * kernel takes the geometry (even Co_l; 64 x 256 tiles for Ci_l <= 64, else 128 x 128); class by class otherwise or with option
 * "dgrad_group" = 0.
 * packed_ws: device workspace of deepim_conv_dgrad_s2_packed_size bytes. */
size_t deepim_conv_dgrad_s2_packed_size(int Co_l, int Ci_l, int k, int pad);
int deepim_conv2d_dgrad_s2(deepim_ctx* ctx, float* dx, const float* dz, const float* w_layer, float* packed_ws, int B, int Ci_l,
                           int Hd, int Wd, int Co_l, int k, int pad);
/* Data gradient of a Convolution layer (weights (Co_l,Ci_l,k,k), stride 1 or 2, pad) from its RAW weights, optionally already
 * multiplied by the activation gradient of the layer below: dx (B,Ci_l,Hd,Wd) = lrelu'(act_y) * (dgrad(dz) [+ add]) — act_y =
 * that layer's saved output, add = the gradient reaching it over a skip connection, both laid out like dx; NULL act_y = plain
 * data gradient (add must then be NULL). Stride 1 = deepim_conv_pack_dgrad + the forward kernel, stride 2 =
 * deepim_conv2d_dgrad_s2; the activation gradient rides in the final stores of the register-fed kernels and their split-K
 * second passes (no pass of its own over dx), other kernel families get it as one extra pass. What module.backward does per
 * encoder layer (deepim/core/module.py:1131-1137). packed_ws: deepim_conv_dgrad_packed_size bytes. */
size_t deepim_conv_dgrad_packed_size(int Co_l, int Ci_l, int k, int stride, int pad);
int deepim_conv2d_dgrad(deepim_ctx* ctx, float* dx, const float* dz, const float* w_layer, float* packed_ws, int B, int Ci_l,
                        int Hd, int Wd, int Co_l, int k, int stride, int pad, const float* act_y, const float* add, float slope);
/* out (BC,Hd,Wd) = in (BC,Ho,Wo) with stride-1 zeros between the samples (data gradient of a strided convolution) */
int deepim_dilate2d(deepim_ctx* ctx, float* out, const float* in, int BC, int Ho, int Wo, int Hd, int Wd, int stride);
/* the same with an offset: out[bc][off_y + stride*y][off_x + stride*x] = in[bc][y][x], zeros elsewhere — also the backward of
 * Crop (stride 1): the gradient of a cropped Deconvolution output put back into the full frame */
int deepim_scatter2d(deepim_ctx* ctx, float* out, const float* in, int BC, int Ho, int Wo, int Hd, int Wd, int stride,
                     int off_y, int off_x);
/* data gradient of deepim_upsample16_crop_forward (depthwise k32 s16 transposed conv with fixed bilinear weights, lr_mult 0:
 * deepIM_flownet.py:185-200,326-340): d_in (B,C,H,W) from dy (B,C,Ho,Wo) */
int deepim_upsample16_crop_backward(deepim_ctx* ctx, float* d_in, const float* dy, const float* w, int B, int C, int H, int W,
                                    int Ho, int Wo, int crop_y, int crop_x, float scale);
/* backward of [Concat slice -> LeakyReLU -> Crop] in front of a Deconvolution, in one walk: out (B,C,hf,wf) = channels
 * [coff, coff+C) of dcat (B,ctotal,ho,wo) times lrelu'(same slice of ycat; NULL: no activation) at offset (off_y, off_x), zeros
 * around; db[c] = its sum (NULL: skipped). deepIM_flownet.py:120-167 */
int deepim_slice_lrelu_bias_scatter(deepim_ctx* ctx, float* out, float* db, const float* dcat, const float* ycat, int B, int ctotal,
                                    int coff, int C, int ho, int wo, int hf, int wf, int off_y, int off_x, float slope);
/* backward of Concat: dst (B,C,hw) = channels [src_coff, src_coff+C) of src (B,src_ctotal,hw) */
int deepim_extract_channels(deepim_ctx* ctx, float* dst, const float* src, int src_ctotal, int src_coff, int C, int B,
                            size_t hw);
/* dw (Cout,Cin,kh,kw) = sum over n, output pixels of dz (B,Cout,Ho,Wo) x the matching taps of x (B,Cin,H,W): MFMA GEMM
 * with the pixels as the reduction dimension; Ho*Wo must be a multiple of 4 */
int deepim_conv2d_wgrad(deepim_ctx* ctx, float* dw, const float* x, const float* dz, int B, int Cin, int H, int W, int Cout,
                        int kh, int kw, int stride, int pad);
/* The launch plan the fp32 weight-gradient entries (deepim_conv2d_wgrad, _tm, _tm_nc8, _bias) give a geometry with option "wgrad_lds"
 * at that value. Host arithmetic from the geometry alone, no context and no device work; the launcher reads the same plan. plan[0..9] =
 * family (0 few-filter stream kernel, 1 LDS-staged MFMA, 2 register-fed MFMA), bm (rows of an output-channel tile), m-tiles, k-tiles
 * (128 columns of Cin*kh*kw each), units (LDS-staged: chunks of 16 pixels of one sample, B*ceil(Ho*Wo/16); register-fed: groups of 8),
 * S (slices of whole units), units per slice, units of the last slice, second pass (0 none: the kernel writes dw itself, 1 scalar
 * walk over the slices, 2 four quarters of ceil(S/4) slices), 1 if the last unit of a sample is ragged (Ho*Wo % 16, % 8) else 0. The
 * few-filter kernel has no units, slices or second pass: 0, 1, 0, 0, 0, 0. Operands of 2 GiB and more take the register-fed kernel
 * whatever the option says: that stays the launcher's decision, the query answers for the option. Geometries the entries refuse
 * (Ho*Wo % 4 != 0, no output pixel) and B < 1 return non-zero here too, and leave plan at -1. */
int deepim_conv_wgrad_plan(int wgrad_lds, int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad,
                           int* plan /*10, host*/);
/* the weight gradient in TAP-MAJOR layout dw_tm (Cout, kh*kw, Cin) — what the LDS-staged kernel produces fastest (one range
 * check and one address per eight channels of a tap). Same sums, same order as deepim_conv2d_wgrad; needs Cin % 8 == 0, Cout > 4,
 * option "wgrad_lds" on. deepim_sgd_mom_update_multi reads it in place; deepim_weight_grad_to_natural gives (Cout,Cin,kh,kw). */
int deepim_conv2d_wgrad_tm(deepim_ctx* ctx, float* dw_tm, const float* x, const float* dz, int B, int Cin, int H, int W, int Cout,
                           int kh, int kw, int stride, int pad);
/* ... with a channel-blocked x operand (x_mode 1 = NC8, 3 = NC8 in space-to-depth order, even H and W): a thread's eight K rows are
 * one 32-byte record of x. Only the loads differ: bit-identical to deepim_conv2d_wgrad_tm on the NCHW copy of the same tensor. */
int deepim_conv2d_wgrad_tm_nc8(deepim_ctx* ctx, float* dw_tm, const float* x_nc8, int x_mode, const float* dz, int B, int Cin, int H,
                               int W, int Cout, int kh, int kw, int stride, int pad);
int deepim_weight_grad_to_natural(deepim_ctx* ctx, float* dw, const float* dw_tm, int Cout, int Cin, int khw);
/* weight AND bias gradient of a layer (db[c] = sum of dz): one launch for the few-filter layers (Cout <= 4, 3x3 / 4x4: the
 * prediction heads), deepim_bias_grad + deepim_conv2d_wgrad otherwise */
int deepim_conv2d_wgrad_bias(deepim_ctx* ctx, float* dw, float* db, const float* x, const float* dz, int B, int Cin, int H, int W,
                             int Cout, int kh, int kw, int stride, int pad);
/* FullyConnected backward: dx (B,I) = dy·w, dw (O,I) = dyT·x, db (O) = sum_b dy; any of dx/dw/db may be NULL */
int deepim_fc_backward(deepim_ctx* ctx, float* dx, float* dw, float* db, const float* dy, const float* x, const float* w,
                       int B, int I, int O);
/* MXNet sgd_mom_update (train.py:296-303): mom = momentum*mom - lr*(rescale*g [clipped to +-clip if clip > 0] + wd*w); w += mom */
int deepim_sgd_mom_update(deepim_ctx* ctx, float* w, float* mom, const float* g, float lr, float wd, float momentum,
                          float rescale, float clip, size_t n);

/* the same update of every parameter in one launch. table (device): `rows` rows of six 64-bit words {w, mom, g (device
 * addresses), n, (bits of float wd) | (first block of the row << 32), layout of g: 0 = like w, else Cin | (kh*kw << 32) = the
 * tap-major gradient of deepim_conv2d_wgrad_tm}; a row owns ceil(n/1024) blocks (four parameters per thread: w, mom and a natural g
 * must be 16-byte aligned), rows in block order, total_blocks = their sum.
 * Results are bit-identical to per-tensor deepim_sgd_mom_update calls on natural gradients. */
int deepim_sgd_mom_update_multi(deepim_ctx* ctx, const unsigned long long* table, int rows, int total_blocks, float lr,
                                float momentum, float rescale, float clip);

/* MXNet 1.2 adam_update (train.py:260-294, TRAIN.optimizer = "adam"), per element in fp32:
 *   g' = rescale*g + wd*w  [clamped to +-clip if clip > 0: the clamp acts on the sum, weight decay included]
 *   mean = beta1*mean + (1-beta1)*g';  var = beta2*var + (1-beta2)*g'*g';  w -= lr_t * mean / (sqrt(var) + epsilon)
 * lr_t = lr * sqrt(1-beta2^t) / (1-beta1^t), t = updates applied so far, this one included; epsilon is outside the bias correction
 * (not torch.optim.Adam's placement). beta1 and 1-beta1 (beta2 likewise) are rounded to float separately, from the doubles given.
 * This single-tensor entry takes lr_t from the caller. g = mean = var = 0 and wd = 0 leave w unchanged bit for bit. */
int deepim_adam_update(deepim_ctx* ctx, float* w, float* mean, float* var, const float* g, float lr_t, float wd, double beta1,
                       double beta2, float epsilon, float rescale, float clip, size_t n);

/* the same update of every parameter in one launch, with the step count kept on the device. table (device): `rows` rows of SEVEN
 * 64-bit words {w, mean, var, g (device addresses), n, (bits of float wd) | (first block of the row << 32), layout of g as in
 * deepim_sgd_mom_update_multi}; blocks, alignment and row order as there.
 * opt_state (device, 4 x 32 bit, zeroed by the owner before the first update): {uint t, float lr_t, float lr_factor, uint 0}. The
 * call first runs a one-thread launch that sets t += 1, lr_factor = sqrt(1-beta2^t)/(1-beta1^t) and lr_t = lr*lr_factor (both
 * evaluated in double, rounded to float once), then the update kernel, which reads lr_t from the state: the step is folded into
 * this call, there is no separate entry for it. amp_state (NULL: none) is the loss-scale state of the fp16 / x3 training modes:
 * while its overflow word is set nothing moves, t included; run deepim_amp_scale_update after the call. No host sync.
 * Results are bit-identical to per-tensor deepim_adam_update calls on natural gradients with the lr_t of the state. */
int deepim_adam_update_multi(deepim_ctx* ctx, const unsigned long long* table, int rows, int total_blocks, unsigned* opt_state,
                             double lr, double beta1, double beta2, float epsilon, float rescale, float clip,
                             const unsigned* amp_state);

/* ---------------------------- mixed-precision training of the encoder (network.FP16_CONV in the training graph) -- */
/* csrc/train_half.hip; DESIGN.md §8f-4c. q(v) = round to fp16 (RNE) and back; S = the loss scale, a power of two. Forward = the
 * FP16_CONV encoder; the backward of encoder layer l (conv6_1 down to flow_conv1) is
 *   e_l   = S·(fc6 data gradient + d_dec61) at conv6_1 (fp32), d_l [+ S·skip_l] below (skip: fp32 decoder gradient of conv5_1 / conv4_1)
 *   dz_l  = q(lrelu'(y_l)·e_l)                          NHWC fp16, lrelu' from the stored fp16 y_l
 *   db_l  = Σ dz_l / S                                  fp32 sums
 *   dW_l  = Σ_pix dz_l ⊗ im2col(y_{l-1}) / S             exact fp16 products, fp32 sums, fp32 result
 *   d_l-1 = q(conv_transpose(dz_l, q(w_l)))              NHWC fp16 (not for flow_conv1)
 * Loss-scale state (device, 4 x 32 bit): {float scale, float inv_scale, uint overflow, uint good_steps}. Every kernel below reads the
 * scale from it; a non-finite dz / dW / db sets `overflow` (a non-finite d shows up in the dz it feeds). */

/* dz (B,H,W,C NHWC fp16; may be d) and db (C fp32) of one layer: e = [d (NHWC fp16)] + [S·add (NCHW fp32)] (at least one of them),
 * dz = q(lrelu'(y)·e) with y the layer's stored NHWC fp16 output, db = Σ dz · inv_scale. C % 64 == 0. Deterministic (fixed slices,
 * fixed-order sums). */
int deepim_lrelu_bias_backward_f16(deepim_ctx* ctx, void* dz_nhwc_f16, float* db, const void* d_nhwc_f16, const float* add_nchw,
                                   const void* y_nhwc_f16, unsigned* state, float slope, int B, int C, int H, int W);
/* Weight gradient of a conv layer (Cout, Cin, k, k; stride, pad) from its NHWC fp16 input x (B,H,W,Cin_pad; channels >= Cin zero)
 * and dz (B,Ho,Wo,Cout): a GEMM with M = Cout, N = k*k*Cin_pad, K = B*Ho*Wo on v_mfma_f32_32x32x16_f16 (LDS-staged, operands read
 * with ds_read_b64_tr_b16). Fixed split-K slices, fixed-order second pass; the epilogue multiplies by inv_scale, raises the
 * overflow word on a non-finite value and writes the Cin real channels only: layout 0 = natural (Cout,Cin,k,k), 1 = tap-major
 * (Cout,k*k,Cin), the layout deepim_sgd_mom_update_multi reads with layout word Cin | k*k << 32. Cin_pad % 8 == 0, Cout % 8 == 0. */
int deepim_conv2d_wgrad_f16(deepim_ctx* ctx, float* dw, const void* x_nhwc_f16, const void* dz_nhwc_f16, unsigned* state, int B, int Cin,
                            int Cin_pad, int H, int W, int Cout, int k, int stride, int pad, int layout);
/* fp16 weights of the convolution that is the data gradient of layer (Co_l, Ci_l, k, k), in deepim_conv2d_f16_forward's packed
 * order (Cout = Ci_l, Cin_pad = Co_l, kernel nky x nkx; deepim_conv_f16_packed_size(Ci_l, Co_l, nky, nkx) bytes): tap (a, b) =
 * q(layer tap (ky0 + st (nky-1-a), kx0 + st (nkx-1-b))) — st = 1 with the full kernel: transposed and flipped; st = 2: one output
 * parity class of a stride-2 layer. Co_l % 8 == 0. */
int deepim_conv_f16_pack_dgrad(deepim_ctx* ctx, void* packed, const float* w_layer, int Co_l, int Ci_l, int k, int ky0, int kx0,
                               int st, int nky, int nkx);
/* Data gradient dx (B,Hd,Wd,Ci_l NHWC fp16) = q(conv_transpose(dz, q(w))) of a conv layer (Co_l,Ci_l,k,k; stride 1 or 2, pad) from
 * dz (B,Ho,Wo,Co_l NHWC fp16) and the layer's fp32 weights. Stride 1: deepim_conv_f16_pack_dgrad + deepim_conv2d_f16_forward
 * (slope 1, no bias, pad k-1-pad). Stride 2: the four output parity classes of the un-dilated dz (the ideal multiply-adds, as
 * deepim_conv2d_dgrad_s2), each a stride-1 fp16 convolution into a class buffer whose window is stitched onto its parity positions.
 * ws: deepim_conv_dgrad_f16_workspace_size bytes (packed weights + class buffer). */
size_t deepim_conv_dgrad_f16_workspace_size(int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad);
int deepim_conv2d_dgrad_f16(deepim_ctx* ctx, void* dx_nhwc_f16, const void* dz_nhwc_f16, const float* w_layer, void* ws, int B,
                            int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad);
/* deepim_sgd_mom_update_multi (the same kernel) guarded by the loss-scale state: while its overflow word is set no weight and no
 * momentum moves. Run deepim_amp_scale_update after it. */
int deepim_sgd_mom_update_multi_amp(deepim_ctx* ctx, const unsigned long long* table, int rows, int total_blocks, float lr,
                                    float momentum, float rescale, float clip, const unsigned* amp_state);
/* the loss-scale step after an update: overflow → scale = max(1, scale / 2), good_steps = 0; else good_steps + 1, and at `window`
 * scale = min(2^24, 2 scale), good_steps = 0. inv_scale follows, the overflow word is cleared. */
int deepim_amp_scale_update(deepim_ctx* ctx, unsigned* state, int window);

/* Split-fp16 ("x3") training (TRAIN.X3_CONV): the encoder backward on the fp16 matrix cores at fp32 grade (csrc/train_half.hip,
 * DESIGN.md §8f-4e). split(v, s): hi = f16(clamp(v·s, ±60000)), lo = f16(clamp(v·s) − hi); a product of two pairs is hi·hi + hi·lo +
 * lo·hi with fp32 accumulation. S = the gradient scale (a power of two), the stored activations y_l are split16 at scale 16:
 *   e_l   S·(fc6 data gradient + d_dec61) at conv6_1; d_l [+ S·skip_l] below
 *   dz_l  = split(lrelu'(y_l)·e_l, 1), lrelu' from the sign of y_l's hi half          split16 NHWC
 *   db_l  = Σ dz_l / S                                                                 fp32 sums in a fixed order
 *   dW_l  = Σ_pix dz_l ⊗ im2col(y_{l-1}) / (16·S)                                      fp32 result
 *   d_l-1 = split(conv_transpose(dz_l, split(w_l, s_w)) / s_w, 1)                      split16 NHWC (not for flow_conv1)
 * The scale state is the fp16 mode's {float scale, float inv_scale, uint overflow, uint good_steps}, updated by
 * deepim_sgd_mom_update_multi_amp / deepim_amp_scale_update. A clamp in any split of the backward, or a non-finite value, sets
 * `overflow`; underflow is not detected (a scaled maximum below about 2^-4 degrades towards fp16 grade). No call syncs the host. */

/* dz (B,H,W,2C split16; may be d) and db (C fp32) of one layer: e = [d (split16, hi + lo)] + [S·add (NCHW fp32)] (at least one of
 * them), dz = split(lrelu'(y)·e, 1) with y the layer's stored split16 output, db = Σ (dz.hi + dz.lo) · inv_scale. C % 64 == 0.
 * Deterministic (fixed slices, fixed-order sums); the arguments of deepim_lrelu_bias_backward_f16. */
int deepim_lrelu_bias_backward_x3(deepim_ctx* ctx, void* dz_split16, float* db, const void* d_split16, const float* add_nchw,
                                  const void* y_split16, unsigned* state, float slope, int B, int C, int H, int W);
/* Weight gradient of a conv layer (Cout, Cin, k, k; stride, pad) from its split16 input x (B,H,W,2 Cin; stored at x_scale) and the
 * split16 dz (B,Ho,Wo,2 Cout): a GEMM with M = Cout, N = k*k*Cin, K = B*Ho*Wo, three v_mfma_f32_32x32x16_f16 per fragment pair
 * (LDS-staged, operands read with ds_read_b64_tr_b16). Fixed split-K slices, fixed-order second pass; the epilogue multiplies by
 * inv_scale / x_scale and raises the overflow word on a non-finite value. layout 0 = natural (Cout,Cin,k,k), 1 = tap-major
 * (Cout,k*k,Cin), as deepim_conv2d_wgrad_f16. Cin % 16 == 0, Cout % 16 == 0 (whole records). */
int deepim_conv2d_wgrad_x3(deepim_ctx* ctx, float* dw, const void* x_split16, const void* dz_split16, unsigned* state, int B, int Cin,
                           int H, int W, int Cout, int k, int stride, int pad, int layout, float x_scale);
/* The launch plan deepim_conv2d_wgrad_f16 (x3 = 0) or deepim_conv2d_wgrad_x3 (x3 = 1, Cin_pad = Cin there) gives a geometry. Host
 * arithmetic from the geometry alone, no context and no device work; the launcher reads the same plan. plan[0..5] = m-tiles (128
 * output channels each), n-tiles (128 GEMM columns of k*k*Cin_pad each), k-steps (32 pixels each), S (split-K slices, 1 = direct
 * store), steps_per_split (the last slice may be shorter), 1 if B*Ho*Wo % 32 != 0 (a ragged last k-step) else 0. Geometries the
 * entry point of the mode refuses return non-zero here too, and leave plan at -1. */
int deepim_conv_wgrad_half_plan(int x3, int B, int Cin_pad, int H, int W, int Cout, int k, int stride, int pad, int* plan /*6, host*/);
/* Split-fp16 weights of the convolution that is the data gradient of layer (Co_l, Ci_l, k, k), in deepim_conv2d_x3_forward's packed
 * order (Cout = Ci_l, Cin = Co_l, kernel nky x nkx; deepim_conv_x3_packed_size(Ci_l, Co_l, nky, nkx) bytes): tap (a, b) =
 * split(layer tap (ky0 + st (nky-1-a), kx0 + st (nkx-1-b)), w_scale). With st = 1 and the full kernel it equals
 * deepim_conv_x3_pack_weights of the transposed, flipped weights bit for bit; st = 2: one output parity class of a stride-2 layer.
 * A weight that w_scale does not hold (|w·w_scale| > 60000) is clamped and sets the overflow word of `state`.
 * Co_l % 32 == 0, Ci_l % 128 == 0. */
int deepim_conv_x3_pack_dgrad(deepim_ctx* ctx, void* packed, const float* w_layer, unsigned* state, int Co_l, int Ci_l, int k, int ky0,
                              int kx0, int st, int nky, int nkx, float w_scale);
/* Data gradient dx (B,Hd,Wd,2 Ci_l split16 at scale 1) = split(conv_transpose(dz, split(w, w_scale)) / w_scale, 1) of a conv layer
 * (Co_l,Ci_l,k,k; stride 1 or 2, pad) from the split16 dz (B,Ho,Wo,2 Co_l) and the layer's fp32 weights. Stride 1:
 * deepim_conv_x3_pack_dgrad + deepim_conv2d_x3_forward (slope 1, no bias, pad k-1-pad). Stride 2: the four output parity classes
 * of the un-dilated dz, each a stride-1 x3 convolution into a class buffer whose window is stitched onto its parity positions, as
 * deepim_conv2d_dgrad_f16. A clamp of dx sets the overflow word of `state` (through deepim_x3_status_to_state).
 * ws: deepim_conv_dgrad_x3_workspace_size bytes (packed weights + class buffer). Co_l % 32 == 0, Ci_l % 128 == 0. */
size_t deepim_conv_dgrad_x3_workspace_size(int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad);
int deepim_conv2d_dgrad_x3(deepim_ctx* ctx, void* dx_split16, const void* dz_split16, const float* w_layer, void* ws, unsigned* state,
                           int B, int Ci_l, int Hd, int Wd, int Co_l, int k, int stride, int pad, float w_scale);
/* The split-fp16 kernels report a clamp through bit 3 of the context's status word. This moves the bit into the overflow word of
 * `state` on the device and clears it in the status word (the scale state carries it from there on). */
int deepim_x3_status_to_state(deepim_ctx* ctx, unsigned* state);
/* deepim_split16_to_nchw_f32 with the device scale taken out as well: out = (hi + lo) · inv_scale · state.inv_scale. Feeds the
 * fp32 kernels that take the two shapes the x3 kernels do not (conv1's weight gradient). */
int deepim_split16_to_nchw_f32_unscaled(deepim_ctx* ctx, float* out, const void* in_split16, const unsigned* state, int B, int C, int H,
                                        int W, float inv_scale);
/* A weight tensor (n floats) against the scale its x3 pack uses: |w·w_scale| > 60000 (where the pack clamps) or a NaN sets the
 * overflow word of `state`, so the step that would run on clamped weights is skipped and reported. */
int deepim_x3_weight_range_check(deepim_ctx* ctx, const float* w, long n, float w_scale, unsigned* state);

/* ------------------------------------- R-group: re-render between iterations -- */
/* Replaces Render_Py.render (lib/render_glumpy/render_py_multi.py:101-129: OpenGL draw + glReadPixels +
 * depth linearisation) and the tensor packing that follows it in the batch updater
 * (lib/pair_matching/batch_updater_py_multi.py:117-133) for a whole batch of poses of ONE mesh, on the device.
 * Camera model of :132-147 (a pixel is covered when its index lies inside the triangle projected with K),
 * GL_LESS depth test, no culling, fragments outside (zNear, zFar) dropped; triangles with a vertex at or behind
 * zNear are dropped whole instead of clipped.
 *   image  (B,3,H,W) device: RGB − pixel_means (pixel_means_host in tensor channel order, NULL = 0); background = −means
 *   depth  (B,1,H,W) device: metric z, 0 = background
 *   vertices (V,3) device, model frame; faces (F,3) int32 device; poses (B,3,4) device [R|t]
 *   texture != NULL: (tex_h,tex_w,3) device, values on the 0..255 scale, row 0 ↔ v = 0, sampled GL_LINEAR/clamp;
 *                    vertex_attr = (V,2) uv.   texture == NULL: vertex_attr = (V,3) RGB on the 0..255 scale.
 *   K_host: 9 floats, row-major intrinsics. */
int deepim_render_forward(deepim_ctx* ctx, float* image, float* depth, const float* vertices,
                          const float* vertex_attr, const int32_t* faces, const float* texture,
                          int tex_h, int tex_w, const float* poses, const float* K_host /*or NULL: camera table*/,
                          const float* pixel_means_host, int V, int F, int B, int H, int W, float znear,
                          float zfar);
/* The same draw fused with the rest of the test-loop update (deepim/core/tester.py:437-449,
 * lib/pair_matching/data_pair.py:94-105): also writes mask_rendered = depth > mask_thresh (B,1,H,W) and, when mask_box
 * is not NULL, the box_rendered rectangle of that mask (see deepim_mask_box_forward) — one pass over the frame instead
 * of three. */
int deepim_render_update_forward(deepim_ctx* ctx, float* image, float* depth, float* mask_rendered,
                                 float* mask_box /*or NULL*/, float mask_thresh, const float* vertices,
                                 const float* vertex_attr, const int32_t* faces, const float* texture,
                                 int tex_h, int tex_w, const float* poses, const float* K_host /*or NULL: camera table*/,
                                 const float* pixel_means_host, int V, int F, int B, int H, int W,
                                 float znear, float zfar);
/* The draw of the ModelNet loops (BASELINE config 5): lib/render_glumpy/render_py_light_modelnet_multi.py:36-80,170-188 — the
 * same rasterisation with the per-fragment diffuse term of its shader, in OpenGL camera coordinates (y, z of the pose flipped):
 *   brightness = clamp(n·(L − p) / (|n|·|L − p|), 0, 1),  colour = texture·((1 − r) + r·brightness)·intensity,
 *   read back as round(clamp(colour, 0, 1)·255) (the reference reads uint8, :162-166);  p, n = the fragment's interpolated
 *   position / normal under the pose;  L = light_offset + (t_x, −t_y, −t_z) of the sample's pose, as the render closures of
 *   deepim/core/tester.py:146-172 and lib/pair_matching/batch_updater_py_multi.py:185-228 set it (offset 0.5·(0,1,1)).
 * normals (V,3) device; light_offset_host 3 floats; light_intensity (B,3) device or NULL (= 1,1,1; the reference draws
 * U(0.9,1.1) per sample); brightness_ratio r (0.7 there). mask_rendered / mask_box may be NULL (see deepim_render_update_forward).
 * OpenGL itself cannot run here: restated, PARITY UNPINNED like the unlit draw (tests: oracle/render.py). */
int deepim_render_lit_forward(deepim_ctx* ctx, float* image, float* depth, float* mask_rendered /*or NULL*/,
                              float* mask_box /*or NULL*/, float mask_thresh, const float* vertices,
                              const float* vertex_attr, const float* normals, const int32_t* faces, const float* texture,
                              int tex_h, int tex_w, const float* poses, const float* K_host /*or NULL: camera table*/, const float* pixel_means_host,
                              const float* light_offset_host, const float* light_intensity /*device (B,3) or NULL*/,
                              float brightness_ratio, int V, int F, int B, int H, int W, float znear, float zfar);
/* The three draws above for a batch whose samples belong to DIFFERENT meshes (BASELINE config 3: all 13 LINEMOD objects in one
 * batch), in one launch group: sample b draws the mesh of class_index[b]. The class ids live on the device and the host never
 * reads them, so a captured graph of the draw replays for any later batch's objects. The meshes are one table of plain device
 * arrays:
 *   vertices    (ΣV,3)  every mesh's positions, back to back
 *   vertex_attr         every mesh's own (V,2) uv or (V,3) RGB block, back to back
 *   normals     (ΣV,3)  or NULL. NULL = the unlit draw (light_offset_host and light_intensity must be NULL too); otherwise the
 *                       lit draw of deepim_render_lit_forward (light_offset_host required, brightness_ratio in [0, 1])
 *   faces       (ΣF,3)  int32, indices LOCAL to their mesh
 *   textures            every textured mesh's (h,w,3) block, back to back; NULL when no mesh is textured
 *   mesh_desc   (n_classes,8) int32 device, one row per class:
 *               {v_off, V, f_off, F, attr_off (floats into vertex_attr), tex_off (floats into textures, −1 = vertex colours),
 *                tex_h, tex_w};  v_off / f_off count vertices / faces
 *   max_V, max_F        the largest V and F of the table (> 0): grids (ceil(max_V/256), B) and (ceil(max_F/256), B), scratch of
 *                       B × max_V projected vertices; a row's V / F beyond them is clipped
 * mask_rendered / mask_box may be NULL as in deepim_render_update_forward (mask_box needs mask_rendered, B <= 4096). The
 * per-sample arithmetic is that of the single-mesh entries: a sample renders bit-identically whichever entry drew it.
 * Since the host never sees the ids a bad one cannot be reported: a sample whose id is outside [0, n_classes) is drawn as an
 * EMPTY FRAME (image = −means, depth = 0, mask_rendered = 0, mask_box = what an empty mask gives: zeros and status bit 2 of
 * deepim_zoom_status) and no memory outside the table is read. The table's own contents (offsets, face indices) are the
 * caller's to get right: Render_Py's packer checks them on the host. */
int deepim_render_classes_forward(deepim_ctx* ctx, float* image, float* depth, float* mask_rendered /*or NULL*/,
                                  float* mask_box /*or NULL*/, float mask_thresh, const int32_t* class_index /*device (B)*/,
                                  const int32_t* mesh_desc /*device (n_classes,8)*/, int n_classes, int max_V, int max_F,
                                  const float* vertices, const float* vertex_attr, const float* normals /*or NULL*/,
                                  const int32_t* faces, const float* textures /*or NULL*/, const float* poses,
                                  const float* K_host /*or NULL: camera table*/, const float* pixel_means_host, const float* light_offset_host /*or NULL*/,
                                  const float* light_intensity /*device (B,3) or NULL*/, float brightness_ratio, int B, int H,
                                  int W, float znear, float zfar);
/* The lit mesh-table draw of deepim_render_classes_forward for SYNTHETIC OBSERVED FRAMES (toolkit/LM6d_ds_1_gen_observed.py:
 * 116-159): every sample has its own light, and the result is written as the decoded frames the I-group entries below read, not
 * as network tensors. The same project and raster passes; the resolve pass differs in two ways:
 *   light    light_offset (B,3), light_intensity (B,3), brightness_ratio (B): DEVICE float arrays, one row per sample (what
 *            deepim_sample_lights draws). The per-pixel arithmetic is that of the lit draw: sample b has the levels
 *            deepim_render_classes_forward gives with B = 1, its own offset / intensity / ratio and pixel_means NULL.
 *   outputs  image (N,H,W,3) uint8 BGR = the lit level rint(clamp(colour) 255), 0 on the background
 *            depth (N,H,W) uint16 = (uint16)(depth * depth_factor): the float32 product truncated (:156); zfar * depth_factor
 *                  must stay below 65536
 *            label (N,H,W) uint8 = label_value[b] (device int32 (B), NULL = 1; its low byte) where depth != 0, else 0 (:151-153)
 *   rows     device int32 (B) or NULL = the identity: sample b is written to row rows[b] of the three outputs, N >= B rows.
 *            Rows not named are not touched; a sample whose row is outside [0, N) is not written. Two samples naming one row
 *            race. The loader places its synthetic frames among the real ones of a batch this way.
 * normals is required (the draw is lit). A lane stores four consecutive pixels with dword stores when H*W % 4 == 0 and the three
 * outputs are 8-byte aligned, single pixels otherwise: the bytes are the same. A class id outside [0, n_classes) gives an empty
 * frame (zeros). Asynchronous, allocates like the other draws (scratch and z-buffer grow outside a capture only). */
int deepim_render_observed_forward(deepim_ctx* ctx, uint8_t* image /*N,H,W,3*/, uint16_t* depth /*N,H,W*/, uint8_t* label /*N,H,W*/,
                                   const int32_t* rows /*device (B) or NULL*/, int N, const int32_t* label_value /*device (B) or NULL*/,
                                   float depth_factor, const int32_t* class_index /*device (B)*/,
                                   const int32_t* mesh_desc /*device (n_classes,8)*/, int n_classes, int max_V, int max_F,
                                   const float* vertices, const float* vertex_attr, const float* normals, const int32_t* faces,
                                   const float* textures /*or NULL*/, const float* poses, const float* K_host /*or NULL: camera table*/,
                                   const float* light_offset /*device (B,3)*/, const float* light_intensity /*device (B,3)*/,
                                   const float* brightness_ratio /*device (B)*/, int B, int H, int W, float znear, float zfar);
/* The UNLIT mesh-table draw of deepim_render_classes_forward (normals NULL) for the INITIAL POSES OF THE TEST PHASE
 * (toolkit/LM6d_3_gen_PoseCNN_pred_rendered.py:149-155 writes them to disk once), stored the way deepim_render_observed_forward
 * stores: rows of decoded frames, not tensors. The same project and raster passes, K_host or NULL = the bound camera table, an
 * id outside [0, n_classes) = an empty frame; rows, N, the out-of-range-row rule, the two store paths and the z-buffer left
 * all-ones are those of the observed entry. The outputs:
 *   image    (N,H,W,3) uint8 BGR = rint(clamp(level, 0, 255)) of the unlit level deepim_render_classes_forward gives with
 *            pixel_means NULL: cv2.imwrite of the float image saturates and rounds to nearest even. 0 on the background
 *   depth    (N,H,W) uint16 = (uint16)(depth * depth_factor), the float32 product truncated (:151); zfar * depth_factor must
 *            stay below 65536 (a host error before any launch)
 *   label    (N,H,W) uint8 as in the observed entry, or NULL: not stored
 *   covered  device int32 (B) or NULL: covered[b] = the number of pixels of sample b whose stored uint16 depth is non-zero,
 *            whether or not the sample's row is stored. The call WRITES it (it is zeroed on the stream first and never
 *            accumulates across calls): one atomic add per wave of the resolve pass. It is what np.sum(depth_rendered) == 0 of
 *            lib/utils/image.py:301-303 asks, kept on the device for deepim_mask_gate; the host never reads it.
 * B <= 65535, H*W < 2^31. Asynchronous, allocates like the other draws (scratch and z-buffer grow outside a capture only). */
int deepim_render_frames_forward(deepim_ctx* ctx, uint8_t* image /*N,H,W,3*/, uint16_t* depth /*N,H,W*/, uint8_t* label /*N,H,W or NULL*/,
                                 int32_t* covered /*device (B) or NULL*/, const int32_t* rows /*device (B) or NULL*/, int N,
                                 const int32_t* label_value /*device (B) or NULL*/, float depth_factor,
                                 const int32_t* class_index /*device (B)*/, const int32_t* mesh_desc /*device (n_classes,8)*/,
                                 int n_classes, int max_V, int max_F, const float* vertices, const float* vertex_attr,
                                 const int32_t* faces, const float* textures /*or NULL*/, const float* poses,
                                 const float* K_host /*or NULL: camera table*/, int B, int H, int W, float znear, float zfar);

/* The lit mesh-table draw of deepim_render_observed_forward for a SCENE: S slots (1..8) per frame share one z-buffer plane, so
 * that objects hide one another. Ours: the reference has no generator for occluded scenes. Sample d = f S + s (frame f < B,
 * slot s < S) has its own class_index[d], poses[d] and label_value[d] (NULL = s + 1); a class id outside the table is an empty
 * slot. The light is per FRAME, light_offset (B,3), light_intensity (B,3), brightness_ratio (B), moved to each slot's own pose as
 * lib/render_glumpy/render_py_light_multi_program.py:370-396 lights the objects of a scene: slot s is shaded exactly as the
 * observed entry shades a sample with that light and the slot's pose, L = offset + (t_x, -t_y, -t_z).
 *   key      float_bits(Z) << 32 | s << 24 | triangle (max_F <= 2^24). Within a slot the winner is the single-object draw's;
 *            between slots the nearer fragment wins and an exact depth tie goes to the LOWER slot.
 *   outputs  row rows[f] (device int32 (B), NULL = f) of image / depth / label (N rows), stored as the observed entry stores
 *            them, four pixels per lane or one; label = the winning slot's label value where depth != 0. Rows not named are not
 *            touched and a frame whose row is outside [0, N) is not written (its pixels are still counted).
 *   visible  device int32 (B,S) or NULL: visible[f,s] = the pixels of frame f won by slot s with a non-zero stored depth. The call
 *            WRITES it (zeroed on the stream first). With S = 1 it is what covered is in deepim_render_frames_forward.
 * With S = 1 the three outputs are the bytes of deepim_render_observed_forward. The z-buffer holds B planes and leaves the call
 * all-ones; the projected-vertex scratch is B S x max_V records. Host errors before any launch: S outside 1..8, B S > 65535,
 * max_F > 2^24, zfar * depth_factor >= 65536, K_host NULL (the bound camera table is per pair, not per slot). Asynchronous,
 * allocates like the other draws (scratch and z-buffer grow outside a capture only). */
int deepim_render_scene_forward(deepim_ctx* ctx, uint8_t* image /*N,H,W,3*/, uint16_t* depth /*N,H,W*/, uint8_t* label /*N,H,W*/,
                                int32_t* visible /*device (B,S) or NULL*/, const int32_t* rows /*device (B) or NULL*/, int N,
                                const int32_t* label_value /*device (B,S) or NULL*/, float depth_factor,
                                const int32_t* class_index /*device (B,S)*/, const int32_t* mesh_desc /*device (n_classes,8)*/,
                                int n_classes, int max_V, int max_F, const float* vertices, const float* vertex_attr,
                                const float* normals, const int32_t* faces, const float* textures /*or NULL*/,
                                const float* poses /*device (B,S,3,4)*/, const float* K_host, const float* light_offset /*device (B,3)*/,
                                const float* light_intensity /*device (B,3)*/, const float* brightness_ratio /*device (B)*/, int B,
                                int S, int H, int W, float znear, float zfar);

/* ------------------------------------------- I-group: ingest of decoded frames -- */
/* csrc/ingest.hip. What lib/utils/image.py does on the host between cv2.imread and the tensors of a batch, on frames that
 * are already on the device as the camera / decoder left them (uint8 / uint16): 1 or 2 bytes per value cross PCIe, not 4.
 * All four run on the context's stream, are asynchronous, allocate nothing and are legal inside deepim_graph_begin/end.
 * Per-sample ids and draws are device int32 arrays the host never reads, so a captured graph follows what they hold at replay.
 *
 * `transform` (image.py:583-594) for a batch: frames (B,H,W,3) uint8 in BGR order (cv2.imread), out (B,3,H,W) fp32,
 *   out[b,i,y,x] = float(frames[b,y,x,2-i]) - means_rgb[i]      (one fp32 subtraction)
 * means_rgb: 3 HOST floats in tensor-channel order (Render_Py's pixel_means), NULL = zeros. bg_frames (B,H,W,3) and
 * fg_labels (B,H,W) uint8, both or neither: the data_syn / REPLACE_OBSERVED_BG_RATIO composite of image.py:147-155 — where
 * fg_labels == 0 the pixel comes from bg_frames (the reference tests != 0, not == mask_idx), for the samples with
 * use_bg[b] != 0; use_bg NULL = every sample. The background is already cropped and resized to H x W. */
int deepim_ingest_bgr8(deepim_ctx* ctx, float* out /*B,3,H,W*/, const uint8_t* frames /*B,H,W,3*/,
                       const uint8_t* bg_frames /*B,H,W,3 or NULL*/, const uint8_t* fg_labels /*B,H,W or NULL*/,
                       const int32_t* use_bg /*device (B) or NULL*/, const float* means_rgb /*host 3 or NULL*/, int B, int H,
                       int W);
/* deepim_ingest_bgr8 with the background of image.py:108-145 made on the fly from a POOL of decoded images that is uploaded
 * once (lib/utils/background.BackgroundPool): the top-left crop to the frame's aspect ratio (:119-141), cv2.resize's 8-bit
 * INTER_LINEAR resample (:143) and the paste at the top-left corner of a black frame (:118,145) happen inside the composite, and
 * no resized background exists in memory. Everything that depends only on an image's size and the frame's is a table:
 *   pool_pixels  the images' (bh,bw,3) uint8 BGR pixels back to back, 4-byte aligned, every image's start too, with 12 readable
 *                bytes behind the last image (the taps are read as aligned 12-byte windows)
 *   pool_desc    (P,4) int64: the image's byte offset in pool_pixels, its row stride in bytes, oh, ow = the size of its
 *                resized crop (oh <= H, ow <= W)
 *   xtab, ytab   (P,W) / (P,H) int32: per output column x0, x1, a0, a1, per output row y0, y1, b0, b1 — the two source indices
 *                inside the crop and their 11-bit weights — packed as i0 << 13 | (i1 != i0) << 12 | w1: i1 is i0 or i0 + 1 and
 *                w0 = 2048 - w1 (an image side < 2^19); zeros from ow / oh on
 * A pixel of pair b with fg_labels != 0, or of a pair with use_bg[b] == 0 (NULL: every pair composites), is the frame's. The
 * others are, per channel, with P the image bg_index[b], for y < oh and x < ow
 *   r0 = P[y0][x0] a0 + P[y0][x1] a1        r1 = P[y1][x0] a0 + P[y1][x1] a1
 *   v  = clamp((((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2, 0, 255)
 * and 0 outside. Then the channel swap and the fp32 subtraction of deepim_ingest_bgr8: the output has the bits
 * deepim_ingest_bgr8 gives from the same frames with a bg_frames holding the resampled, padded images. Lanes without a
 * label-0 pixel read nothing of the pool; no LDS, nothing allocated, legal inside a graph capture. H*W < 2^31.
 * Since the host never sees the draws a bad one cannot be reported: a compositing pair whose bg_index is outside [0, P) reads
 * nothing outside the pool, gets a black background and sets bit 5 (32) of the status word (deepim_zoom_status); the other
 * pairs are unaffected. The tables' own contents are the caller's to get right: BackgroundPool builds and checks them on the host. */
int deepim_ingest_bgr8_pool(deepim_ctx* ctx, float* out /*B,3,H,W*/, const uint8_t* frames /*B,H,W,3*/,
                            const uint8_t* fg_labels /*B,H,W*/, const int32_t* use_bg /*device (B) or NULL*/,
                            const int32_t* bg_index /*device (B)*/, const uint8_t* pool_pixels, const int64_t* pool_desc,
                            const int32_t* xtab /*P,W*/, const int32_t* ytab /*P,H*/, int P,
                            const float* means_rgb /*host 3 or NULL*/, int B, int H, int W);
/* image.py:178-181, :203-219: out[b,0,y,x] = float(depth[b,y,x]) / depth_factor, a correctly rounded fp32 division as numpy's.
 * labels (B,H,W) uint8 and mask_idx (B), both or neither: the value is 0 where labels != mask_idx[b] (image.py:211,
 * tester.py:556). */
int deepim_ingest_depth16(deepim_ctx* ctx, float* out /*B,1,H,W*/, const uint16_t* depth /*B,H,W*/,
                          const uint8_t* labels /*B,H,W or NULL*/, const int32_t* mask_idx /*device (B) or NULL*/,
                          float depth_factor, int B, int H, int W);
/* image.py:255-260, :308-312: out[b,0,y,x] = labels[b,y,x] == mask_idx[b] ? 1 : 0 */
int deepim_ingest_label_mask(deepim_ctx* ctx, float* out /*B,1,H,W*/, const uint8_t* labels /*B,H,W*/,
                             const int32_t* mask_idx /*device (B)*/, int B, int H, int W);
/* The two maps above for a batch whose pairs look at SHARED frames: depth / labels are (N,H,W) and pair b reads frame
 * frame_index[b] (device int32 (B), never read by the host) instead of sample b; out is still (B,1,H,W) fp32 with the bits the
 * per-sample entries give on depth[frame_index] / labels[frame_index]. mask_idx stays per pair. N >= 1. A pair whose
 * frame_index is outside [0, N) reads nothing outside the frames, gets an all-zero plane and sets bit 4 (16) of the status
 * word (deepim_zoom_status); the other pairs are unaffected. */
int deepim_ingest_depth16_frames(deepim_ctx* ctx, float* out /*B,1,H,W*/, const uint16_t* depth /*N,H,W*/,
                                 const uint8_t* labels /*N,H,W or NULL*/, const int32_t* frame_index /*device (B)*/,
                                 const int32_t* mask_idx /*device (B) or NULL*/, float depth_factor, int N, int B, int H,
                                 int W);
int deepim_ingest_label_mask_frames(deepim_ctx* ctx, float* out /*B,1,H,W*/, const uint8_t* labels /*N,H,W*/,
                                    const int32_t* frame_index /*device (B)*/, const int32_t* mask_idx /*device (B)*/, int N,
                                    int B, int H, int W);
/* deepim_ingest_bgr8 (without a ready-made background) and deepim_ingest_bgr8_pool for frames read THROUGH AN INDEX: frames is
 * (N,H,W,3), fg_labels (N,H,W), and pair b reads frame frame_index[b] of both; use_bg and bg_index stay per pair. N may be a
 * whole device-resident dataset (core/resident.ResidentObserved): every offset into the arrays is 64-bit. out has the bits the
 * per-sample entry gives on frames[frame_index] (and fg_labels[frame_index]). A pair whose index is outside [0, N) reads
 * nothing outside the arrays, gets the empty-frame value (0 - mean) in all three planes, composites no background and sets
 * bit 4 (16) of the status word; the other pairs are unaffected. No LDS, nothing allocated, legal inside a capture; the host
 * never reads frame_index. The 12-byte loads need a dword-aligned base and H*W % 4 == 0 (frame f starts at byte 3 H W f);
 * otherwise every pixel is read on its own, each from its own pair's frame. */
int deepim_ingest_bgr8_frames(deepim_ctx* ctx, float* out /*B,3,H,W*/, const uint8_t* frames /*N,H,W,3*/,
                              const int32_t* frame_index /*device (B)*/, int N, const float* means_rgb /*host 3 or NULL*/,
                              int B, int H, int W);
int deepim_ingest_bgr8_pool_frames(deepim_ctx* ctx, float* out /*B,3,H,W*/, const uint8_t* frames /*N,H,W,3*/,
                                   const uint8_t* fg_labels /*N,H,W*/, const int32_t* frame_index /*device (B)*/, int N,
                                   const int32_t* use_bg /*device (B) or NULL*/, const int32_t* bg_index /*device (B)*/,
                                   const uint8_t* pool_pixels, const int64_t* pool_desc, const int32_t* xtab /*P,W*/,
                                   const int32_t* ytab /*P,H*/, int P, const float* means_rgb /*host 3 or NULL*/, int B, int H,
                                   int W);
/* out[b] = table[index[b]] for b < B: rows of row_words 4-byte words (any type), table of n_rows rows, index device int32 (B)
 * the host never reads. One lane per 16 bytes when row_words % 4 == 0 and out and table are 16-byte aligned, else per word;
 * every pointer 4-byte aligned, out != table. An index outside [0, n_rows) reads nothing, gives a zero row and sets bit 4 (16)
 * of the status word. The table offset is 64-bit (rows may be whole frames of a resident set). Asynchronous, allocates
 * nothing, legal inside a capture. */
int deepim_gather_rows(deepim_ctx* ctx, void* out, const void* table, const int32_t* index /*device (B)*/, int n_rows,
                       long row_words, int B);
/* lib/utils/mask_dilate.py:19-47 with the random draws handed in: thickness (B,4) int32, columns in the order of the file's
 * four blocks — the origin mask shifted down (:24), up (:30), right (:36), left (:42) by that many pixels; 0 = that side is
 * not dilated. Where mask != 0 the output is mask, clamped to 1 where it exceeds 1; elsewhere 1 if an enabled side has a
 * non-zero origin pixel exactly its thickness away, else 0. A thickness >= H (or W) contributes nothing (empty slices).
 * out == mask is refused: the gather cannot run in place. */
int deepim_mask_dilate(deepim_ctx* ctx, float* out /*B,1,H,W*/, const float* mask /*B,1,H,W*/,
                       const int32_t* thickness /*device (B,4)*/, int B, int H, int W);
/* lib/utils/image.py:301-303 (test phase) for a batch, in place: the planes mask[b] of the samples with covered[b] == 0 (what
 * deepim_render_frames_forward counted: an empty initial render) become zero, whatever TEST.INIT_MASK made them; the other
 * planes are neither read nor written. Asynchronous, allocates nothing, legal inside a capture. B <= 65535. */
int deepim_mask_gate(deepim_ctx* ctx, float* mask /*B,1,H,W, in place*/, const int32_t* covered /*device (B)*/, int B, int H, int W);

/* ------------------------------------------------ training metrics (csrc/metric.hip) -- */
/* The sums the reference's metrics take on the host once per batch (deepim/core/metric.py:51-137), as one fused reduction.
 * Slot order: 0 flow_loss, 1 rot_loss, 2 trans_loss, 3 point_matching_loss, 4 mask. Slots 0-3 are the plain sum of the tensor's
 * n floats; slot 4 is the sum over n_mask pixels of -(g*log(p + 1e-19) + (1 - g)*log(1 - p + 1e-19)) (:135) with p = mask_prob,
 * g = mask_gt, every operation of the element in float32 as numpy evaluates it on float32 inputs (p == 1 gives log(1e-19f)),
 * logf on the device. Every accumulation is in double. step (5 doubles or NULL) is overwritten with the sums of this call;
 * totals (5 doubles or NULL) receives totals[s] += step[s]. A NULL tensor leaves its slot of totals untouched and writes 0 into
 * step; mask_prob and mask_gt are both NULL or both set; n == 0 is legal. The tensors need only be 4-byte aligned. Partials are
 * combined in a fixed order without atomics: the same inputs give the same bytes. Asynchronous on the context's stream, never
 * synchronises the host, two launches whatever the sizes; scratch grows on a first call only, outside a capture; legal inside
 * deepim_graph_begin/end after one eager call. */
int deepim_train_metrics(deepim_ctx* ctx, double* totals /*5, accumulated; or NULL*/, double* step /*5, overwritten; or NULL*/,
                         const float* flow_loss, long n_flow, const float* rot_loss, long n_rot,
                         const float* trans_loss, long n_trans, const float* pm_loss, long n_pm,
                         const float* mask_prob, const float* mask_gt, long n_mask);
/* out[r] = the 2-norm of row r of `table`, a DEVICE array of rows x {pointer to floats (4-byte aligned), count}: the weight-norm
 * line of deepim/core/module.py:1113-1122 without a read-back per parameter. Squares and sums in double, sqrtf of the sum rounded
 * to float; fixed order, no atomics. Asynchronous; scratch (rows x 2 KB) grows outside a capture only. rows <= 65535. */
int deepim_l2_norms_multi(deepim_ctx* ctx, float* out /*rows*/, const uint64_t* table /*rows x {ptr, count}*/, int rows);

/* ------------------------------------------ R-group: the loader's random draws (csrc/sample.hip) -- */
/* A counter-based generator, Philox4x32-10, and on top of it the rendered-pose rule of toolkit/LM6d_1_gen_rendered_pose.py:80-107
 * and the draws of lib/utils/mask_dilate.py and of the background replacement (lib/utils/image.py:97-116). Every draw is a pure
 * function of (seed, draw id, attempt, stream):
 *   key     = (seed low word, seed high word)
 *   counter = (draw id low, draw id high, attempt, stream)      streams 0, 1: the two blocks of a pose draw; 2: mask dilate;
 *                                                               3: background; 4, 5: the two blocks of an observed-pose draw;
 *                                                               6: light; 7, 8: the placement and rotation blocks of a
 *                                                               scene's occluders (attempt = the slot)
 * so a pair's draw does not depend on the batch size, its position in the batch or the order of launches. The draw id of pair b
 * is draw_ids[b] where draw_ids (device, B) is given, else draw_base + b (draw_base is not added to given ids).
 * A 32-bit word x becomes the uniform u = (x + 0.5) 2^-32 in double, strictly inside (0,1); six normals come pairwise from the
 * first six of a candidate's eight words by Box-Muller in double, r = sqrt(-2 ln u0), z0 = r cos 2 pi u1, z1 = r sin 2 pi u1
 * (block 0: z0..z3, block 1: z4, z5). A word maps to [0, n) as (uint64(x) n) >> 32: the bias is at most n 2^-32.
 * All entries of this group are asynchronous on the context's stream, allocate nothing and read nothing back. B >= 0.
 *
 * deepim_selfcheck_philox: out[i] = Philox4x32-10(ctr[i], key[i]), the generator alone (known-answer tests). */
int deepim_selfcheck_philox(deepim_ctx* ctx, unsigned int* out /*n,4 dev*/, const unsigned int* ctr /*n,4 dev*/,
                            const unsigned int* key /*n,2 dev*/, int n);
/* One candidate of the rule from GIVEN normals, in double:
 *   tgt_euler = mat2euler(R_src) + z[0:3] angle_std pi/180      tgt_trans = T_src + z[3:6] (x_std, y_std, z_std)
 *   R_tgt = euler2mat(tgt_euler)      r_dist = the angle of R_src^T R_tgt in degrees (atan2 of half the norm of the antisymmetric
 *   part and (trace - 1)/2)           (cx, cy) = the projection of tgt_trans through K
 *   accept iff r_dist <= angle_max and border < cx < width - border and border < cy < height - border and tgt_trans.z > 0
 * (z > 0 is not the toolkit's, which divides by z unguarded). pose_out is the candidate rounded to float, accepted or not;
 * stat_out may be NULL. K: 9 HOST floats; noise: 5 HOST floats, stds >= 0. pose_out must not overlap pose_src. */
int deepim_pose_perturb(deepim_ctx* ctx, float* pose_out /*B,3,4*/, double* stat_out /*B,4: r_dist deg, cx, cy, accept*/,
                        const float* pose_src, const double* normals /*B,6 dev*/, const float* K /*host 3x3*/,
                        const float* noise /*host 5: angle_std deg, angle_max deg, x,y,z std*/, int width, int height,
                        float border, int B);
/* The toolkit's loop with a bound: candidates of attempt 0 .. max_attempts-1 (>= 1) are drawn and tried until one is accepted.
 * Accepted: pose_out = that candidate, attempts[b] = the number of candidates drawn (1 .. max_attempts), normals_out[b] = its
 * normals. None accepted: pose_out = pose_src unchanged, attempts[b] = 0, normals_out[b] = zeros (the toolkit loops for ever). */
int deepim_sample_rendered_poses(deepim_ctx* ctx, float* pose_out /*B,3,4*/, int32_t* attempts /*B dev*/,
                                 double* normals_out /*B,6 or NULL: the accepted draw's*/, const float* pose_src,
                                 const float* K, const float* noise, int width, int height, float border, int max_attempts,
                                 unsigned long long seed, unsigned long long draw_base,
                                 const unsigned long long* draw_ids /*B dev or NULL: draw_base + b*/, int B);
/* lib/utils/mask_dilate.py:19-47's draws for B pairs, as deepim_mask_dilate takes them: word 0 of the stream-2 call with
 * attempt 0 is the direction in [0,10); words 1..3 of that call and word 0 of the call with attempt 1 are the four sides'
 * randint(max_thickness) + 1 (max_thickness >= 1) in the order of the file's four blocks; a side is 0 where the file skips it
 * for the direction. thickness must be 16-byte aligned. */
int deepim_sample_mask_dilate(deepim_ctx* ctx, int32_t* thickness /*B,4 dev*/, int max_thickness, unsigned long long seed,
                              unsigned long long draw_base, const unsigned long long* draw_ids, int B);
/* The background draws of lib/utils/image.py:97-116 for B pairs, as deepim_ingest_bgr8_pool takes them, from the stream-3 call
 * with attempt 0: word 0 as the uniform u stands for the np.random.rand() of :99, word 1 mapped to [0, pool_size) for
 * random.randint's choice of the image (:113):
 *   use_bg[b]   = (always != NULL && always[b] != 0) || u < ratio ? 1 : 0      always: the pairs' data_syn flags (:98)
 *   bg_index[b] = (uint64(word 1) pool_size) >> 32                             drawn for every pair, used or not
 * ratio: TRAIN.REPLACE_OBSERVED_BG_RATIO in [0, 1] (0: never, since u > 0; 1: always, since u < 1); pool_size >= 1. */
int deepim_sample_backgrounds(deepim_ctx* ctx, int32_t* use_bg /*B dev*/, int32_t* bg_index /*B dev*/,
                              const int32_t* always /*B dev or NULL*/, double ratio, int pool_size, unsigned long long seed,
                              unsigned long long draw_base, const unsigned long long* draw_ids, int B);
/* The loader's running counts, kept on the device: totals[0] += B, totals[1] += the sum of attempts, totals[2] += the pairs with
 * attempts == 0 (exhausted). */
int deepim_sample_stats_accumulate(deepim_ctx* ctx, unsigned long long* totals /*3 dev*/, const int32_t* attempts /*B dev*/, int B);
/* Synthetic observed poses: the rule of toolkit/LM6d_ds_0_gen_observed_poses.py:200-250, one thread per pair, in double.
 * table (n_classes,22) double, device, one row per class (lib/pair_matching/pose_sampler.pack_observed_table):
 *   trans_mean[3], trans_std[3], pz_mean[3], angle_max (degrees), fallback pose [12]
 * Candidate a of a draw id: stream 4, attempt a gives four normals (both Box-Muller pairs), stream 5, attempt a three (the first
 * pair and the first normal of the second).
 *   tgt_quat = the first four normalised, negated if w < 0      tgt_trans = trans_mean + z[4:7] trans_std
 *   R = quat2mat(tgt_quat) in RT_transform.quat2mat's expression order
 *   deg = the angle of R e_z to pz_mean as :74-78 (clip, arccos, degrees)      (cx, cy) = the projection of tgt_trans through K
 *   accept iff deg <= angle_max and border < cx < width - border and border < cy < height - border and tgt_trans.z > 0
 * (z > 0 is not the toolkit's, which divides by z unguarded; border is the file's 48 at 640 x 480). The first accepted candidate of
 * attempts 0 .. max_attempts-1 is the pose; attempts[b] = the candidates drawn, normals_out[b] / stat_out[b] (both may be NULL)
 * = its seven normals / deg, cx, cy, 1. None accepted: pose = the class's fallback row, attempts[b] = 0, zeros in normals_out
 * and stat_out (the toolkit loops for ever). class_index[b] outside [0, n_classes): an all-zero pose, attempts[b] = -1, the table
 * is not read; the draws render such a pair as an empty frame. deepim_sample_stats_accumulate adds attempts as they are, so
 * a caller that feeds it keeps -1 out (core/loader.py checks its class ids on the host when it is built). K: 9 HOST floats. */
int deepim_sample_observed_poses(deepim_ctx* ctx, float* pose_out /*B,3,4*/, int32_t* attempts /*B dev*/,
                                 double* normals_out /*B,7 or NULL*/, double* stat_out /*B,4 or NULL*/,
                                 const int32_t* class_index /*B dev*/, const double* table /*n_classes,22 dev*/, int n_classes,
                                 const float* K, int width, int height, float border, int max_attempts, unsigned long long seed,
                                 unsigned long long draw_base, const unsigned long long* draw_ids /*B dev or NULL*/, int B);
/* One candidate of that rule from GIVEN normals (B,7), accepted or not, as deepim_pose_perturb is to the rendered-pose rule:
 * pose_out = the candidate rounded to float, stat_out (or NULL) = deg, cx, cy, accept flag. A class id outside the table: zeros. */
int deepim_observed_pose_candidate(deepim_ctx* ctx, float* pose_out /*B,3,4*/, double* stat_out /*B,4 or NULL*/,
                                   const int32_t* class_index /*B dev*/, const double* table /*n_classes,22 dev*/, int n_classes,
                                   const double* normals /*B,7 dev*/, const float* K, int width, int height, float border, int B);
/* The light of toolkit/LM6d_ds_1_gen_observed.py:116-144 for B frames, as deepim_render_observed_forward takes it; the draw id
 * stands for the frame's running index:
 *   light_offset[b]     = 0.5 x row (draw id mod 6) of [1,0,1], [1,1,1], [0,1,1], [-1,1,1], [-1,0,1], [0,0,1]; the draw adds
 *                         (t_x, -t_y, -t_z) of the sample's pose itself (:133-135)
 *   light_intensity[b]  = colour * (0.9 + 0.2 u[0:3]): stream 6, attempt 0, words 0-2 as uniforms, word 3 mapped to [0, 7) picks
 *                         the colour row of [0,0,1], [0,1,0], [0,1,1], [1,0,0], [1,0,1], [1,1,0], [1,1,1] (:138-141)
 *   brightness_ratio[b] = ratios[k], k = word 0 of stream 6, attempt 1 mapped to [0, n_ratios) (:144)
 * ratios: 1 to 8 HOST floats in [0, 1] (the file's are 0.2, 0.25, 0.3, 0.35, 0.4). All outputs float32, device. */
int deepim_sample_lights(deepim_ctx* ctx, float* light_offset /*B,3*/, float* light_intensity /*B,3*/,
                         float* brightness_ratio /*B*/, const float* ratios /*host*/, int n_ratios, unsigned long long seed,
                         unsigned long long draw_base, const unsigned long long* draw_ids /*B dev or NULL*/, int B);

/* The occluders of a synthetic scene (ours: the reference has no such generator), one thread per pair, in double, rounded to
 * float. Outputs for S = max_occluders + 1 slots: class_out (B,S) int32, pose_out (B,S,3,4), label_value_out (B,S) = s + 1.
 * Slot 0 is the target (target_class[b], target_pose[b]) copied through. Streams 7 and 8 of the pair's draw id:
 *   stream 7, attempt 0, word 0 -> the count n, uniform in [min_occluders, max_occluders] (no draw when max_occluders = 0)
 *   stream 7, attempt s = 1..n: word 0 -> the class, uniform over occluder_classes (it may be the target's); words 1-3 as
 *       uniforms -> rho in [lateral_lo, lateral_hi], phi in [0, 2 pi), tau in [toward_lo, toward_hi];
 *       t = t_target + d (rho cos phi, rho sin phi, -tau), d = diameters[target class] in metres
 *   stream 8, attempt s: four normals -> the unit quaternion, negated if w < 0 -> quat2mat, as stream 4's
 * Slots beyond n, and an occluder with t_z <= 0, are empty: class -1 and a zero pose. occluder_classes: device int32
 * (n_occluder_classes); diameters: device float (n_classes), indexed by class id. 0 <= min <= max <= 7. */
int deepim_sample_occluders(deepim_ctx* ctx, int32_t* class_out /*B,S dev*/, float* pose_out /*B,S,3,4*/,
                            int32_t* label_value_out /*B,S dev*/, const int32_t* target_class /*B dev*/,
                            const float* target_pose /*B,3,4*/, const int32_t* occluder_classes /*dev*/, int n_occluder_classes,
                            const float* diameters /*n_classes dev*/, int n_classes, int min_occluders, int max_occluders,
                            float lateral_lo, float lateral_hi, float toward_lo, float toward_hi, unsigned long long seed,
                            unsigned long long draw_base, const unsigned long long* draw_ids /*B dev or NULL*/, int B);
/* The fallback for a synthetic scene (csrc/ingest.hip), one launch. visible (B,S): deepim_render_scene_forward's counts of the
 * scene; full (B): its counts of the target drawn alone (S = 1). Pair b is KEPT iff full[b] > 0 and (double)visible[b,0] >=
 * (double)min_visible full[b] (lib/utils/mask_augment.py:91-93 falls back below 0.4). With row = rows[b] (device int32, NULL = b)
 * of the batch arrays (N rows) and the alone frames as B compact rows:
 *   always      depth_gt[row] <- the alone depth (the flow labels and point clouds are made from the target alone)
 *   not kept    image[row], label[row] and, where given, depth_observed[row] <- the alone frame's
 * kept (B) int32 is written. totals (3 device uint64, or NULL) += B, the pairs kept, and the slots s >= 1 of slot_class (B,S, or
 * NULL) that hold a class (>= 0). A row outside [0, N) is not written. Allocates nothing; legal inside a capture. */
int deepim_occlusion_gate(deepim_ctx* ctx, uint8_t* image /*N,H,W,3*/, uint16_t* depth_gt /*N,H,W*/, uint8_t* label /*N,H,W*/,
                          uint16_t* depth_observed /*N,H,W or NULL*/, int32_t* kept /*B dev*/, unsigned long long* totals /*3 dev or NULL*/,
                          const int32_t* rows /*B dev or NULL*/, int N, const uint8_t* alone_image /*B,H,W,3*/,
                          const uint16_t* alone_depth /*B,H,W*/, const uint8_t* alone_label /*B,H,W*/, const int32_t* visible /*B,S dev*/,
                          const int32_t* full /*B dev*/, const int32_t* slot_class /*B,S dev or NULL*/, float min_visible, int B, int S,
                          int H, int W);

#ifdef __cplusplus
}
#endif
#endif  /* DEEPIM_HIP_H_ */
