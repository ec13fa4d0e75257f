// The launch plan of the fp32 Winograd kernels of csrc/wino.hip: which block shape runs a layer, on which grid, with which K split or
// stream-K cut — as a function of the options and the layer's geometry only. Plain C++ (no HIP, no pointers, no device calls): the
// launcher (wino_forward_impl), deepim_conv_wino_plan and the deepim_conv_wino_preferred* queries all read it from here.
#pragma once
#include <algorithm>
#include <stddef.h>

#define DI_WINO_COUNTERS 16384   /* arrival counters per context (64 KB): tile blocks of one Winograd launch that can finish in-kernel */

// deepim_set_option's "wino_*" options (deepim_ctx::wino); these initialisers are the defaults of a fresh context and of every query
// made without one
struct WinoOptions {
  int s2d_skip = 1;     // 1: stride-2 Winograd layers skip the positions whose weights are identically zero; 0: all 16 (A/B measurements)
  int shared = 1;       // 1: Winograd layers with Cout % 64 == 0 on the 8-wave shared-transform kernel (conv_wino8_kernel); 0: the round-4 one-wave kernel
  int wide = 1;         // block shape of the shared-transform kernel: 1 = per layer by the work per CU, 0 = 64 ch x 64 tiles, 3 = 128 x 32, 2 = 64 x 32 on four waves (two blocks per CU), 4 = 256 x 32 on nine accumulator tuples (3x3 stride-2 walk, Cout % 256 == 0; elsewhere as 3)
  int split = 0;        // K-split of the shared-transform kernel: 0 = the plan of wino8_split_plan, 1 = never, n = at most n slices
  int streamk = 1;      // 1: where a grid leaves a partly filled last round, the persistent blocks share the work granule by granule (stream-K; needs `persistent`, off with split = 1); 2: wherever it applies, whatever the cost model says; 0: never
  int fin = 0;          // 1: a K-split Winograd layer is finished inside the kernel by the block whose slice arrives last (no second pass); 0: wino_reduce_kernel — the serial finish of the last slices costs more than the parallel second pass at every batch size (profiles/r06_b4_share.md)
  int persistent = 1;   // 1: the shared-transform kernel's grid is one block per resident slot, each walking its share of the tiles; 0: one block per tile block
  int two_wave = 0;     // 0: Winograd layers on the one-wave 16-position kernel; 1: the two-waves-per-SIMD kernel (measured slower on the big layers)
  bool canonical = false;   // the canonical-summation-order configuration ("conv_max_split" = 1): no layer prefers Winograd. Not stored: wino_options() (csrc/wino.hip) fills it from the context where the options are read
};

// The layer as the kernels see it: a 3x3 stride-1 pad-1 problem, or that problem over the space-to-depth input of a stride-2 layer
enum WinoGeom { WINO_3X3 = 0, WINO_S2D_5X5 = 1, WINO_S2D_3X3 = 2 };

// Block shapes. From WINO_64X64 on: the shared-transform kernel's, in the order deepim_conv_wino_plan reports them (plan[0] = shape - WINO_64X64)
enum WinoShape { WINO_ONE_WAVE, WINO_TWO_WAVE, WINO_64X64, WINO_128X32, WINO_64X32_4W, WINO_256X32_NINE, WINO_SHAPES };
struct WinoShapeInfo { int channels, tiles, threads, slots; };   // per block: output channels, 2x2 tiles, threads; resident blocks on the chip's 256 CUs (0: the grid is not persistent)
constexpr WinoShapeInfo WINO_SHAPE[WINO_SHAPES] = {
    {32, 128, 256, 0},     // conv_wino_kernel: four waves of 32 tiles, all of Cin per block
    {32, 64, 256, 0},      // conv_wino2_kernel
    {64, 64, 512, 256},    // conv_wino8_kernel<.., 0>
    {128, 32, 512, 256},   // conv_wino8_kernel<.., 1>
    {64, 32, 256, 512},    // conv_wino4_kernel: two blocks per CU
    {256, 32, 512, 256},   // conv_wino9_kernel
};

struct WinoPlan {
  WinoShape shape;
  int walk;          // K loop: 0 = all 16 positions of every 8-channel block, 1 = the 5x5 stride-2 layers' walk of the four input phases with their zero positions dropped, 2 = the 3x3 stride-2 layers'
  int gx, gy;        // tile blocks, channel blocks
  // the rest describes the shared-transform kernel's walk; the one- and two-wave kernels launch gx * gy blocks of one slice (grid0 = nvb = 1)
  int grid0;         // tile blocks x channel blocks of the layer, including the padding of the XCD deal
  int nvb;           // grid0 x S virtual blocks
  int grid;          // blocks launched: nvb, or the resident slots where the blocks are persistent
  int S, ks;         // K slices, and K steps (8-channel blocks) per slice
  int gran;          // K steps between two possible cuts: 2 (slot parity) or 8 (a phase walk's loop body)
  int sk_G;          // stream-K: granules per tile block, 0 = off (whole tile blocks per block)
  int sk_q, sk_rem;  // granules of the last round per persistent block; the first sk_rem blocks of an XCD take one more
  int sk_F;          // whole tile blocks per persistent block before them
  bool fin;          // the K slices are summed inside the kernel (no wino_reduce_kernel) ...
  bool fin_nchw;     // ... into an NCHW output: the partials are dense, the finish writes the real channel slice
  int copies;        // raw copies of the output taken from the scratch: S of a K split, the most pieces stream-K cuts a tile block into, else 0
};

static inline int wino_div_up(long a, long b) { return (int)((a + b - 1) / b); }

// K-split plan of conv_wino8_kernel for a grid of `blocks` full-K blocks of nK steps on the chip's 256 CUs (one block per CU at a
// time): S slices of ks steps each so that blocks x S fills whole rounds; cost model = rounds x (steps + per-block prologue/epilogue,
// ~6 steps' worth) + the second pass (S + 1 passes over the output at ~4 TB/s, in steps of ~1.7 us). Deterministic: a function of
// the geometry only. step_granule: 2 (slot parity) or 8 (the stride-2 form's loop body).
static inline int wino8_split_plan(long blocks, int nK, int step_granule, double out_mb, int max_split, int* kslice, int slots = 256,
                                   double* cost_out = nullptr) {
  int best = 1;
  double best_cost = 1e30;
  for (int S = 1; S <= 16; ++S) {
    if (max_split > 0 && S > max_split) break;
    int ks = wino_div_up(wino_div_up(nK, S), step_granule) * step_granule;
    if (S > 1 && ks < 8) break;
    const int Seff = wino_div_up(nK, ks);
    if (Seff != S) continue;
    const double rounds = (double)wino_div_up(blocks * S, slots);
    double cost = rounds * (ks + 6.0);
    if (S > 1) cost += (S + 1) * out_mb / 4000.0 / 1.7e-3 + 1.5;   // MB / (MB per ms) -> ms -> steps; + a launch boundary
    if (cost < best_cost - 1e-9) { best_cost = cost; best = S; *kslice = ks; }
  }
  if (best == 1) *kslice = nK;
  if (cost_out) *cost_out = best_cost;
  return best;
}

// Stream-K of the last round of the same grid (WinoParams::sk_*): F whole tile blocks per persistent block, then every block an equal
// run (+- 1) of the remaining tile blocks' granules — at the price of up to two more pieces per block and the read-back of the cut tile
// blocks. Same cost unit as wino8_split_plan (steps). Returns the granules per tile block, 0 where it does not apply: the XCD deal
// needs grid % 8 == 0, and no tile block is cut into more than W8_SK_MAX_COPIES pieces.
#define W8_SK_MAX_COPIES 8
#define W8_SK_MAX_TILE_BLOCKS DI_WINO_COUNTERS   /* counters per context (64 KB) */
static inline int wino8_streamk_plan(long grid, int nK, int step_granule, int slots, double* cost, int* F, int* q, int* rem) {
  if (grid % 8 != 0 || nK % step_granule != 0 || grid > W8_SK_MAX_TILE_BLOCKS) return 0;
  const int G = nK / step_granule, nlb = slots / 8;
  const long ltiles = grid / 8;
  *F = (int)(ltiles / nlb);
  const long units = (ltiles - (long)*F * nlb) * G;
  if (units == 0) return 0;
  *q = (int)(units / nlb); *rem = (int)(units % nlb);
  if (*q < 1 || wino_div_up(G, *q) + 1 > W8_SK_MAX_COPIES) return 0;
  *cost = (double)*F * (nK + 6.0) + ((double)*q + (*rem ? 1 : 0)) * step_granule + 2 * 6.0 + 2.0;
  return G;
}

// ---- which kernel, which walk, which shape: each question answered once ----

// the 8-wave shared-transform kernel (the default) runs the layer: a two-wave context runs none of it, other channel counts fall back to the one-wave kernel
static inline bool wino_shared_kernel(const WinoOptions& o, int Cout) { return !o.two_wave && o.shared && (Cout & 63) == 0; }
// the K loop can walk the four input phases of a stride-2 layer and drop their zero positions: an even number of 8-channel blocks per phase
static inline bool wino_phase_walk(const WinoOptions& o, WinoGeom geom, int Cin) { return geom != WINO_3X3 && (Cin % 64) == 0 && o.s2d_skip; }
// the nine-accumulator 256 x 32 blocks exist for the layer: the 3x3 stride-2 walk with its dead positions dropped, Cout % 256 == 0
static inline bool wino_nine_exists(const WinoOptions& o, WinoGeom geom, int Cin, int Cout) {
  return wino_shared_kernel(o, Cout) && geom == WINO_S2D_3X3 && wino_phase_walk(o, geom, Cin) && (Cout & 255) == 0;
}

// The block shape (WinoOptions::wide): 0 = 64 x 64; 3 = 128 channels x 32 tiles where Cout % 128 == 0; 2 = 64 x 32 on four waves, two blocks
// per CU; 1 (default) = by the work per CU: the wide blocks share each V among 128 channels and win the long grids (2-4 %), the
// four-wave blocks overlap one block's prologue / epilogue with the other's loop and win where a CU sees few blocks — measured
// (tools/bench_wino.py at B = 4 / 8 / 32, both forms): the crossover sits near 100 steps of 8 input channels per CU.
// 4 = the nine-accumulator blocks where they exist, anywhere else as 3. Under the default (1) the 3x3 stride-2 walk keeps the 128 x 32
// blocks unless the caller asks for the nine-accumulator shape (want_nine): the caller that wants it where it measured faster asks
// deepim_conv_wino_preferred_s2d3_wide and calls deepim_conv2d_wino_forward_s2d3_wide, as the network does (profiles/r13_s2d3_nine_tuples.md)
static inline WinoShape wino_block_shape(const WinoOptions& o, int ntiles, int Cin, int Cout, WinoGeom geom, bool want_nine) {
  if (o.two_wave) return WINO_TWO_WAVE;
  if (!wino_shared_kernel(o, Cout)) return WINO_ONE_WAVE;
  if (wino_nine_exists(o, geom, Cin, Cout) && (o.wide == 4 || (want_nine && o.wide == 1))) return WINO_256X32_NINE;
  bool four_wave = o.wide == 2;
  if (o.wide == 1) {
    const long wide_blocks = (long)wino_div_up(ntiles, 32) * wino_div_up(Cout, 128);
    // the 3x3 stride-2 geometry (25 MFMA blocks per 8-step body, not 49 / 64): the wide blocks win at every batch measured (B = 4 / 8 / 32,
    // tools/bench_wino.py; profiles/r09_stride2_wino.md)
    four_wave = (geom != WINO_S2D_3X3 && wide_blocks * (Cin / 8) <= 100L * 256) || (Cout & 127) != 0;
  }
  if (four_wave) return WINO_64X32_4W;
  return ((Cout & 127) == 0 && o.wide != 0) ? WINO_128X32 : WINO_64X64;
}

// The plan of a layer (B, Cin, H, W) -> Cout as the kernels see it (a stride-2 layer: its space-to-depth problem). out_nc8: 0 = NCHW output,
// else channel-blocked. Arguments as wino_forward_impl has checked them (B > 0, Cout % 32 == 0, Cin % 8 == 0, tensors below 2 GB).
static inline WinoPlan wino_plan(const WinoOptions& o, int B, int Cin, int H, int W, int Cout, int out_nc8, WinoGeom geom, bool want_nine) {
  WinoPlan pl = {};
  const int ntiles = B * ((H + 1) / 2) * ((W + 1) / 2), nK = Cin / 8;
  pl.shape = wino_block_shape(o, ntiles, Cin, Cout, geom, want_nine);
  const WinoShapeInfo& sh = WINO_SHAPE[pl.shape];
  // (the one-wave kernel's 5x5 walk skips a subset of the 3x3 stride-2 geometry's zero positions: it serves both; the two-wave kernel has none)
  pl.walk = (pl.shape != WINO_TWO_WAVE && wino_phase_walk(o, geom, Cin)) ? (int)geom : 0;
  pl.gx = wino_div_up(ntiles, sh.tiles);
  pl.gy = Cout / sh.channels;
  pl.grid = pl.gx * pl.gy;
  pl.grid0 = 1; pl.nvb = 1; pl.S = 1; pl.ks = nK;
  pl.gran = pl.walk ? 8 : 2;   // the phases are walked two 8-channel blocks of each per loop body
  if (sh.slots == 0) return pl;
  // block -> (channel block, tile block) as conv_wino8_kernel maps it: gy < 8 dividing 8 deals 8 / gy XCDs to each channel block
  pl.grid0 = ((pl.gy & 7) != 0 && (8 % pl.gy) == 0) ? 8 * wino_div_up(pl.gx, 8 / pl.gy) : pl.grid;
  // under-filled grids split the input channels (conv5_1 / conv6_1 at B = 32, every layer at the per-GPU shares of an 8-GPU node)
  const size_t out_elems = (size_t)B * Cout * H * W;
  double cost_split = 0, cost_sk = 0;
  if (o.split != 1) pl.S = wino8_split_plan(pl.grid0, nK, pl.gran, out_elems * 4 / 1e6, o.split, &pl.ks, sh.slots, &cost_split);
  int skF = 0, skq = 0, skrem = 0;
  const int skG = (o.split != 1 && o.persistent && o.streamk && out_nc8 && out_elems * 4 < (1ull << 31))
                      ? wino8_streamk_plan(pl.grid0, nK, pl.gran, sh.slots, &cost_sk, &skF, &skq, &skrem) : 0;
  // measured (bench.py A/B in one box): +1 % at B = 32 (4-18 whole rounds before the cut one), -1 % at B = 4 (one): from two whole rounds on
  // (the arrival counters are allocated with the context, deepim_create: nothing is allocated at launch time)
  const bool streamk = skG > 0 && (o.streamk == 2 || (skF >= 2 && cost_sk < cost_split * 0.98));   // 2: wherever it applies (tests)
  if (streamk) {
    pl.S = 1; pl.ks = nK;
    pl.sk_G = skG; pl.sk_q = skq; pl.sk_rem = skrem; pl.sk_F = skF;
    pl.copies = wino_div_up(skG, skq) + 1;   // a tile block of G granules cut by runs of >= q: at most that many pieces
  } else if (pl.S > 1) {
    pl.copies = pl.S;
  }
  pl.nvb = pl.grid0 * pl.S;
  pl.grid = streamk ? sh.slots : o.persistent ? (int)std::min<long>(pl.nvb, sh.slots) : pl.nvb;   // one block per resident slot, each walks its share
  // K slices finished inside the kernel: the block whose slice of a tile block arrives last adds the S raw copies in slice order, the bias
  // and the activation — the sums wino_reduce_kernel would form, without its launch and its pass over the whole output
  pl.fin = pl.S > 1 && o.fin && pl.grid0 <= DI_WINO_COUNTERS && out_elems * 4 < (1ull << 31);
  pl.fin_nchw = pl.fin && !out_nc8;
  return pl;
}

// ---- where Winograd pays (deepim_conv_wino_preferred*): the measured thresholds ----

// Whether the layer should take the Winograd path. Cout % 64 == 0 (every encoder layer): the shared-transform kernel splits the input
// channels where the grid would not fill the chip, so it pays from two tile blocks on (measured at B = 4 / 8 / 32, tools/bench_wino.py:
// 1.45-2.1x over the direct kernels on every layer, conv5_1 / conv6_1 at B = 4 included); other channel counts fall back to the
// one-wave kernel, which walks all of Cin per block and needs >= 128 (stride-2 form: 256) blocks of 32 channels x 128 tiles.
// conv_max_split == 1 is the canonical-summation-order configuration (bit-exact against the oracle's default order): no Winograd there.
#ifndef WINO_MIN_BLOCKS
#define WINO_MIN_BLOCKS 128
#endif
#ifndef WINO_MIN_BLOCKS_S2D
#define WINO_MIN_BLOCKS_S2D 256
#endif
#ifndef WINO_MIN_TILES
#define WINO_MIN_TILES 64
#endif
static inline bool wino_pays(const WinoOptions& o, int B, int H, int W, int Cout, long min_blocks) {
  if (o.canonical) return false;
  const long tiles = (long)B * ((H + 1) / 2) * ((W + 1) / 2);
  if (wino_shared_kernel(o, Cout)) return tiles >= WINO_MIN_TILES;
  const WinoShapeInfo& sh = WINO_SHAPE[WINO_ONE_WAVE];
  return (long)wino_div_up(tiles, sh.tiles) * (Cout / sh.channels) >= min_blocks;
}

// A 3x3 stride-2 pad-1 layer with input (B, Cin, H, W), run over its space-to-depth form: shared-transform kernel only, and where it was
// measured faster than the direct kernel: from WINO_S2D3_MIN_WORK output tiles x
// 8-channel input blocks (profiles/r09_stride2_wino.md: conv4 / conv5 at B = 8 = 76 800 / 40 960 units gain 8 / 14 %, at B = 4 = 38 400 /
// 20 480 units they are within noise of the direct kernel).
#ifndef WINO_S2D3_MIN_WORK
#define WINO_S2D3_MIN_WORK 40000
#endif
static inline bool wino_s2d3_pays(const WinoOptions& o, int B, int Cin, int H, int W, int Cout) {
  if (o.canonical || !wino_shared_kernel(o, Cout)) return false;
  return (long)B * ((H / 2 + 1) / 2) * ((W / 2 + 1) / 2) * (Cin / 8) >= WINO_S2D3_MIN_WORK;
}

// where deepim_conv_wino_preferred_s2d3_wide sends a 3x3 stride-2 layer to the nine-accumulator blocks: where they measured faster than the
// 128 x 32 blocks (profiles/r13_s2d3_nine_tuples.md §3, nb = blocks of 256 channels x 32 tiles on 256 slots). From two whole rounds on
// (conv4 at B = 32: nb = 600, -5 %), stream-K levels the rest; one partly filled round that covers a third of the chip or more (conv5 at
// B = 32 / 16: nb = 160 / 80, -7 / -10 %; conv4 at B = 8: 150, -5 %) runs every block at once. Between one and two rounds the second
// round is nearly empty (conv4 at B = 16: nb = 300, +6 %), and below 80 blocks too few CUs work (conv5 at B = 8: nb = 40, +3 %).
#ifndef WINO_NINE_MIN_BLOCKS
#define WINO_NINE_MIN_BLOCKS 80
#endif
static inline bool wino_nine_pays(long nb) { return nb >= 2 * 256 || (nb >= WINO_NINE_MIN_BLOCKS && nb <= 256); }
