// The layer graph of the VGG16-U-Net extractor and the row / column plans of its launches, each stated once: the stored maps
// (forward activations and gradients: resolution, channels, whether the folded decoder geometry applies), what every forward,
// data-gradient and weight-gradient launch reads and writes, and which rows and columns a launch computes under first_row8 /
// first_col32.  vgg.hip and vgg_backward.hip walk these tables; nothing here launches anything.  Plain C++ (no HIP include): a
// stand-alone host program can include it (tests/test_vgg_graph_cpu.py).
#pragma once
#include <stddef.h>

constexpr int kPackedLayers = 11;   // conv0..dec2.3: what level 3 and the backward pass use
constexpr int kAllLayers = 13;      // + conv_dec3.1/3 (level 4, forward only)

// ---- the stored maps.  All NHWC.  div: the map is [H/div, W/div]; fold: under HLA_VGG_FOLD_DECODER (VGGUnet_G2S, VGG.py:278-310)
// the maps behind the encoder are read as [2h, w/2] -- on NHWC storage the same buffer, so only the geometry a launch is given changes
struct VggMapDef { int div, C, fold; };
struct VggHW { int h, w; };
static inline VggHW vgg_map_hw(const VggMapDef& m, int H, int W, bool fold) {
  const int h = H / m.div, w = W / m.div;
  return (fold && m.fold) ? VggHW{2 * h, w / 2} : VggHW{h, w};
}
static inline size_t vgg_map_elems(const VggMapDef& m, int H, int W) { return (size_t)(H / m.div) * (W / m.div) * m.C; }      // per sample

// forward activations, stored post-ReLU (VggPlan::act, in this order).  The id is also the map's slot among the per-sample maxima
// of split mode ([kAmaxSlots][B]).  x2 / d3a / x24: level 4 only (x24: 16 real of 64 channels); a0: training only.
// (conf0 reads the UNFOLDED x15 also under the fold, VGG.py:322, and dec1.1 takes its geometry from d1a: x15 is never folded)
enum { AM_X3 = 0, AM_A5, AM_X8, AM_A10, AM_A12, AM_X15, AM_D1A, AM_X18, AM_D2A, AM_X21, AM_X2, AM_D3A, AM_X24, AM_A0, AM_N, kAmaxSlots = 16 };
static const VggMapDef kActMaps[AM_N] = {{2, 64, 0}, {2, 128, 0}, {4, 128, 0}, {4, 256, 0}, {4, 256, 0}, {8, 256, 0}, {4, 128, 1},
                                         {4, 128, 1}, {2, 64, 1}, {2, 64, 1}, {1, 64, 0}, {1, 64, 1}, {1, 64, 1}, {1, 64, 0}};
// the pool argmax maps (u8, training only): one byte per element of the pooled map
enum { IDX_3 = 0, IDX_8, IDX_15, IDX_N };
static const int kIdxOf[IDX_N] = {AM_X3, AM_X8, AM_X15};
// the returned feature levels: the raw map of level l is the pre-ReLU output of the layer that writes kLevelMap[l]
static const int kLevelMap[4] = {AM_X15, AM_X18, AM_X21, AM_X24};

// gradient maps of the backward (BwdPlan::g).  [0, M_N): the maps of the level-3 walk, which the data-dependent trimming tracks
// (bwd_fan_kernel; *P: the gradient a skip connection carries, added by the consumer's producer); behind them the level-4 maps
// and the side buffers that hold the L2-norm gradient of a raw map until a data gradient's epilogue adds it.
// ga: the map's slot among the per-sample maxima of split mode ([kGradAmaxSlots][B]), -1: no convolution reads it
enum { M_X21, M_D2A, M_X3P, M_X18, M_D1A, M_X8P, M_X15, M_A12, M_A10, M_X8, M_A5, M_X3, M_A0, M_N,
       M_X24 = M_N, M_D3A, M_X2P, M_C2, M_L2_15, M_L2_18, M_L2_21, M_ALL };
enum { GA_X21 = 0, GA_D2A, GA_X18, GA_X3P, GA_D1A, GA_X15, GA_X8P, GA_A12, GA_A10, GA_X8, GA_A5, GA_X3, GA_A0, GA_X24, GA_D3A,
       GA_X2P, GA_C2, kGradAmaxSlots = 24 };
struct VggGradMapDef { VggMapDef m; int ga; };
static const VggGradMapDef kGradMaps[M_ALL] = {
    {{2, 64, 1}, GA_X21}, {{2, 64, 1}, GA_D2A}, {{2, 64, 0}, GA_X3P}, {{4, 128, 1}, GA_X18}, {{4, 128, 1}, GA_D1A}, {{4, 128, 0}, GA_X8P},
    {{8, 256, 0}, GA_X15}, {{4, 256, 0}, GA_A12}, {{4, 256, 0}, GA_A10}, {{4, 128, 0}, GA_X8}, {{2, 128, 0}, GA_A5}, {{2, 64, 0}, GA_X3},
    {{1, 64, 0}, GA_A0}, {{1, 64, 1}, GA_X24}, {{1, 64, 1}, GA_D3A}, {{1, 64, 0}, GA_X2P}, {{1, 64, 0}, GA_C2},
    {{8, 256, 0}, -1}, {{4, 128, 1}, -1}, {{2, 64, 1}, -1}};
// the order of the maps in the backward workspace: level 3, then (behind the scratch regions) level 4
static const int kBwdPlanOrder[] = {M_X21, M_D2A, M_X18, M_L2_18, M_D1A, M_X15, M_L2_15, M_A12, M_A10, M_X8, M_X8P, M_A5, M_X3, M_X3P, M_A0};
static const int kBwdPlanOrder4[] = {M_X24, M_D3A, M_X2P, M_C2, M_L2_21};

// ---- the forward launches, by layer: out = conv(relu(cat(up(src), skip))) with every input stored post-ReLU; skip >= 0 makes src
// the 2x nearest-upsampled one.  level >= 0: the layer also writes the raw map of that feature level and its sum of squares.
// idx >= 0: the layer's kernel ends in the 2x2 max-pool and (training) writes that argmax map.  Rows 0 and 1 run fused as conv02_kernel.
struct VggFwdLaunch { int src, skip, out, level, idx; };
static const VggFwdLaunch kFwd[kAllLayers] = {
    {-1, -1, AM_A0, -1, -1}, {AM_A0, -1, AM_X3, -1, IDX_3},                                      // conv0 (reads the image), conv2 + pool
    {AM_X3, -1, AM_A5, -1, -1}, {AM_A5, -1, AM_X8, -1, IDX_8},                                   // conv5, conv7 + pool
    {AM_X8, -1, AM_A10, -1, -1}, {AM_A10, -1, AM_A12, -1, -1}, {AM_A12, -1, AM_X15, 0, IDX_15},  // conv10, conv12, conv14 + pool
    {AM_X15, AM_X8, AM_D1A, -1, -1}, {AM_D1A, -1, AM_X18, 1, -1},                                // dec1.1, dec1.3 (VGG.py:144-146)
    {AM_X18, AM_X3, AM_D2A, -1, -1}, {AM_D2A, -1, AM_X21, 2, -1},                                // dec2.1, dec2.3 (VGG.py:148-151)
    {AM_X21, AM_X2, AM_D3A, -1, -1}, {AM_D3A, -1, AM_X24, 3, -1}};                               // dec3.1, dec3.3 (level 4, VGG.py:153-155)
// the geometry layer l is launched on (forward, and its data / weight gradient): its output map's, doubled where it ends in the pool
static inline bool vgg_layer_pools(int l) { return kFwd[l].idx >= 0; }
static inline VggHW vgg_layer_hw(int l, int H, int W, bool fold) {
  const VggHW g = vgg_map_hw(kActMaps[kFwd[l].out], H, W, fold);
  return vgg_layer_pools(l) ? VggHW{2 * g.h, 2 * g.w} : g;
}
static inline int vgg_layer_div(int l) { return kActMaps[kFwd[l].out].div / (vgg_layer_pools(l) ? 2 : 1); }
// sum-of-squares partials per sample of feature level `level`: one per (8 x 32 tile, 128-cout block) of the launch that writes it
static inline int vgg_level_partials(int l, int H, int W, bool fold, int row_begin = 0) {
  const VggHW g = vgg_layer_hw(l, H, W, fold);
  const int C = kActMaps[kFwd[l].out].C;
  return ((g.w + 31) / 32) * ((g.h - row_begin + 7) / 8) * (C >= 128 ? C / 128 : 1);
}

// ---- the backward launches.  A data gradient is a forward conv on layer `layer`'s transposed weights restricted to its input
// channels [c0, c0 + C(out)): it reads gradient map src (through the argmax map `unpool` where the layer ended in the pool), masks
// with the forward activation `mask`, adds gradient map `add` and writes `out`; pool_sum: the launch runs at the layer's resolution
// and sums 2x2 (the backward of the upsample) into out at half of it.  level: 0 = both, 3 / 4 = that level only.
// DC_* / DW_*: the launches of the level-3 walk, which have live-tile lists (DynLayout); the level-4 rows behind them have none.
enum { DC_10, DC_9U, DC_9S, DC_8, DC_7U, DC_7S, DC_6, DC_5, DC_4, DC_3, DC_2, DC_1, DC_N, DC_ALL = DC_N + 4 };
struct VggDgradLaunch { int layer, c0, src, unpool, out, mask, add, pool_sum, level; };
static const VggDgradLaunch kDgrad[DC_ALL] = {
    {10, 0, M_X21, -1, M_D2A, AM_D2A, -1, 0, 0},
    {9, 0, M_D2A, -1, M_X18, AM_X18, M_L2_18, 1, 0},            // up(x18) branch
    {9, 128, M_D2A, -1, M_X3P, AM_X3, -1, 0, 0},                // x3 skip branch
    {8, 0, M_X18, -1, M_D1A, AM_D1A, -1, 0, 0},
    {7, 0, M_D1A, -1, M_X15, AM_X15, M_L2_15, 1, 0},            // up(x15) branch
    {7, 256, M_D1A, -1, M_X8P, AM_X8, -1, 0, 0},                // x8 skip branch
    {6, 0, M_X15, IDX_15, M_A12, AM_A12, -1, 0, 0},             // conv14 is followed by the pool (no ReLU in between)
    {5, 0, M_A12, -1, M_A10, AM_A10, -1, 0, 0},
    {4, 0, M_A10, -1, M_X8, AM_X8, M_X8P, 0, 0},
    {3, 0, M_X8, IDX_8, M_A5, AM_A5, -1, 0, 0},
    {2, 0, M_A5, -1, M_X3, AM_X3, M_X3P, 0, 0},
    {1, 0, M_X3, IDX_3, M_A0, AM_A0, -1, 0, 3},
    // level 4: x21 also feeds conv_dec3 (its L2-norm gradient waits in l2_21); conv2's output also fed it, so the gradient of
    // conv2's output is materialised (g_c2 = unpool(g_x3) + g_x2p, unpool_add_kernel) before conv2's data gradient
    {12, 0, M_X24, -1, M_D3A, AM_D3A, -1, 0, 4},
    {11, 0, M_D3A, -1, M_X21, AM_X21, M_L2_21, 1, 4},           // up(x21) branch
    {11, 64, M_D3A, -1, M_X2P, AM_X2, -1, 0, 4},                // x2 skip branch
    {1, 0, M_C2, -1, M_A0, AM_A0, -1, 0, 4}};
// A weight gradient contracts gradient map g (through `unpool`) with the layer's forward input cat(up(x1), x2) (x2 >= 0 makes x1
// the upsampled one).  DW_0 (conv0: its input is the image) is launched by its own code; its row serves the live-tile lists.
enum { DW_10, DW_9, DW_8, DW_7, DW_6, DW_5, DW_4, DW_3, DW_2, DW_1, DW_0, DW_N, DW_ALL = DW_N + 3 };
struct VggWgradLaunch { int layer, x1, x2, g, unpool, level; };
static const VggWgradLaunch kWgrad[DW_ALL] = {
    {10, AM_D2A, -1, M_X21, -1, 0}, {9, AM_X18, AM_X3, M_D2A, -1, 0}, {8, AM_D1A, -1, M_X18, -1, 0}, {7, AM_X15, AM_X8, M_D1A, -1, 0},
    {6, AM_A12, -1, M_X15, IDX_15, 0}, {5, AM_A10, -1, M_A12, -1, 0}, {4, AM_X8, -1, M_A10, -1, 0}, {3, AM_A5, -1, M_X8, IDX_8, 0},
    {2, AM_X3, -1, M_A5, -1, 0}, {1, AM_A0, -1, M_X3, IDX_3, 3}, {0, -1, -1, M_A0, -1, 0},
    {12, AM_D3A, -1, M_X24, -1, 4}, {11, AM_X21, AM_X2, M_D3A, -1, 4}, {1, AM_A0, -1, M_C2, -1, 4}};
static inline bool vgg_level_runs(int row_level, bool level4) { return row_level == 0 || row_level == (level4 ? 4 : 3); }

// ---- row plan of the forward.  first_row8 = f > 0: the caller reads the returned maps only from rows f (x15), 2f (x18), 4f (x21)
// on, so every layer only has to produce the rows those depend on -- a 3x3 conv needs one more input row, a 2x upsample halves, a
// 2x2 pool doubles:
//   x21 <- dec2.3 [4f..] <- dec2.1 [4f-1..] <- {up(x18) [2f-1..], x3 [4f-2..]};  x18 <- dec1.3 [2f-1..] <- dec1.1 [2f-2..] <-
//   {up(x15) [f-2..], x8 [2f-3..]};  x15 [f-2..] <- pool(conv14 [2f-4..]) <- conv12 [2f-5..] <- conv10 [2f-6..] <- x8 [2f-7..]
//   <- pool(conv7 [4f-14..]) <- conv5 [4f-15..] <- x3 [4f-16..] = conv2 row 8f-32  (<- image row 8f-34: `dead_ground_rows`).
// Each launch starts exactly at its first needed row, so the one halo row above it is the first row its producer wrote.
// The 3x3 confidence heads read one row above the first confidence row that is used, so with them the decoder starts one
// row earlier (the encoder's needs do not change: x15 [f-2..] and x8 [2f-4..] are covered).
// Level 4 and training compute every row.  row[l]: first row of layer l's launch, in the launch's resolution ([0]: unused,
// [1]: conv0 + conv2 fused, in image rows).
struct VggFwdRows { int row[kAllLayers]; };
static inline VggFwdRows vgg_fwd_rows(int first_row8, bool level4, bool train, bool want_conf) {
  VggFwdRows r{};
  const int f = (level4 || train) ? 0 : first_row8, wc = want_conf ? 1 : 0;
  if (!f) return r;
  const int rows[kPackedLayers] = {0, 8 * f - 32, 4 * f - 15, 4 * f - 14, 2 * f - 6, 2 * f - 5, 2 * f - 4,
                                   2 * f - 2 - wc, 2 * f - 1 - wc, 4 * f - 1 - wc, 4 * f - wc};
  for (int l = 0; l < kPackedLayers; ++l) r.row[l] = rows[l] < 0 ? 0 : rows[l];
  return r;
}

// ---- column plan of the forward.  first_col32 = c > 0 (level 3, inference; never the folded geometry): every layer starts at
// tile column c, 2c or 4c of its own resolution -- the same COLUMN of the image at every resolution, so the three 2x2 pools and
// the 32-pixel tiles stay aligned.  A layer's left halo column was then never written by its producer and is read as zero
// (ConvArgs::col_begin), so its first columns are not the full run's: with conv2 exact from its first column (it computes conv0's
// halo itself) the first exact column is 64c (x3), 64c+1 (conv5), 64c+2 (conv7) -> 32c+1 (x8), 32c+2 / +3 / +4 (conv10 / 12 / 14)
// -> 16c+2 (x15), 32c+5 / +6 (dec1.1 / dec1.3 = x18), 64c+13 / +14 (dec2.1 / dec2.3 = x21).
// fixup (the pass behind it, col_gate): the same layers over the columns that pass left wrong -- the skipped strip and, but for
// conv2, the tile column behind it.  tiles == 0: every tile column from `begin` on.
struct VggCols { int begin, tiles; };
static inline VggCols vgg_cols(int l, int first_col32, bool fixup) {
  const int strip = first_col32 * (4 / vgg_layer_div(l));      // tile columns of this layer's resolution the trimmed pass skips
  return fixup ? VggCols{0, strip + (l <= 1 ? 0 : 1)} : VggCols{strip, 0};
}

// ---- row plan of the backward.  first_row8 = f > 0 is the caller's promise that d_feat[0..2] are zero above rows f / 2f / 4f (the
// LM loop only ever reads rows h_l/2.. of the ground maps, so that is where its gradient lives).  The gradient of every activation
// is then exactly zero above a first row that follows from the layer graph -- a 3x3 conv widens the support by one row, a 2x
// upsample / 2x2 pool halves / doubles it -- and every launch starts at that row (ConvArgs::row_begin, even where a pool is
// involved), reading its sources as zero above THEIR first row (src_row_lo / add_row_lo: those rows are never written).  With
// confidence heads the support of the three raw-map gradients starts one row higher.  Level 4 and the two-pass L2 backward (which
// leaves rounding noise above the support) compute every row.
// n[m]: first row of gradient map m in its own resolution (the L2-norm backward starts at n[x15] / n[x18] / n[x21] as well: the rows
// of d_feat[l] above them are neither read nor written); dc_*[i], dw_row[i]: launch i, in the launch's resolution.
struct VggBwdRows { int n[M_N], dc_row[DC_N], dc_src_lo[DC_N], dc_add_lo[DC_N], dw_row[DW_N]; };
static inline VggBwdRows vgg_bwd_rows(int first_row8, bool level4, bool scale_invariant, bool with_conf) {
  VggBwdRows r{};
  const int f = (level4 || !scale_invariant) ? 0 : first_row8;
  auto nn = [](int v) { return v < 0 ? 0 : v; };
  r.n[M_X21] = f ? 4 * f - (with_conf ? 1 : 0) : 0;
  for (int i = 0; i < DC_N; ++i) {      // (in launch order: a map's producer comes before its consumers)
    const VggDgradLaunch& d = kDgrad[i];
    r.dc_src_lo[i] = d.unpool >= 0 ? 2 * r.n[d.src] : r.n[d.src];
    if (d.pool_sum) {      // an even row of the launch, so that a 2x2 sum is whole: covers the map's own L2 / conf gradient
      r.dc_row[i] = nn(r.dc_src_lo[i] - 1) & ~1;
      r.n[d.out] = r.dc_row[i] / 2;
    } else
      r.dc_row[i] = r.n[d.out] = nn(r.dc_src_lo[i] - 1);
    r.dc_add_lo[i] = (d.add >= 0 && d.add < M_N) ? r.n[d.add] : 0;
  }
  for (int i = 0; i < DW_N; ++i) r.dw_row[i] = kWgrad[i].unpool >= 0 ? 2 * r.n[kWgrad[i].g] : r.n[kWgrad[i].g];
  return r;
}
