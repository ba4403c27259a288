// Host-side layer table, packed-weight layout and workspace plan shared by vgg.hip and vgg_backward.hip.
#pragma once
#include "common.h"
#include "vgg_graph.h"

struct LayerDef { int cin, cout, has_bias; };      // (what its launch reads and writes: kFwd, vgg_graph.h)
// state-dict order (VGG.py:23-56): conv0,2,5,7,10,12,14, dec1.1, dec1.3, dec2.1, dec2.3, dec3.1, dec3.3
static const LayerDef kLayers[13] = {
    {3, 64, 1}, {64, 64, 1}, {64, 128, 1}, {128, 128, 1}, {128, 256, 1}, {256, 256, 1}, {256, 256, 1},
    {384, 128, 0}, {128, 128, 0}, {192, 64, 0}, {64, 64, 0},
    // conv_dec3.1 (128 -> 32) and conv_dec3.3 (32 -> 16) are run on ZERO-PADDED weights (the host pads them to 64 output /
    // 64 input channels), so every kernel keeps its 64-channel granularity; the padded channels are exactly zero
    {128, 64, 0}, {64, 64, 0}};

// bytes per stored activation element / per packed weight (split mode: fp32 activations, (hi, lo) fp16 weight pairs)
static inline size_t hla_elem_bytes(int dtype) { return (dtype == HLA_F32 || dtype == HLA_F16X3) ? 4 : 2; }
constexpr size_t kPackTailBytes = 256;   // HLA_F16X3: float[16] weight scales, float[16] = conv0 L1 bound, 32 scratch words

static inline size_t packed_bytes(int l, int dtype) {
  const size_t es = hla_elem_bytes(dtype);
  if (l == 0) return (size_t)2 * 32 * 32 * es;   // 2 ntiles x 32 (padded K) x 32 couts
  return (size_t)kLayers[l].cin * kLayers[l].cout * 9 * es + 4096;   // + two taps of fragments: prefetch overrun
}
static inline size_t packed_offset(int l, int dtype) {
  size_t o = 0;
  for (int i = 0; i < l; ++i) o += hla_align_up(packed_bytes(i, dtype), 256);
  return o;
}

// Forward workspace: every activation a later layer (or the backward pass) reads (the maps: vgg_graph.h), T elements.
struct VggPlan {
  size_t act[AM_N];                                          // post-ReLU activations; 0: not in this plan (level 4 / training only)
  size_t ss[4], inv;                                         // sum-of-squares partials, 1/norm
  size_t idx[IDX_N];                                         // training only: pool argmax (u8)
  size_t amax;                                               // split mode: [kAmaxSlots][B] per-sample max |activation| (fp32 bits)
  int np[4];
  size_t total;
};

// fold: the plan of a forward made with HLA_VGG_FOLD_DECODER (the decoder's tile counts are those of [2h, w/2]); every other
// offset is the same
static inline void vgg_plan(int B, int H, int W, int dtype, bool train, VggPlan* p, bool level4 = false, bool fold = false) {
  const size_t es = hla_elem_bytes(dtype);
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += hla_align_up(bytes, 256); return r; };
  auto maps = [&](int m0, int m1, bool on) {
    for (int m = m0; m < m1; ++m) p->act[m] = on ? take((size_t)B * vgg_map_elems(kActMaps[m], H, W) * es) : 0;
  };
  maps(AM_X3, AM_X2, true);
  for (int l = 0; l < kAllLayers; ++l)
    if (kFwd[l].level >= 0) p->np[kFwd[l].level] = vgg_level_partials(l, H, W, fold);
  for (int i = 0; i < 4; ++i) p->ss[i] = take((size_t)B * p->np[i] * sizeof(double));
  p->inv = take((size_t)4 * B * sizeof(double));
  p->amax = take((size_t)kAmaxSlots * B * sizeof(unsigned));
  maps(AM_X2, AM_A0, level4);
  maps(AM_A0, AM_N, train);
  for (int i = 0; i < IDX_N; ++i) p->idx[i] = train ? take((size_t)B * vgg_map_elems(kActMaps[kIdxOf[i]], H, W)) : 0;
  p->total = o;
}
