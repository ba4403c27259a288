// VGG16-U-Net forward: host orchestration (kernels live in conv_kernels.h).  VGG.py:13-203, 511-514.
#include "conv_kernels.h"
#include "vgg_layers.h"
#include <type_traits>

template <typename T>
void vgg_pack_all(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st) {
  constexpr bool SPLIT = Prec<T>::SPLIT;
  std::conditional_t<SPLIT, SplitPackTable, PackTable> tb{};
  if constexpr (!SPLIT) tb.b0 = prm->b[0];
  int n = 0;
  for (int l = 0; l < kAllLayers; ++l) {
    if (l >= kPackedLayers && !prm->w[l]) continue;      // conv_dec3.* only when the caller supplies its padded weights
    tb.w[n] = prm->w[l]; tb.off[n] = packed_offset(l, dtype); tb.cout[n] = kLayers[l].cout; tb.cin[n] = kLayers[l].cin;
    tb.first[n] = l == 0 ? 1 : 0;
    if constexpr (SPLIT) tb.slot[n] = l;
    // the layout of the MFMA shape the layer's forward kernel class runs on; conv0 / conv2 (conv02_kernel) keep 32x32x16
    else tb.shape[n] = l >= 2 ? conv_shape<T, false>(conv_class(kLayers[l].cout, vgg_layer_pools(l))) : SHAPE_32x32x16;
    ++n;
  }
  if constexpr (!SPLIT) {
    hla_prof_begin(K_PACK, 0, (double)packed_offset(kAllLayers, dtype) * (1.0 + 4.0 / sizeof(T)), st);
    hipLaunchKernelGGL((pack_weights_multi_kernel<T>), dim3(256, n), dim3(256), 0, st, tb, packed);
  } else {      // two launches for the whole network: the |w| maxima, then the (hi, lo) fragments scaled by them
    // the tail behind the last layer holds float[16] per-layer weight scales, float[16..31] (slot 16 = conv0's L1 bound) and
    // 32 scratch words for the two reductions
    float* tail = (float*)(packed + packed_offset(kAllLayers, dtype));
    unsigned* scratch = (unsigned*)tail + 32;
    (void)hipMemsetAsync(tail, 0, kPackTailBytes, st);
    hla_prof_begin(K_PACK, 0, (double)packed_offset(kAllLayers, dtype) * 3.0, st);
    hipLaunchKernelGGL(absmax_multi_kernel, dim3(64, n), dim3(256), 0, st, tb, scratch, (unsigned*)tail + 16);
    hipLaunchKernelGGL(pack_weights_split_multi_kernel, dim3(256, n), dim3(256), 0, st, tb, packed, (const unsigned*)scratch, tail);
  }
  hla_prof_end(st);
}

// One forward call: what hla_vgg_forward_cols, hla_vgg_fixup or one branch of hla_vgg_forward_pair was given, checked and
// completed (first_col32 where it applies, the plan) by vgg_forward_check
struct VggFwdCall {
  const float* x; size_t x_plane; const hla_vgg_params* prm; const char* packed;
  void* const* feat; float* const* conf; double* inv_norm; char* ws; size_t ws_bytes;
  int B, H, W, level, dtype, flags, first_row8, first_col32;
  const int* col_gate;            // the fix-up pass of a forward made with first_col32 > 0
  hipStream_t st;
  VggPlan pl;
};

// Everything a forward launches for its convolution layers, as argument blocks.  The geometry (which rows a layer computes, its
// sources, its epilogue's outputs: vgg_graph.h) is applied once, here, for the plain forward and for the paired one.
struct VggConvSet {
  Conv02Args c02;
  ConvArgs conv[kAllLayers];      // by layer index (vgg_graph.h); [0], [1] unused: conv0 + conv2 are c02
  bool used[kAllLayers], pool[kAllLayers];
  int np_used[4];                 // sum-of-squares partials per sample the feature layers actually write
};
template <typename T>
static void vgg_build_convs(const VggFwdCall& c, bool want_conf, VggConvSet& S) {
  const VggPlan& pl = c.pl;
  const int B = c.B, H = c.H, W = c.W, flags = c.flags;
  const bool level4 = c.level == 4, fold = (flags & HLA_VGG_FOLD_DECODER) != 0, train = (flags & HLA_VGG_SAVE_FOR_BACKWARD) != 0;
  const bool fixup = c.col_gate != nullptr;
  auto W_ = [&](int l) { return (const uint4*)(c.packed + packed_offset(l, c.dtype)); };
  char* w = c.ws;
  auto act = [&](int m) { return m >= 0 ? w + pl.act[m] : (char*)nullptr; };
  constexpr bool SPLIT = Prec<T>::SPLIT;
  const float* wtail = (const float*)(c.packed + packed_offset(kAllLayers, c.dtype));   // split mode: weight scales
  unsigned* amax = (unsigned*)(w + pl.amax);                                           // split mode: [slot][B]
  auto AM = [&](int slot) { return (SPLIT && slot >= 0) ? amax + (size_t)slot * B : (unsigned*)nullptr; };
  const VggFwdRows rows = vgg_fwd_rows(c.first_row8, level4, train, want_conf);
  S = VggConvSet{};
  for (int l = 0; l < 4; ++l) S.np_used[l] = pl.np[l];
  // conv0 + conv2 + pool fused (VGG.py:123-128): relu(x3)
  {
    Conv02Args& a = S.c02;
    a.x_plane = c.x_plane ? c.x_plane : (size_t)H * W;
    a.x = c.x; a.w0 = W_(0); a.b0 = c.prm->b[0]; a.w2 = W_(1); a.b2 = c.prm->b[1];
    a.out_act = act(AM_X3);
    if (train) {
      a.a0_out = act(AM_A0);
      a.idx_out = (unsigned char*)(w + pl.idx[IDX_3]);
    }
    if (level4) a.a2_out = act(AM_X2);
    a.wtail = wtail; a.amax_out = AM(AM_X3); a.amax_a2_out = level4 ? AM(AM_X2) : nullptr;
    a.amax_a0_out = train ? AM(AM_A0) : nullptr;
    a.row_begin = rows.row[1];
    const VggCols cc = vgg_cols(1, c.first_col32, fixup);
    a.col_begin = cc.begin;
    a.gate = c.col_gate;
    const int txf = (W + 31) / 32;
    a.B = B; a.H = H; a.W = W; a.tiles_y = (H - a.row_begin + 7) / 8;
    a.tiles_x = cc.tiles ? (cc.tiles < txf ? cc.tiles : txf) : txf - a.col_begin;
  }
  // relu(x21) feeds conv_dec3 (level 4), the conf2 head and the training backward only: without them the 16-bit feature path
  // stores just the raw map
  const bool x21r_dead = !level4 && !want_conf && !train && (flags & HLA_VGG_FEAT16) && sizeof(T) == 2;
  // encoder (VGG.py:129-141; ReLU commutes with max-pool, so pooled maps are stored post-ReLU), then the decoder (VGG.py:144-155)
  for (int l = 2; l < (level4 ? kAllLayers : kPackedLayers); ++l) {
    const VggFwdLaunch& f = kFwd[l];
    const VggHW g = vgg_layer_hw(l, H, W, fold);
    ConvArgs& a = S.conv[l];
    S.used[l] = true; S.pool[l] = vgg_layer_pools(l);
    void* raw = f.level >= 0 ? c.feat[f.level] : nullptr;
    a.raw16 = (raw && (flags & HLA_VGG_FEAT16)) ? 1 : 0;
    a.row_begin = rows.row[l];
    const VggCols cc = vgg_cols(l, c.first_col32, fixup);
    a.col_begin = cc.begin; a.col_tiles = cc.tiles;
    a.gate = c.col_gate;
    a.idx_out = (train && f.idx >= 0) ? (unsigned char*)(w + pl.idx[f.idx]) : nullptr;
    a.src1 = act(f.src); a.src2 = act(f.skip);
    a.C1 = kActMaps[f.src].C; a.C2 = f.skip >= 0 ? kActMaps[f.skip].C : 0; a.up1 = f.skip >= 0 ? 1 : 0; a.wpk = W_(l);
    a.bias = kLayers[l].has_bias ? c.prm->b[l] : nullptr;
    a.out_act = (f.out == AM_X21 && x21r_dead) ? (char*)nullptr : act(f.out); a.out_raw = (float*)raw;
    a.sumsq = f.level >= 0 ? (double*)(w + pl.ss[f.level]) : nullptr;
    a.B = B; a.H = g.h; a.W = g.w; a.Cout = kLayers[l].cout;
    a.relu_act = 1;
    if (SPLIT) {      // which per-sample maxima the layer reads (its one or two sources) and writes (its activation output)
      a.amax1 = AM(f.src); a.amax2 = AM(f.skip); a.amax_out = AM(f.out); a.wscale = wtail + l;
    }
    if (f.level >= 0) S.np_used[f.level] = vgg_level_partials(l, H, W, fold, a.row_begin);      // the partials this launch writes
  }
}

// conv0 + conv2: one network, or (a1) the two networks of a paired forward as the two segments of one launch
template <typename T>
static int launch_conv02(hipStream_t st, Conv02Args a, const Conv02Args* a1) {
  constexpr int lds_bytes = conv02_lds_bytes<T>();
#if HLA_CONV_STAMPS
  a.stamps = nullptr;      // (tooling build: want = -10 - k arms the k-th PLAIN conv02 launch since the call; paired ones are not counted)
  if (!a1 && g_hla_stamp.buf && g_hla_stamp.want <= -10 && g_hla_stamp.want++ == -10) {
    a.stamps = g_hla_stamp.buf; g_hla_stamp.want = -1000;
    g_hla_stamp.grid_x = a.tiles_x * a.tiles_y * a.B; g_hla_stamp.grid_y = 1;
  }
#endif
  auto P = [](const Conv02Args& c) {
    const int x1 = (c.col_begin + c.tiles_x) * 32;
    return (double)c.B * (c.H - c.row_begin) * ((x1 < c.W ? x1 : c.W) - c.col_begin * 32);
  };
  const double Pt = P(a) + (a1 ? P(*a1) : 0.0);
  static HlaPerDeviceOnce attr_once[2];
  HLA_CHECK_HIP(attr_once[a1 ? 1 : 0].run([a1] {
    const void* fn = a1 ? (const void*)conv02_pair_kernel<T, 2> : (const void*)conv02_kernel<T, 2>;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  }));
  hla_prof_begin(K_CONV02, 2.0 * 9 * (3 + 64) * 64 * Pt, Pt * (3 * 4 + 16 * sizeof(T)), st);
  if (a1) {
    PairArgs<Conv02Args> pa{{a, *a1}, a.tiles_x * a.tiles_y * a.B};
#if HLA_CONV_STAMPS
    pa.s[1].stamps = nullptr;
#endif
    hipLaunchKernelGGL((conv02_pair_kernel<T, 2>), dim3(pa.n0 + a1->tiles_x * a1->tiles_y * a1->B), dim3(256), lds_bytes, st, pa);
  } else
    hipLaunchKernelGGL((conv02_kernel<T, 2>), dim3(a.tiles_x * a.tiles_y * a.B), dim3(256), lds_bytes, st, a);
  hla_prof_end(st);
  return HLA_OK;
}

// L2 normalisation: 1/||x|| per sample (always) for the NL levels of `nb` networks in one launch, then the in-place scaling unless
// the caller folds it downstream
static int vgg_norms(int nb, const VggFwdCall* const* net, const VggConvSet* S, int NL) {
  const VggFwdCall& c0 = *net[0];
  const int B = c0.B;
  hipStream_t st = c0.st;
  InvNormArgs ia{};
  ia.gate = c0.col_gate;
  double bytes = 0;
  for (int k = 0; k < nb; ++k)
    for (int l = 0; l < NL; ++l) {
      const VggFwdCall& n = *net[k];
      ia.ss[k * NL + l] = (const double*)(n.ws + n.pl.ss[l]); ia.np[k * NL + l] = S[k].np_used[l];
      ia.inv[k * NL + l] = (n.inv_norm ? n.inv_norm : (double*)(n.ws + n.pl.inv)) + (size_t)l * B;
      bytes += (double)B * n.pl.np[l] * 8;
    }
  hla_prof_begin(K_L2NORM, 0, bytes, st);
  hipLaunchKernelGGL(inv_norm_multi_kernel, dim3(B, nb * NL), dim3(256), 0, st, ia);
  hla_prof_end(st);
  for (int k = 0; k < nb; ++k)
    for (int l = 0; l < NL; ++l) {
      if (c0.flags & HLA_VGG_DEFER_NORM) continue;
      const size_t per = vgg_map_elems(kActMaps[kLevelMap[l]], net[k]->H, net[k]->W);
      int bps = (int)(per / 4 / 256 / 4);
      bps = bps < 1 ? 1 : (bps > 64 ? 64 : bps);
      hla_prof_begin(K_L2NORM, 0, (double)B * per * 8, st);
      hipLaunchKernelGGL(scale_kernel, dim3(B * bps), dim3(256), 0, st, (float*)net[k]->feat[l], ia.inv[k * NL + l], per, bps);
      hla_prof_end(st);
    }
  return HLA_OK;
}

template <typename T>
int vgg_forward_t(const VggFwdCall& c) {
  const VggPlan& pl = c.pl;
  const int NL = c.level == 4 ? 4 : 3, B = c.B;
  hipStream_t st = c.st;
  constexpr bool SPLIT = Prec<T>::SPLIT;
  if (SPLIT) HLA_CHECK_HIP(hipMemsetAsync(c.ws + pl.amax, 0, (size_t)kAmaxSlots * B * sizeof(unsigned), st));
  const bool want_conf = (c.flags & HLA_VGG_WANT_CONF) && c.conf;
  VggConvSet S;
  vgg_build_convs<T>(c, want_conf, S);
  if (const int rc = launch_conv02<T>(st, S.c02, nullptr)) return rc;
  bool launch_ok = true;
  for (int l = 2; l < kAllLayers; ++l)
    if (S.used[l] && !launch_conv<T>(st, S.conv[l], S.pool[l])) launch_ok = false;
  // confidence heads on the ReLU'd maps
  if (want_conf) {
    using CT = std::conditional_t<SPLIT, float, T>;      // split mode stores fp32 activations: the heads run in plain fp32
    for (int l = 0; l < NL; ++l) {
      if (!c.conf[l]) continue;
      const VggMapDef& m = kActMaps[kLevelMap[l]];
      const VggHW g = vgg_map_hw(m, c.H, c.W, (c.flags & HLA_VGG_FOLD_DECODER) != 0);
      const CT* act = (const CT*)(c.ws + pl.act[kLevelMap[l]]);
      const size_t npix = (size_t)B * g.h * g.w;
      const int grid = B * ((g.h + CONF_TH - 1) / CONF_TH) * ((g.w + CONF_TW - 1) / CONF_TW);
      hla_prof_begin(K_CONF, 2.0 * 9 * m.C * (double)npix, (double)npix * (m.C * sizeof(CT) + 4), st);
      if (m.C == 256) hipLaunchKernelGGL((conf_kernel<CT, 256>), dim3(grid), dim3(256), 0, st, act, c.prm->w[13 + l], c.conf[l], B, g.h, g.w);
      else if (m.C == 128) hipLaunchKernelGGL((conf_kernel<CT, 128>), dim3(grid), dim3(256), 0, st, act, c.prm->w[13 + l], c.conf[l], B, g.h, g.w);
      else hipLaunchKernelGGL((conf_kernel<CT, 64>), dim3(grid), dim3(256), 0, st, act, c.prm->w[13 + l], c.conf[l], B, g.h, g.w);
      hla_prof_end(st);
    }
  }
  const VggFwdCall* net = &c;
  if (const int rc = vgg_norms(1, &net, &S, NL)) return rc;
  HLA_CHECK_HIP(hipGetLastError());
  return launch_ok ? HLA_OK : HLA_ERR_ARG;
}

// The fix-up pass (col_gate) as ONE launch, a workgroup per sample: vgg_fixup_loop (conv_kernels.h) walks the argument blocks that
// vgg_forward_t would have launched one by one, with the tile counts conv_plan gives them, and forms inv_norm at its end.  The
// caller has checked that the column trim applies (vgg_first_col32: level 3, inference, deferred norm, no heads, no fold).
template <typename T>
int vgg_fixup_t(const VggFwdCall& c) {
  static_assert(sizeof(T) == 2, "vgg_fixup_loop: bf16 / fp16");
  VggConvSet S;
  vgg_build_convs<T>(c, false, S);
  VggFixupArgs fa{};
  fa.c02 = S.c02;
  for (int k = 0; k < kFixupConvs; ++k) {
    const int l = k + 2;
    ConvArgs a = S.conv[l];
    const bool ok = S.used[l] && (a.Cout >= 128 || !S.pool[l]) && !a.idx_out;
    HLA_REQUIRE(ok, "vgg_fixup: layer %d is not one of the level-3 inference launches", l);
    if (conv_plan<T, false>(a, S.pool[l]).small) a.tiles_y = (a.H - a.row_begin + 7) / 8;      // (the loop's tiles are 8 rows)
    fa.conv[k] = a;
    if (S.pool[l]) fa.pooled |= 1 << k;
  }
  for (int l = kFixupConvs + 2; l < kAllLayers; ++l) HLA_REQUIRE(!S.used[l], "vgg_fixup: level 3 only");
  for (int l = 0; l < 3; ++l) {      // (as vgg_norms fills inv_norm_multi_kernel's rows)
    fa.ss[l] = (const double*)(c.ws + c.pl.ss[l]); fa.np[l] = S.np_used[l];
    fa.inv[l] = (c.inv_norm ? c.inv_norm : (double*)(c.ws + c.pl.inv)) + (size_t)l * c.B;
  }
  fa.gate = c.col_gate;
  constexpr int lds_bytes = vgg_fixup_lds_bytes<T>();
  static HlaPerDeviceOnce attr_once;
  HLA_CHECK_HIP(attr_once.run([] {
    return hipFuncSetAttribute((const void*)vgg_fixup_loop<T>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  }));
  hipLaunchKernelGGL((vgg_fixup_loop<T>), dim3(c.B), dim3(256), lds_bytes, c.st, fa);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

// Inference forward of TWO networks (the satellite and the ground extractor) whose every convolution layer runs as ONE launch of
// two segments.  The caller (hla_vgg_forward_pair) has checked both calls; returns HLA_PAIR_FALLBACK with nothing launched when a
// layer's two segments would not take the same kernel instantiation (the two sides of CONV_SMALL_GRID).
constexpr int HLA_PAIR_FALLBACK = -1000;
template <typename T>
int vgg_forward_pair_t(const VggFwdCall c[2]) {
  constexpr bool SPLIT = Prec<T>::SPLIT;
  hipStream_t st = c[0].st;
  VggConvSet S[2];
  for (int k = 0; k < 2; ++k) vgg_build_convs<T>(c[k], false, S[k]);
  for (int l = 2; l < kAllLayers; ++l) {
    if (S[0].used[l] != S[1].used[l]) return HLA_PAIR_FALLBACK;
    if (!S[0].used[l]) continue;
    ConvArgs a0 = S[0].conv[l], a1 = S[1].conv[l];
    if (conv_plan<T, false>(a0, S[0].pool[l]).small != conv_plan<T, false>(a1, S[1].pool[l]).small) return HLA_PAIR_FALLBACK;
  }
  if (SPLIT)
    for (int k = 0; k < 2; ++k)
      HLA_CHECK_HIP(hipMemsetAsync(c[k].ws + c[k].pl.amax, 0, (size_t)kAmaxSlots * c[k].B * sizeof(unsigned), st));
  if (const int rc = launch_conv02<T>(st, S[0].c02, &S[1].c02)) return rc;
  bool launch_ok = true;
  for (int l = 2; l < kAllLayers; ++l)
    if (S[0].used[l] && !launch_conv_pair<T>(st, S[0].conv[l], S[1].conv[l], S[0].pool[l])) launch_ok = false;
  const VggFwdCall* nets[2] = {&c[0], &c[1]};
  if (const int rc = vgg_norms(2, nets, S, 3)) return rc;
  HLA_CHECK_HIP(hipGetLastError());
  return launch_ok ? HLA_OK : HLA_ERR_ARG;
}

// One forward 3x3 convolution of ANY channel counts through launch_conv, outside the network's layer graph (the layer-level tests,
// tests/test_conv_weight_ring.py: stage counts and kernel classes the fixed layers do not combine).  out = relu([pool](conv(src)))
// in the activation type; with `raw` + `sumsq` the layer also writes the fp32 map before the ReLU and its sum-of-squares partials
// -- a feature layer's epilogue, which takes 8-row tiles at any grid size (conv_plan).  No bias.  Two segments: one paired launch.
struct HlaConvLayerSeg {
  const void* src;      // NHWC T [B,H,W,Cin]
  const float* w;       // [Cout,Cin,3,3]
  void* wpk;            // scratch for the packed weights: Cout * (Cin * 9 * sizeof(T) + 256 * sizeof(T)) bytes (two taps of padding)
  void* out;            // NHWC T [B,Ho,Wo,Cout]
  float* raw;           // NHWC fp32 [B,Ho,Wo,Cout] or null
  double* sumsq;        // with raw: [B, ceil(H/8) * ceil(W/32) * max(1, Cout/128)]
  int H, W;
};
struct HlaConvLayerCall { int B, Cin, Cout, pool, nseg; HlaConvLayerSeg seg[2]; hipStream_t st; };
template <typename T>
int vgg_conv_layer_t(const HlaConvLayerCall& c) {
  ConvArgs a[2] = {};
  for (int k = 0; k < c.nseg; ++k) {
    const HlaConvLayerSeg& s = c.seg[k];
    PackTable tb{};
    tb.w[0] = s.w; tb.off[0] = 0; tb.cout[0] = c.Cout; tb.cin[0] = c.Cin; tb.first[0] = 0;
    tb.shape[0] = conv_shape<T, false>(conv_class(c.Cout, c.pool != 0));
    hipLaunchKernelGGL((pack_weights_multi_kernel<T>), dim3(64, 1), dim3(256), 0, c.st, tb, (char*)s.wpk);
    a[k].src1 = s.src; a[k].wpk = (const uint4*)s.wpk; a[k].out_act = s.out; a[k].out_raw = s.raw; a[k].sumsq = s.raw ? s.sumsq : nullptr;
    a[k].C1 = c.Cin; a[k].B = c.B; a[k].H = s.H; a[k].W = s.W; a[k].Cout = c.Cout; a[k].relu_act = 1;
  }
  const bool ok = c.nseg == 2 ? launch_conv_pair<T>(c.st, a[0], a[1], c.pool != 0) : launch_conv<T>(c.st, a[0], c.pool != 0);
  HLA_CHECK_HIP(hipGetLastError());
  return ok ? HLA_OK : HLA_ERR_ARG;
}

#if HLA_TU_DTYPE >= 0
#if HLA_TU_DTYPE == 1 || HLA_TU_DTYPE == 2
template int vgg_conv_layer_t<TuT>(const HlaConvLayerCall& c);
#endif
template void vgg_pack_all<TuT>(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st);
template int vgg_forward_t<TuT>(const VggFwdCall& c);
template int vgg_forward_pair_t<TuT>(const VggFwdCall c[2]);
#if HLA_TU_DTYPE == 1 || HLA_TU_DTYPE == 2
template int vgg_fixup_t<TuT>(const VggFwdCall& c);
#endif
#else
#define HLA_EXTERN_T(T) \
  extern template void vgg_pack_all<T>(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st); \
  extern template int vgg_forward_t<T>(const VggFwdCall& c); \
  extern template int vgg_forward_pair_t<T>(const VggFwdCall c[2]);
HLA_EXTERN_T(float) HLA_EXTERN_T(bf16) HLA_EXTERN_T(f16) HLA_EXTERN_T(split32)
extern template int vgg_fixup_t<bf16>(const VggFwdCall& c);
extern template int vgg_fixup_t<f16>(const VggFwdCall& c);
extern template int vgg_conv_layer_t<bf16>(const HlaConvLayerCall& c);
extern template int vgg_conv_layer_t<f16>(const HlaConvLayerCall& c);

// The test hook of vgg_conv_layer_t (not part of include/hla.h): seg = HlaConvLayerSeg[nseg], nseg 1 (plain launch) or 2 (paired).
extern "C" int hla_debug_conv_layer(int dtype, int B, int Cin, int Cout, int pool, const void* seg, int nseg, hla_stream_t stream) {
  HLA_REQUIRE(seg && (nseg == 1 || nseg == 2), "hla_debug_conv_layer: one or two segments");
  HLA_REQUIRE(dtype == HLA_BF16 || dtype == HLA_F16, "hla_debug_conv_layer: bf16 / fp16 only");
  HLA_REQUIRE(B > 0 && Cin >= 32 && Cin % 32 == 0 && (Cout == 64 || (Cout >= 128 && Cout % 128 == 0)),
              "hla_debug_conv_layer: Cin a multiple of 32, Cout 64 or a multiple of 128 (got %d, %d)", Cin, Cout);
  HlaConvLayerCall c{B, Cin, Cout, pool, nseg, {}, (hipStream_t)stream};
  for (int k = 0; k < nseg; ++k) {
    c.seg[k] = ((const HlaConvLayerSeg*)seg)[k];
    const HlaConvLayerSeg& s = c.seg[k];
    HLA_REQUIRE(s.src && s.w && s.wpk && s.out && s.H > 0 && s.W > 0 && (!pool || (s.H % 2 == 0 && s.W % 2 == 0)) && (!s.raw || s.sumsq),
                "hla_debug_conv_layer: segment %d: null argument, odd size under the pool, or raw without sumsq", k);
  }
  return dtype == HLA_BF16 ? vgg_conv_layer_t<bf16>(c) : vgg_conv_layer_t<f16>(c);
}

extern "C" size_t hla_vgg_packed_weight_bytes(int dtype) {
  return packed_offset(kAllLayers, dtype) + (dtype == HLA_F16X3 ? kPackTailBytes : 0);
}

extern "C" int hla_vgg_pack_weights(const hla_vgg_params* params, void* packed, int dtype, hla_stream_t stream) {
  HLA_REQUIRE(params && packed, "hla_vgg_pack_weights: null argument");
  HLA_REQUIRE(hla_dtype_ok(dtype), "hla_vgg_pack_weights: bad dtype %d", dtype);
  HLA_REQUIRE(params->w[0] && params->b[0], "hla_vgg_pack_weights: conv0's weight and bias are required (the bias is packed with it)");
  hla_dispatch_dtype(dtype, [&](auto t) { vgg_pack_all<typename decltype(t)::type>(params, (char*)packed, dtype, (hipStream_t)stream); });
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

extern "C" size_t hla_vgg_workspace_bytes(int B, int H, int W, int level, int dtype) {
  VggPlan p;
  vgg_plan(B, H, W, dtype, /*train=*/true, &p, level == 4);   // sized for training so one buffer serves both modes
  return p.total;
}

extern "C" size_t hla_vgg_workspace_bytes_flags(int B, int H, int W, int level, int dtype, int flags) {
  VggPlan p;
  vgg_plan(B, H, W, dtype, /*train=*/true, &p, level == 4, (flags & HLA_VGG_FOLD_DECODER) != 0);
  return p.total;
}

// Where first_col32 applies (include/hla.h); 0 elsewhere.  Not in split-fp16 mode: there every layer scales its operands by the
// per-sample maximum of the WHOLE source map, which a trimmed forward does not know.
static inline int vgg_first_col32(int first_col32, int level, int dtype, int flags) {
  const bool ok = level == 3 && dtype != HLA_F16X3 && (flags & HLA_VGG_DEFER_NORM) &&
                  !(flags & (HLA_VGG_SAVE_FOR_BACKWARD | HLA_VGG_FOLD_DECODER | HLA_VGG_WANT_CONF));
  return ok ? first_col32 : 0;
}

// The argument checks of a forward call; then its column trim where that applies, its plan and the workspace check.  Returns
// HLA_OK or the code to return, with the message set unless `silent` (hla_vgg_forward_pair: a call that fails here is made, and
// reported, by the plain entry).  A fix-up pass with nothing to fix (col_gate && !first_col32 on return) is not planned.
static int vgg_forward_check(VggFwdCall& c, bool silent) {
#define VGG_REQUIRE(cond, ...) \
  do { if (!(cond)) { if (!silent) hla_set_error(__VA_ARGS__); return HLA_ERR_ARG; } } while (0)
  const int H = c.H, W = c.W, level = c.level, dtype = c.dtype, flags = c.flags, first_row8 = c.first_row8, first_col32 = c.first_col32;
  VGG_REQUIRE(c.x && c.prm && c.packed && c.feat && c.ws, "hla_vgg_forward: null argument");
  VGG_REQUIRE(hla_dtype_ok(dtype), "hla_vgg_forward: dtype must be HLA_F32, HLA_BF16, HLA_F16 or HLA_F16X3 (got %d)", dtype);
  VGG_REQUIRE(c.B > 0 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0, "hla_vgg_forward: H and W must be multiples of 8");
  VGG_REQUIRE(c.x_plane == 0 || c.x_plane >= (size_t)H * W, "hla_vgg_forward: x_plane (%zu) must be 0 or >= H*W", c.x_plane);
  // the conv kernels address a sample's activation map with signed 32-bit byte offsets (largest map: H x W x 64 fp32)
  VGG_REQUIRE((size_t)H * W * 64 * 4 < ((size_t)1 << 31), "hla_vgg_forward: image too large (H*W must be below 2^23 pixels)");
  VGG_REQUIRE(level == 3 || level == 4, "hla_vgg_forward: level must be 3 (x15,x18,x21) or 4 (+x24), got %d", level);
  VGG_REQUIRE(c.feat[0] && c.feat[1] && c.feat[2], "hla_vgg_forward: feat[0..2] are required");
  VGG_REQUIRE(level == 3 || (c.feat[3] && c.prm->w[11] && c.prm->w[12]),
              "hla_vgg_forward: level 4 needs feat[3] ([B,H,W,64], 16 real channels) and the zero-padded conv_dec3 weights in w[11], w[12]");
  VGG_REQUIRE(level == 3 || !(flags & HLA_VGG_WANT_CONF) || !c.conf || !c.conf[3] || c.prm->w[16], "hla_vgg_forward: conf[3] needs w[16]");
  VGG_REQUIRE(!(flags & HLA_VGG_DEFER_NORM) || c.inv_norm, "hla_vgg_forward: HLA_VGG_DEFER_NORM needs inv_norm");
  VGG_REQUIRE(!(flags & HLA_VGG_FEAT16) || ((dtype == HLA_BF16 || dtype == HLA_F16) && (flags & HLA_VGG_DEFER_NORM) &&
                                            !(flags & HLA_VGG_SAVE_FOR_BACKWARD) && level == 3),
              "hla_vgg_forward: HLA_VGG_FEAT16 needs dtype HLA_BF16 / HLA_F16, HLA_VGG_DEFER_NORM, level 3 and no HLA_VGG_SAVE_FOR_BACKWARD");
  VGG_REQUIRE(first_row8 == 0 || (first_row8 >= 4 && first_row8 < H / 8), "hla_vgg_forward: first_row8 must be 0 or in [4, H/8)");
  // folded decoder: the narrowest folded map (x15, W/16 wide) is up-sampled 2x into the W/8-wide dec1 geometry, so W/8 must be
  // even; the 32-px / 8-row conv tiles take partial tiles at the right / bottom edge as for any other width (the partial-sum
  // slots of the folded tile counts are planned by hla_vgg_workspace_bytes_flags, vgg_layers.h); every row of every map is read
  VGG_REQUIRE(!(flags & HLA_VGG_FOLD_DECODER) || (W % 16 == 0 && first_row8 == 0 && !(flags & HLA_VGG_FEAT16)),
              "hla_vgg_forward: HLA_VGG_FOLD_DECODER needs W %% 16 == 0 (folded maps are W/16, W/8, W/4 wide), first_row8 == 0 and no "
              "HLA_VGG_FEAT16 (got W = %d, first_row8 = %d)", W, first_row8);
  VGG_REQUIRE(first_col32 >= 0 && (first_col32 == 0 || 128 * first_col32 < W),
              "hla_vgg_forward_cols: first_col32 must be 0 or leave a column of the map (128 * first_col32 < W; got %d, W = %d)", first_col32, W);
  VGG_REQUIRE(!c.col_gate || first_col32 > 0, "hla_vgg_forward_cols: col_gate is the fix-up pass of a forward made with first_col32 > 0");
#undef VGG_REQUIRE
  c.first_col32 = vgg_first_col32(first_col32, level, dtype, flags);
  if (c.col_gate && !c.first_col32) return HLA_OK;      // that forward computed every column: nothing to fix
  vgg_plan(c.B, H, W, dtype, (flags & HLA_VGG_SAVE_FOR_BACKWARD) != 0, &c.pl, level == 4, (flags & HLA_VGG_FOLD_DECODER) != 0);
  if (c.ws_bytes < c.pl.total) {
    if (!silent) hla_set_error("hla_vgg_forward: workspace %zu < %zu", c.ws_bytes, c.pl.total);
    return HLA_ERR_WORKSPACE;
  }
  return HLA_OK;
}

// hla_vgg_forward_cols; fixup_one_launch: a fix-up pass (col_gate) may run as vgg_fixup_loop
static int vgg_forward_cols_impl(VggFwdCall c, bool fixup_one_launch) {
  if (const int rc = vgg_forward_check(c, false)) return rc;
  if (c.col_gate && !c.first_col32) return HLA_OK;
  // The fix-up pass as one launch: the 16-bit types (first_col32 > 0 here says the rest: level 3, inference, deferred norm, no
  // confidence heads, no folded decoder).  fp32 and a profiled run, whose records are per layer, keep the ten gated launches.
  const bool one_launch = c.col_gate && fixup_one_launch && !hla_prof_on();
  return hla_dispatch_dtype(c.dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    if constexpr (std::is_same_v<T, bf16> || std::is_same_v<T, f16>)
      if (one_launch) return vgg_fixup_t<T>(c);
    return vgg_forward_t<T>(c);
  });
}

extern "C" int hla_vgg_forward(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights,
                               void* const feat[4], float* const conf[4], double* inv_norm, void* workspace,
                               size_t workspace_bytes, int B, int H, int W, int level, int dtype, int flags,
                               int first_row8, hla_stream_t stream) {
  return hla_vgg_forward_cols(x, x_plane, params, packed_weights, feat, conf, inv_norm, workspace, workspace_bytes, B, H, W, level, dtype,
                              flags, first_row8, 0, nullptr, stream);
}

extern "C" int hla_vgg_forward_cols(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights,
                                    void* const feat[4], float* const conf[4], double* inv_norm, void* workspace,
                                    size_t workspace_bytes, int B, int H, int W, int level, int dtype, int flags,
                                    int first_row8, int first_col32, const int* col_gate, hla_stream_t stream) {
  return vgg_forward_cols_impl(VggFwdCall{x, x_plane, params, (const char*)packed_weights, feat, conf, inv_norm, (char*)workspace,
                                          workspace_bytes, B, H, W, level, dtype, flags, first_row8, first_col32, col_gate,
                                          (hipStream_t)stream, {}}, true);
}

extern "C" int hla_vgg_fixup(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights,
                             void* const feat[4], double* inv_norm, void* workspace, size_t workspace_bytes, int B, int H, int W,
                             int level, int dtype, int flags, int first_row8, int first_col32, const int* col_gate, int one_launch,
                             hla_stream_t stream) {
  HLA_REQUIRE(col_gate, "hla_vgg_fixup: col_gate is required");
  return vgg_forward_cols_impl(VggFwdCall{x, x_plane, params, (const char*)packed_weights, feat, nullptr, inv_norm, (char*)workspace,
                                          workspace_bytes, B, H, W, level, dtype, flags, first_row8, first_col32, col_gate,
                                          (hipStream_t)stream, {}}, one_launch != 0);
}

extern "C" int hla_vgg_forward_pair(const hla_vgg_branch br[2], int B, int level, int dtype, int flags, int* paired_out, hla_stream_t stream) {
  HLA_REQUIRE(br, "hla_vgg_forward_pair: null argument");
  if (paired_out) *paired_out = 0;
  auto plain = [&]() -> int {
    for (int k = 0; k < 2; ++k)
      if (const int rc = hla_vgg_forward_cols(br[k].x, br[k].x_plane, br[k].params, br[k].packed_weights, br[k].feat, br[k].conf, br[k].inv_norm,
                                         br[k].workspace, br[k].workspace_bytes, B, br[k].H, br[k].W, level, dtype, flags, br[k].first_row8,
                                         br[k].first_col32, nullptr, stream))
        return rc;
    return HLA_OK;
  };
  if (level != 3 || (flags & (HLA_VGG_SAVE_FOR_BACKWARD | HLA_VGG_FOLD_DECODER | HLA_VGG_WANT_CONF)) || !hla_dtype_ok(dtype)) return plain();
  // the argument checks of hla_vgg_forward, per network (a failed one is reported by the plain call)
  VggFwdCall c[2];
  for (int k = 0; k < 2; ++k) {
    const hla_vgg_branch& b = br[k];
    c[k] = VggFwdCall{b.x, b.x_plane, b.params, (const char*)b.packed_weights, b.feat, nullptr, b.inv_norm, (char*)b.workspace,
                      b.workspace_bytes, B, b.H, b.W, level, dtype, flags, b.first_row8, b.first_col32, nullptr, (hipStream_t)stream, {}};
    if (vgg_forward_check(c[k], true) != HLA_OK) return plain();
  }
  const int rc = hla_dispatch_dtype(dtype, [&](auto t) { return vgg_forward_pair_t<typename decltype(t)::type>(c); });
  if (rc == HLA_PAIR_FALLBACK) return plain();
  if (rc == HLA_OK && paired_out) *paired_out = 1;
  return rc;
}
#endif
