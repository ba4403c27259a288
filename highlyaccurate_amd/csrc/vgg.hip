// VGG16-U-Net forward: host orchestration (kernels live in conv_kernels.h).  VGG.py:13-203, 511-514.
#include "conv_kernels.h"
#include "vgg_layers.h"
#include <type_traits>

template <typename T>
void vgg_pack_all(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st) {
  // split mode: the tail behind the last layer holds float[16] per-layer weight scales, float[16..31] (slot 16 = conv0's
  // L1 bound) and 32 scratch words for the two reductions
  float* tail = (float*)(packed + packed_offset(kAllLayers, dtype));
  unsigned* scratch = (unsigned*)tail + 32;
  if (Prec<T>::SPLIT) (void)hipMemsetAsync(tail, 0, kPackTailBytes, st);
  if constexpr (!Prec<T>::SPLIT) {
    PackTable tb{};
    tb.b0 = prm->b[0];
    int n = 0;
    for (int l = 0; l < kAllLayers; ++l) {
      if (l >= kPackedLayers && !prm->w[l]) continue;      // conv_dec3.* only when the caller supplies its padded weights
      tb.w[n] = prm->w[l]; tb.off[n] = packed_offset(l, dtype); tb.cout[n] = kLayers[l].cout; tb.cin[n] = kLayers[l].cin;
      tb.first[n] = l == 0 ? 1 : 0;
      // the layout of the MFMA shape the layer's forward kernel class runs on; conv0 / conv2 (conv02_kernel) keep 32x32x16
      tb.shape[n] = l >= 2 ? conv_shape<T, false>(conv_class(kLayers[l].cout, kLayers[l].pool != 0)) : SHAPE_32x32x16;
      ++n;
    }
    hla_prof_begin(K_PACK, 0, (double)packed_offset(kAllLayers, dtype) * (1.0 + 4.0 / sizeof(T)), st);
    hipLaunchKernelGGL((pack_weights_multi_kernel<T>), dim3(256, n), dim3(256), 0, st, tb, packed);
    hla_prof_end(st);
    return;
  }
  if constexpr (Prec<T>::SPLIT) {      // two launches for the whole network: the |w| maxima, then the (hi, lo) fragments scaled by them
    SplitPackTable tb{};
    int n = 0;
    for (int l = 0; l < kAllLayers; ++l) {
      if (l >= kPackedLayers && !prm->w[l]) continue;        // conv_dec3.* only when the caller supplies its padded weights
      tb.w[n] = prm->w[l]; tb.off[n] = packed_offset(l, dtype); tb.cout[n] = kLayers[l].cout; tb.cin[n] = kLayers[l].cin;
      tb.first[n] = l == 0 ? 1 : 0; tb.slot[n] = l;
      ++n;
    }
    hla_prof_begin(K_PACK, 0, (double)packed_offset(kAllLayers, dtype) * 3.0, st);
    hipLaunchKernelGGL(absmax_multi_kernel, dim3(64, n), dim3(256), 0, st, tb, scratch, (unsigned*)tail + 16);
    hipLaunchKernelGGL(pack_weights_split_multi_kernel, dim3(256, n), dim3(256), 0, st, tb, packed, (const unsigned*)scratch, tail);
    hla_prof_end(st);
  }
}

// Everything a forward launches for its convolution layers, as argument blocks.  The geometry (which rows a layer computes, its
// sources, its epilogue's outputs) is decided once, here, for the plain forward and for the paired one (vgg_forward_pair_t).
struct VggConvSet {
  Conv02Args c02;
  ConvArgs conv[kAllLayers];      // by layer index (vgg_layers.h); [0], [1] unused: conv0 + conv2 are c02
  bool used[kAllLayers], pool[kAllLayers];
  int np_used[4];                 // sum-of-squares partials per sample the feature layers actually write
  bool ok;
};
template <typename T>
static void vgg_build_convs(const float* x, size_t x_plane, const hla_vgg_params* prm, const char* packed, int dtype, void* const feat[4],
                            bool want_conf, char* ws, const VggPlan& pl, int B, int H, int W, int flags, int first_row8, int first_col32,
                            const int* col_gate, VggConvSet& S) {
  const bool level4 = pl.x2r != 0;
  // HLA_VGG_FOLD_DECODER (VGGUnet_G2S, VGG.py:278-310): the maps behind the encoder are read as [2h, w/2].  On NHWC storage
  // that is the same buffer, so only the geometry the decoder launches are given changes: dH(d), dW(d) for the 1/d maps.
  const bool fold = (flags & HLA_VGG_FOLD_DECODER) != 0;
  auto dH = [&](int d) { return fold ? 2 * (H / d) : H / d; };
  auto dW = [&](int d) { return fold ? (W / d) / 2 : W / d; };
  auto W_ = [&](int l) { return (const uint4*)(packed + packed_offset(l, dtype)); };
  char* w = ws;
  constexpr bool SPLIT = Prec<T>::SPLIT;
  const float* wtail = (const float*)(packed + packed_offset(kAllLayers, dtype));       // split mode: weight scales
  unsigned* amax = (unsigned*)(w + pl.amax);                                           // split mode: [slot][B]
  auto AM = [&](int slot) { return (SPLIT && slot >= 0) ? amax + (size_t)slot * B : (unsigned*)nullptr; };
  const bool train = flags & HLA_VGG_SAVE_FOR_BACKWARD;
  // first_col32 = c > 0 (hla_vgg_forward has checked that nothing else reads the maps): every layer starts at tile column c, 2c or
  // 4c of its own resolution -- the same COLUMN of the image at every resolution, so the three 2x2 pools and the 32-pixel tiles
  // stay aligned.  A layer's left halo column was then never written by its producer and is read as zero (ConvArgs::col_begin),
  // so its first columns are not the full run's: with conv2 exact from its first column (it computes conv0's halo itself) the
  // first exact column is 64c (x3), 64c+1 (conv5), 64c+2 (conv7) -> 32c+1 (x8), 32c+2 / +3 / +4 (conv10 / 12 / 14) -> 16c+2 (x15),
  // 32c+5 / +6 (dec1.1 / dec1.3 = x18), 64c+13 / +14 (dec2.1 / dec2.3 = x21).
  // col_gate (the fix-up pass): the same layers over the columns that pass left wrong -- the skipped strip and, but for conv2, the
  // tile column behind it -- for the samples whose gate is set.  Every map is then the full run's in every column.
  const int c = first_col32;
  auto cols = [&](int scale, bool exact_from_start, int& begin, int& tiles) {
    begin = col_gate ? 0 : c * scale;
    tiles = col_gate ? c * scale + (exact_from_start ? 0 : 1) : 0;
  };
  S = VggConvSet{};
  S.ok = true;
  for (int l = 0; l < 4; ++l) S.np_used[l] = pl.np[l];
  // conv0 + conv2 + pool fused (VGG.py:123-128): relu(x3)
  {
    Conv02Args& a = S.c02;
    a.x_plane = x_plane ? x_plane : (size_t)H * W;
    a.x = x; a.w0 = W_(0); a.b0 = prm->b[0]; a.w2 = W_(1); a.b2 = prm->b[1];
    a.out_act = w + pl.x3;
    if (train) {
      a.a0_out = w + pl.a0;
      a.idx_out = (unsigned char*)(w + pl.idx3);
    }
    if (level4) a.a2_out = w + pl.x2r;
    a.wtail = wtail; a.amax_out = AM(AM_X3); a.amax_a2_out = level4 ? AM(AM_X2) : nullptr;
    a.amax_a0_out = train ? AM(AM_A0) : nullptr;
    // (first_row8, see below: x3 is needed from row 4f-16 on = conv2 row 8f-32)
    const int f0 = (level4 || train) ? 0 : first_row8;
    a.row_begin = f0 ? 8 * f0 - 32 : 0;
    int ct;
    cols(4, true, a.col_begin, ct);
    a.gate = col_gate;
    const int txf = (W + 31) / 32;
    a.B = B; a.H = H; a.W = W; a.tiles_x = ct ? (ct < txf ? ct : txf) : txf - a.col_begin; a.tiles_y = (H - a.row_begin + 7) / 8;
  }
  auto conv = [&](int l, const void* s1, int C1, int H_, int W_h, void* act, int relu, bool pool, const void* s2 = nullptr,
                  int C2 = 0, int up1 = 0, void* raw = nullptr, double* ss = nullptr, unsigned char* idx = nullptr,
                  int row_begin = 0, int norm_level = -1) {
    // the packer laid the layer's weights out for the kernel class kLayers[l].pool puts it in: the launch must pick the same one
    if (pool != (kLayers[l].pool != 0)) {
      hla_set_error("vgg_forward: layer %d launched with pool = %d, the layer table says %d", l, (int)pool, kLayers[l].pool);
      S.ok = false;
      return;
    }
    ConvArgs& a = S.conv[l];
    S.used[l] = true; S.pool[l] = pool;
    a.raw16 = (raw && (flags & HLA_VGG_FEAT16)) ? 1 : 0;
    a.row_begin = row_begin < 0 ? 0 : row_begin;
    cols(c ? W_h / (W / 4) : 1, false, a.col_begin, a.col_tiles);      // (c > 0: never the folded or the level-4 geometry)
    a.gate = col_gate;
    a.idx_out = train ? idx : nullptr;
    a.src1 = s1; a.src2 = s2;
    a.C1 = C1; a.C2 = C2; a.up1 = up1; a.wpk = W_(l);
    a.bias = kLayers[l].has_bias ? prm->b[l] : nullptr;
    a.out_act = act; a.out_raw = (float*)raw; a.sumsq = ss;
    a.B = B; a.H = H_; a.W = W_h; a.Cout = kLayers[l].cout;
    a.relu_act = relu;
    if (SPLIT) {      // which per-sample maxima the layer reads (its one or two sources) and writes (its activation output)
      static const signed char kAm[13][3] = {{-1, -1, -1}, {-1, -1, -1}, {AM_X3, -1, AM_A5}, {AM_A5, -1, AM_X8}, {AM_X8, -1, AM_A10},
                                             {AM_A10, -1, AM_A12}, {AM_A12, -1, AM_X15}, {AM_X15, AM_X8, AM_D1A}, {AM_D1A, -1, AM_X18},
                                             {AM_X18, AM_X3, AM_D2A}, {AM_D2A, -1, AM_X21}, {AM_X21, AM_X2, AM_D3A}, {AM_D3A, -1, AM_X24}};
      a.amax1 = AM(kAm[l][0]); a.amax2 = AM(kAm[l][1]); a.amax_out = AM(kAm[l][2]); a.wscale = wtail + l;
    }
    if (norm_level >= 0)      // sum-of-squares partials actually written by this launch: one per (tile, 128-cout block)
      S.np_used[norm_level] = ((W_h + 31) / 32) * ((H_ - a.row_begin + 7) / 8) * (a.Cout >= 128 ? a.Cout / 128 : 1);
  };
  // first_row8 = f > 0: the caller reads the returned maps only from rows f (x15), 2f (x18), 4f (x21) on, so every layer only
  // has to produce the rows those depend on -- a 3x3 conv needs one more input row, a 2x upsample halves, a 2x2 pool doubles:
  //   x21 <- dec2.3 [4f..] <- dec2.1 [4f-1..] <- {up(x18) [2f-1..], x3 [4f-2..]};  x18 <- dec1.3 [2f-1..] <- dec1.1 [2f-2..] <-
  //   {up(x15) [f-2..], x8 [2f-3..]};  x15 [f-2..] <- pool(conv14 [2f-4..]) <- conv12 [2f-5..] <- conv10 [2f-6..] <- x8 [2f-7..]
  //   <- pool(conv7 [4f-14..]) <- conv5 [4f-15..] <- x3 [4f-16..]  (<- image row 8f-34: `dead_ground_rows`).
  // Each launch starts exactly at its first needed row, so the one halo row above it is the first row its producer wrote.
  // The 3x3 confidence heads read one row above the first confidence row that is used, so with them the decoder starts one
  // row earlier (the encoder's needs do not change: x15 [f-2..] and x8 [2f-4..] are covered).
  const int f = (level4 || train) ? 0 : first_row8;
  const int wc = want_conf ? 1 : 0;
  const int r_c5 = f ? 4 * f - 15 : 0, r_c7 = f ? 4 * f - 14 : 0, r_c10 = f ? 2 * f - 6 : 0, r_c12 = f ? 2 * f - 5 : 0,
            r_c14 = f ? 2 * f - 4 : 0, r_d11 = f ? 2 * f - 2 - wc : 0, r_d13 = f ? 2 * f - 1 - wc : 0,
            r_d21 = f ? 4 * f - 1 - wc : 0, r_d23 = f ? 4 * f - wc : 0;
  // encoder (VGG.py:129-141).  ReLU commutes with max-pool, so pooled maps are stored post-ReLU.
  conv(2, w + pl.x3, 64, H / 2, W / 2, w + pl.a5, 1, false, nullptr, 0, 0, nullptr, nullptr, nullptr, r_c5);      // conv5
  conv(3, w + pl.a5, 128, H / 2, W / 2, w + pl.x8, 1, true, nullptr, 0, 0, nullptr, nullptr,
       (unsigned char*)(w + pl.idx8), r_c7);                                          // conv7 + pool -> relu(x8)
  conv(4, w + pl.x8, 128, H / 4, W / 4, w + pl.a10, 1, false, nullptr, 0, 0, nullptr, nullptr, nullptr, r_c10);   // conv10
  conv(5, w + pl.a10, 256, H / 4, W / 4, w + pl.a12, 1, false, nullptr, 0, 0, nullptr, nullptr, nullptr, r_c12);  // conv12
  conv(6, w + pl.a12, 256, H / 4, W / 4, w + pl.x15r, 1, true, nullptr, 0, 0, feat[0],
       (double*)(w + pl.ss[0]), (unsigned char*)(w + pl.idx15), r_c14, 0);            // conv14 + pool -> x15
  // decoder (VGG.py:144-151): conv(relu(cat(up(a), skip))) with both inputs stored post-ReLU
  conv(7, w + pl.x15r, 256, dH(4), dW(4), w + pl.d1a, 1, false, w + pl.x8, 128, 1, nullptr, nullptr, nullptr, r_d11);   // dec1.1
  conv(8, w + pl.d1a, 128, dH(4), dW(4), w + pl.x18r, 1, false, nullptr, 0, 0, feat[1],
       (double*)(w + pl.ss[1]), nullptr, r_d13, 1);                                   // dec1.3 -> x18
  // relu(x21) feeds conv_dec3 (level 4), the conf2 head and the training backward only: without them the 16-bit feature path
  // stores just the raw map
  const bool x21r_dead = !level4 && !wc && !train && (flags & HLA_VGG_FEAT16) && sizeof(T) == 2;
  conv(9, w + pl.x18r, 128, dH(2), dW(2), w + pl.d2a, 1, false, w + pl.x3, 64, 1, nullptr, nullptr, nullptr, r_d21);    // dec2.1
  conv(10, w + pl.d2a, 64, dH(2), dW(2), x21r_dead ? (char*)nullptr : w + pl.x21r, 1, false, nullptr, 0, 0, feat[2],
       (double*)(w + pl.ss[2]), nullptr, r_d23, 2);                                   // dec2.3 -> x21
  if (level4) {      // VGG.py:153-155: conv_dec3 on cat(up(x21), x2), zero-padded to 64 channels (vgg_layers.h)
    conv(11, w + pl.x21r, 64, dH(1), dW(1), w + pl.d3a, 1, false, w + pl.x2r, 64, 1);          // dec3.1
    conv(12, w + pl.d3a, 64, dH(1), dW(1), w + pl.x24r, 1, false, nullptr, 0, 0, feat[3],
         (double*)(w + pl.ss[3]), nullptr, 0, 3);                                      // dec3.3 -> x24 (16 real channels)
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
  if (a1) {
    static HlaPerDeviceOnce attr_once;
    HLA_CHECK_HIP(attr_once.run([] {
      return hipFuncSetAttribute((const void*)conv02_pair_kernel<T, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    }));
    PairArgs<Conv02Args> pa{{a, *a1}, a.tiles_x * a.tiles_y * a.B};
#if HLA_CONV_STAMPS
    pa.s[1].stamps = nullptr;
#endif
    hla_prof_begin(K_CONV02, 2.0 * 9 * (3 + 64) * 64 * Pt, Pt * (3 * 4 + 16 * sizeof(T)), st);
    hipLaunchKernelGGL((conv02_pair_kernel<T, 2>), dim3(pa.n0 + a1->tiles_x * a1->tiles_y * a1->B), dim3(256), lds_bytes, st, pa);
    hla_prof_end(st);
    return HLA_OK;
  }
  static HlaPerDeviceOnce attr_once;
  HLA_CHECK_HIP(attr_once.run([] {
    return hipFuncSetAttribute((const void*)conv02_kernel<T, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  }));
  hla_prof_begin(K_CONV02, 2.0 * 9 * (3 + 64) * 64 * Pt, Pt * (3 * 4 + 16 * sizeof(T)), st);
  hipLaunchKernelGGL((conv02_kernel<T, 2>), dim3(a.tiles_x * a.tiles_y * a.B), dim3(256), lds_bytes, st, a);
  hla_prof_end(st);
  return HLA_OK;
}

// L2 normalisation: 1/||x|| per sample (always) for the NL levels of `nb` networks in one launch, then the in-place scaling unless
// the caller folds it downstream
struct VggNormNet { const VggConvSet* S; char* ws; const VggPlan* pl; double* inv_norm; void* const* feat; int H, W; };
static int vgg_norms(hipStream_t st, int nb, const VggNormNet* net, int B, int NL, int flags, const int* gate = nullptr) {
  InvNormArgs ia{};
  ia.gate = gate;
  double bytes = 0;
  for (int k = 0; k < nb; ++k)
    for (int l = 0; l < NL; ++l) {
      const VggNormNet& n = net[k];
      ia.ss[k * NL + l] = (const double*)(n.ws + n.pl->ss[l]); ia.np[k * NL + l] = n.S->np_used[l];
      ia.inv[k * NL + l] = (n.inv_norm ? n.inv_norm : (double*)(n.ws + n.pl->inv)) + (size_t)l * B;
      bytes += (double)B * n.pl->np[l] * 8;
    }
  hla_prof_begin(K_L2NORM, 0, bytes, st);
  hipLaunchKernelGGL(inv_norm_multi_kernel, dim3(B, nb * NL), dim3(256), 0, st, ia);
  hla_prof_end(st);
  for (int k = 0; k < nb; ++k) {
    const int H = net[k].H, W = net[k].W;
    const size_t per[4] = {(size_t)(H / 8) * (W / 8) * 256, (size_t)(H / 4) * (W / 4) * 128, (size_t)(H / 2) * (W / 2) * 64, (size_t)H * W * 64};
    for (int l = 0; l < NL; ++l) {
      if (flags & HLA_VGG_DEFER_NORM) continue;
      int bps = (int)(per[l] / 4 / 256 / 4);
      bps = bps < 1 ? 1 : (bps > 64 ? 64 : bps);
      hla_prof_begin(K_L2NORM, 0, (double)B * per[l] * 8, st);
      hipLaunchKernelGGL(scale_kernel, dim3(B * bps), dim3(256), 0, st, (float*)net[k].feat[l], ia.inv[k * NL + l], per[l], bps);
      hla_prof_end(st);
    }
  }
  return HLA_OK;
}

template <typename T>
int vgg_forward_t(const float* x, size_t x_plane, const hla_vgg_params* prm, const char* packed, int dtype, void* const feat[4],
                         float* const conf[4], double* inv_norm, char* ws, const VggPlan& pl, int B, int H, int W,
                         int flags, int first_row8, int first_col32, const int* col_gate, hipStream_t st) {
  const bool level4 = pl.x2r != 0;
  const int NL = level4 ? 4 : 3;
  const bool fold = (flags & HLA_VGG_FOLD_DECODER) != 0;
  auto dH = [&](int d) { return fold ? 2 * (H / d) : H / d; };
  auto dW = [&](int d) { return fold ? (W / d) / 2 : W / d; };
  char* w = ws;
  constexpr bool SPLIT = Prec<T>::SPLIT;
  if (SPLIT) HLA_CHECK_HIP(hipMemsetAsync(w + pl.amax, 0, (size_t)kAmaxSlots * B * sizeof(unsigned), st));
  const bool want_conf = (flags & HLA_VGG_WANT_CONF) && conf;
  VggConvSet S;
  vgg_build_convs<T>(x, x_plane, prm, packed, dtype, feat, want_conf, ws, pl, B, H, W, flags, first_row8, first_col32, col_gate, S);
  if (!S.ok) return HLA_ERR_ARG;
  if (const int rc = launch_conv02<T>(st, S.c02, nullptr)) return rc;
  bool launch_ok = true;
  for (int l = 2; l < kAllLayers; ++l)
    if (S.used[l] && !launch_conv<T>(st, S.conv[l], S.pool[l])) launch_ok = false;
  // confidence heads on the ReLU'd maps
  if (want_conf) {
    using CT = std::conditional_t<SPLIT, float, T>;      // split mode stores fp32 activations: the heads run in plain fp32
    const CT* acts[4] = {(const CT*)(w + pl.x15r), (const CT*)(w + pl.x18r), (const CT*)(w + pl.x21r), (const CT*)(w + pl.x24r)};
    // (conf0 reads the UNFOLDED x15 also under HLA_VGG_FOLD_DECODER: VGG.py:322)
    const int Cs[4] = {256, 128, 64, 64}, hs[4] = {H / 8, dH(4), dH(2), dH(1)}, wsz[4] = {W / 8, dW(4), dW(2), dW(1)};
    for (int l = 0; l < NL; ++l) {
      if (!conf[l]) continue;
      const size_t npix = (size_t)B * hs[l] * wsz[l];
      const int grid = B * ((hs[l] + CONF_TH - 1) / CONF_TH) * ((wsz[l] + CONF_TW - 1) / CONF_TW);
      hla_prof_begin(K_CONF, 2.0 * 9 * Cs[l] * (double)npix, (double)npix * (Cs[l] * sizeof(CT) + 4), st);
      if (Cs[l] == 256) hipLaunchKernelGGL((conf_kernel<CT, 256>), dim3(grid), dim3(256), 0, st, acts[l], prm->w[13 + l], conf[l], B, hs[l], wsz[l]);
      else if (Cs[l] == 128) hipLaunchKernelGGL((conf_kernel<CT, 128>), dim3(grid), dim3(256), 0, st, acts[l], prm->w[13 + l], conf[l], B, hs[l], wsz[l]);
      else hipLaunchKernelGGL((conf_kernel<CT, 64>), dim3(grid), dim3(256), 0, st, acts[l], prm->w[13 + l], conf[l], B, hs[l], wsz[l]);
      hla_prof_end(st);
    }
  }
  {
    const VggNormNet net{&S, ws, &pl, inv_norm, feat, H, W};
    if (const int rc = vgg_norms(st, 1, &net, B, NL, flags, col_gate)) return rc;
  }
  HLA_CHECK_HIP(hipGetLastError());
  return launch_ok ? HLA_OK : HLA_ERR_ARG;
}

// The fix-up pass (col_gate) as ONE launch, a workgroup per sample: vgg_fixup_loop (conv_kernels.h) walks the argument blocks that
// vgg_forward_t would have launched one by one, with the tile counts conv_plan gives them, and forms inv_norm at its end.  The
// caller has checked that the column trim applies (vgg_first_col32: level 3, inference, deferred norm, no heads, no fold).
template <typename T>
int vgg_fixup_t(const float* x, size_t x_plane, const hla_vgg_params* prm, const char* packed, int dtype, void* const feat[4],
                double* inv_norm, char* ws, const VggPlan& pl, int B, int H, int W, int flags, int first_row8, int first_col32,
                const int* col_gate, hipStream_t st) {
  static_assert(sizeof(T) == 2, "vgg_fixup_loop: bf16 / fp16");
  VggConvSet S;
  vgg_build_convs<T>(x, x_plane, prm, packed, dtype, feat, false, ws, pl, B, H, W, flags, first_row8, first_col32, col_gate, S);
  if (!S.ok) return HLA_ERR_ARG;
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
    fa.ss[l] = (const double*)(ws + pl.ss[l]); fa.np[l] = S.np_used[l];
    fa.inv[l] = (inv_norm ? inv_norm : (double*)(ws + pl.inv)) + (size_t)l * B;
  }
  fa.gate = col_gate;
  constexpr int lds_bytes = vgg_fixup_lds_bytes<T>();
  static HlaPerDeviceOnce attr_once;
  HLA_CHECK_HIP(attr_once.run([] {
    return hipFuncSetAttribute((const void*)vgg_fixup_loop<T>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  }));
  hipLaunchKernelGGL((vgg_fixup_loop<T>), dim3(B), dim3(256), lds_bytes, st, fa);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

// Inference forward of TWO networks (the satellite and the ground extractor) whose every convolution layer runs as ONE launch of
// two segments.  The caller (hla_vgg_forward_pair) has checked the flags; returns HLA_PAIR_FALLBACK with nothing launched when a
// layer's two segments would not take the same kernel instantiation (the two sides of CONV_SMALL_GRID).
constexpr int HLA_PAIR_FALLBACK = -1000;
// Where first_col32 applies (include/hla.h); 0 elsewhere.  Not in split-fp16 mode: there every layer scales its operands by the
// per-sample maximum of the WHOLE source map, which a trimmed forward does not know.
static inline int vgg_first_col32(int first_col32, int level, int dtype, int flags) {
  const bool ok = level == 3 && dtype != HLA_F16X3 && (flags & HLA_VGG_DEFER_NORM) &&
                  !(flags & (HLA_VGG_SAVE_FOR_BACKWARD | HLA_VGG_FOLD_DECODER | HLA_VGG_WANT_CONF));
  return ok ? first_col32 : 0;
}
static inline int pair_first_col32(const hla_vgg_branch& b, int dtype, int flags) { return vgg_first_col32(b.first_col32, 3, dtype, flags); }
template <typename T>
int vgg_forward_pair_t(const hla_vgg_branch br[2], const VggPlan pl[2], int B, int dtype, int flags, hipStream_t st) {
  constexpr bool SPLIT = Prec<T>::SPLIT;
  VggConvSet S[2];
  for (int k = 0; k < 2; ++k) {
    vgg_build_convs<T>(br[k].x, br[k].x_plane, br[k].params, (const char*)br[k].packed_weights, dtype, br[k].feat, false,
                       (char*)br[k].workspace, pl[k], B, br[k].H, br[k].W, flags, br[k].first_row8, pair_first_col32(br[k], dtype, flags), nullptr, S[k]);
    if (!S[k].ok) return HLA_ERR_ARG;
  }
  for (int l = 2; l < kAllLayers; ++l) {
    if (S[0].used[l] != S[1].used[l]) return HLA_PAIR_FALLBACK;
    if (!S[0].used[l]) continue;
    ConvArgs a0 = S[0].conv[l], a1 = S[1].conv[l];
    if (conv_plan<T, false>(a0, S[0].pool[l]).small != conv_plan<T, false>(a1, S[1].pool[l]).small) return HLA_PAIR_FALLBACK;
  }
  if (SPLIT)
    for (int k = 0; k < 2; ++k)
      HLA_CHECK_HIP(hipMemsetAsync((char*)br[k].workspace + pl[k].amax, 0, (size_t)kAmaxSlots * B * sizeof(unsigned), st));
  if (const int rc = launch_conv02<T>(st, S[0].c02, &S[1].c02)) return rc;
  bool launch_ok = true;
  for (int l = 2; l < kAllLayers; ++l)
    if (S[0].used[l] && !launch_conv_pair<T>(st, S[0].conv[l], S[1].conv[l], S[0].pool[l])) launch_ok = false;
  {
    const VggNormNet nets[2] = {{&S[0], (char*)br[0].workspace, &pl[0], br[0].inv_norm, br[0].feat, br[0].H, br[0].W},
                                {&S[1], (char*)br[1].workspace, &pl[1], br[1].inv_norm, br[1].feat, br[1].H, br[1].W}};
    if (const int rc = vgg_norms(st, 2, nets, B, 3, flags)) return rc;
  }
  HLA_CHECK_HIP(hipGetLastError());
  return launch_ok ? HLA_OK : HLA_ERR_ARG;
}

#if HLA_TU_DTYPE >= 0
template void vgg_pack_all<TuT>(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st);
template int vgg_forward_t<TuT>(const float* x, size_t x_plane, const hla_vgg_params* prm, const char* packed, int dtype, void* const feat[4],
                              float* const conf[4], double* inv_norm, char* ws, const VggPlan& pl, int B, int H, int W,
                              int flags, int first_row8, int first_col32, const int* col_gate, hipStream_t st);
template int vgg_forward_pair_t<TuT>(const hla_vgg_branch br[2], const VggPlan pl[2], int B, int dtype, int flags, hipStream_t st);
#if HLA_TU_DTYPE == 1 || HLA_TU_DTYPE == 2
template int vgg_fixup_t<TuT>(const float* x, size_t x_plane, const hla_vgg_params* prm, const char* packed, int dtype, void* const feat[4],
                double* inv_norm, char* ws, const VggPlan& pl, int B, int H, int W, int flags, int first_row8, int first_col32,
                const int* col_gate, hipStream_t st);
#endif
#else
#define HLA_EXTERN_T(T) \
  extern template void vgg_pack_all<T>(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st); \
  extern template int vgg_forward_t<T>(const float* x, size_t x_plane, const hla_vgg_params* prm, const char* packed, int dtype, void* const feat[4],                               float* const conf[4], double* inv_norm, char* ws, const VggPlan& pl, int B, int H, int W,                               int flags, int first_row8, int first_col32, const int* col_gate, hipStream_t st);
HLA_EXTERN_T(float) HLA_EXTERN_T(bf16) HLA_EXTERN_T(f16) HLA_EXTERN_T(split32)
#define HLA_EXTERN_PAIR_T(T) \
  extern template int vgg_forward_pair_t<T>(const hla_vgg_branch br[2], const VggPlan pl[2], int B, int dtype, int flags, hipStream_t st);
HLA_EXTERN_PAIR_T(float) HLA_EXTERN_PAIR_T(bf16) HLA_EXTERN_PAIR_T(f16) HLA_EXTERN_PAIR_T(split32)
extern template int vgg_fixup_t<bf16>(const float* x, size_t x_plane, const hla_vgg_params* prm, const char* packed, int dtype, void* const feat[4],
                double* inv_norm, char* ws, const VggPlan& pl, int B, int H, int W, int flags, int first_row8, int first_col32,
                const int* col_gate, hipStream_t st);
extern template int vgg_fixup_t<f16>(const float* x, size_t x_plane, const hla_vgg_params* prm, const char* packed, int dtype, void* const feat[4],
                double* inv_norm, char* ws, const VggPlan& pl, int B, int H, int W, int flags, int first_row8, int first_col32,
                const int* col_gate, hipStream_t st);

extern "C" size_t hla_vgg_packed_weight_bytes(int dtype) {
  return packed_offset(kAllLayers, dtype) + (dtype == HLA_F16X3 ? kPackTailBytes : 0);
}

extern "C" int hla_vgg_pack_weights(const hla_vgg_params* params, void* packed, int dtype, hla_stream_t stream) {
  HLA_REQUIRE(params && packed, "hla_vgg_pack_weights: null argument");
  HLA_REQUIRE(hla_dtype_ok(dtype), "hla_vgg_pack_weights: bad dtype %d", dtype);
  HLA_REQUIRE(params->w[0] && params->b[0], "hla_vgg_pack_weights: conv0's weight and bias are required (the bias is packed with it)");
  if (dtype == HLA_BF16) vgg_pack_all<bf16>(params, (char*)packed, dtype, (hipStream_t)stream);
  else if (dtype == HLA_F16) vgg_pack_all<f16>(params, (char*)packed, dtype, (hipStream_t)stream);
  else if (dtype == HLA_F16X3) vgg_pack_all<split32>(params, (char*)packed, dtype, (hipStream_t)stream);
  else vgg_pack_all<float>(params, (char*)packed, dtype, (hipStream_t)stream);
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

extern "C" int hla_vgg_forward(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights,
                               void* const feat[4], float* const conf[4], double* inv_norm, void* workspace,
                               size_t workspace_bytes, int B, int H, int W, int level, int dtype, int flags,
                               int first_row8, hla_stream_t stream) {
  return hla_vgg_forward_cols(x, x_plane, params, packed_weights, feat, conf, inv_norm, workspace, workspace_bytes, B, H, W, level, dtype,
                              flags, first_row8, 0, nullptr, stream);
}

// hla_vgg_forward_cols; fixup_one_launch: a fix-up pass (col_gate) may run as vgg_fixup_loop
static int vgg_forward_cols_impl(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights,
                                 void* const feat[4], float* const conf[4], double* inv_norm, void* workspace,
                                 size_t workspace_bytes, int B, int H, int W, int level, int dtype, int flags,
                                 int first_row8, int first_col32, const int* col_gate, bool fixup_one_launch, hla_stream_t stream) {
  HLA_REQUIRE(x && params && packed_weights && feat && workspace, "hla_vgg_forward: null argument");
  HLA_REQUIRE(hla_dtype_ok(dtype), "hla_vgg_forward: dtype must be HLA_F32, HLA_BF16, HLA_F16 or HLA_F16X3 (got %d)", dtype);
  HLA_REQUIRE(B > 0 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0, "hla_vgg_forward: H and W must be multiples of 8");
  HLA_REQUIRE(x_plane == 0 || x_plane >= (size_t)H * W, "hla_vgg_forward: x_plane (%zu) must be 0 or >= H*W", x_plane);
  // the conv kernels address a sample's activation map with signed 32-bit byte offsets (largest map: H x W x 64 fp32)
  HLA_REQUIRE((size_t)H * W * 64 * 4 < ((size_t)1 << 31), "hla_vgg_forward: image too large (H*W must be below 2^23 pixels)");
  HLA_REQUIRE(level == 3 || level == 4, "hla_vgg_forward: level must be 3 (x15,x18,x21) or 4 (+x24), got %d", level);
  HLA_REQUIRE(feat[0] && feat[1] && feat[2], "hla_vgg_forward: feat[0..2] are required");
  HLA_REQUIRE(level == 3 || (feat[3] && params->w[11] && params->w[12]),
              "hla_vgg_forward: level 4 needs feat[3] ([B,H,W,64], 16 real channels) and the zero-padded conv_dec3 weights in w[11], w[12]");
  HLA_REQUIRE(level == 3 || !(flags & HLA_VGG_WANT_CONF) || !conf || !conf[3] || params->w[16], "hla_vgg_forward: conf[3] needs w[16]");
  HLA_REQUIRE(!(flags & HLA_VGG_DEFER_NORM) || inv_norm, "hla_vgg_forward: HLA_VGG_DEFER_NORM needs inv_norm");
  HLA_REQUIRE(!(flags & HLA_VGG_FEAT16) || ((dtype == HLA_BF16 || dtype == HLA_F16) && (flags & HLA_VGG_DEFER_NORM) &&
                                            !(flags & HLA_VGG_SAVE_FOR_BACKWARD) && level == 3),
              "hla_vgg_forward: HLA_VGG_FEAT16 needs dtype HLA_BF16 / HLA_F16, HLA_VGG_DEFER_NORM, level 3 and no HLA_VGG_SAVE_FOR_BACKWARD");
  HLA_REQUIRE(first_row8 == 0 || (first_row8 >= 4 && first_row8 < H / 8), "hla_vgg_forward: first_row8 must be 0 or in [4, H/8)");
  // folded decoder: the narrowest folded map (x15, W/16 wide) is up-sampled 2x into the W/8-wide dec1 geometry, so W/8 must be
  // even; the 32-px / 8-row conv tiles take partial tiles at the right / bottom edge as for any other width (the partial-sum
  // slots of the folded tile counts are planned by hla_vgg_workspace_bytes_flags, vgg_layers.h); every row of every map is read
  HLA_REQUIRE(!(flags & HLA_VGG_FOLD_DECODER) || (W % 16 == 0 && first_row8 == 0 && !(flags & HLA_VGG_FEAT16)),
              "hla_vgg_forward: HLA_VGG_FOLD_DECODER needs W %% 16 == 0 (folded maps are W/16, W/8, W/4 wide), first_row8 == 0 and no "
              "HLA_VGG_FEAT16 (got W = %d, first_row8 = %d)", W, first_row8);
  HLA_REQUIRE(first_col32 >= 0 && (first_col32 == 0 || 128 * first_col32 < W),
              "hla_vgg_forward_cols: first_col32 must be 0 or leave a column of the map (128 * first_col32 < W; got %d, W = %d)", first_col32, W);
  HLA_REQUIRE(!col_gate || first_col32 > 0, "hla_vgg_forward_cols: col_gate is the fix-up pass of a forward made with first_col32 > 0");
  first_col32 = vgg_first_col32(first_col32, level, dtype, flags);
  if (col_gate && !first_col32) return HLA_OK;      // that forward computed every column: nothing to fix
  VggPlan pl;
  vgg_plan(B, H, W, dtype, (flags & HLA_VGG_SAVE_FOR_BACKWARD) != 0, &pl, level == 4, (flags & HLA_VGG_FOLD_DECODER) != 0);
  if (workspace_bytes < pl.total) {
    hla_set_error("hla_vgg_forward: workspace %zu < %zu", workspace_bytes, pl.total);
    return HLA_ERR_WORKSPACE;
  }
  // The fix-up pass as one launch: the 16-bit types (first_col32 > 0 here says the rest: level 3, inference, deferred norm, no
  // confidence heads, no folded decoder).  fp32 and a profiled run, whose records are per layer, keep the ten gated launches.
  if (col_gate && fixup_one_launch && (dtype == HLA_BF16 || dtype == HLA_F16) && !hla_prof_on()) {
    if (dtype == HLA_BF16)
      return vgg_fixup_t<bf16>(x, x_plane, params, (const char*)packed_weights, dtype, feat, inv_norm, (char*)workspace, pl, B, H, W, flags,
                               first_row8, first_col32, col_gate, (hipStream_t)stream);
    return vgg_fixup_t<f16>(x, x_plane, params, (const char*)packed_weights, dtype, feat, inv_norm, (char*)workspace, pl, B, H, W, flags,
                            first_row8, first_col32, col_gate, (hipStream_t)stream);
  }
  if (dtype == HLA_BF16)
    return vgg_forward_t<bf16>(x, x_plane, params, (const char*)packed_weights, dtype, feat, conf, inv_norm, (char*)workspace, pl,
                               B, H, W, flags, first_row8, first_col32, col_gate, (hipStream_t)stream);
  if (dtype == HLA_F16)
    return vgg_forward_t<f16>(x, x_plane, params, (const char*)packed_weights, dtype, feat, conf, inv_norm, (char*)workspace, pl,
                              B, H, W, flags, first_row8, first_col32, col_gate, (hipStream_t)stream);
  if (dtype == HLA_F16X3)
    return vgg_forward_t<split32>(x, x_plane, params, (const char*)packed_weights, dtype, feat, conf, inv_norm, (char*)workspace, pl,
                                  B, H, W, flags, first_row8, first_col32, col_gate, (hipStream_t)stream);
  return vgg_forward_t<float>(x, x_plane, params, (const char*)packed_weights, dtype, feat, conf, inv_norm, (char*)workspace, pl,
                              B, H, W, flags, first_row8, first_col32, col_gate, (hipStream_t)stream);
}

extern "C" int hla_vgg_forward_cols(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights,
                                    void* const feat[4], float* const conf[4], double* inv_norm, void* workspace,
                                    size_t workspace_bytes, int B, int H, int W, int level, int dtype, int flags,
                                    int first_row8, int first_col32, const int* col_gate, hla_stream_t stream) {
  return vgg_forward_cols_impl(x, x_plane, params, packed_weights, feat, conf, inv_norm, workspace, workspace_bytes, B, H, W, level, dtype,
                               flags, first_row8, first_col32, col_gate, true, stream);
}

extern "C" int hla_vgg_fixup(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights,
                             void* const feat[4], double* inv_norm, void* workspace, size_t workspace_bytes, int B, int H, int W,
                             int level, int dtype, int flags, int first_row8, int first_col32, const int* col_gate, int one_launch,
                             hla_stream_t stream) {
  HLA_REQUIRE(col_gate, "hla_vgg_fixup: col_gate is required");
  return vgg_forward_cols_impl(x, x_plane, params, packed_weights, feat, nullptr, inv_norm, workspace, workspace_bytes, B, H, W, level,
                               dtype, flags, first_row8, first_col32, col_gate, one_launch != 0, stream);
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
  VggPlan pl[2];
  for (int k = 0; k < 2; ++k) {
    const hla_vgg_branch& b = br[k];
    const bool ok = b.x && b.params && b.packed_weights && b.workspace && B > 0 && b.H >= 8 && b.W >= 8 && b.H % 8 == 0 && b.W % 8 == 0 &&
                    (b.x_plane == 0 || b.x_plane >= (size_t)b.H * b.W) && (size_t)b.H * b.W * 64 * 4 < ((size_t)1 << 31) &&
                    b.feat[0] && b.feat[1] && b.feat[2] && (!(flags & HLA_VGG_DEFER_NORM) || b.inv_norm) &&
                    (!(flags & HLA_VGG_FEAT16) || ((dtype == HLA_BF16 || dtype == HLA_F16) && (flags & HLA_VGG_DEFER_NORM))) &&
                    (b.first_row8 == 0 || (b.first_row8 >= 4 && b.first_row8 < b.H / 8)) &&
                    b.first_col32 >= 0 && (b.first_col32 == 0 || 128 * b.first_col32 < b.W);
    if (!ok) return plain();
    vgg_plan(B, b.H, b.W, dtype, false, &pl[k], false, false);
    if (b.workspace_bytes < pl[k].total) return plain();
  }
  int rc;
  if (dtype == HLA_BF16) rc = vgg_forward_pair_t<bf16>(br, pl, B, dtype, flags, (hipStream_t)stream);
  else if (dtype == HLA_F16) rc = vgg_forward_pair_t<f16>(br, pl, B, dtype, flags, (hipStream_t)stream);
  else if (dtype == HLA_F16X3) rc = vgg_forward_pair_t<split32>(br, pl, B, dtype, flags, (hipStream_t)stream);
  else rc = vgg_forward_pair_t<float>(br, pl, B, dtype, flags, (hipStream_t)stream);
  if (rc == HLA_PAIR_FALLBACK) return plain();
  if (rc == HLA_OK && paired_out) *paired_out = 1;
  return rc;
}
#endif
