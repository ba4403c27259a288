// hla_s2g_pose_score: the objective LM_update minimises (models_kitti.py:982-996, models_ford.py:414-430), evaluated at K candidate
// poses per sample on ONE level's feature maps, without Jacobians -- what a pose search ranks its candidates by.
//   s = bilinearly sampled satellite feature x (ground mask x in-bounds)      (lm_pixel's weights, lm_common.h)
//   g = ground feature x ground mask,   w = grd_conf x ground mask (using_weight) or the ground mask
//   sums[b,k,0..7] = sum s^2, sum g^2, sum s g, sum w s^2, sum w g^2, sum w s g, #(ground mask AND in view), #(ground mask)
//   cost[b,k]      = sum w (s/||s|| - g/||g||)^2, both norms clamped at 1e-6, formed in fp64 from the sums and rounded once
// Two launches:
//   ps_accum  a block owns (sample, pixel tile, chunk of PS_KC hypotheses).  It reads the tile's points, weights and ground
//             vectors ONCE -- the ground vectors stay in registers, PS_NPL pixels of 16 bytes per lane -- and walks the chunk's
//             hypotheses over them: per batch of hypotheses the fp64 pixel set-up (lm_pixel) of every (hypothesis, pixel) pair goes
//             to LDS, then every wave gathers the four satellite taps of its pixels with lm_accum's lane layout (lanes over the
//             channel axis, 16 B per lane and tap).  Per-tile fp32 partials go to the workspace with plain stores.
//   ps_close  one wave per (sample, hypothesis): fixed-order fp64 reduction of the tile partials, the deferred-norm rescaling,
//             the cost.
// The tile size follows from the level alone (C and the element type), and a hypothesis never shares an accumulator with
// another one: sums and cost of (b, k) do not depend, bit for bit, on the other hypotheses, on k, on K, on B or on repeats.
#include "lm_host.h"

constexpr int PS_KC = 32;        // hypotheses per block
constexpr int PS_NPL = 4;        // pixels per lane (their ground vectors live in registers)
constexpr int PS_PP = 512;       // (hypothesis, pixel) set-ups per LDS batch; also the largest tile
constexpr int PS_NS = 8;         // values per (sample, hypothesis, tile)

struct PsArgs {
  const void* sat;      // [B,A,A,C] F
  const void* grd;      // [B,hs,w,C] F
  const float* conf;    // [B,hs,w] or null
  LmPoints pts;
  const float* poses;   // [B,K,3]
  const float* R_FL;    // [B,3,3] / [B,3] (Ford) or null
  const float* T_FL;
  LmGeom geom;
  float* part;          // [B,K,nt,PS_NS]
  int A, h, w, row0, npix, TP, nt, nch, K, B, xcd_affine;
  int hs, rskip;
};

// (lm_accum's channel-pair idiom, lm_solve.hip: two fp32 in adjacent registers so that the loop compiles to packed fp32 ops)
typedef float ps_f2 __attribute__((ext_vector_type(2)));
template <typename F> __device__ __forceinline__ ps_f2 ps_pair(const uint4& v, int ep);
template <> __device__ __forceinline__ ps_f2 ps_pair<float>(const uint4& v, int ep) {
  ps_f2 r;
  r.x = __uint_as_float(ep == 0 ? v.x : v.z);
  r.y = __uint_as_float(ep == 0 ? v.y : v.w);
  return r;
}
template <> __device__ __forceinline__ ps_f2 ps_pair<__bf16>(const uint4& v, int ep) {
  const unsigned w = ep == 0 ? v.x : ep == 1 ? v.y : ep == 2 ? v.z : v.w;
  ps_f2 r;
  r.x = __uint_as_float(w << 16);
  r.y = __uint_as_float(w & 0xffff0000u);
  return r;
}
template <> __device__ __forceinline__ ps_f2 ps_pair<_Float16>(const uint4& v, int ep) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const unsigned w = ep == 0 ? v.x : ep == 1 ? v.y : ep == 2 ? v.z : v.w;
  const h2 h = __builtin_bit_cast(h2, w);
  ps_f2 r;
  r.x = (float)h[0];
  r.y = (float)h[1];
  return r;
}

// pixels per block: PS_NPL wave-iterations of lm_accum's lane layout.  16 (C = 256, fp32) .. 512 (C = 16, 16-bit)
static inline int ps_tile(int C, int feat_dtype) {
  const int epl = feat_dtype == HLA_F32 ? 4 : 8;
  return 4 * (64 / (C / epl)) * PS_NPL;
}
static LmTiling ps_tiling(const hla_s2g_level& v) { return lm_tiling(lm_npix_s2g(v), [&](int) { return ps_tile(v.C, v.feat_dtype); }); }

template <int C, bool USE_W, typename F>
__global__ __launch_bounds__(256) void ps_accum(PsArgs a) {
  constexpr int EPL = 16 / (int)sizeof(F);   // channels per lane (16 B)
  constexpr int LPP = C / EPL;               // lanes per pixel
  constexpr int PPW = 64 / LPP;              // pixels per wave-iteration
  constexpr int TP = 4 * PPW * PS_NPL;
  constexpr int HB = (PS_PP / TP) < PS_KC ? (PS_PP / TP) : PS_KC;      // hypotheses per LDS batch
  static_assert(TP <= PS_PP && HB >= 1, "tile larger than the set-up buffer");
  __shared__ PixParam pp[PS_PP];
  __shared__ double scf[PS_KC][COEF_N];
  __shared__ float pq[TP][3];
  __shared__ float pgm[TP], pcw[TP];
  __shared__ float red[HB][4][6];

  int b, j;
  if (!lm_block_map(a.xcd_affine, a.nt * a.nch, a.B, b, j)) return;
  const int tile = j % a.nt, k0 = (j / a.nt) * PS_KC;
  const int nk = min(PS_KC, a.K - k0);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p0 = tile * TP;
  const int np = min(TP, a.npix - p0);

  if (t < nk) {
    const float* ps = a.poses + ((size_t)b * a.K + k0 + t) * 3;
    lm_coefficients(a.geom, (double)ps[0], (double)ps[1], (double)ps[2], a.R_FL ? a.R_FL + (size_t)b * 9 : nullptr,
                    a.T_FL ? a.T_FL + (size_t)b * 3 : nullptr, scf[t]);
  }
  for (int tt = t; tt < np; tt += 256) {
    const int p = p0 + tt;
    const int r = a.row0 + p / a.w, c = p % a.w;
    float q[3];
    const bool gm = lm_point(a.pts, b, r, c, a.w, q);
    pq[tt][0] = q[0]; pq[tt][1] = q[1]; pq[tt][2] = q[2];
    pgm[tt] = gm ? 1.f : 0.f;
    pcw[tt] = USE_W ? a.conf[((size_t)b * a.hs + (r - a.rskip)) * a.w + c] : 1.f;
  }
  __syncthreads();

  const int sub = lane / LPP, cl = (lane % LPP) * EPL;
  const bool first = (lane % LPP) == 0;      // the lane that counts its pixel
  const F* satb = (const F*)a.sat + (size_t)b * a.A * a.A * C + cl;
  const F* grdb = (const F*)a.grd + ((size_t)b * a.hs * a.w + (size_t)(a.row0 - a.rskip) * a.w + p0) * C + cl;

  // the tile's ground vectors, read once; sum g^2 and sum w g^2 do not depend on the hypothesis
  uint4 gg[PS_NPL];
  float aG = 0.f, aWG = 0.f, cG = 0.f;
#pragma unroll
  for (int n = 0; n < PS_NPL; ++n) {
    const int i = wave * PPW + sub + n * 4 * PPW;
    gg[n] = make_uint4(0u, 0u, 0u, 0u);
    if (i < np) {
      gg[n] = *(const uint4*)(grdb + (size_t)i * C);
      const float gm = pgm[i];
      ps_f2 g2 = {0.f, 0.f};
#pragma unroll
      for (int ep = 0; ep < EPL / 2; ++ep) {
        const ps_f2 g = ps_pair<F>(gg[n], ep) * gm;
        g2 += g * g;
      }
      const float Sgg = g2.x + g2.y;
      aG += Sgg;
      if (USE_W) aWG += (pcw[i] * gm) * Sgg;
      if (first) cG += gm;
    }
  }
  aG = wave_sum_f32(aG);
  aWG = wave_sum_f32(aWG);
  cG = wave_sum_f32(cG);
  if (lane == 0) { red[0][wave][0] = aG; red[0][wave][1] = aWG; red[0][wave][2] = cG; }
  __syncthreads();
  const float tG = (red[0][0][0] + red[0][1][0]) + (red[0][2][0] + red[0][3][0]);
  const float tWG = (red[0][0][1] + red[0][1][1]) + (red[0][2][1] + red[0][3][1]);
  const float tCG = (red[0][0][2] + red[0][1][2]) + (red[0][2][2] + red[0][3][2]);

  for (int h0 = 0; h0 < nk; h0 += HB) {
    const int nh = min(HB, nk - h0);
    __syncthreads();                         // the previous batch's pp / red have been consumed
    for (int e = t; e < nh * np; e += 256) {
      const int hh = e / np, i = e - hh * np;
      const float q[3] = {pq[i][0], pq[i][1], pq[i][2]};
      pp[hh * TP + i] = lm_pixel<C>(scf[h0 + hh], q, pgm[i] != 0.f, a.A, pcw[i]);
    }
    __syncthreads();
    for (int hh = 0; hh < nh; ++hh) {
      float aS = 0.f, aSG = 0.f, aWS = 0.f, aWSG = 0.f, cM = 0.f;
#pragma unroll
      for (int n = 0; n < PS_NPL; ++n) {
        const int i = wave * PPW + sub + n * 4 * PPW;
        if (i < np) {
          const PixParam P = pp[hh * TP + i];
          const uint4 t00 = *(const uint4*)(satb + P.off);
          const uint4 t01 = *(const uint4*)(satb + P.off + P.dxo);
          const uint4 t10 = *(const uint4*)(satb + P.off + P.dyo);
          const uint4 t11 = *(const uint4*)(satb + P.off + P.dyo + P.dxo);
          ps_f2 ss2 = {0.f, 0.f}, sg2 = ss2;
#pragma unroll
          for (int ep = 0; ep < EPL / 2; ++ep) {
            const ps_f2 c00 = ps_pair<F>(t00, ep), c01 = ps_pair<F>(t01, ep), c10 = ps_pair<F>(t10, ep), c11 = ps_pair<F>(t11, ep);
            const ps_f2 top = P.wx0 * c00 + P.wx1 * c01;
            const ps_f2 bot = P.wx0 * c10 + P.wx1 * c11;
            const ps_f2 s = P.wy0 * top + P.wy1 * bot;
            const ps_f2 g = ps_pair<F>(gg[n], ep) * P.gm;
            ss2 += s * s; sg2 += s * g;
          }
          const float Sss = ss2.x + ss2.y, Ssg = sg2.x + sg2.y;
          aS += Sss; aSG += Ssg;
          if (USE_W) { aWS += P.wt * Sss; aWSG += P.wt * Ssg; }
          if (first) cM += P.m;
        }
      }
      aS = wave_sum_f32(aS); aSG = wave_sum_f32(aSG); cM = wave_sum_f32(cM);
      if (USE_W) { aWS = wave_sum_f32(aWS); aWSG = wave_sum_f32(aWSG); }
      if (lane == 0) {
        red[hh][wave][0] = aS; red[hh][wave][1] = aSG; red[hh][wave][2] = aWS; red[hh][wave][3] = aWSG; red[hh][wave][4] = cM;
      }
    }
    __syncthreads();
    if (t < nh * PS_NS) {
      const int hh = t / PS_NS, k = t % PS_NS;
      // slot k of this tile: s^2, g^2, s g, w s^2, w g^2, w s g, in-view count, ground count (3..5 unused without weights)
      const int src = k == 0 ? 0 : k == 2 ? 1 : k == 3 ? 2 : k == 5 ? 3 : 4;
      float v = (red[hh][0][src] + red[hh][1][src]) + (red[hh][2][src] + red[hh][3][src]);
      if (k == 1) v = tG;
      if (k == 4) v = tWG;
      if (k == 7) v = tCG;
      a.part[(((size_t)b * a.K + k0 + h0 + hh) * a.nt + tile) * PS_NS + k] = v;
    }
  }
}

// one wave per (sample, hypothesis)
__global__ __launch_bounds__(64) void ps_close(const float* __restrict__ part, const double* __restrict__ sat_inv,
                                               const double* __restrict__ grd_inv, double* __restrict__ sums,
                                               float* __restrict__ cost, int nt, int K, int using_weight) {
  const size_t bk = blockIdx.x;
  const int lane = threadIdx.x, b = (int)(bk / K);
  double s[PS_NS];
#pragma unroll
  for (int k = 0; k < PS_NS; ++k) s[k] = 0.0;
  for (int i = lane; i < nt; i += 64) {
    const float* p = part + (bk * nt + i) * PS_NS;
#pragma unroll
    for (int k = 0; k < PS_NS; ++k) s[k] += (double)p[k];
  }
#pragma unroll
  for (int k = 0; k < PS_NS; ++k) s[k] = wave_sum_f64(s[k]);
  if (lane == 0) {
    // deferred L2_norm (VGG.py:511-514): s -> as*s, g -> ag*g
    const double as = sat_inv ? sat_inv[b] : 1.0, ag = grd_inv ? grd_inv[b] : 1.0;
    s[0] *= as * as; s[1] *= ag * ag; s[2] *= as * ag;
    if (using_weight) { s[3] *= as * as; s[4] *= ag * ag; s[5] *= as * ag; }
    else { s[3] = s[0]; s[4] = s[1]; s[5] = s[2]; }
#pragma unroll
    for (int k = 0; k < PS_NS; ++k) sums[bk * PS_NS + k] = s[k];
    const double ns = fmax(sqrt(s[0]), 1e-6), ng = fmax(sqrt(s[1]), 1e-6);      // models_kitti.py:982-990
    cost[bk] = (float)(s[3] / (ns * ns) + s[4] / (ng * ng) - 2.0 * s[5] / (ns * ng));
  }
}

template <bool W, typename F>
static void ps_launch_f(int C, dim3 grid, hipStream_t st, const PsArgs& a) {
  lm_dispatch_c<256, 128, 64, 16>(C, [&](auto c) { hipLaunchKernelGGL((ps_accum<decltype(c)::value, W, F>), grid, dim3(256), 0, st, a); });
}
template <bool W>
static void ps_launch(int C, int feat_dtype, dim3 grid, hipStream_t st, const PsArgs& a) {
  if (feat_dtype == HLA_BF16) ps_launch_f<W, __bf16>(C, grid, st, a);
  else if (feat_dtype == HLA_F16) ps_launch_f<W, _Float16>(C, grid, st, a);
  else ps_launch_f<W, float>(C, grid, st, a);
}

static int ps_check(const char* who, const hla_s2g_config* cfg, const hla_s2g_level* v, int B, int K) {
  HLA_REQUIRE(cfg && v, "%s: null argument", who);
  HLA_REQUIRE(B > 0 && K >= 1, "%s: need B > 0 and K >= 1", who);
  HLA_REQUIRE(!cfg->keep, "%s: cfg->keep (dropout) is not supported: a pose is scored on every pixel", who);
  HLA_REQUIRE(!v->depth, "%s: a level with depth != NULL is not supported (depth-lifted scoring is not built)", who);
  const int C = v->C;
  HLA_REQUIRE(C == 256 || C == 128 || C == 64 || C == 16, "%s: unsupported channel count %d", who, C);
  HLA_REQUIRE(v->feat_dtype == HLA_F32 || v->feat_dtype == HLA_BF16 || v->feat_dtype == HLA_F16,
              "%s: feat_dtype must be HLA_F32, HLA_BF16 or HLA_F16", who);
  HLA_REQUIRE(v->sat_feat && v->grd_feat && v->xyz, "%s: the level has null maps", who);
  HLA_REQUIRE(!cfg->using_weight || v->grd_conf, "%s: using_weight needs grd_conf", who);
  HLA_REQUIRE(v->A > 0 && v->h > 0 && v->w > 0, "%s: bad sizes", who);
  HLA_REQUIRE(v->row0 >= 0 && v->row0 < v->h, "%s: bad row0", who);
  HLA_REQUIRE(v->grd_row_skip >= 0 && v->grd_row_skip <= v->row0, "%s: grd_row_skip must be in [0,row0]", who);
  HLA_REQUIRE((size_t)v->A * v->A * C < (1u << 31), "%s: satellite map too large", who);
  HLA_REQUIRE((long long)(v->h - v->row0) * v->w < (1LL << 31), "%s: ground map too large", who);
  const long long blocks = (long long)lm_grid_blocks(1, B, 1) * ps_tiling(*v).nt * ((K + PS_KC - 1) / PS_KC);
  HLA_REQUIRE(blocks < (1LL << 31) && (long long)B * K < (1LL << 31), "%s: B * K too large for one launch", who);
  return HLA_OK;
}

// the one region: the tile partials [B,K,nt,PS_NS]
static size_t ps_ws_bytes(int B, int K, const LmTiling& t) { return lm_one_region_bytes((size_t)B * K * t.nt * PS_NS * sizeof(float)); }

extern "C" size_t hla_s2g_pose_score_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* level, int B, int K) {
  if (ps_check("hla_s2g_pose_score_workspace_bytes", cfg, level, B, K)) return 0;
  return ps_ws_bytes(B, K, ps_tiling(*level));
}

extern "C" int hla_s2g_pose_score(const hla_s2g_config* cfg, const hla_s2g_level* level, const float* R_FL, const float* T_FL,
                                  const float* poses, int K, double* sums, float* cost, void* workspace, size_t workspace_bytes,
                                  int B, hla_stream_t stream) {
  const int rc = ps_check("hla_s2g_pose_score", cfg, level, B, K);
  if (rc) return rc;
  HLA_REQUIRE(poses && sums && cost && workspace, "hla_s2g_pose_score: null argument");
  HLA_REQUIRE(!cfg->ford || (R_FL && T_FL), "hla_s2g_pose_score: Ford mode needs R_FL and T_FL");
  const hla_s2g_level& v = *level;
  PsArgs a{};
  a.sat = v.sat_feat; a.grd = v.grd_feat; a.conf = v.grd_conf; a.pts = lm_points_of(v);
  a.poses = poses; a.R_FL = cfg->ford ? R_FL : nullptr; a.T_FL = cfg->ford ? T_FL : nullptr;
  a.geom = lm_geom_of(cfg, v);
  const LmTiling til = ps_tiling(v);
  lm_fill_s2g_dims(a, v, til);
  a.nch = (K + PS_KC - 1) / PS_KC;
  a.K = K; a.B = B; a.xcd_affine = lm_xcd_affine(B);
  const size_t need = ps_ws_bytes(B, K, til);
  if (workspace_bytes < need) return lm_workspace_short("hla_s2g_pose_score", workspace_bytes, need);
  a.part = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = lm_grid_blocks(a.xcd_affine, B, a.nt * a.nch);
  const double esz = v.feat_dtype == HLA_F32 ? 4.0 : 2.0;
  hla_prof_begin(lm_prof_id(v.C), 0, (double)B * ((double)v.A * v.A + (double)a.npix * a.nch) * v.C * esz, st);
  if (cfg->using_weight) ps_launch<true>(v.C, v.feat_dtype, dim3(nblk), st, a);
  else ps_launch<false>(v.C, v.feat_dtype, dim3(nblk), st, a);
  hla_prof_end(st);
  hla_prof_begin(K_LMSOLVE, 0, (double)B * K * a.nt * PS_NS * 4.0, st);
  hipLaunchKernelGGL(ps_close, dim3((unsigned)((size_t)B * K)), dim3(64), 0, st, (const float*)a.part, v.sat_inv_norm, v.grd_inv_norm,
                     sums, cost, a.nt, K, cfg->using_weight ? 1 : 0);
  hla_prof_end(st);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// hla_s2g_pose_score_bwd: d(sum_bk d_cost[b,k] cost[b,k]) / d(the L2-normalised maps, the confidence), poses constant.
// With s, g the masked normalised values, N = sums[0], G = sums[1], a = sums[3], e = sums[4], c = sums[5], ns = max(sqrt N, 1e-6),
// ng alike (a clamped norm is a constant), w = conf x ground mask (using_weight) or the ground mask:
//   d cost/d s    = 2 w s/ns^2 - 2 a s/ns^4 - 2 w g/(ns ng) + 2 c s/(ns^3 ng)       pixels in view
//   d cost/d g    = 2 w g/ng^2 - 2 e g/ng^4 - 2 w s/(ns ng) + 2 c g/(ng^3 ns)       pixels with the ground mask
//   d cost/d conf = ground mask x sum_channels (s/ns - g/ng)^2
// (the second and fourth terms are absent where the norm is clamped; without weights and unclamped a = N, e = G: the first two
// terms cancel identically and only the other two are formed).
// Two launches behind one zero-fill (d_sat, the stored ground rows above row0):
//   psb_coef   one block per sample: the per-(sample, hypothesis) scalars, d_cost folded in, formed in fp64 from the sums and
//              rounded once; the parts of d cost/d g that multiply g are sums over k of scalars -- added in fp64 in a fixed order
//              and applied once per pixel.  A hypothesis with d_cost == 0 or nothing in view is marked inactive.
//   psb_accum  a block owns (sample, pixel tile) for ALL K hypotheses: ps_accum's set-up (lm_coefficients / lm_point / lm_pixel
//              through LDS batches) with lanes over the channel axis, four channels per lane.  A lane group owns a RUN of PSB_NPL
//              consecutive pixels.  The tile's ground vectors and its d_grd / d_conf sums stay in registers over the hypothesis
//              loop (k ascending) and are stored once with plain stores: bitwise reproducible, independent of B.  d_sat goes out
//              as fp32 atomics; the contributions of consecutive pixels of a run that fall into one texel cell are merged in
//              registers first (lm_bwd_accum's idiom) and a cell is flushed when it changes and at the end of a hypothesis.  An
//              inactive hypothesis is skipped with a block-uniform branch (no set-up, no loads); a pixel out of view loads no
//              tap and issues no atomic.
// Measured at KITTI shapes, B = 32, K = 126 (EXPERIMENTS.md, "Pose search: score_loss"; the kernel runs at the rate of its atomics):
//   ps_accum's lane layout (16 B per lane and tap) and runs of 4: 37 / 74 / 148 ms per level -- an atomic wave-instruction then
//   touches every fourth float of the lines it covers; lm_bwd_accum's layout (a lane owns channels j, j + LPP, ..: whole 64-B
//   requests) 9.1 / 28 / 66 ms; runs of 8 on top of it (more pixels per texel cell; 197 VGPRs, 2 waves per SIMD) 6.4 / 14.7 / 30.2 ms.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int PSB_NC = 8;        // floats per (sample, hypothesis): k0 k1 k2 1/ns 1/ng d_cost active pad
constexpr int PSB_NB = 4;        // floats per sample: sum_k gw, sum_k g1, sum over the inactive k of d_cost / ng^2, pad
constexpr int PSB_NPL = 8;       // consecutive pixels per lane group: the run whose texel cells are merged before the atomics

// pixels per block: 32 (C = 256) .. 512 (C = 16); a function of C alone
static inline int psb_tile(int C) { return 4 * (64 / (C / 4)) * PSB_NPL; }
static LmTiling psb_tiling(const hla_s2g_level& v) { return lm_tiling(lm_npix_s2g(v), [&](int) { return psb_tile(v.C); }); }

__global__ __launch_bounds__(256) void psb_coef(const double* __restrict__ sums, const float* __restrict__ d_cost,
                                                float* __restrict__ kc, float* __restrict__ kb, int K, int using_weight) {
  __shared__ double red[3][256];
  const int b = blockIdx.x, t = threadIdx.x;
  double aGW = 0.0, aG1 = 0.0, aC0 = 0.0;
  for (int k = t; k < K; k += 256) {
    const size_t bk = (size_t)b * K + k;
    const double* s = sums + bk * PS_NS;
    const double dc = (double)d_cost[bk];
    const double rs = sqrt(s[0]), rg = sqrt(s[1]);
    const bool fs = rs >= 1e-6, fg = rg >= 1e-6;          // the norm is a function of the map (else the constant 1e-6)
    const double is = 1.0 / (fs ? rs : 1e-6), ig = 1.0 / (fg ? rg : 1e-6);
    double k0 = 2.0 * dc * is * is, k1 = 0.0, gw = 2.0 * dc * ig * ig, g1 = 0.0;
    if (using_weight) {
      if (fs) k1 = dc * (-2.0 * s[3] * is * is * is * is + 2.0 * s[5] * is * is * is * ig);
      if (fg) g1 = dc * (-2.0 * s[4] * ig * ig * ig * ig + 2.0 * s[5] * ig * ig * ig * is);
    } else {
      if (fs) { k0 = 0.0; k1 = 2.0 * dc * s[5] * is * is * is * ig; }
      if (fg) { gw = 0.0; g1 = 2.0 * dc * s[5] * ig * ig * ig * is; }
    }
    const bool active = dc != 0.0 && s[6] > 0.0;
    float* o = kc + bk * PSB_NC;
    o[0] = (float)k0; o[1] = (float)k1; o[2] = (float)(2.0 * dc * is * ig); o[3] = (float)is; o[4] = (float)ig; o[5] = (float)dc;
    o[6] = active ? 1.f : 0.f; o[7] = 0.f;
    aGW += gw; aG1 += g1;
    if (!active) aC0 += dc * ig * ig;
  }
  red[0][t] = aGW; red[1][t] = aG1; red[2][t] = aC0;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                     // fixed tree: the same bits whatever else runs
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
    __syncthreads();
  }
  if (t < PSB_NB) kb[(size_t)b * PSB_NB + t] = t < 3 ? (float)red[t][0] : 0.f;
}

struct PsbArgs {
  const float* sat; const float* grd; const float* conf;
  LmPoints pts;
  const float* poses; const float* R_FL; const float* T_FL;
  LmGeom geom;
  const float* kc; const float* kb;
  const double* sat_inv; const double* grd_inv;
  float* d_sat; float* d_grd; float* d_conf;
  int A, h, w, row0, npix, TP, nt, K, B, xcd_affine;
  int hs, rskip;
};

template <int C, bool USE_W>
__global__ __launch_bounds__(256) void psb_accum(PsbArgs a) {
  constexpr int EPL = 4;                     // channels per lane (16 B of fp32)
  constexpr int LPP = C / EPL;               // lanes per pixel
  constexpr int PPW = 64 / LPP;              // lane groups per wave
  constexpr int TP = 4 * PPW * PSB_NPL;       // = psb_tile(C)
  constexpr int HB = (PS_PP / TP) < PS_KC ? (PS_PP / TP) : PS_KC;      // hypotheses per LDS batch
  static_assert(TP <= PS_PP && HB >= 1, "tile larger than the set-up buffer");
  __shared__ PixParam pp[PS_PP];
  __shared__ double scf[PS_KC][COEF_N];
  __shared__ float skc[PS_KC][PSB_NC];
  __shared__ float pq[TP][3];
  __shared__ float pgm[TP], pcw[TP];

  int b, tile;
  if (!lm_block_map(a.xcd_affine, a.nt, a.B, b, tile)) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p0 = tile * TP;
  const int np = min(TP, a.npix - p0);
  for (int tt = t; tt < np; tt += 256) {
    const int p = p0 + tt;
    const int r = a.row0 + p / a.w, c = p % a.w;
    float q[3];
    const bool gm = lm_point(a.pts, b, r, c, a.w, q);
    pq[tt][0] = q[0]; pq[tt][1] = q[1]; pq[tt][2] = q[2];
    pgm[tt] = gm ? 1.f : 0.f;
    pcw[tt] = USE_W ? a.conf[((size_t)b * a.hs + (r - a.rskip)) * a.w + c] : 1.f;
  }
  __syncthreads();

  auto uni = [](float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
  const float as = uni(a.sat_inv ? (float)a.sat_inv[b] : 1.f), ag = uni(a.grd_inv ? (float)a.grd_inv[b] : 1.f);
  const float sGW = uni(a.kb[(size_t)b * PSB_NB + 0]), sG1 = uni(a.kb[(size_t)b * PSB_NB + 1]), sC0 = uni(a.kb[(size_t)b * PSB_NB + 2]);
  // lane j of a pixel's LPP lanes owns channels j, j + LPP, j + 2 LPP, j + 3 LPP (lm_bwd_accum's layout): every load, store and
  // atomic instruction covers LPP consecutive floats per pixel -- whole 64-B requests at the memory side, where the atomics execute
  const int sub = lane / LPP, cl = lane % LPP;
  const int grp = wave * PPW + sub;          // this lane group's pixels: grp * PSB_NPL + n
  const float* satb = a.sat + (size_t)b * a.A * a.A * C + cl;
  float* dsatb = a.d_sat + (size_t)b * a.A * a.A * C + cl;
  const size_t grd_first = ((size_t)b * a.hs * a.w + (size_t)(a.row0 - a.rskip) * a.w + p0) * C + cl;

  // the run's masked, normalised ground vectors, its weights and what it accumulates over the hypotheses
  float gt[PSB_NPL][EPL], ax[PSB_NPL][EPL], wv[PSB_NPL], cc[PSB_NPL], sgg[PSB_NPL];
#pragma unroll
  for (int n = 0; n < PSB_NPL; ++n) {
    const int i = grp * PSB_NPL + n;
    wv[n] = 0.f; cc[n] = 0.f; sgg[n] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) { gt[n][e] = 0.f; ax[n][e] = 0.f; }
    if (i < np) {
      const float* g = a.grd + grd_first + (size_t)i * C;
      const float m = ag * pgm[i];
#pragma unroll
      for (int e = 0; e < EPL; ++e) gt[n][e] = g[e * LPP] * m;
      wv[n] = USE_W ? pcw[i] * pgm[i] : 1.f;
      sgg[n] = (gt[n][0] * gt[n][0] + gt[n][1] * gt[n][1]) + (gt[n][2] * gt[n][2] + gt[n][3] * gt[n][3]);
    }
  }

  for (int k0 = 0; k0 < a.K; k0 += PS_KC) {
    const int nk = min(PS_KC, a.K - k0);
    __syncthreads();                         // the previous chunk's scalars have been consumed
    if (t < nk) {
      const float* src = a.kc + ((size_t)b * a.K + k0 + t) * PSB_NC;
#pragma unroll
      for (int e = 0; e < PSB_NC; ++e) skc[t][e] = src[e];
      if (src[6] != 0.f) {
        const float* ps = a.poses + ((size_t)b * a.K + k0 + t) * 3;
        lm_coefficients(a.geom, (double)ps[0], (double)ps[1], (double)ps[2], a.R_FL ? a.R_FL + (size_t)b * 9 : nullptr,
                        a.T_FL ? a.T_FL + (size_t)b * 3 : nullptr, scf[t]);
      }
    }
    __syncthreads();
    for (int h0 = 0; h0 < nk; h0 += HB) {
      const int nh = min(HB, nk - h0);
      __syncthreads();                       // the previous batch's set-ups have been consumed
      for (int e = t; e < nh * np; e += 256) {
        const int hh = e / np, i = e - hh * np;
        if (skc[h0 + hh][6] != 0.f) {
          const float q[3] = {pq[i][0], pq[i][1], pq[i][2]};
          pp[hh * TP + i] = lm_pixel<C>(scf[h0 + hh], q, pgm[i] != 0.f, a.A, pcw[i]);
        }
      }
      __syncthreads();
      for (int hh = 0; hh < nh; ++hh) {
        const float* kk = skc[h0 + hh];
        if (kk[6] == 0.f) continue;          // block-uniform: d_cost == 0 or nothing in view
        const float K0 = kk[0], K1 = kk[1], K2 = kk[2], ins = kk[3], ing = kk[4], dc = kk[5];
        int cur_off = -1, cur_dxo = 0, cur_dyo = 0;
        float c00[EPL], c01[EPL], c10[EPL], c11[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) c00[e] = c01[e] = c10[e] = c11[e] = 0.f;
        auto flush_cell = [&]() {
          if (cur_off >= 0) {
            float* o = dsatb + cur_off;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              atomicAdd(o + e * LPP, c00[e]); atomicAdd(o + cur_dxo + e * LPP, c01[e]);
              atomicAdd(o + cur_dyo + e * LPP, c10[e]); atomicAdd(o + cur_dyo + cur_dxo + e * LPP, c11[e]);
            }
          }
        };
#pragma unroll
        for (int n = 0; n < PSB_NPL; ++n) {
          const int i = grp * PSB_NPL + n;
          if (i < np) {
            const PixParam P = pp[hh * TP + i];
            if (P.m != 0.f) {
              if (P.off != cur_off || P.dxo != cur_dxo || P.dyo != cur_dyo) {
                flush_cell();
                cur_off = P.off; cur_dxo = P.dxo; cur_dyo = P.dyo;
#pragma unroll
                for (int e = 0; e < EPL; ++e) c00[e] = c01[e] = c10[e] = c11[e] = 0.f;
              }
              const float* sp = satb + P.off;
              float v00[EPL], v01[EPL], v10[EPL], v11[EPL];
#pragma unroll
              for (int e = 0; e < EPL; ++e) {
                v00[e] = sp[e * LPP]; v01[e] = sp[P.dxo + e * LPP];
                v10[e] = sp[P.dyo + e * LPP]; v11[e] = sp[P.dyo + P.dxo + e * LPP];
              }
              const float w = wv[n];
              const float ks = w * K0 + K1, kg = w * K2;
              const float w00 = P.wy0 * P.wx0, w01 = P.wy0 * P.wx1, w10 = P.wy1 * P.wx0, w11 = P.wy1 * P.wx1;
              float dd = 0.f;
#pragma unroll
              for (int e = 0; e < EPL; ++e) {
                const float top = P.wx0 * v00[e] + P.wx1 * v01[e], bot = P.wx0 * v10[e] + P.wx1 * v11[e];
                const float s = (P.wy0 * top + P.wy1 * bot) * as;
                const float g = gt[n][e];
                const float gs = ks * s - kg * g;
                c00[e] += gs * w00; c01[e] += gs * w01; c10[e] += gs * w10; c11[e] += gs * w11;
                ax[n][e] += K2 * s;
                if (USE_W) { const float d = s * ins - g * ing; dd += d * d; }
              }
              if (USE_W) cc[n] += dc * dd;
            } else if (USE_W) {
              cc[n] += (dc * ing * ing) * sgg[n];        // s = 0: the residual is -g / ng
            }
          }
        }
        flush_cell();
      }
    }
  }

  // one plain store per element
#pragma unroll
  for (int n = 0; n < PSB_NPL; ++n) {
    const int i = grp * PSB_NPL + n;
    if (i < np) {
      const float w = wv[n], kgg = w * sGW + sG1;
      float* o = a.d_grd + grd_first + (size_t)i * C;
#pragma unroll
      for (int e = 0; e < EPL; ++e) o[e * LPP] = kgg * gt[n][e] - w * ax[n][e];
      if (USE_W) {
        float qw = cc[n] + sC0 * sgg[n];     // (the LPP lanes of a pixel share `i`: they are all inside this branch together)
#pragma unroll
        for (int x = LPP >> 1; x > 0; x >>= 1) qw += __shfl_xor(qw, x, 64);
        if (cl == 0) {
          const int p = p0 + i;
          const int r = a.row0 + p / a.w, c = p % a.w;
          a.d_conf[((size_t)b * a.hs + (r - a.rskip)) * a.w + c] = qw * pgm[i];
        }
      }
    }
  }
}

template <bool W>
static void psb_launch(int C, dim3 grid, hipStream_t st, const PsbArgs& a) {
  lm_dispatch_c<256, 128, 64, 16>(C, [&](auto c) { hipLaunchKernelGGL((psb_accum<decltype(c)::value, W>), grid, dim3(256), 0, st, a); });
}

static int psb_check(const char* who, const hla_s2g_config* cfg, const hla_s2g_level* v, int B, int K) {
  const int rc = ps_check(who, cfg, v, B, K);
  if (rc) return rc;
  HLA_REQUIRE(v->feat_dtype == HLA_F32, "%s: feat_dtype must be HLA_F32: the backward reads fp32 maps (every training path keeps "
              "them), 16-bit maps are not supported", who);
  HLA_REQUIRE(!cfg->deterministic, "%s: cfg->deterministic is not supported (d_sat_feat is summed with fp32 atomics; d_grd_feat and "
              "d_grd_conf are reproducible as they are)", who);
  return HLA_OK;
}

struct PsbWs { size_t kc, kb, total; };
static PsbWs psb_ws(int B, int K) {
  PsbWs W{};
  LmBump ws;
  W.kc = ws.take((size_t)B * K * PSB_NC * sizeof(float));
  W.kb = ws.take((size_t)B * PSB_NB * sizeof(float));
  W.total = ws.o;
  return W;
}

extern "C" size_t hla_s2g_pose_score_bwd_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* level, int B, int K) {
  if (psb_check("hla_s2g_pose_score_bwd_workspace_bytes", cfg, level, B, K)) return 0;
  return psb_ws(B, K).total;
}

extern "C" int hla_s2g_pose_score_bwd(const hla_s2g_config* cfg, const hla_s2g_level* level, const hla_s2g_level_grad* grad,
                                      const float* R_FL, const float* T_FL, const float* poses, int K, const double* sums,
                                      const float* d_cost, void* workspace, size_t workspace_bytes, int B, hla_stream_t stream) {
  const int rc = psb_check("hla_s2g_pose_score_bwd", cfg, level, B, K);
  if (rc) return rc;
  HLA_REQUIRE(grad && poses && sums && d_cost && workspace, "hla_s2g_pose_score_bwd: null argument");
  HLA_REQUIRE(grad->d_sat_feat && grad->d_grd_feat, "hla_s2g_pose_score_bwd: gradient buffers missing");
  HLA_REQUIRE(!cfg->using_weight || grad->d_grd_conf, "hla_s2g_pose_score_bwd: using_weight needs d_grd_conf");
  HLA_REQUIRE(!cfg->ford || (R_FL && T_FL), "hla_s2g_pose_score_bwd: Ford mode needs R_FL and T_FL");
  const hla_s2g_level& v = *level;
  const PsbWs W = psb_ws(B, K);
  if (workspace_bytes < W.total) return lm_workspace_short("hla_s2g_pose_score_bwd", workspace_bytes, W.total);
  hipStream_t st = (hipStream_t)stream;
  PsbArgs a{};
  a.sat = (const float*)v.sat_feat; a.grd = (const float*)v.grd_feat; a.conf = v.grd_conf; a.pts = lm_points_of(v);
  a.poses = poses; a.R_FL = cfg->ford ? R_FL : nullptr; a.T_FL = cfg->ford ? T_FL : nullptr;
  a.geom = lm_geom_of(cfg, v);
  a.kc = (const float*)((char*)workspace + W.kc); a.kb = (const float*)((char*)workspace + W.kb);
  a.sat_inv = v.sat_inv_norm; a.grd_inv = v.grd_inv_norm;
  a.d_sat = grad->d_sat_feat; a.d_grd = grad->d_grd_feat; a.d_conf = cfg->using_weight ? grad->d_grd_conf : nullptr;
  const LmTiling til = psb_tiling(v);
  lm_fill_s2g_dims(a, v, til);
  a.K = K; a.B = B; a.xcd_affine = lm_xcd_affine(B);

  // what the kernels do not store: the satellite gradient the atomics add to, and the stored ground rows above row0
  hla_fill_region reg[3];
  int nr = 0;
  const size_t sat_bytes = (size_t)B * v.A * v.A * v.C * sizeof(float);
  reg[nr++] = hla_fill_region{a.d_sat, sat_bytes, sat_bytes, 1};
  const size_t top = (size_t)(v.row0 - v.grd_row_skip) * v.w, all = (size_t)a.hs * v.w;
  if (top > 0) {
    reg[nr++] = hla_fill_region{a.d_grd, top * v.C * sizeof(float), all * v.C * sizeof(float), B};
    if (a.d_conf) reg[nr++] = hla_fill_region{a.d_conf, top * sizeof(float), all * sizeof(float), B};
  }
  const int frc = hla_zero_fill(reg, nr, 0, stream);
  if (frc) return frc;

  hla_prof_begin(K_LMSOLVE, 0, (double)B * K * (PS_NS * 8.0 + PSB_NC * 4.0), st);
  hipLaunchKernelGGL(psb_coef, dim3(B), dim3(256), 0, st, sums, d_cost, (float*)((char*)workspace + W.kc),
                     (float*)((char*)workspace + W.kb), K, cfg->using_weight ? 1 : 0);
  hla_prof_end(st);
  const int nblk = lm_grid_blocks(a.xcd_affine, B, a.nt);
  hla_prof_begin(K_LMBWD, 0, (double)B * ((double)v.A * v.A * 2.0 + (double)a.npix * 2.0) * v.C * 4.0, st);
  if (cfg->using_weight) psb_launch<true>(v.C, dim3(nblk), st, a);
  else psb_launch<false>(v.C, dim3(nblk), st, a);
  hla_prof_end(st);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}
