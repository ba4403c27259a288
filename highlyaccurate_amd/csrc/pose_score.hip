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
