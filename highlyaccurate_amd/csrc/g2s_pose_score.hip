// hla_g2s_pose_score: LM_G2SP's matching term (project_grd_to_map, models_kitti.py:163-303, or inplane_grd_to_map, 289-332, and
// the residual of LM_update, 333-379) evaluated at K candidate poses per sample on ONE level's feature maps, without Jacobians --
// what a pose search in the ground -> satellite direction ranks its candidates by.  For every pixel of the A x A satellite map:
//   f = the ground feature sampled where the pixel projects (g2s_pixel / g2s_ip_pixel of lm_g2s.h: the loop's own set-up)
//   s = the satellite feature,   w = the projected confidence (using_weight) or 1,   "in view" = the projection is in bounds
//   sums[b,k,0..7] = sum f^2, sum s^2, sum f s, sum w f^2, sum w s^2, sum w f s over the pixels in view, #(in view), sum s^2 over ALL
//   cost[b,k]      = sum w (f/||f|| - s/||s||)^2 over the overlap, norms clamped at 1e-6, formed in fp64 from the sums and rounded
//                    once; +inf when nothing is in view
// (The loop itself does not renormalise; its raw objective would reward a pose for seeing less, hence the overlap-normalised form.)
// Two launches, the structure of pose_score.hip with the roles swapped:
//   gps_accum  a block owns (sample, tile of satellite pixels, chunk of GPS_KC hypotheses).  It reads the tile's satellite vectors
//              ONCE -- they stay in registers, GPS_NPL pixels of 16 bytes per lane, with each pixel's ||s||^2 share -- and walks
//              the chunk's hypotheses over them: per batch of hypotheses the fp64 pixel set-up of every (hypothesis, pixel) pair
//              goes to LDS, then every wave gathers the four ground taps of its pixels IN VIEW with g2s_accum's lane layout (lanes
//              over the channel axis, 16 B per lane and tap); a pixel out of view issues no load and adds nothing, which leaves
//              every accumulator bit for bit what adding its zeros would.  Per-tile fp32 partials go to the workspace with plain stores.
//   gps_close  one wave per (sample, hypothesis): fixed-order fp64 reduction of the tile partials, the deferred-norm rescaling,
//              the cost.
// The tile size follows from C alone, and a hypothesis never shares an accumulator with another one: sums and cost of (b, k) do
// not depend, bit for bit, on the other hypotheses, on k, on K, on B or on repeats.
// (hla_g2s_pose_score_bwd, the gradient of the cost with respect to the maps, is the second half of this file.)
#include "lm_g2s.h"
#include "lm_host.h"

constexpr int GPS_KC = 32;        // hypotheses per block
constexpr int GPS_NPL = 4;        // pixels per lane (their satellite vectors live in registers)
constexpr int GPS_PP = 512;       // (hypothesis, pixel) set-ups per LDS batch; also the largest tile
constexpr int GPS_NS = 8;         // values per (sample, hypothesis, tile)

struct __attribute__((aligned(16))) GpsPix {
  int off, dxo, dyo;              // taps as in G2sPix; off = -1 marks a pixel out of view
  float wx0, wx1, wy0, wy1;
  float wt;                       // projected confidence (or 1)
};

struct GpsArgs {
  const float* grd;     // [B,h,w,C] (gathered)
  const float* sat;     // [B,A,A,C]
  const float* conf;    // [B,h,w] or null
  const float* poses;   // [B,K,3]
  const float* camera_k;   // [B,3,3] (proj 0)
  G2sGeom geom;
  float* part;          // [B,K,nt,GPS_NS]
  int A, h, w, ctr, npix, nt, nch, K, B, xcd_affine;
};

// pixels per block: GPS_NPL wave-iterations of g2s_accum's lane layout.  16 (C = 256) .. 256 (C = 16)
static inline int gps_tile(int C) { return 4 * (64 / (C / 4)) * GPS_NPL; }
static LmTiling gps_tiling(const hla_s2g_level& v) { return lm_tiling(lm_npix_g2s(v), [&](int) { return gps_tile(v.C); }); }

// The loop's pixel set-up without its Jacobian columns.  In view <=> in bounds, which the loop's records show as a nonzero weight
// or, for the one in-bounds point whose four clamped-corner weights vanish (u = w-1 and v = h-1 exactly), a nonzero offset.
template <int C, bool USE_W, int PROJ>
__device__ __forceinline__ GpsPix gps_pixel(const double* cf, int row, int col, int ctr, int h, int w, const float* conf) {
  GpsPix o;
  if constexpr (PROJ == 1) {
    const G2sIpPix q = g2s_ip_pixel<C>(cf, row, col, h, w);
    o.off = q.off; o.dxo = q.dxo; o.dyo = q.dyo; o.wx0 = q.wx0; o.wx1 = q.wx1; o.wy0 = q.wy0; o.wy1 = q.wy1; o.wt = 1.f;
  } else {
    const G2sPix q = g2s_pixel<C, USE_W>(cf, row, col, ctr, h, w, conf);
    o.off = q.off; o.dxo = q.dxo; o.dyo = q.dyo; o.wx0 = q.wx0; o.wx1 = q.wx1; o.wy0 = q.wy0; o.wy1 = q.wy1; o.wt = q.wt;
  }
  const bool view = (o.wx0 + o.wx1 + o.wy0 + o.wy1) != 0.f || o.off != 0;
  if (!view) o.off = -1;
  return o;
}

template <int C, bool USE_W, int PROJ>
__global__ __launch_bounds__(256) void gps_accum(GpsArgs a) {
  constexpr int LPP = C / 4;                 // lanes per pixel (16 B of fp32 per lane)
  constexpr int PPW = 64 / LPP;              // pixels per wave-iteration
  constexpr int TP = 4 * PPW * GPS_NPL;
  constexpr int HB = (GPS_PP / TP) < GPS_KC ? (GPS_PP / TP) : GPS_KC;      // hypotheses per LDS batch
  static_assert(TP <= GPS_PP && HB >= 1, "tile larger than the set-up buffer");
  __shared__ GpsPix pp[GPS_PP];
  __shared__ double scf[GPS_KC][G2S_COEF_N];
  __shared__ float red[HB][4][7];

  int b, j;
  if (!lm_block_map(a.xcd_affine, a.nt * a.nch, a.B, b, j)) return;
  const int tile = j % a.nt, k0 = (j / a.nt) * GPS_KC;
  const int nk = min(GPS_KC, a.K - k0);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p0 = tile * TP;
  const int np = min(TP, a.npix - p0);

  if (t < nk) {
    const float* ps = a.poses + ((size_t)b * a.K + k0 + t) * 3;
    if (PROJ == 1) g2s_ip_coefficients(a.geom, (double)ps[0], (double)ps[1], (double)ps[2], scf[t]);
    else g2s_coefficients(a.geom, (double)ps[0], (double)ps[1], (double)ps[2], a.camera_k + (size_t)b * 9, scf[t]);
  }

  const int sub = lane / LPP, cl = (lane % LPP) * 4;
  const bool first = (lane % LPP) == 0;      // the lane that counts its pixel
  const float* grdb = a.grd + (size_t)b * a.h * a.w * C + cl;
  const float* satb = a.sat + ((size_t)b * a.npix + p0) * C + cl;
  const float* confb = USE_W ? a.conf + (size_t)b * a.h * a.w : nullptr;

  // the tile's satellite vectors, read once, and this lane's share of every pixel's ||s||^2
  float4 ss[GPS_NPL];
  float sq[GPS_NPL];
  float aAll = 0.f;
#pragma unroll
  for (int n = 0; n < GPS_NPL; ++n) {
    const int i = wave * PPW + sub + n * 4 * PPW;
    ss[n] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < np) ss[n] = *(const float4*)(satb + (size_t)i * C);
    sq[n] = (ss[n].x * ss[n].x + ss[n].y * ss[n].y) + (ss[n].z * ss[n].z + ss[n].w * ss[n].w);
    aAll += sq[n];
  }
  aAll = wave_sum_f32(aAll);
  if (lane == 0) red[0][wave][0] = aAll;
  __syncthreads();                           // (also: scf is written)
  const float tAll = (red[0][0][0] + red[0][1][0]) + (red[0][2][0] + red[0][3][0]);      // sum s^2 over the whole tile

  for (int h0 = 0; h0 < nk; h0 += HB) {
    const int nh = min(HB, nk - h0);
    __syncthreads();                         // the previous batch's pp / red have been consumed
    for (int e = t; e < nh * np; e += 256) {
      const int hh = e / np, i = e - hh * np, p = p0 + i;
      pp[hh * TP + i] = gps_pixel<C, USE_W, PROJ>(scf[h0 + hh], p / a.A, p % a.A, a.ctr, a.h, a.w, confb);
    }
    __syncthreads();
    for (int hh = 0; hh < nh; ++hh) {
      float aF = 0.f, aS = 0.f, aFS = 0.f, aWF = 0.f, aWS = 0.f, aWFS = 0.f, cM = 0.f;
#pragma unroll
      for (int n = 0; n < GPS_NPL; ++n) {
        const int i = wave * PPW + sub + n * 4 * PPW;
        if (i < np) {
          const GpsPix P = pp[hh * TP + i];
          if (P.off >= 0) {              // in view; a wave-iteration with no such pixel issues no gather
            const float4 t00 = *(const float4*)(grdb + P.off);
            const float4 t01 = *(const float4*)(grdb + P.off + P.dxo);
            const float4 t10 = *(const float4*)(grdb + P.off + P.dyo);
            const float4 t11 = *(const float4*)(grdb + P.off + P.dyo + P.dxo);
            const float a00[4] = {t00.x, t00.y, t00.z, t00.w}, a01[4] = {t01.x, t01.y, t01.z, t01.w};
            const float a10[4] = {t10.x, t10.y, t10.z, t10.w}, a11[4] = {t11.x, t11.y, t11.z, t11.w};
            const float as[4] = {ss[n].x, ss[n].y, ss[n].z, ss[n].w};
            float ff[4], fs[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float top = P.wx0 * a00[e] + P.wx1 * a01[e];
              const float bot = P.wx0 * a10[e] + P.wx1 * a11[e];
              const float f = P.wy0 * top + P.wy1 * bot;                     // projected ground feature (g2s_accum's form)
              ff[e] = f * f; fs[e] = f * as[e];
            }
            const float Sff = (ff[0] + ff[1]) + (ff[2] + ff[3]), Sfs = (fs[0] + fs[1]) + (fs[2] + fs[3]);
            aF += Sff; aS += sq[n]; aFS += Sfs;
            if (USE_W) { aWF += P.wt * Sff; aWS += P.wt * sq[n]; aWFS += P.wt * Sfs; }
            if (first) cM += 1.f;
          }
        }
      }
      aF = wave_sum_f32(aF); aS = wave_sum_f32(aS); aFS = wave_sum_f32(aFS); cM = wave_sum_f32(cM);
      if (USE_W) { aWF = wave_sum_f32(aWF); aWS = wave_sum_f32(aWS); aWFS = wave_sum_f32(aWFS); }
      if (lane == 0) {
        red[hh][wave][0] = aF; red[hh][wave][1] = aS; red[hh][wave][2] = aFS;
        red[hh][wave][3] = aWF; red[hh][wave][4] = aWS; red[hh][wave][5] = aWFS; red[hh][wave][6] = cM;
      }
    }
    __syncthreads();
    if (t < nh * GPS_NS) {
      const int hh = t / GPS_NS, k = t % GPS_NS;
      // slot k of this tile: f^2, s^2, f s, w f^2, w s^2, w f s, in-view count, s^2 of the whole tile (3..5 unused without weights)
      const int src = k < 7 ? k : 0;
      float v = (red[hh][0][src] + red[hh][1][src]) + (red[hh][2][src] + red[hh][3][src]);
      if (k == 7) v = tAll;
      a.part[(((size_t)b * a.K + k0 + h0 + hh) * a.nt + tile) * GPS_NS + k] = v;
    }
  }
}

// one wave per (sample, hypothesis)
__global__ __launch_bounds__(64) void gps_close(const float* __restrict__ part, const double* __restrict__ grd_inv,
                                                const double* __restrict__ sat_inv, double* __restrict__ sums,
                                                float* __restrict__ cost, int nt, int K, int using_weight) {
  const size_t bk = blockIdx.x;
  const int lane = threadIdx.x, b = (int)(bk / K);
  double s[GPS_NS];
#pragma unroll
  for (int k = 0; k < GPS_NS; ++k) s[k] = 0.0;
  for (int i = lane; i < nt; i += 64) {
    const float* p = part + (bk * nt + i) * GPS_NS;
#pragma unroll
    for (int k = 0; k < GPS_NS; ++k) s[k] += (double)p[k];
  }
#pragma unroll
  for (int k = 0; k < GPS_NS; ++k) s[k] = wave_sum_f64(s[k]);
  if (lane == 0) {
    // deferred L2_norm (VGG.py:511-514), as g2s_solve applies it to its own sums: f -> af*f, s -> as*s
    const double af = grd_inv ? grd_inv[b] : 1.0, as = sat_inv ? sat_inv[b] : 1.0;
    s[0] *= af * af; s[1] *= as * as; s[2] *= af * as; s[7] *= as * as;
    if (using_weight) { s[3] *= af * af; s[4] *= as * as; s[5] *= af * as; }
    else { s[3] = s[0]; s[4] = s[1]; s[5] = s[2]; }
#pragma unroll
    for (int k = 0; k < GPS_NS; ++k) sums[bk * GPS_NS + k] = s[k];
    const double nf = fmax(sqrt(s[0]), 1e-6), ns = fmax(sqrt(s[1]), 1e-6);
    const double c = s[3] / (nf * nf) + s[4] / (ns * ns) - 2.0 * s[5] / (nf * ns);
    cost[bk] = s[6] == 0.0 ? __builtin_inff() : (float)c;
  }
}

template <bool W, int PROJ>
static void gps_launch(int C, dim3 grid, hipStream_t st, const GpsArgs& a) {
  auto go = [&](auto c) { hipLaunchKernelGGL((gps_accum<decltype(c)::value, W, PROJ>), grid, dim3(256), 0, st, a); };
  if constexpr (PROJ == 1) lm_dispatch_c<256, 128, 64, 16>(C, go);      // (16 channels exist under proj 1 only, g2s_validate)
  else lm_dispatch_c<256, 128, 64>(C, go);
}

static int gps_check(const char* who, const hla_s2g_config* cfg, const hla_s2g_level* v, const float* camera_k, int ori_h,
                     int ori_w, int B, int K, bool need_camera) {
  HLA_REQUIRE(cfg && v, "%s: null argument", who);
  HLA_REQUIRE(B > 0 && K >= 1, "%s: need B > 0 and K >= 1", who);
  HLA_REQUIRE(!cfg->ford, "%s: LM_G2SP is KITTI-only (models_kitti.py:22-499)", who);
  hla_s2g_config one = *cfg;
  one.n_levels = 1;
  if (const int rc = g2s_validate(who, &one, v, camera_k, ori_h, ori_w, need_camera)) return rc;
  HLA_REQUIRE(v->feat_dtype == HLA_F32, "%s: fp32 feature maps only", who);
  HLA_REQUIRE(v->sat_feat && v->grd_feat, "%s: the level has null maps", who);
  HLA_REQUIRE(!cfg->using_weight || v->grd_conf, "%s: using_weight needs grd_conf", who);
  HLA_REQUIRE(v->grd_row_skip == 0, "%s: the whole ground map is sampled (grd_row_skip must be 0)", who);
  HLA_REQUIRE(!v->depth, "%s: a depth map belongs to hla_s2g_* (LM_G2SP ignores gt_depth)", who);
  HLA_REQUIRE((long long)v->h * v->w >= 2, "%s: a 1 x 1 ground map is not supported", who);
  HLA_REQUIRE((size_t)v->A * v->A * v->C < (1u << 31), "%s: satellite map too large", who);
  const long long blocks = (long long)lm_grid_blocks(1, B, 1) * gps_tiling(*v).nt * ((K + GPS_KC - 1) / GPS_KC);
  HLA_REQUIRE(blocks < (1LL << 31) && (long long)B * K < (1LL << 31), "%s: B * K too large for one launch", who);
  return HLA_OK;
}

// the one region: the tile partials [B,K,nt,GPS_NS]
static size_t gps_ws_bytes(int B, int K, const LmTiling& t) { return lm_one_region_bytes((size_t)B * K * t.nt * GPS_NS * sizeof(float)); }

extern "C" size_t hla_g2s_pose_score_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* level, int B, int K) {
  if (gps_check("hla_g2s_pose_score_workspace_bytes", cfg, level, nullptr, 0, 0, B, K, false)) return 0;
  return gps_ws_bytes(B, K, gps_tiling(*level));
}

extern "C" int hla_g2s_pose_score(const hla_s2g_config* cfg, const hla_s2g_level* level, const float* camera_k, int ori_h, int ori_w,
                                  const float* poses, int K, double* sums, float* cost, void* workspace, size_t workspace_bytes,
                                  int B, hla_stream_t stream) {
  const int rc = gps_check("hla_g2s_pose_score", cfg, level, camera_k, ori_h, ori_w, B, K, true);
  if (rc) return rc;
  HLA_REQUIRE(poses && sums && cost && workspace, "hla_g2s_pose_score: null argument");
  const hla_s2g_level& v = *level;
  GpsArgs a{};
  a.grd = (const float*)v.grd_feat; a.sat = (const float*)v.sat_feat; a.conf = v.grd_conf;
  a.poses = poses; a.camera_k = camera_k; a.geom = g2s_geom_of(cfg, v, ori_h, ori_w);
  const LmTiling til = gps_tiling(v);
  lm_fill_g2s_dims(a, v, til);
  a.nch = (K + GPS_KC - 1) / GPS_KC;
  a.K = K; a.B = B; a.xcd_affine = lm_xcd_affine(B);
  const size_t need = gps_ws_bytes(B, K, til);
  if (workspace_bytes < need) return lm_workspace_short("hla_g2s_pose_score", workspace_bytes, need);
  a.part = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = lm_grid_blocks(a.xcd_affine, B, a.nt * a.nch);
  hla_prof_begin(lm_prof_id(v.C), 0, (double)B * ((double)v.h * v.w + (double)a.npix * a.nch) * v.C * 4.0, st);
  if (cfg->proj) gps_launch<false, 1>(v.C, dim3(nblk), st, a);
  else if (cfg->using_weight) gps_launch<true, 0>(v.C, dim3(nblk), st, a);
  else gps_launch<false, 0>(v.C, dim3(nblk), st, a);
  hla_prof_end(st);
  hla_prof_begin(K_LMSOLVE, 0, (double)B * K * a.nt * GPS_NS * 4.0, st);
  hipLaunchKernelGGL(gps_close, dim3((unsigned)((size_t)B * K)), dim3(64), 0, st, (const float*)a.part, v.grd_inv_norm, v.sat_inv_norm,
                     sums, cost, a.nt, K, cfg->using_weight ? 1 : 0);
  hla_prof_end(st);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// hla_g2s_pose_score_bwd: d(sum_bk d_cost[b,k] cost[b,k]) / d(the L2-normalised maps, the confidence), poses constant.
// With f, s, w as above, N = sums[0], S = sums[1], a = sums[3], e = sums[4], c = sums[5], nf = max(sqrt N, 1e-6), ns alike (a
// clamped norm is a constant), per pixel IN VIEW and per channel:
//   d cost/d f = 2 w f/nf^2 - 2 a f/nf^4 - 2 w s/(nf ns) + 2 c f/(nf^3 ns)      spread to the four ground taps (gps_pixel's weights)
//   d cost/d s = 2 w s/ns^2 - 2 e s/ns^4 - 2 w f/(nf ns) + 2 c s/(ns^3 nf)      on the satellite pixel itself
//   d cost/d w = sum_channels (f/nf - s/ns)^2                                   spread to the same four taps of grd_conf
// (the second and fourth terms are absent where the norm is clamped; without weights and unclamped a = N, e = S: the first two
// terms cancel identically and only the other two are formed).  A pixel out of view gets nothing; sums[7] does not enter.
// Two launches behind one zero-fill (d_grd, d_conf):
//   gpsb_coef   one thread per (sample, hypothesis): the scalars above, d_cost folded in, formed in fp64 from the sums and rounded
//               once.  A hypothesis with d_cost == 0 or nothing in view is marked inactive.
//   gpsb_accum  a block owns (sample, tile of satellite pixels) for ALL K hypotheses, k ascending: gps_accum's set-up
//               (g2s_coefficients / g2s_ip_coefficients and gps_pixel through LDS batches: the forward's in-view decision, bit
//               for bit) with lm_bwd_accum's lane layout (lane j of a pixel's LPP lanes owns channels j, j + LPP, ..: every
//               atomic instruction covers whole 64-B requests; the other layout cost 4x in psb_accum).  A lane group owns a RUN
//               of GPSB_NPL consecutive satellite pixels.  The run's satellite vectors and its d_sat sums stay in registers over
//               the hypothesis loop and are stored once with plain stores, zeros included: d_sat_feat is bitwise reproducible
//               and independent of B and of repeats.  d_grd_feat and d_grd_conf go out as fp32 atomics -- NOT bitwise
//               reproducible -- after the contributions of consecutive pixels of a run that fall into one texel cell have been
//               merged in registers (g2s_bwd_accum's flush_cell idiom: under proj 0 the satellite pixels far ahead of the camera
//               crowd into a few ground texels; under proj 1 the warp has unit scale and a cell is rarely shared); a cell is
//               flushed when it changes and at the end of a hypothesis.  An inactive hypothesis is skipped with a block-uniform
//               branch (no set-up, no loads, no atomics); a pixel out of view loads no tap and issues no atomic.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int GPSB_NC = 8;       // floats per (sample, hypothesis): F0 F1 K2 S0 S1 1/nf 1/ns d_cost (0 marks an inactive one)
constexpr int GPSB_NPL = 8;      // consecutive pixels per lane group: the run whose texel cells are merged before the atomics

// pixels per block: 32 (C = 256) .. 512 (C = 16); a function of C alone
static inline int gpsb_tile(int C) { return 4 * (64 / (C / 4)) * GPSB_NPL; }
static LmTiling gpsb_tiling(const hla_s2g_level& v) { return lm_tiling(lm_npix_g2s(v), [&](int) { return gpsb_tile(v.C); }); }

__global__ __launch_bounds__(256) void gpsb_coef(const double* __restrict__ sums, const float* __restrict__ d_cost,
                                                 float* __restrict__ kc, long long BK, int using_weight) {
  const long long bk = (long long)blockIdx.x * 256 + threadIdx.x;
  if (bk >= BK) return;
  const double* s = sums + bk * GPS_NS;
  const double dc = (double)d_cost[bk];
  const double rf = sqrt(s[0]), rs = sqrt(s[1]);
  const bool ff = rf >= 1e-6, fs = rs >= 1e-6;            // the norm is a function of the map (else the constant 1e-6)
  const double jf = 1.0 / (ff ? rf : 1e-6), js = 1.0 / (fs ? rs : 1e-6);
  double F0 = 2.0 * dc * jf * jf, F1 = 0.0, S0 = 2.0 * dc * js * js, S1 = 0.0;
  if (using_weight) {
    if (ff) F1 = dc * (-2.0 * s[3] * jf * jf * jf * jf + 2.0 * s[5] * jf * jf * jf * js);
    if (fs) S1 = dc * (-2.0 * s[4] * js * js * js * js + 2.0 * s[5] * js * js * js * jf);
  } else {
    if (ff) { F0 = 0.0; F1 = 2.0 * dc * s[5] * jf * jf * jf * js; }
    if (fs) { S0 = 0.0; S1 = 2.0 * dc * s[5] * js * js * js * jf; }
  }
  const bool active = dc != 0.0 && s[6] > 0.0;
  float* o = kc + bk * GPSB_NC;
  o[0] = (float)F0; o[1] = (float)F1; o[2] = (float)(2.0 * dc * jf * js); o[3] = (float)S0; o[4] = (float)S1;
  o[5] = (float)jf; o[6] = (float)js; o[7] = active ? (float)dc : 0.f;
}

struct GpsbArgs {
  const float* grd; const float* sat; const float* conf;
  const float* poses; const float* camera_k;
  G2sGeom geom;
  const float* kc;
  const double* grd_inv; const double* sat_inv;
  float* d_sat; float* d_grd; float* d_conf;
  int A, h, w, ctr, npix, nt, K, B, xcd_affine;
};

template <int C, bool USE_W, int PROJ>
__global__ __launch_bounds__(256) void gpsb_accum(GpsbArgs a) {
  constexpr int EPL = 4;                     // channels per lane
  constexpr int LPP = C / EPL;               // lanes per pixel
  constexpr int PPW = 64 / LPP;              // lane groups per wave
  constexpr int TP = 4 * PPW * GPSB_NPL;     // = gpsb_tile(C)
  constexpr int HB = (GPS_PP / TP) < GPS_KC ? (GPS_PP / TP) : GPS_KC;      // hypotheses per LDS batch
  static_assert(TP <= GPS_PP && HB >= 1, "tile larger than the set-up buffer");
  __shared__ GpsPix pp[GPS_PP];
  __shared__ double scf[GPS_KC][G2S_COEF_N];
  __shared__ float skc[GPS_KC][GPSB_NC];

  int b, tile;
  if (!lm_block_map(a.xcd_affine, a.nt, a.B, b, tile)) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int p0 = tile * TP;
  const int np = min(TP, a.npix - p0);

  auto uni = [](float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
  const float af = uni(a.grd_inv ? (float)a.grd_inv[b] : 1.f), as = uni(a.sat_inv ? (float)a.sat_inv[b] : 1.f);
  const int sub = lane / LPP, cl = lane % LPP;      // lane j owns channels j, j + LPP, j + 2 LPP, j + 3 LPP
  const int grp = wave * PPW + sub;          // this lane group's pixels: grp * GPSB_NPL + n
  const size_t grd_base = (size_t)b * a.h * a.w * C + cl;
  const float* grdb = a.grd + grd_base;
  float* dgrdb = a.d_grd + grd_base;
  const size_t sat_first = ((size_t)b * a.npix + p0) * C + cl;
  const float* confb = USE_W ? a.conf + (size_t)b * a.h * a.w : nullptr;
  float* dconfb = USE_W ? a.d_conf + (size_t)b * a.h * a.w : nullptr;

  // the run's normalised satellite vectors and what it accumulates over the hypotheses: d_sat = cs * s - ax
  float st[GPSB_NPL][EPL], ax[GPSB_NPL][EPL], cs[GPSB_NPL];
#pragma unroll
  for (int n = 0; n < GPSB_NPL; ++n) {
    const int i = grp * GPSB_NPL + n;
    cs[n] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) { st[n][e] = 0.f; ax[n][e] = 0.f; }
    if (i < np) {
      const float* g = a.sat + sat_first + (size_t)i * C;
#pragma unroll
      for (int e = 0; e < EPL; ++e) st[n][e] = g[e * LPP] * as;
    }
  }

  for (int k0 = 0; k0 < a.K; k0 += GPS_KC) {
    const int nk = min(GPS_KC, a.K - k0);
    __syncthreads();                         // the previous chunk's scalars have been consumed
    if (t < nk) {
      const float* src = a.kc + ((size_t)b * a.K + k0 + t) * GPSB_NC;
#pragma unroll
      for (int e = 0; e < GPSB_NC; ++e) skc[t][e] = src[e];
      if (src[7] != 0.f) {
        const float* ps = a.poses + ((size_t)b * a.K + k0 + t) * 3;
        if (PROJ == 1) g2s_ip_coefficients(a.geom, (double)ps[0], (double)ps[1], (double)ps[2], scf[t]);
        else g2s_coefficients(a.geom, (double)ps[0], (double)ps[1], (double)ps[2], a.camera_k + (size_t)b * 9, scf[t]);
      }
    }
    __syncthreads();
    for (int h0 = 0; h0 < nk; h0 += HB) {
      const int nh = min(HB, nk - h0);
      __syncthreads();                       // the previous batch's set-ups have been consumed
      for (int e = t; e < nh * np; e += 256) {
        const int hh = e / np, i = e - hh * np, p = p0 + i;
        if (skc[h0 + hh][7] != 0.f) pp[hh * TP + i] = gps_pixel<C, USE_W, PROJ>(scf[h0 + hh], p / a.A, p % a.A, a.ctr, a.h, a.w, confb);
      }
      __syncthreads();
      for (int hh = 0; hh < nh; ++hh) {
        const float* kk = skc[h0 + hh];
        if (kk[7] == 0.f) continue;          // block-uniform: d_cost == 0 or nothing in view
        const float F0 = kk[0], F1 = kk[1], K2 = kk[2], S0 = kk[3], S1 = kk[4], inf = kk[5], ins = kk[6], dc = kk[7];
        int cur_off = -1, cur_dxo = 0, cur_dyo = 0;
        float c00[EPL], c01[EPL], c10[EPL], c11[EPL], cw[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < EPL; ++e) c00[e] = c01[e] = c10[e] = c11[e] = 0.f;
        auto flush_cell = [&]() {
          if (cur_off >= 0) {
            float* o = dgrdb + cur_off;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              atomicAdd(o + e * LPP, c00[e]); atomicAdd(o + cur_dxo + e * LPP, c01[e]);
              atomicAdd(o + cur_dyo + e * LPP, c10[e]); atomicAdd(o + cur_dyo + cur_dxo + e * LPP, c11[e]);
            }
            if (USE_W) {                     // (the LPP lanes of a pixel share its cell: they are all inside this branch together)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int x = LPP >> 1; x > 0; x >>= 1) cw[q] += __shfl_xor(cw[q], x, 64);
              }
              if (cl == 0) {
                float* oc = dconfb + cur_off / C;
                const int dx = cur_dxo / C, dy = cur_dyo / C;
                atomicAdd(oc, cw[0]); atomicAdd(oc + dx, cw[1]); atomicAdd(oc + dy, cw[2]); atomicAdd(oc + dy + dx, cw[3]);
              }
            }
          }
        };
#pragma unroll
        for (int n = 0; n < GPSB_NPL; ++n) {
          const int i = grp * GPSB_NPL + n;
          if (i < np) {
            const GpsPix P = pp[hh * TP + i];
            if (P.off >= 0) {                // in view: the forward's decision
              if (P.off != cur_off || P.dxo != cur_dxo || P.dyo != cur_dyo) {
                flush_cell();
                cur_off = P.off; cur_dxo = P.dxo; cur_dyo = P.dyo;
#pragma unroll
                for (int e = 0; e < EPL; ++e) c00[e] = c01[e] = c10[e] = c11[e] = 0.f;
                cw[0] = cw[1] = cw[2] = cw[3] = 0.f;
              }
              const float* gp = grdb + P.off;
              float v00[EPL], v01[EPL], v10[EPL], v11[EPL];
#pragma unroll
              for (int e = 0; e < EPL; ++e) {
                v00[e] = gp[e * LPP]; v01[e] = gp[P.dxo + e * LPP];
                v10[e] = gp[P.dyo + e * LPP]; v11[e] = gp[P.dyo + P.dxo + e * LPP];
              }
              const float w = USE_W ? P.wt : 1.f;
              const float kf = w * F0 + F1, kx = w * K2;
              const float w00 = P.wy0 * P.wx0, w01 = P.wy0 * P.wx1, w10 = P.wy1 * P.wx0, w11 = P.wy1 * P.wx1;
              cs[n] += w * S0 + S1;
              float dd = 0.f;
#pragma unroll
              for (int e = 0; e < EPL; ++e) {
                const float top = P.wx0 * v00[e] + P.wx1 * v01[e], bot = P.wx0 * v10[e] + P.wx1 * v11[e];
                const float f = (P.wy0 * top + P.wy1 * bot) * af;
                const float s = st[n][e];
                const float gf = kf * f - kx * s;
                c00[e] += gf * w00; c01[e] += gf * w01; c10[e] += gf * w10; c11[e] += gf * w11;
                ax[n][e] += kx * f;
                if (USE_W) { const float d = f * inf - s * ins; dd += d * d; }
              }
              if (USE_W) {
                const float gw = dc * dd;    // this lane's channels' share of d/d(projected confidence)
                cw[0] += gw * w00; cw[1] += gw * w01; cw[2] += gw * w10; cw[3] += gw * w11;
              }
            }
          }
        }
        flush_cell();
      }
    }
  }

  // one plain store per element, zeros included
#pragma unroll
  for (int n = 0; n < GPSB_NPL; ++n) {
    const int i = grp * GPSB_NPL + n;
    if (i < np) {
      float* o = a.d_sat + sat_first + (size_t)i * C;
#pragma unroll
      for (int e = 0; e < EPL; ++e) o[e * LPP] = cs[n] * st[n][e] - ax[n][e];
    }
  }
}

template <bool W, int PROJ>
static void gpsb_launch(int C, dim3 grid, hipStream_t st, const GpsbArgs& a) {
  auto go = [&](auto c) { hipLaunchKernelGGL((gpsb_accum<decltype(c)::value, W, PROJ>), grid, dim3(256), 0, st, a); };
  if constexpr (PROJ == 1) lm_dispatch_c<256, 128, 64, 16>(C, go);
  else lm_dispatch_c<256, 128, 64>(C, go);
}

static int gpsb_check(const char* who, const hla_s2g_config* cfg, const hla_s2g_level* v, const float* camera_k, int ori_h,
                      int ori_w, int B, int K, bool need_camera) {
  const int rc = gps_check(who, cfg, v, camera_k, ori_h, ori_w, B, K, need_camera);
  if (rc) return rc;
  HLA_REQUIRE(!cfg->keep, "%s: cfg->keep (dropout) is not supported: a pose is scored on every pixel", who);
  HLA_REQUIRE(!cfg->deterministic, "%s: cfg->deterministic is not supported (d_grd_feat and d_grd_conf are summed with fp32 atomics; "
              "d_sat_feat is reproducible as it is)", who);
  return HLA_OK;
}

// the one region: the scalars [B,K,GPSB_NC]
static size_t gpsb_ws_bytes(int B, int K) { return lm_one_region_bytes((size_t)B * K * GPSB_NC * sizeof(float)); }

extern "C" size_t hla_g2s_pose_score_bwd_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* level, int B, int K) {
  if (gpsb_check("hla_g2s_pose_score_bwd_workspace_bytes", cfg, level, nullptr, 0, 0, B, K, false)) return 0;
  return gpsb_ws_bytes(B, K);
}

extern "C" int hla_g2s_pose_score_bwd(const hla_s2g_config* cfg, const hla_s2g_level* level, const hla_s2g_level_grad* grad,
                                      const float* camera_k, int ori_h, int ori_w, const float* poses, int K, const double* sums,
                                      const float* d_cost, void* workspace, size_t workspace_bytes, int B, hla_stream_t stream) {
  const int rc = gpsb_check("hla_g2s_pose_score_bwd", cfg, level, camera_k, ori_h, ori_w, B, K, true);
  if (rc) return rc;
  HLA_REQUIRE(grad && poses && sums && d_cost && workspace, "hla_g2s_pose_score_bwd: null argument");
  HLA_REQUIRE(grad->d_sat_feat && grad->d_grd_feat, "hla_g2s_pose_score_bwd: gradient buffers missing");
  HLA_REQUIRE(!cfg->using_weight || grad->d_grd_conf, "hla_g2s_pose_score_bwd: using_weight needs d_grd_conf");
  const hla_s2g_level& v = *level;
  const size_t need = gpsb_ws_bytes(B, K);
  if (workspace_bytes < need) return lm_workspace_short("hla_g2s_pose_score_bwd", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  GpsbArgs a{};
  a.grd = (const float*)v.grd_feat; a.sat = (const float*)v.sat_feat; a.conf = v.grd_conf;
  a.poses = poses; a.camera_k = camera_k; a.geom = g2s_geom_of(cfg, v, ori_h, ori_w);
  a.kc = (const float*)workspace;
  a.grd_inv = v.grd_inv_norm; a.sat_inv = v.sat_inv_norm;
  a.d_sat = grad->d_sat_feat; a.d_grd = grad->d_grd_feat; a.d_conf = cfg->using_weight ? grad->d_grd_conf : nullptr;
  const LmTiling til = gpsb_tiling(v);
  lm_fill_g2s_dims(a, v, til);
  a.K = K; a.B = B; a.xcd_affine = lm_xcd_affine(B);

  // what the atomics add to
  hla_fill_region reg[2];
  int nr = 0;
  const size_t grd_px = (size_t)B * v.h * v.w;
  reg[nr++] = hla_fill_region{a.d_grd, grd_px * v.C * sizeof(float), grd_px * v.C * sizeof(float), 1};
  if (a.d_conf) reg[nr++] = hla_fill_region{a.d_conf, grd_px * sizeof(float), grd_px * sizeof(float), 1};
  const int frc = hla_zero_fill(reg, nr, 0, stream);
  if (frc) return frc;

  const long long BK = (long long)B * K;
  hla_prof_begin(K_LMSOLVE, 0, (double)BK * (GPS_NS * 8.0 + GPSB_NC * 4.0), st);
  hipLaunchKernelGGL(gpsb_coef, dim3((unsigned)((BK + 255) / 256)), dim3(256), 0, st, sums, d_cost, (float*)workspace, BK,
                     cfg->using_weight ? 1 : 0);
  hla_prof_end(st);
  const int nblk = lm_grid_blocks(a.xcd_affine, B, a.nt);
  hla_prof_begin(K_LMBWD, 0, (double)B * ((double)v.h * v.w * 2.0 + (double)a.npix * 2.0) * v.C * 4.0, st);
  if (cfg->proj) gpsb_launch<false, 1>(v.C, dim3(nblk), st, a);
  else if (cfg->using_weight) gpsb_launch<true, 0>(v.C, dim3(nblk), st, a);
  else gpsb_launch<false, 0>(v.C, dim3(nblk), st, a);
  hla_prof_end(st);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}
