// Multi-view localisation on the Ford chain: ONE LM loop over V ground images per satellite tile, each with its own rigid
// transform (R_v, T_v) to the one body pose being solved for (hla_s2g_lm_solve_views, include/hla.h).  One step is the
// reference's LM_update (models_ford.py:384-466) on the UNION of the views' pixels: every view's 14 sums are formed and
// de-normalised as hla_s2g_lm_solve forms them, added in fp64 in view order, and the unchanged lm_solve_step solves from the total.
//
// Two launches per step on the caller's stream, no tickets, no side streams, no atomics:
//   lmv_accum<C>  grid (tiles x pseudo-samples j = b * V + v): the tile body of lm_accum (lm_tile_body.h) on view v of sample b;
//                 the tile's 14 partials are published with plain stores for the next launch
//   lmv_close     one wave per sample: per view, in order, the fixed-order fp64 reduction of its tiles (as lm_solve_body does
//                 it), the de-normalisation and the add into the total; then the solve, the pose update and re-initialisation
//                 rule, the trace row, and the projection coefficients of all V views for the NEXT step's level
// The init launch is lmv_close without partials.  Nothing of sample b depends on B, on its batch mates or on repeats.
#include "lm_fwd.h"
#include "lm_views.h"

static_assert(LMV_COEF_N == COEF_N && LMV_PART_N == PART_N, "lm_views.h restates COEF_N / PART_N of lm_common.h");

template <int C, bool USE_W, typename F>
__global__ __launch_bounds__(256, LM_OCC) void lmv_accum(AccumArgs in, int V) {
  __shared__ PixParam pp[FWD_MAX_TP];
  __shared__ float red[4][14];
  __shared__ double redd[14];
  int j, tile;
  if (!lm_block_map(in.xcd_affine, in.nt, in.nb, j, tile)) return;
  // The fragment sees a batch of ONE (its b is 0): every array it indexes by b is handed over at this pseudo-sample's element --
  // ground map, confidence and partial-sum rows at j, the satellite map at sample j / V, the table at view j % V.  Nothing of
  // the fragment changes, so lm_accum and lm_repair_loop compile to what they compiled to before this kernel existed.
  AccumArgs a = in;
  a.sat = (const F*)in.sat + lmv_sat_offset(j, V, in.A, C);
  a.grd = (const F*)in.grd + lmv_grd_offset(j, in.hs, in.w, C);
  if (USE_W) a.conf = in.conf + lmv_conf_offset(j, in.hs, in.w);
  a.pts.xyz = in.pts.xyz + lmv_table_offset(j, V, in.h, in.w);
  a.part = in.part + lmv_part_offset(j, 0, in.part_ld);
  constexpr int b = 0;
  const int t = threadIdx.x;
  constexpr bool active = true;
#define LM_TILE_COEF (in.coef + lmv_coef_offset(j))
#define LM_TILE_BEFORE_PUBLISH
#include "lm_tile_body.h"
#undef LM_TILE_COEF
#undef LM_TILE_BEFORE_PUBLISH
  (void)lane; (void)wave;
}

struct LmvCloseArgs {
  const double* part;    // [B*V,part_ld,PART_N] of the step being closed, or null (init launch)
  const double* sat_inv; // [B] or null
  const double* grd_inv; // [B*V] or null
  int nt, part_ld, V;
  float* pose;           // [B,3] running pose
  float* trace_out;      // &trace[0][iter][level][0] of this step (sample stride = trace_stride)
  int trace_stride;
  const float* rand_uv;  // [2,B] of this step, or null
  double* normal_eq;     // [B,16] of this step, or null: the TOTAL sums
  double* view_sums;     // [B,V,16] of this step, or null: each view's de-normalised sums
  double* coef;          // [B*V,COEF_N] out for the next step, or null
  const float* R;        // [B,V,3,3]
  const float* T;        // [B,V,3]
  int B, reinit, zero_pose;
  LmSolveCfg cfg;
  LmGeom next;           // geometry of the level the NEXT step runs on
};

__global__ __launch_bounds__(64) void lmv_close(LmvCloseArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, V = a.V;
  float su = a.pose[b * 3 + 0], sv = a.pose[b * 3 + 1], th = a.pose[b * 3 + 2];
  if (!a.part && a.zero_pose) {
    su = sv = th = 0.f;
    if (lane < 3) a.pose[b * 3 + lane] = 0.f;
  }
  if (a.part) {
    double tot[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) tot[k] = 0.0;
    const double as = a.sat_inv ? a.sat_inv[b] : 1.0;
    for (int v = 0; v < V; ++v) {
      const int j = lmv_pseudo(b, v, V);
      double s[14];
#pragma unroll
      for (int k = 0; k < 14; ++k) s[k] = 0.0;
      for (int i = lane; i < a.nt; i += 64) {
        const double* p = a.part + lmv_part_offset(j, i, a.part_ld);
#pragma unroll
        for (int k = 0; k < 14; ++k) s[k] += p[k];
      }
#pragma unroll
      for (int k = 0; k < 14; ++k) s[k] = wave_sum_f64(s[k]);      // (every lane ends with the same bits)
      // deferred L2_norm, as lm_solve_body: s -> as*s, J -> as*J, g -> ag*g, with THIS view's ground norm
      const double ag = a.grd_inv ? a.grd_inv[j] : 1.0;
      s[0] *= as * as; s[1] *= ag * ag;
#pragma unroll
      for (int k = 2; k < 11; ++k) s[k] *= as * as;
#pragma unroll
      for (int k = 11; k < 14; ++k) s[k] *= as * ag;
      if (a.view_sums && lane < 16) {
        double val = 0.0;
#pragma unroll
        for (int k = 0; k < 14; ++k) val = lane == k ? s[k] : val;
        a.view_sums[lmv_view_sums_offset(b, v, V) + lane] = val;
      }
#pragma unroll
      for (int k = 0; k < 14; ++k) tot[k] += s[k];                 // view order: ((0 + s_0) + s_1) + ...
    }
    if (lane == 0) {
      if (a.normal_eq) {
        for (int k = 0; k < 14; ++k) a.normal_eq[(size_t)b * 16 + k] = tot[k];
        a.normal_eq[(size_t)b * 16 + 14] = 0.0;
        a.normal_eq[(size_t)b * 16 + 15] = 0.0;
      }
      double H[3][3], g[3], Mi[3][3], d[3], ns, ng;
      lm_solve_step(a.cfg, tot, H, g, Mi, d, ns, ng);
      su = (float)((double)su - d[0]);
      sv = (float)((double)sv - d[1]);
      th = (float)((double)th - d[2]);
      if (a.reinit) {                // models_ford.py:460-465, with the caller's draws
        const float ru = a.rand_uv[b], rv = a.rand_uv[a.B + b];
        su = (su > -2.5f && su < 2.5f) ? su : ru;
        sv = (sv > -2.5f && sv < 2.5f) ? sv : rv;
      }
      a.pose[b * 3 + 0] = su; a.pose[b * 3 + 1] = sv; a.pose[b * 3 + 2] = th;
      float* tr = a.trace_out + (size_t)b * a.trace_stride;
      tr[0] = su; tr[1] = sv; tr[2] = th;
    }
    su = __shfl(su, 0, 64); sv = __shfl(sv, 0, 64); th = __shfl(th, 0, 64);
  }
  if (a.coef && lane < V) {          // lane v: view v's coefficients at the common pose
    const int j = lmv_pseudo(b, lane, V);
    lm_coefficients(a.next, su, sv, th, a.R + (size_t)j * 9, a.T + (size_t)j * 3, a.coef + lmv_coef_offset(j));
  }
}

// ---------------------------------------------------------------------------------------------
static int lmv_part_ld(const hla_s2g_config* cfg, const hla_s2g_level* lv) { return lm_max_nt(cfg, lv, fwd_tiling); }

static bool lmv_sizes_ok(const hla_s2g_config* cfg, const hla_s2g_level* lv, int B, int V) {
  return cfg && lv && B > 0 && V >= 1 && V <= LMV_MAX_VIEWS && cfg->n_levels >= 1 && cfg->n_levels <= 4 && cfg->n_iters >= 1 &&
         (long long)B * V < (1ll << 24);
}

extern "C" size_t hla_s2g_views_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* lv, int B, int V) {
  if (!lmv_sizes_ok(cfg, lv, B, V)) {
    hla_set_error("hla_s2g_views_workspace_bytes: null argument, bad sizes or V outside 1..%d", LMV_MAX_VIEWS);
    return 0;
  }
  return lmv_layout(B, V, lmv_part_ld(cfg, lv)).total;
}

template <bool W, typename F>
static void lmv_launch_accum_f(int C, dim3 grid, hipStream_t st, const AccumArgs& a, int V) {
  lm_dispatch_c<256, 128, 64, 16>(C, [&](auto c) { hipLaunchKernelGGL((lmv_accum<decltype(c)::value, W, F>), grid, dim3(256), 0, st, a, V); });
}
template <bool W>
static void lmv_launch_accum(int C, int feat_dtype, dim3 grid, hipStream_t st, const AccumArgs& a, int V) {
  if (feat_dtype == HLA_BF16) lmv_launch_accum_f<W, __bf16>(C, grid, st, a, V);
  else if (feat_dtype == HLA_F16) lmv_launch_accum_f<W, _Float16>(C, grid, st, a, V);
  else lmv_launch_accum_f<W, float>(C, grid, st, a, V);
}

extern "C" int hla_s2g_lm_solve_views(const hla_s2g_config* cfg, const hla_s2g_level* lv, int V, const float* R, const float* T,
                                      const float* pose0, const float* rand_uv, float* trace, double* normal_eq,
                                      double* view_sums, void* workspace, size_t workspace_bytes, int B, hla_stream_t stream) {
  const char* who = "hla_s2g_lm_solve_views";
  HLA_REQUIRE(trace && workspace, "%s: null argument", who);
  HLA_REQUIRE(cfg && cfg->ford == 1, "%s: the Ford chain only (cfg->ford must be 1): the KITTI chain has no extrinsics", who);
  HLA_REQUIRE(V >= 1 && V <= LMV_MAX_VIEWS, "%s: V = %d, must be 1..%d", who, V, LMV_MAX_VIEWS);
  const int rc = hla_s2g_validate(who, cfg, lv, R, T, B);      // (sizes, dof, proj, reach_mode, channel counts, map types, depth)
  if (rc) return rc;
  HLA_REQUIRE(lmv_sizes_ok(cfg, lv, B, V), "%s: bad sizes", who);
  HLA_REQUIRE(!cfg->keep, "%s: cfg->keep (dropout) is not built for the views loop", who);
  HLA_REQUIRE(!cfg->count_in_view, "%s: cfg->count_in_view is not built for the views loop", who);
  HLA_REQUIRE(cfg->optimizer == 0 || cfg->optimizer == 3, "%s: optimizer must be 0 (LM) or 3 (GN)", who);
  HLA_REQUIRE(cfg->optimizer == 0 || !cfg->level_first, "%s: GN exists for the iteration-first loop only", who);
  HLA_REQUIRE(rand_uv, "%s: rand_uv required", who);
  for (int l = 0; l < cfg->n_levels; ++l)      // the pseudo-batch's ground maps are indexed with size_t; the tables with V * h * w * 3
    HLA_REQUIRE((size_t)V * lv[l].h * lv[l].w * 3 < (1u << 31), "%s: level %d: tables too large", who, l);
  const int J = B * V, part_ld = lmv_part_ld(cfg, lv);
  const LmvLayout W = lmv_layout(B, V, part_ld);
  if (workspace_bytes < W.total) return lm_workspace_short(who, workspace_bytes, W.total);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* coef = (double*)(ws + W.coef);
  float* pose = (float*)(ws + W.pose);
  double* part = (double*)(ws + W.part);

  if (pose0) HLA_CHECK_HIP(hipMemcpyAsync(pose, pose0, (size_t)B * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
  const LmPlan plan = lm_plan_of(cfg);
  const int steps = plan.steps();

  LmvCloseArgs ca{};
  ca.V = V; ca.part_ld = part_ld; ca.pose = pose; ca.B = B; ca.reinit = 1; ca.R = R; ca.T = T;
  ca.cfg = lm_solve_cfg_of(cfg);
  // init launch: the start pose and the coefficients of step 0
  ca.part = nullptr; ca.zero_pose = pose0 ? 0 : 1; ca.coef = coef; ca.next = lm_geom_of(cfg, lv[plan.level(0)]);
  hla_prof_begin(K_LMVCLOSE, 0, 0, st);
  hipLaunchKernelGGL(lmv_close, dim3(B), dim3(64), 0, st, ca);
  hla_prof_end(st);
  ca.zero_pose = 0;

  for (int k = 0; k < steps; ++k) {
    const hla_s2g_level& v = lv[plan.level(k)];
    AccumArgs aa{};
    aa.sat = v.sat_feat; aa.grd = v.grd_feat; aa.conf = v.grd_conf; aa.pts = lm_points_of(v); aa.coef = coef; aa.part = part;
    lm_fill_s2g_dims(aa, v, fwd_tiling(v));
    aa.part_ld = part_ld; aa.xcd_affine = lm_xcd_affine(J); aa.b0 = 0; aa.nb = J;
    const int nblk = lm_grid_blocks(aa.xcd_affine, J, aa.nt);
    const double esz = v.feat_dtype == HLA_F32 ? 4.0 : 2.0;
    hla_prof_begin(K_LMVACCUM, 0, ((double)B * v.A * v.A + (double)J * aa.npix) * v.C * esz, st);
    if (cfg->using_weight) lmv_launch_accum<true>(v.C, v.feat_dtype, dim3(nblk), st, aa, V);
    else lmv_launch_accum<false>(v.C, v.feat_dtype, dim3(nblk), st, aa, V);
    hla_prof_end(st);

    ca.part = part; ca.nt = aa.nt; ca.sat_inv = v.sat_inv_norm; ca.grd_inv = v.grd_inv_norm;
    ca.trace_out = trace + plan.slot(k); ca.trace_stride = plan.trace_stride();
    ca.rand_uv = rand_uv + (size_t)k * 2 * B;
    ca.normal_eq = normal_eq ? normal_eq + (size_t)k * B * 16 : nullptr;
    ca.view_sums = view_sums ? view_sums + (size_t)k * J * 16 : nullptr;
    if (k + 1 < steps) { ca.coef = coef; ca.next = lm_geom_of(cfg, lv[plan.level(k + 1)]); }
    else ca.coef = nullptr;
    hla_prof_begin(K_LMVCLOSE, 0, (double)J * aa.nt * PART_N * 8.0, st);
    hipLaunchKernelGGL(lmv_close, dim3(B), dim3(64), 0, st, ca);
    hla_prof_end(st);
  }
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}
