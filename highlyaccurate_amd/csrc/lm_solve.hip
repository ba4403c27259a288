// Fused satellite->ground projection + bilinear gather + feature Jacobian + normal equations,
// and the per-sample damped 3x3 solve: the LM pose loop of
//   models_kitti.py:700-1041 (grd2cam2world2sat, project_map_to_grd, LM_update), loop 1176-1283
//   models_ford.py:173-466, loop 682-835
//   jacobian.py:138-205 (grid_sample)
//
// HBM-bound.  One step = two launches on the caller's stream:
//   lm_accum<C>  grid (tiles x samples): every wave walks ground pixels with its lanes spread over
//                the channel axis (NHWC, 16 B per lane => each bilinear tap is one fully coalesced
//                C*4-byte read), and accumulates the 14 sums that define the normal equations.
//                The [3,B,C,h,w] Jacobian of the reference (>=369 MB/sample/step) is never formed.
//   lm_solve     one wave per sample: fixed-order fp64 reduction of the tile partials (bitwise
//                deterministic), 3x3/2x2/1x1 damped solve, pose update + re-initialisation rule,
//                and the projection coefficients of the NEXT step (so no extra launch for them).
#include "lm_fwd.h"
#include <cstring>
#include <mutex>

struct SolveArgs {
  const double* part;    // [B,part_ld,PART_N] of the step being closed (nt tiles used), or null (init launch)
  const double* sat_inv; // [B] or null: feature maps are stored un-normalised, sums are rescaled here
  const double* grd_inv;
  int nt, part_ld;
  float* pose;           // [B,3] running pose (shift_u, shift_v, theta), fp32 like the reference
  float* trace_out;      // &trace[0][iter][level][0] of this step (sample stride = trace_stride)
  int trace_stride;
  const float* rand_uv;  // [2,B] for this step, or null
  double* normal_eq;     // [B,16] for this step, or null
  double* coef;          // [B,COEF_N] out for the next step, or null
  const float* R_FL;     // [B,3,3]
  const float* T_FL;     // [B,3]
  int B, reinit;         // B: the WHOLE batch (row stride of rand_uv and of the arrival counters), whatever range a launch covers
  int optimizer, t;      // 0 LM; 1 SGD; 2 ADAM (t = step index in execution order); 3 GN (cfg.gn)
  double beta1, beta2;
  double* adam;          // [B,6] first / second moment of the three pose components (ADAM only)
  const int* in_view;    // [B] pixels in view in this step (count_in_view), or null
  LmSolveCfg cfg;
  LmGeom next;           // geometry of the level the NEXT step runs on
  // init launch only (part == null): what used to be two hipMemsetAsync launches in front of every forward
  unsigned* zero_ticket; // [steps][B] arrival counters of all steps, or null
  int zero_steps, zero_pose;   // zero_pose: no initial pose was given, start from 0
  int* reach_clear;      // init launch, hla_s2g_config.reach_mode = 1: [B] reach flags to clear, or null
  const int* gate;       // reach_mode = 2: [B] reach flags; the launches leave a sample whose flag is 0 alone.  Else null
};

// One wave closes a step for sample b.  COHERENT: the tile partials were written by OTHER workgroups of the same launch
// (the fused accumulate + solve kernel): read them with agent-scope (sc1) loads, which bypass this CU's L1.
// LOCAL (lm_repair_loop): the step reads its pose from lpose [3] and leaves the new pose there and the next step's coefficients in
// lcoef [COEF_N] (null: there is no next step) -- shared memory -- instead of the sample's rows of a.pose / a.coef.
template <bool COHERENT, bool LOCAL = false>
__device__ __forceinline__ void lm_solve_body(const SolveArgs& a, int b, int lane, float* lpose = nullptr, double* lcoef = nullptr) {
  float su = LOCAL ? lpose[0] : a.pose[b * 3 + 0], sv = LOCAL ? lpose[1] : a.pose[b * 3 + 1], th = LOCAL ? lpose[2] : a.pose[b * 3 + 2];
  if (!a.part) {          // the init launch also clears this sample's arrival counters and, without an initial pose, its pose
    if (a.reach_clear && lane == 0) a.reach_clear[b] = 0;
    if (a.zero_ticket)
      for (int k = lane; k < a.zero_steps; k += 64) a.zero_ticket[(size_t)k * a.B + b] = 0u;
    if (a.zero_pose) {
      su = sv = th = 0.f;
      if (lane < 3) (LOCAL ? lpose[lane] : a.pose[b * 3 + lane]) = 0.f;
    }
  }

  if (a.part) {
    double s[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) s[k] = 0.0;
    for (int i = lane; i < a.nt; i += 64) {
      const double* p = a.part + ((size_t)b * a.part_ld + i) * PART_N;
#pragma unroll
      for (int k = 0; k < 14; ++k)
        s[k] += COHERENT ? __hip_atomic_load(p + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p[k];
    }
#pragma unroll
    for (int k = 0; k < 14; ++k) s[k] = wave_sum_f64(s[k]);

    if (lane == 0) {
      // deferred L2_norm (VGG.py:511-514): s -> as*s, J -> as*J, g -> ag*g
      const double as = a.sat_inv ? a.sat_inv[b] : 1.0, ag = a.grd_inv ? a.grd_inv[b] : 1.0;
      s[0] *= as * as; s[1] *= ag * ag;
      for (int k = 2; k < 11; ++k) s[k] *= as * as;
      for (int k = 11; k < 14; ++k) s[k] *= as * ag;
      if (a.normal_eq) {
        for (int k = 0; k < 14; ++k) a.normal_eq[(size_t)b * 16 + k] = s[k];
        a.normal_eq[(size_t)b * 16 + 14] = a.in_view ? (double)a.in_view[b] : 0.0;
        a.normal_eq[(size_t)b * 16 + 15] = 0.0;
      }
      double H[3][3], g[3], Mi[3][3], d[3], ns, ng;
      if (a.optimizer == 0 || a.optimizer == 3) {
        lm_solve_step(a.cfg, s, H, g, Mi, d, ns, ng);
      } else {                       // ablation optimisers on the raw residual: delta_pose = sum 2 r J (models_kitti.py:1075-1076)
        for (int p = 0; p < 3; ++p) d[p] = 2.0 * (s[8 + p] - s[11 + p]);
        if (a.optimizer == 2) {      // ADAM_update, 1110-1116
          double* mv = a.adam + (size_t)b * 6;
          for (int p = 0; p < 3; ++p) {
            const double m = a.beta1 * mv[p] + (1.0 - a.beta1) * d[p];
            const double v = a.beta2 * mv[3 + p] + (1.0 - a.beta2) * d[p] * d[p];
            mv[p] = m; mv[3 + p] = v;
            d[p] = (m / (1.0 - pow(a.beta1, a.t + 1))) / (sqrt(v / (1.0 - pow(a.beta2, a.t + 1))) + 1e-8);
          }
        }
        for (int p = 0; p < 3; ++p) d[p] *= 0.01;
      }
      su = (float)((double)su - d[0]);
      sv = (float)((double)sv - d[1]);
      th = (float)((double)th - d[2]);
      if (a.reinit) {                // models_kitti.py:1028-1033
        const float ru = a.rand_uv[b], rv = a.rand_uv[a.B + b];
        su = (su > -2.5f && su < 2.5f) ? su : ru;
        sv = (sv > -2.5f && sv < 2.5f) ? sv : rv;
      }
      if (LOCAL) { lpose[0] = su; lpose[1] = sv; lpose[2] = th; }
      else { a.pose[b * 3 + 0] = su; a.pose[b * 3 + 1] = sv; a.pose[b * 3 + 2] = th; }
      float* tr = a.trace_out + (size_t)b * a.trace_stride;
      tr[0] = su; tr[1] = sv; tr[2] = th;
    }
  }
  if ((LOCAL ? lcoef : a.coef) && lane == 0)
    lm_coefficients(a.next, su, sv, th, a.R_FL ? a.R_FL + (size_t)b * 9 : nullptr, a.T_FL ? a.T_FL + (size_t)b * 3 : nullptr,
                    LOCAL ? lcoef : a.coef + (size_t)b * COEF_N);
}

// stand-alone launch: the coefficients of step 0 (part == null)
__global__ __launch_bounds__(64) void lm_solve(SolveArgs a) {
  if (a.gate && a.gate[blockIdx.x] == 0) return;      // (nothing of a skipped sample is cleared or written)
  lm_solve_body<false>(a, blockIdx.x, threadIdx.x);
}

// The last tile of a sample to finish (an arrival ticket per sample) reduces the sample's tile partials in fixed order and
// closes the step: no separate solve launch.  Publication follows the write-through recipe of cdna_hip_programming.md
// Guideline 16: 8-byte agent-scope (sc1) stores of the partials -> s_waitcnt vmcnt(0) -> relaxed agent-scope ticket; the
// last arriver reads with agent-scope loads.  Which tile arrives last never changes a bit of the result.
// (AccumArgs, the channel-pair helpers, LM_OCC / LM_UNROLL and the forward tile size: lm_fwd.h)
template <int C, bool USE_W, typename F>
__global__ __launch_bounds__(256, LM_OCC) void lm_accum(AccumArgs a, SolveArgs sa) {
  __shared__ PixParam pp[FWD_MAX_TP];
  __shared__ float red[4][14];
  __shared__ double redd[14];
  int b, tile;
  if (!lm_block_map(a.xcd_affine, a.nt, a.nb, b, tile, a.b0)) return;
  if (a.gate && a.gate[b] == 0) return;      // workgroup-uniform, ahead of the first barrier
  const int t = threadIdx.x;
  constexpr bool active = true;
#define LM_TILE_COEF (a.coef + (size_t)b * COEF_N)
#define LM_TILE_BEFORE_PUBLISH if (wave != 0) return;
#include "lm_tile_body.h"      // (declares lane and wave)
#undef LM_TILE_COEF
#undef LM_TILE_BEFORE_PUBLISH
  const unsigned old = lm_draw_ticket(a.ticket + b, lane);      // (publication recipe: lm_common.h)
  if (old + 1 != (unsigned)a.nt) return;
  lm_solve_body<true>(sa, b, lane);
}

// ---------------------------------------------------------------------------------------------
// hla_s2g_config.reach_mode = 2: the whole loop of a flagged sample in ONE launch.  The multi-launch loop needs a launch per step
// because a step's tiles are spread over the chip and hand their sums over grid-wide; here a sample is one workgroup, so the
// hand-over is a barrier and nothing of one workgroup ever waits on another (no ticket, no spinning: an unflagged sample's
// workgroup returns at once, and a flagged one depends on nobody).  1024 threads = four 256-thread groups, each with the shared
// arrays of one lm_accum workgroup; group v runs the tile body (lm_tile_body.h) on tiles v, v + 4, ... of the step with its thread id t & 255, so a
// tile's 14 partials are bit for bit what lm_accum publishes, and wave 0 then closes the step with lm_solve_body<true> like
// lm_accum's last arriver: same fixed-order reduction over the tiles, same draws, same keep masks, same trace / normal_eq rows.
// What one step leaves for the next inside the launch:
//   * pose and coefficients live in SHARED MEMORY (s_pose, s_cf) for the whole launch -- a block-uniform const double* in the
//     workspace would be read through the scalar cache, a plain vector load through this CU's L1, and neither sees a store made
//     earlier in the same launch; the final pose is copied to the workspace at the end, where the multi-launch loop leaves it;
//   * the tile partials go through the workspace rows of the sample exactly as in lm_accum: agent-scope (sc1) stores, s_waitcnt
//     vmcnt(0), the barrier, agent-scope loads in lm_solve_body<true> (the recipe of lm_draw_ticket with the barrier in the
//     ticket's place).
struct RepairLevel {
  const void* sat; const void* grd;
  LmPoints pts;
  const double* sat_inv; const double* grd_inv;
  int A, h, w, row0, npix, TP, nt, hs, rskip, C;
  double mpp, ctr;
};
struct RepairArgs {
  RepairLevel lv[4];
  SolveArgs sa;          // what every step shares; .gate = the reach flags, .next holds the level-independent part of the geometry
  double* part;
  const unsigned char* keep; size_t keep_stride;
  float* trace; const float* rand_uv; double* normal_eq;
  int L, N, level_first;
};
#define LM_REPAIR_GROUPS 4

template <typename F>
__global__ __launch_bounds__(256 * LM_REPAIR_GROUPS) void lm_repair_loop(RepairArgs ra) {
  __shared__ PixParam s_pp[LM_REPAIR_GROUPS][FWD_MAX_TP];
  __shared__ float s_red[LM_REPAIR_GROUPS][4][14];
  __shared__ double s_redd[LM_REPAIR_GROUPS][14];
  __shared__ double s_cf[COEF_N];
  __shared__ float s_pose[3];
  const int b = blockIdx.x;
  if (ra.sa.gate[b] == 0) return;      // workgroup-uniform, ahead of the first barrier
  const int wt = threadIdx.x, vg = wt >> 8, vt = wt & 255;      // thread of the workgroup, its 256-thread group, its id in it
  const int L = ra.L, N = ra.N, steps = L * N;
  auto step_level = [&](int k) { return ra.level_first ? k / N : k % L; };

  // the init step: the start pose (the workspace holds pose0 when one was given) and the coefficients of step 0
  if (wt < 3) s_pose[wt] = ra.sa.pose[b * 3 + wt];
  __syncthreads();      // wave 0's 64 lanes read what its lanes 0-2 wrote
  if (wt < 64) {
    SolveArgs sa = ra.sa;
    const RepairLevel& n = ra.lv[step_level(0)];
    sa.part = nullptr; sa.next.mpp = n.mpp; sa.next.ctr = n.ctr;
    lm_solve_body<false, true>(sa, b, wt, s_pose, s_cf);
  }
  __syncthreads();

  for (int k = 0; k < steps; ++k) {
    const int l = step_level(k), it = ra.level_first ? k % N : k / L;
    const RepairLevel& lv = ra.lv[l];
    AccumArgs a{};
    a.sat = lv.sat; a.grd = lv.grd; a.pts = lv.pts; a.part = ra.part;
    a.A = lv.A; a.h = lv.h; a.w = lv.w; a.row0 = lv.row0; a.npix = lv.npix; a.TP = lv.TP; a.nt = lv.nt; a.part_ld = ra.sa.part_ld;
    a.hs = lv.hs; a.rskip = lv.rskip;
    a.keep = ra.keep ? ra.keep + (size_t)k * ra.keep_stride : nullptr;
    for (int tile0 = 0; tile0 < lv.nt; tile0 += LM_REPAIR_GROUPS) {
      const int tile = tile0 + vg;
      const bool active = tile < lv.nt;
      constexpr bool USE_W = false;
      const int t = vt;
      PixParam* const pp = s_pp[vg];
      float (*const red)[14] = s_red[vg];
      double* const redd = s_redd[vg];
#define LM_TILE_COEF s_cf
#define LM_TILE_BEFORE_PUBLISH
      switch (lv.C) {
        case 256: {
          constexpr int C = 256;
#include "lm_tile_body.h"
        } break;
        case 128: {
          constexpr int C = 128;
#include "lm_tile_body.h"
        } break;
        default: {
          constexpr int C = 64;
#include "lm_tile_body.h"
        } break;
      }
#undef LM_TILE_COEF
#undef LM_TILE_BEFORE_PUBLISH
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the partials have left this CU before the barrier lets wave 0 read them
    __syncthreads();
    if (wt < 64) {
      SolveArgs sa = ra.sa;
      sa.t = k;
      sa.part = ra.part; sa.nt = lv.nt; sa.sat_inv = lv.sat_inv; sa.grd_inv = lv.grd_inv;
      sa.trace_out = ra.trace + ((size_t)it * L + l) * 3; sa.trace_stride = N * L * 3;
      sa.rand_uv = ra.sa.reinit ? ra.rand_uv + (size_t)k * 2 * ra.sa.B : nullptr;
      sa.normal_eq = ra.normal_eq ? ra.normal_eq + (size_t)k * ra.sa.B * 16 : nullptr;
      if (k + 1 < steps) {
        const RepairLevel& n = ra.lv[step_level(k + 1)];
        sa.next.mpp = n.mpp; sa.next.ctr = n.ctr;
      }
      lm_solve_body<true, true>(sa, b, wt, s_pose, k + 1 < steps ? s_cf : nullptr);
    }
    __syncthreads();      // the next step's coefficients are in s_cf (and every read of this step's is behind us)
  }
  if (wt < 3) ra.sa.pose[b * 3 + wt] = s_pose[wt];
}

// ---------------------------------------------------------------------------------------------
// hla_s2g_config.count_in_view: the quantity jacobian.py:172 asserts on -- how many pixels of the WHOLE level map (all rows,
// whatever their ground mask) have satellite coordinates inside the map.  Geometry only; one thread per pixel.  With a depth map
// the points are the lifted ones (lm_point); the mask is still ignored.
__global__ __launch_bounds__(256) void lm_inview_kernel(const double* __restrict__ coef, LmPoints pts, int w, int A,
                                                        int npix, int* __restrict__ count, int b0) {
  const int b = b0 + blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const double* cf = coef + (size_t)b * COEF_N;
  int in = 0;
  if (p < npix) {
    float q[3];
    (void)lm_point(pts, b, p / w, p % w, w, q);
    const double X = q[0], Y = q[1], Z = q[2];
    const double u = cf[0] * X + cf[1] * Y + cf[2] * Z + cf[3];
    const double v = cf[4] * X + cf[5] * Y + cf[6] * Z + cf[7];
    const double lim = (double)(A - 1);
    in = ((u >= 0.0) && (u <= lim) && (v >= 0.0) && (v <= lim)) ? 1 : 0;
  }
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count + b, __popcll(m));
}

// ---------------------------------------------------------------------------------------------
struct FwdWs { size_t coef, pose, part, ticket, in_view, adam, total; int part_ld; };
static FwdWs fwd_ws(const hla_s2g_config* cfg, const hla_s2g_level* lv, int B) {
  FwdWs W{};
  W.part_ld = lm_max_nt(cfg, lv, fwd_tiling);
  const size_t per_step = (size_t)B * cfg->n_levels * cfg->n_iters;
  LmBump ws;
  W.coef = ws.take((size_t)B * COEF_N * sizeof(double));
  W.pose = ws.take((size_t)B * 3 * sizeof(float));
  W.part = ws.take((size_t)B * W.part_ld * PART_N * sizeof(double));
  W.ticket = ws.take(per_step * sizeof(unsigned));      // arrival tickets, one per step and sample
  W.in_view = ws.take(per_step * sizeof(int));          // in-view counts (count_in_view)
  W.adam = ws.take((size_t)B * 6 * sizeof(double));     // ADAM moments
  W.total = ws.o;
  return W;
}

extern "C" size_t hla_s2g_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* levels, int B) {
  return fwd_ws(cfg, levels, B).total;
}

template <bool W, typename F>
static void launch_accum_f(int C, dim3 grid, hipStream_t st, const AccumArgs& a, const SolveArgs& sa) {
  lm_dispatch_c<256, 128, 64, 16>(C, [&](auto c) { hipLaunchKernelGGL((lm_accum<decltype(c)::value, W, F>), grid, dim3(256), 0, st, a, sa); });
}
template <bool W>
static void launch_accum(int C, int feat_dtype, dim3 grid, hipStream_t st, const AccumArgs& a, const SolveArgs& sa) {
  if (feat_dtype == HLA_BF16) launch_accum_f<W, __bf16>(C, grid, st, a, sa);
  else if (feat_dtype == HLA_F16) launch_accum_f<W, _Float16>(C, grid, st, a, sa);
  else launch_accum_f<W, float>(C, grid, st, a, sa);
}

int hla_s2g_validate(const char* who, const hla_s2g_config* cfg, const hla_s2g_level* lv, const float* R_FL,
                     const float* T_FL, int B) {
  HLA_REQUIRE(cfg && lv, "%s: null argument", who);
  HLA_REQUIRE(B > 0 && cfg->n_levels >= 1 && cfg->n_levels <= 4 && cfg->n_iters >= 1, "%s: bad sizes", who);
  HLA_REQUIRE(cfg->dof >= 1 && cfg->dof <= 3, "%s: dof must be 1..3", who);
  HLA_REQUIRE(cfg->proj == 0, "%s: cfg->proj selects the projection of hla_g2s_* only (must be 0 here)", who);
  HLA_REQUIRE(!cfg->ford || (R_FL && T_FL), "%s: Ford mode needs R_FL and T_FL", who);
  HLA_REQUIRE(cfg->reach_mode == 0 || (!strcmp(who, "hla_s2g_lm_solve") && cfg->reach_mode >= 1 && cfg->reach_mode <= 2 && cfg->reach_flag),
              "%s: cfg->reach_mode is 0, or 1 / 2 with reach_flag in hla_s2g_lm_solve", who);
  for (int l = 0; l < cfg->n_levels; ++l) {
    const int C = lv[l].C;
    HLA_REQUIRE(C == 256 || C == 128 || C == 64 || C == 16, "%s: unsupported channel count %d", who, C);
    HLA_REQUIRE(lv[l].feat_dtype == HLA_F32 || lv[l].feat_dtype == HLA_BF16 || lv[l].feat_dtype == HLA_F16,
                "%s: level %d feat_dtype must be HLA_F32, HLA_BF16 or HLA_F16", who, l);
    HLA_REQUIRE(lv[l].sat_feat && lv[l].grd_feat && lv[l].xyz, "%s: level %d has null maps", who, l);
    HLA_REQUIRE(!cfg->using_weight || lv[l].grd_conf, "%s: using_weight needs grd_conf", who);
    HLA_REQUIRE(lv[l].row0 >= 0 && lv[l].row0 < lv[l].h, "%s: bad row0", who);
    HLA_REQUIRE(lv[l].grd_row_skip >= 0 && lv[l].grd_row_skip <= lv[l].row0, "%s: grd_row_skip must be in [0,row0]", who);
    HLA_REQUIRE((size_t)lv[l].A * lv[l].A * C < (1u << 31), "%s: satellite map too large", who);
    HLA_REQUIRE(cfg->reach_mode != 1 || (cfg->reach_col0[l] >= 0 && cfg->reach_col0[l] < lv[l].A),
                "%s: cfg->reach_col0[%d] must be in [0, A)", who, l);
    if (lv[l].depth) {      // args.use_gt_depth (hla.h): KITTI chain only, all of the depth fields together
      HLA_REQUIRE(!cfg->ford, "%s: level %d: a depth map is not supported with cfg->ford = 1 (models_ford.py has no gt_depth)", who, l);
      HLA_REQUIRE(lv[l].ray && lv[l].depth_row && lv[l].depth_col && lv[l].depth_h > 0 && lv[l].depth_w > 0,
                  "%s: level %d: depth needs ray, depth_row, depth_col and depth_h, depth_w > 0", who, l);
      HLA_REQUIRE((size_t)B * lv[l].depth_h * lv[l].depth_w < (1u << 31), "%s: level %d: depth map too large", who, l);
    } else {
      HLA_REQUIRE(!lv[l].ray && !lv[l].depth_row && !lv[l].depth_col && !lv[l].depth_h && !lv[l].depth_w,
                  "%s: level %d: ray / depth_row / depth_col / depth_h / depth_w given without depth", who, l);
    }
  }
  return HLA_OK;
}

// ---------------------------------------------------------------------------------------------
// Stream groups.  Every launch of the loop ends in a tail during which the chip is nearly idle: one wave per sample reduces the
// partials, solves in fp64 on one lane and writes the next coefficients, and a launch boundary follows.  Samples are independent
// (and a sample's result does not depend on its batch mates, bit for bit), so the loop runs as LM_GROUPS sample ranges, each an
// in-order chain of launches on its own stream: one group's gather fills the other's tail.  Group 0 runs on the caller's stream,
// the others on streams the library owns (one set per device, created on first use); they fork from the caller's stream behind
// the init launch and are joined on it before hla_s2g_lm_solve returns, so the caller sees one stream's worth of ordering.
// Group boundaries are multiples of 8: the XCD-affine block map keeps every sample on the XCD it has in a whole-batch launch.
// Both constants are reasoned, NOT measured (EXPERIMENTS.md, "LM loop on stream groups"): the tail to hide is shorter than one
// group's gather, so a third group has nothing left to fill; 16 is the smallest batch whose two groups are whole XCD octets.
constexpr int LM_GROUPS = 2;
constexpr int LM_SPLIT_MIN = 16;    // smallest batch that is split
static_assert(LM_GROUPS >= 2 && LM_GROUPS <= 4 && LM_SPLIT_MIN > 8, "a batch of up to 8 samples is one XCD octet and never splits");

// One set per device, made on the first split call on it.  `mu` is held while a call enqueues its loop: the fork / join events
// and the side streams are shared by every caller on the device (two callers interleaving record and wait would fork one
// caller's side stream behind the other's init launch).
struct LmSideStreams {
  std::mutex mu;
  bool ready = false, failed = false;
  hipStream_t side[LM_GROUPS] = {};     // [0] unused: group 0 is the caller's stream
  hipEvent_t fork = nullptr, join[LM_GROUPS] = {};
};
static LmSideStreams g_lm_side[64];

// (mu held)  false: no stream to be had -- remembered, the loop stays on the caller's stream now and later
static bool lm_side_create(LmSideStreams& S) {
  if (S.ready || S.failed) return S.ready;
  hipError_t r = hipEventCreateWithFlags(&S.fork, hipEventDisableTiming);
  for (int g = 1; g < LM_GROUPS && r == hipSuccess; ++g) {
    r = hipStreamCreateWithFlags(&S.side[g], hipStreamNonBlocking);
    if (r == hipSuccess) r = hipEventCreateWithFlags(&S.join[g], hipEventDisableTiming);
  }
  if (r != hipSuccess) {
    (void)hipGetLastError();
    if (S.fork) (void)hipEventDestroy(S.fork);
    for (int g = 1; g < LM_GROUPS; ++g) {
      if (S.join[g]) (void)hipEventDestroy(S.join[g]);
      if (S.side[g]) (void)hipStreamDestroy(S.side[g]);
    }
    S.failed = true;
    return false;
  }
  S.ready = true;
  return true;
}

extern "C" int hla_s2g_lm_solve(const hla_s2g_config* cfg, const hla_s2g_level* lv, const float* R_FL,
                                const float* T_FL, const float* pose0, const float* rand_uv, float* trace,
                                double* normal_eq, void* workspace, size_t workspace_bytes, int B,
                                hla_stream_t stream) {
  HLA_REQUIRE(trace && workspace, "hla_s2g_lm_solve: null argument");
  const int rc = hla_s2g_validate("hla_s2g_lm_solve", cfg, lv, R_FL, T_FL, B);
  if (rc) return rc;
  HLA_REQUIRE(cfg->optimizer >= 0 && cfg->optimizer <= 3, "hla_s2g_lm_solve: optimizer must be 0 (LM), 1 (SGD), 2 (ADAM) or 3 (GN)");
  HLA_REQUIRE(cfg->optimizer == 0 || !cfg->level_first, "hla_s2g_lm_solve: SGD / ADAM / GN exist for the iteration-first loop only");
  HLA_REQUIRE(cfg->optimizer != 3 || cfg->ford, "hla_s2g_lm_solve: GN_update exists in the Ford model only");
  const bool newton = lm_newton(cfg), reinit = lm_reinit(cfg);
  HLA_REQUIRE(!reinit || rand_uv, "hla_s2g_lm_solve: rand_uv required");
  const FwdWs W = fwd_ws(cfg, lv, B);
  if (workspace_bytes < W.total) return lm_workspace_short("hla_s2g_lm_solve", workspace_bytes, W.total);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* coef = (double*)(ws + W.coef);
  float* pose = (float*)(ws + W.pose);
  double* part = (double*)(ws + W.part);
  unsigned* ticket = (unsigned*)(ws + W.ticket);
  int* in_view = (int*)(ws + W.in_view);
  double* adam = (double*)(ws + W.adam);

  if (pose0) HLA_CHECK_HIP(hipMemcpyAsync(pose, pose0, (size_t)B * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
  // (otherwise the init launch below starts the pose at zero; it also clears the arrival counters: two memset launches less)

  const LmPlan plan = lm_plan_of(cfg);
  const int L = plan.L, steps = plan.steps();
  const bool count = cfg->count_in_view && normal_eq;
  if (count) HLA_CHECK_HIP(hipMemsetAsync(in_view, 0, (size_t)B * steps * sizeof(int), st));
  if (cfg->optimizer == 2) HLA_CHECK_HIP(hipMemsetAsync(adam, 0, (size_t)B * 6 * sizeof(double), st));
  SolveArgs sa{};
  sa.optimizer = cfg->optimizer; sa.beta1 = cfg->beta1; sa.beta2 = cfg->beta2; sa.adam = adam;
  sa.pose = pose; sa.B = B; sa.part_ld = W.part_ld; sa.reinit = reinit ? 1 : 0; sa.R_FL = R_FL; sa.T_FL = T_FL;
  sa.cfg = lm_solve_cfg_of(cfg);
  sa.coef = coef;

  // reach_mode 2: the init step and all steps of the flagged samples as one launch of lm_repair_loop, a workgroup per sample.
  // Outside what that kernel is built for -- confidence weights, count_in_view (its counting launches read each step's
  // coefficients from the workspace), SGD / ADAM, 16 channels, levels of different map types, fp32 maps -- the gated multi-launch
  // loop below does the same work, bit for bit.  (fp32 maps: built and measured -- in that kernel the optimiser leaves the
  // operands of three a * b + c * d adds of the fp32 gather the other way round than in lm_accum<C, false, float>, so the other
  // product is fused: normal_eq entries 1e-7 relative off.  The instructions: EXPERIMENTS.md, "Repair loop as one launch".)
  bool repair = cfg->reach_mode == 2 && newton && !cfg->using_weight && !count && lv[0].feat_dtype != HLA_F32;
  for (int l = 0; l < L && repair; ++l) repair = lv[l].C != 16 && lv[l].feat_dtype == lv[0].feat_dtype;
  if (repair) {
    RepairArgs ra{};
    for (int l = 0; l < L; ++l) {
      const hla_s2g_level& v = lv[l];
      RepairLevel& r = ra.lv[l];
      r.sat = v.sat_feat; r.grd = v.grd_feat; r.pts = lm_points_of(v); r.sat_inv = v.sat_inv_norm; r.grd_inv = v.grd_inv_norm;
      lm_fill_s2g_dims(r, v, fwd_tiling(v));
      r.C = v.C; r.mpp = v.meter_per_pixel; r.ctr = v.centre;
    }
    ra.sa = sa;
    ra.sa.next = lm_geom_of(cfg, lv[0]);      // (mpp and ctr are set per step, from the level the next step runs on)
    ra.sa.zero_pose = pose0 ? 0 : 1;
    ra.sa.gate = cfg->reach_flag;
    ra.part = part;
    ra.keep = cfg->keep; ra.keep_stride = (size_t)cfg->keep_stride;
    ra.trace = trace; ra.rand_uv = rand_uv; ra.normal_eq = normal_eq;
    ra.L = L; ra.N = plan.N; ra.level_first = plan.level_first;
    hla_prof_begin(K_LMREPAIR, 0, 0, st);
    if (lv[0].feat_dtype == HLA_BF16) hipLaunchKernelGGL(lm_repair_loop<__bf16>, dim3(B), dim3(256 * LM_REPAIR_GROUPS), 0, st, ra);
    else hipLaunchKernelGGL(lm_repair_loop<_Float16>, dim3(B), dim3(256 * LM_REPAIR_GROUPS), 0, st, ra);
    hla_prof_end(st);
    HLA_CHECK_HIP(hipGetLastError());
    return HLA_OK;
  }

  // init launch: coefficients of step 0
  sa.part = nullptr; sa.next = lm_geom_of(cfg, lv[plan.level(0)]);
  sa.zero_ticket = ticket; sa.zero_steps = steps; sa.zero_pose = pose0 ? 0 : 1;
  // (reach_mode 2: the arrival counters and the pose of a skipped sample are never looked at, so they need no care)
  sa.reach_clear = cfg->reach_mode == 1 ? cfg->reach_flag : nullptr;
  sa.gate = cfg->reach_mode == 2 ? cfg->reach_flag : nullptr;
  hipLaunchKernelGGL(lm_solve, dim3(B), dim3(64), 0, st, sa);
  sa.zero_ticket = nullptr; sa.zero_steps = 0; sa.zero_pose = 0; sa.reach_clear = nullptr;

  // Sample ranges of the stream groups (comment above LM_GROUPS).  One group -- today's loop on the caller's stream -- for a
  // small batch, under the event profiler (its event pairs sit on the launch stream, and a per-kernel time must stay the time
  // of a kernel that has the chip to itself), while the caller's stream is being captured, and when no side stream can be had.
  int ng = 1, gb0[LM_GROUPS + 1] = {0};
  LmSideStreams* side = nullptr;
  std::unique_lock<std::mutex> side_lock;
  if (B >= LM_SPLIT_MIN && !hla_prof_on() && cfg->reach_mode != 2) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    int d = -1;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = -1; }
    if (cap == hipStreamCaptureStatusNone && d >= 0 && d < 64) {
      side_lock = std::unique_lock<std::mutex>(g_lm_side[d].mu);
      if (lm_side_create(g_lm_side[d])) side = &g_lm_side[d];
      else side_lock.unlock();
    }
  }
  if (side) {
    const int oct = (B + 7) / 8;
    ng = oct < LM_GROUPS ? oct : LM_GROUPS;
    for (int g = 0; g < ng; ++g) gb0[g + 1] = gb0[g] + 8 * (oct / ng + (g < oct % ng ? 1 : 0));
  }
  gb0[ng] = B;
  hipStream_t gst[LM_GROUPS];
  gst[0] = st;
  int forked = 0;                                        // side streams that wait on the fork event: they are joined whatever follows
  hipError_t err = hipSuccess;
  if (ng > 1) {
    err = hipEventRecord(side->fork, st);                // behind the pose copy, the memsets and the init launch
    for (int g = 1; g < ng && err == hipSuccess; ++g) {
      gst[g] = side->side[g];
      err = hipStreamWaitEvent(gst[g], side->fork, 0);
      if (err == hipSuccess) forked = g;
    }
  }

  // steps interleaved over the groups: each group's launches stay in order on its own stream
  for (int k = 0; k < steps && err == hipSuccess; ++k) {
    const int l = plan.level(k);
    const hla_s2g_level& v = lv[l];
    AccumArgs aa{};
    aa.sat = v.sat_feat; aa.grd = v.grd_feat; aa.conf = v.grd_conf; aa.pts = lm_points_of(v); aa.coef = coef; aa.part = part;
    lm_fill_s2g_dims(aa, v, fwd_tiling(v));
    aa.keep = cfg->keep ? cfg->keep + (size_t)k * cfg->keep_stride : nullptr;
    aa.part_ld = W.part_ld; aa.xcd_affine = lm_xcd_affine(B);
    aa.ticket = ticket + (size_t)k * B;
    if (cfg->reach_mode == 1) { aa.col0 = cfg->reach_col0[l]; aa.reach_flag = cfg->reach_flag; }
    aa.gate = sa.gate;
    // the step's closing solve runs inside the same launch (last tile of each sample): its arguments
    sa.t = k;
    sa.part = part; sa.nt = aa.nt; sa.sat_inv = v.sat_inv_norm; sa.grd_inv = v.grd_inv_norm;
    sa.trace_out = trace + plan.slot(k); sa.trace_stride = plan.trace_stride();
    sa.rand_uv = reinit ? rand_uv + (size_t)k * 2 * B : nullptr;
    sa.normal_eq = normal_eq ? normal_eq + (size_t)k * B * 16 : nullptr;
    sa.in_view = count ? in_view + (size_t)k * B : nullptr;
    if (k + 1 < steps) { sa.coef = coef; sa.next = lm_geom_of(cfg, lv[plan.level(k + 1)]); }
    else sa.coef = nullptr;
    const double esz = v.feat_dtype == HLA_F32 ? 4.0 : 2.0;
    for (int g = 0; g < ng; ++g) {
      hipStream_t gs = gst[g];
      aa.b0 = gb0[g]; aa.nb = gb0[g + 1] - gb0[g];
      if (count)
        hipLaunchKernelGGL(lm_inview_kernel, dim3((v.h * v.w + 255) / 256, aa.nb), dim3(256), 0, gs, coef, aa.pts, v.w, v.A, v.h * v.w,
                           in_view + (size_t)k * B, aa.b0);
      const int nblk = lm_grid_blocks(aa.xcd_affine, aa.nb, aa.nt);
      hla_prof_begin(lm_prof_id(v.C), 0, (double)aa.nb * ((double)v.A * v.A + (double)aa.npix) * v.C * esz, gs);
      if (cfg->using_weight && newton) launch_accum<true>(v.C, v.feat_dtype, dim3(nblk), gs, aa, sa);   // SGD / ADAM ignore the confidence
      else launch_accum<false>(v.C, v.feat_dtype, dim3(nblk), gs, aa, sa);
      hla_prof_end(gs);
    }
  }
  // join: behind this point the caller's stream orders every launch of the loop -- also after a failure above, so that work
  // already on a side stream (it touches the workspace) is never left outside the caller's ordering
  for (int g = 1; g <= forked; ++g) {
    hipError_t e = hipEventRecord(side->join[g], gst[g]);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, side->join[g], 0);
    if (err == hipSuccess) err = e;
  }
  HLA_CHECK_HIP(err);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}
