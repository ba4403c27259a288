// Host side of the LM entry points (lm_solve.hip, lm_backward.hip, lm_g2s.hip, pose_score.hip, g2s_pose_score.hip): the decisions
// every one of them takes before it enqueues a kernel, each stated once -- the order of the steps and their rows in the trace, the
// tiling of a level and the grid it needs, the workspace allocator and its "too small" return, hla_s2g_config -> kernel scalars,
// hla_s2g_level -> the dimension fields of an argument struct, and the dispatch on the channel count.  No device code, and nothing
// here allocates: plain structs, lambdas and templates only (at B = 1 the forward is a chain of dependent launches of a few
// microseconds each, so the host's enqueue rate is part of its time).
#pragma once
#include "lm_common.h"
#include <type_traits>

// The step plan: step k of the L * N steps runs level level(k) in iteration iter(k) -- iteration-first (k = iter * L + level,
// models_kitti.py:1176-1283) or, level_first, level-first (k = level * N + iter) -- and leaves its pose in trace [B,N,L,3] at
// float offset slot(k) of the sample's row.  The ground -> satellite entry points require level_first = 0.
// (lm_repair_loop walks the same order on the device with its own step_level: kernel code.)
struct LmPlan {
  int L, N, level_first;
  int steps() const { return L * N; }
  int level(int k) const { return level_first ? k / N : k % L; }
  int iter(int k) const { return level_first ? k % N : k / L; }
  size_t slot(int k) const { return ((size_t)iter(k) * L + level(k)) * 3; }
  int trace_stride() const { return N * L * 3; }      // floats per sample
  // is step k the first visit of its level when the steps are walked in reverse?  (= its last visit: either order ends every
  // level in the last iteration)
  bool first_visit_reversed(int k) const { return iter(k) == N - 1; }
};
static inline LmPlan lm_plan_of(const hla_s2g_config* cfg) { return LmPlan{cfg->n_levels, cfg->n_iters, cfg->level_first}; }

// Tiling.  A level's npix pixels are cut into nt tiles of TP = pick(npix) pixels, one block each.  Every entry point keeps its own
// pick function (lm_pick_tile_fwd, lm_pick_tile_bwd, lm_pick_tile, ps_tile / gps_tile: they differ on purpose, see the measured
// tables next to them) and its own pixel count; its workspace size function and its launcher get nt from the SAME call.
struct LmTiling { int npix, TP, nt; };
template <class Pick>
static inline LmTiling lm_tiling(int npix, Pick pick) {
  const int tp = pick(npix);
  return LmTiling{npix, tp, (npix + tp - 1) / tp};
}
static inline int lm_npix_s2g(const hla_s2g_level& v) { return (v.h - v.row0) * v.w; }      // ground pixels from row0 down
static inline int lm_npix_g2s(const hla_s2g_level& v) { return v.A * v.A; }                // the whole satellite map

// the largest nt over the levels (>= 1): the row count of a sample in the partial-sum region
template <class TilingOf>
static inline int lm_max_nt(const hla_s2g_config* cfg, const hla_s2g_level* lv, TilingOf tiling_of) {
  int m = 1;
  for (int l = 0; l < cfg->n_levels; ++l) m = max(m, tiling_of(lv[l]).nt);
  return m;
}

// blocks of a launch over nb samples with `per` blocks each, under lm_block_map (lm_common.h): the XCD-affine map deals whole
// octets of samples, so a partial octet launches idle blocks
static inline int lm_xcd_affine(int B) { return B >= 8 ? 1 : 0; }
static inline int lm_grid_blocks(int xcd_affine, int nb, int per) { return xcd_affine ? 8 * ((nb + 7) / 8) * per : nb * per; }

// Workspace.  A layout is a struct of named byte offsets that ONE function fills by taking its regions in order from this
// allocator; hla_*_workspace_bytes and the launcher both call that function, so there is no second statement of a layout.
struct LmBump {
  size_t o = 0;
  size_t take(size_t bytes) { const size_t at = o; o += hla_align_up(bytes, 256); return at; }
};
static inline size_t lm_one_region_bytes(size_t bytes) { LmBump ws; ws.take(bytes); return ws.o; }      // a layout of one region
static inline int lm_workspace_short(const char* who, size_t have, size_t need) {
  hla_set_error("%s: workspace %zu < %zu", who, have, need);
  return HLA_ERR_WORKSPACE;
}

// hla_s2g_config -> kernel scalars
static inline bool lm_newton(const hla_s2g_config* cfg) { return cfg->optimizer == 0 || cfg->optimizer == 3; }      // LM or GN
// re-initialise a shift that left the search range (models_kitti.py:1028-1033); SGD_update / ADAM_update never do
static inline bool lm_reinit(const hla_s2g_config* cfg) { return (cfg->ford || cfg->dof == 3) && lm_newton(cfg); }
static inline LmGeom lm_geom_of(const hla_s2g_config* cfg, const hla_s2g_level& v) {
  LmGeom g{};
  g.ford = cfg->ford; g.lat = cfg->shift_range_lat; g.lon = cfg->shift_range_lon; g.rot = cfg->rotation_range;
  g.mpp = v.meter_per_pixel; g.ctr = v.centre;
  return g;
}
static inline LmSolveCfg lm_solve_cfg_of(const hla_s2g_config* cfg) {
  LmSolveCfg s{};
  s.gn = cfg->optimizer == 3 ? 1 : 0;
  s.dof = cfg->dof; s.use_hessian = s.gn ? 0 : cfg->use_hessian;
  for (int i = 0; i < 3; ++i) s.lam[i] = s.gn ? 0.0 : cfg->damping[i];      // GN_update: delta = -H^-1 J^T W r
  return s;
}

// hla_s2g_level -> the dimension fields an argument struct shares with its kin (AccumArgs, RepairLevel, BwdAccumArgs, PsArgs;
// G2sAccumArgs, G2sBwdAccumArgs, GpsArgs, GpsbArgs)
template <class Args>
static inline void lm_fill_s2g_dims(Args& a, const hla_s2g_level& v, const LmTiling& t) {
  a.A = v.A; a.h = v.h; a.w = v.w; a.row0 = v.row0; a.npix = t.npix; a.TP = t.TP; a.nt = t.nt;
  a.hs = v.h - v.grd_row_skip; a.rskip = v.grd_row_skip;
}
template <class Args>
static inline void lm_fill_g2s_dims(Args& a, const hla_s2g_level& v, const LmTiling& t) {      // (TP: GpsArgs has none, its kernel derives it)
  a.A = v.A; a.h = v.h; a.w = v.w; a.ctr = v.A / 2; a.npix = t.npix; a.nt = t.nt;
}
// the profiler id of an accumulate launch
static inline int lm_prof_id(int C) { return C == 256 ? K_LM256 : C == 128 ? K_LM128 : C == 64 ? K_LM64 : K_LM16; }

// Channel dispatch: calls f(std::integral_constant<int, c>) for the c of the list that equals C, and nothing for any other C (the
// entry points have validated it).  The list IS the set of kernel instantiations: a kernel without a 16-channel instance is
// dispatched without 16.  (Recursive, not a fold: the instantiations then reach the compiler in list order, as a switch's cases
// do, and the code object keeps its kernels in that order.)
template <int C0, int... Cs, class F>
static inline void lm_dispatch_c(int C, F&& f) {
  if (C == C0) f(std::integral_constant<int, C0>{});
  else if constexpr (sizeof...(Cs) > 0) lm_dispatch_c<Cs...>(C, f);
}
