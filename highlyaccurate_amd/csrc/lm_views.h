// Index and workspace arithmetic of the multi-view LM loop (lm_views.hip), in plain C++: the kernels and the launcher include it,
// and so does the host sweep of tests/test_lm_views_ref_cpu.py, which walks every index they form (the pattern of g2s_corr_tile.h).
//
// V views of one body pose: view v of sample b is PSEUDO-SAMPLE j = b * V + v.  Ground map, confidence map, ground inverse norm,
// projection coefficients, extrinsics (R, T) and the rows of the partial sums are per pseudo-sample; the satellite map, its
// inverse norm, the pose, the re-initialisation draws and the trace are per sample; the ground-point table is per view.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define LMV_HD __host__ __device__ inline
#else
#define LMV_HD inline
#endif

constexpr int LMV_MAX_VIEWS = 8;      // a cap, not a measurement: Ford carries seven cameras
constexpr int LMV_COEF_N = 16;        // = COEF_N (lm_common.h; lm_views.hip asserts it)
constexpr int LMV_PART_N = 16;        // = PART_N

LMV_HD int lmv_pseudo(int b, int v, int V) { return b * V + v; }
LMV_HD int lmv_sample(int j, int V) { return j / V; }
LMV_HD int lmv_view(int j, int V) { return j % V; }

// element offsets of what pseudo-sample j reads and writes
LMV_HD size_t lmv_sat_offset(int j, int V, int A, int C) { return (size_t)lmv_sample(j, V) * A * A * C; }
LMV_HD size_t lmv_grd_offset(int j, int hs, int w, int C) { return (size_t)j * hs * w * C; }      // hs: stored rows
LMV_HD size_t lmv_conf_offset(int j, int hs, int w) { return (size_t)j * hs * w; }
LMV_HD size_t lmv_table_offset(int j, int V, int h, int w) { return (size_t)lmv_view(j, V) * h * w * 3; }
LMV_HD size_t lmv_coef_offset(int j) { return (size_t)j * LMV_COEF_N; }
LMV_HD size_t lmv_part_offset(int j, int tile, int part_ld) { return ((size_t)j * part_ld + tile) * LMV_PART_N; }
LMV_HD size_t lmv_view_sums_offset(int b, int v, int V) { return (size_t)lmv_pseudo(b, v, V) * 16; }

LMV_HD size_t lmv_align(size_t x) { return (x + 255) / 256 * 256; }

// byte offsets into the workspace; part_ld = the largest tile count over the levels
struct LmvLayout { size_t coef, pose, part, total; };
LMV_HD LmvLayout lmv_layout(int B, int V, int part_ld) {
  LmvLayout L{};
  const size_t J = (size_t)B * V;
  size_t o = 0;
  L.coef = o; o += lmv_align(J * LMV_COEF_N * 8);                      // [B*V,COEF_N] fp64
  L.pose = o; o += lmv_align((size_t)B * 3 * 4);                       // [B,3] fp32
  L.part = o; o += lmv_align(J * part_ld * LMV_PART_N * 8);            // [B*V,part_ld,PART_N] fp64
  L.total = o;
  return L;
}
