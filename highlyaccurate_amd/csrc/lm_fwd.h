// What the forward accumulate kernels of the satellite -> ground LM loop share: the argument struct of one accumulate launch, the
// channel-pair helpers of the gather loop, the occupancy / unroll constants and the forward tile size.  Included by lm_solve.hip
// (lm_accum, lm_repair_loop) and lm_views.hip (lmv_accum), the kernels that include the text fragment lm_tile_body.h.
#pragma once
#include "lm_host.h"

struct AccumArgs {
  const void* sat;    // [B,A,A,C]  F elements (fp32, or bf16 / fp16 in the reduced-precision inference modes)
  const void* grd;    // [B,h,w,C]
  const float* conf;  // [B,h,w] or null
  LmPoints pts;       // the pixels' 3-D points: shared table, or ray table x per-sample depth (lm_common.h)
  const double* coef; // [B,COEF_N]
  double* part;       // [B,part_ld,PART_N]: a sample's rows do not move with the level, so that stream groups on different
                      // steps (levels with different nt) never share a row
  int A, h, w, row0, npix, TP, nt, part_ld, xcd_affine;
  int b0, nb;         // this launch covers samples [b0, b0 + nb) of the batch; every per-sample array is indexed by the global b
  int hs, rskip;      // stored rows of grd/conf (h - grd_row_skip) and the skip itself
  const unsigned char* keep;   // dropout: [npix] of this step, 1 = pixel takes part; or null
  unsigned* ticket;   // [B] arrival counters of this step (zeroed before the loop): the LAST tile of a sample closes the step
  int col0;           // reach_mode = 1: first valid column of sat at this level, and
  int* reach_flag;    //   [B] flags a sample's pixels set when they read left of it (lm_pixel); else 0 / null
  const int* gate;    // reach_mode = 2: see SolveArgs::gate
};

// channel pair ep (compile-time after unrolling) of a 16-byte vector of F, as two fp32 in ADJACENT registers: the gather loop is
// written on such pairs so that it compiles to v_pk_{mul,add,fma}_f32 without operand shuffling.  (Left to itself the SLP
// vectoriser paired unrelated scalars: a third of the loop was v_mov_b32, and the kernel is VALU-issue-bound -- 80 % VALU busy.)
typedef float lm_f2 __attribute__((ext_vector_type(2)));
// w * x + y as ONE fused multiply-add per element, w a scalar
__device__ __forceinline__ lm_f2 lm_fma2(float w, lm_f2 x, lm_f2 y) { return __builtin_elementwise_fma(lm_f2{w, w}, x, y); }
template <typename F> __device__ __forceinline__ lm_f2 lm_pair(const uint4& v, int ep);
template <> __device__ __forceinline__ lm_f2 lm_pair<float>(const uint4& v, int ep) {
  lm_f2 r;
  r.x = __uint_as_float(ep == 0 ? v.x : v.z);
  r.y = __uint_as_float(ep == 0 ? v.y : v.w);
  return r;
}
template <> __device__ __forceinline__ lm_f2 lm_pair<__bf16>(const uint4& v, int ep) {      // bf16 -> fp32 is a 16-bit shift
  const unsigned w = ep == 0 ? v.x : ep == 1 ? v.y : ep == 2 ? v.z : v.w;
  lm_f2 r;
  r.x = __uint_as_float(w << 16);
  r.y = __uint_as_float(w & 0xffff0000u);
  return r;
}
template <> __device__ __forceinline__ lm_f2 lm_pair<_Float16>(const uint4& v, int ep) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const unsigned w = ep == 0 ? v.x : ep == 1 ? v.y : ep == 2 ? v.z : v.w;
  const h2 h = __builtin_bit_cast(h2, w);
  lm_f2 r;
  r.x = (float)h[0];
  r.y = (float)h[1];
  return r;
}

// (6 waves per SIMD = 80 registers: what the gather loop needs; the closing solve, one wave per sample, may spill a little)
// (measured: 3, 4 or 8 waves per SIMD with 1-4 pixels in flight per lane change nothing -- the kernel waits on its dependent taps)
#define LM_OCC 6
#define LM_UNROLL(F) (sizeof(F) == 4 ? 2 : 1)
// Pixels per block of the forward accumulate kernels (level-dependent only, like lm_pick_tile: a sample's partial-sum grouping
// must not depend on its batch mates).  Larger than the backward's tiles: a block's fixed cost -- the fp64 pixel set-up, the
// reductions, the published partials, the ticket -- is what these kernels spend their time on.
#define FWD_MAX_TP 512
// (measured on one box against 256 / 128 / 64: lm_accum<64> 72.3 -> 70.8 us, <128> 45.3 -> 41.7, <256> 30.8 -> 29.5; with 512 / 512 / 256
// the two coarse levels lose 10-30 %)
static inline int lm_pick_tile_fwd(int npix) { return npix >= 16384 ? 512 : (npix >= 4096 ? 256 : 128); }
static inline LmTiling fwd_tiling(const hla_s2g_level& v) { return lm_tiling(lm_npix_s2g(v), lm_pick_tile_fwd); }

// lm_solve.hip: what every hla_s2g_* entry point checks of its config and levels
int hla_s2g_validate(const char* who, const hla_s2g_config* cfg, const hla_s2g_level* lv, const float* R_FL,
                     const float* T_FL, int B);
