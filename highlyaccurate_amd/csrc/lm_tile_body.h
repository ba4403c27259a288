// The per-tile part of the forward LM accumulate kernels, as TEXT: lm_accum (csrc/lm_solve.hip) includes it once, lm_repair_loop
// once per channel count, lmv_accum (csrc/lm_views.hip) once.  One tile of one sample, by 256 threads: pixel set-up into pp[], the gather loop, the wave and block
// reductions and the tile's 14 published partials (row `tile` of the sample's rows of a.part).
//
// Why not a __forceinline__ function: the gather's sums are written as a * b + c * d and -ffp-contract=fast lets the backend fuse
// EITHER product; which one it takes follows the operand order the optimiser happens to leave, and that order moved when the body
// was inlined through a function boundary (built and measured: same registers, same instruction counts, but the other product
// fused in `top`, `bot`, `s` and `dsx` -- poses 1 ulp off the previous build's in 11 of 96 values of the benchmark's dump).
// Included as text, lm_accum compiles to the instruction stream it had before this file existed.
//
// In scope at the point of inclusion:
//   C, USE_W, F      compile-time: channels, confidence weights, map element type
//   AccumArgs a; int b, tile; int t (0..255: the thread's id within the 256)
//   bool active      false: these 256 threads have no tile (np = 0, nothing published) but still meet the three barriers
//   PixParam pp[FWD_MAX_TP]; float red[4][14]; double redd[14]      shared arrays of these 256 threads
//   LM_TILE_COEF            expression: const double* to the sample's COEF_N projection coefficients
//   LM_TILE_BEFORE_PUBLISH  statement(s) between the last barrier and the publication (lm_accum: waves 1-3 leave)
// Everything the fragment indexes by b -- a.sat, a.grd, a.conf, a.part, the depth map of a.pts, a.reach_flag -- it indexes by the
// SAME b.  A kernel whose arrays do not share one index (lmv_accum: ground map per view, satellite map per sample, table per
// view) hands the fragment copies of those pointers moved to its elements and b = 0, and leaves this text alone.
// The barriers are __syncthreads(): in lm_accum the 256 threads are the workgroup; in lm_repair_loop four such groups share one
// and walk their tiles in lockstep.  Declares p0, np, cf, lane, wave, ... : include it inside a block of its own.
// An inactive group is kept from every memory access by np = 0 ALONE: both pixel loops run `< np`, the address arithmetic in
// front of them dereferences nothing, and the publication tests `active`.  Code added here must keep that.
// Not pinned (left to -ffp-contract=fast, held by tests/test_lm_repair_launch.py): the per-pixel sums b1, b2, Q, U3, V3 -- written
// as fmaf they no longer vectorise, none of the 32 choices keeps lm_accum's instruction stream -- and the fp64 publication sums.
#if !defined(LM_TILE_COEF) || !defined(LM_TILE_BEFORE_PUBLISH)
#error "lm_tile_body.h is a text fragment of lm_accum / lm_repair_loop / lmv_accum: define LM_TILE_COEF and LM_TILE_BEFORE_PUBLISH"
#endif
  const int p0 = tile * a.TP;
  const int np = active ? min(a.TP, a.npix - p0) : 0;
  const double* cf = LM_TILE_COEF;

  for (int tt = t; tt < np; tt += 256) {
    const int p = p0 + tt;
    const int r = a.row0 + p / a.w, c = p % a.w;
    const float cw = USE_W ? a.conf[((size_t)b * a.hs + (r - a.rskip)) * a.w + c] : 1.f;
    float q[3];
    const bool gm = lm_point(a.pts, b, r, c, a.w, q);
    const bool kept = !a.keep || a.keep[p];
    PixParam P = lm_pixel<C>(cf, q, gm, a.A, cw, a.col0, (a.reach_flag && kept) ? a.reach_flag + b : nullptr);
    if (!kept) {          // dropped by args.dropout: the pixel leaves every sum (models_kitti.py:968-974)
      P.wx0 = P.wx1 = P.wy0 = P.wy1 = 0.f; P.off = a.col0 * C; P.dxo = P.dyo = 0; P.j2u = P.j2v = 0.f; P.gm = P.wt = P.m = 0.f;
    }
    pp[tt] = P;
  }
  __syncthreads();

  const float j0u = (float)cf[8], j0v = (float)cf[9], j1u = (float)cf[10], j1v = (float)cf[11];
  constexpr int EPL = 16 / (int)sizeof(F);   // channels per lane (16 B)
  constexpr int LPP = C / EPL;        // lanes per pixel
  constexpr int PPW = 64 / LPP;       // pixels per wave-iteration
  const int lane = t & 63, wave = t >> 6;
  const int sub = lane / LPP, cl = (lane % LPP) * EPL;
  const F* satb = (const F*)a.sat + (size_t)b * a.A * a.A * C + cl;
  const F* grdb = (const F*)a.grd + ((size_t)b * a.hs * a.w + (size_t)(a.row0 - a.rskip) * a.w + p0) * C + cl;

  // With J_a = dsx*a_u + dsy*a_v (a = u, v, theta) and only the theta row's (a_u, a_v) = (j2u, j2v) varying per pixel, every
  // normal-equation sum is a combination of CHANNEL sums of a pixel -- Sxx = sum dsx^2, Sxy, Syy, Sxs = sum dsx*s, Sys, Sxg, Syg --
  // with per-pixel (j2u, j2v, weight) or per-sample (j0*, j1*) coefficients.  So the inner loop only forms those nine channel
  // sums (9 FMAs per element instead of 6 for the J's + 14), the per-pixel step folds in what varies per pixel, and the
  // per-sample coefficients are applied once per block, in fp64, after the reduction:
  //   T1..3 = sum w (Sxx, Sxy, Syy)        B1 = sum w (j2u Sxx + j2v Sxy)   B2 = sum w (j2u Sxy + j2v Syy)
  //   Q = sum (j2u b1 + j2v b2) = H22      U1,2 = sum w (Sxs, Sys)   U3 = sum w (j2u Sxs + j2v Sys)   V likewise with g
  float aS = 0, aG = 0, T1 = 0, T2 = 0, T3 = 0, B1 = 0, B2 = 0, Q = 0, U1 = 0, U2 = 0, U3 = 0, V1 = 0, V2 = 0, V3 = 0;

  constexpr int UNR = LM_UNROLL(F);
#pragma unroll UNR
  // (measured with the gather loop compiled out: a launch's FIXED cost -- the fp64 pixel set-up, the reductions, the published
  // partials, the ticket round trip, the closing solve -- is 31 / 20 / 13 us of the 73 / 43 / 30 us at C = 64 / 128 / 256)
  for (int i = wave * PPW + sub; i < np; i += 4 * PPW) {
    const PixParam P = pp[i];
    const uint4 t00 = *(const uint4*)(satb + P.off);
    const uint4 t01 = *(const uint4*)(satb + P.off + P.dxo);
    const uint4 t10 = *(const uint4*)(satb + P.off + P.dyo);
    const uint4 t11 = *(const uint4*)(satb + P.off + P.dyo + P.dxo);
    const uint4 gg = *(const uint4*)(grdb + (size_t)i * C);
    lm_f2 xx = {0.f, 0.f}, xy = xx, yy = xx, xs = xx, ys = xx, xg = xx, yg = xx, ss2 = xx, gg2 = xx;
#pragma unroll
    for (int ep = 0; ep < EPL / 2; ++ep) {
      const lm_f2 c00 = lm_pair<F>(t00, ep), c01 = lm_pair<F>(t01, ep), c10 = lm_pair<F>(t10, ep), c11 = lm_pair<F>(t11, ep);
      // (a * b + c * d: WHICH product is fused is written out -- left to -ffp-contract=fast it follows the operand order the
      // optimiser leaves, which differs between the kernels that include this text, and the two roundings differ by an ulp)
      const lm_f2 top = lm_fma2(P.wx0, c00, P.wx1 * c01);
      const lm_f2 bot = lm_fma2(P.wx0, c10, P.wx1 * c11);
      const lm_f2 s = lm_fma2(P.wy0, top, P.wy1 * bot);
      const lm_f2 dsy = bot - top;
      const lm_f2 dsx = lm_fma2(P.wy0, c01 - c00, P.wy1 * (c11 - c10));
      const lm_f2 g = lm_pair<F>(gg, ep) * P.gm;
      xx += dsx * dsx; xy += dsx * dsy; yy += dsy * dsy;
      xs += dsx * s; ys += dsy * s; xg += dsx * g; yg += dsy * g;
      ss2 += s * s; gg2 += g * g;
    }
    float Sxx = xx.x + xx.y, Sxy = xy.x + xy.y, Syy = yy.x + yy.y, Sxs = xs.x + xs.y, Sys = ys.x + ys.y;
    float Sxg = xg.x + xg.y, Syg = yg.x + yg.y;
    const float Sss = ss2.x + ss2.y, Sgg = gg2.x + gg2.y;
    aS += Sss; aG += Sgg;
    if (USE_W) { Sxx *= P.wt; Sxy *= P.wt; Syy *= P.wt; Sxs *= P.wt; Sys *= P.wt; Sxg *= P.wt; Syg *= P.wt; }
    T1 += Sxx; T2 += Sxy; T3 += Syy;
    const float b1 = P.j2u * Sxx + P.j2v * Sxy, b2 = P.j2u * Sxy + P.j2v * Syy;
    B1 += b1; B2 += b2;
    Q += P.j2u * b1 + P.j2v * b2;
    U1 += Sxs; U2 += Sys; U3 += P.j2u * Sxs + P.j2v * Sys;
    V1 += Sxg; V2 += Syg; V3 += P.j2u * Sxg + P.j2v * Syg;
  }

  float acc[14] = {aS, aG, T1, T2, T3, B1, B2, Q, U1, U2, U3, V1, V2, V3};
#pragma unroll
  for (int k = 0; k < 14; ++k) acc[k] = wave_sum_f32(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 14; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (t < 14) redd[t] = ((double)red[0][t] + (double)red[1][t]) + ((double)red[2][t] + (double)red[3][t]);
  __syncthreads();
  LM_TILE_BEFORE_PUBLISH
  if (active && t < PART_N) {
    // the per-sample rows of d(uv)/d(pose): fp32 values (the gather used to apply them in fp32), combined in fp64
    const double au = (double)j0u, av = (double)j0v, bu = (double)j1u, bv = (double)j1v;
    const double t1 = redd[2], t2 = redd[3], t3 = redd[4], b1 = redd[5], b2 = redd[6];
    double v = 0.0;
    switch (t) {
      case 0: v = redd[0]; break;                                             // sum s^2
      case 1: v = redd[1]; break;                                             // sum g^2
      case 2: v = au * au * t1 + 2.0 * au * av * t2 + av * av * t3; break;    // H00
      case 3: v = au * bu * t1 + (au * bv + av * bu) * t2 + av * bv * t3; break;   // H01
      case 4: v = au * b1 + av * b2; break;                                   // H02
      case 5: v = bu * bu * t1 + 2.0 * bu * bv * t2 + bv * bv * t3; break;    // H11
      case 6: v = bu * b1 + bv * b2; break;                                   // H12
      case 7: v = redd[7]; break;                                             // H22
      case 8: v = au * redd[8] + av * redd[9]; break;                         // J^T W s
      case 9: v = bu * redd[8] + bv * redd[9]; break;
      case 10: v = redd[10]; break;
      case 11: v = au * redd[11] + av * redd[12]; break;                      // J^T W g
      case 12: v = bu * redd[11] + bv * redd[12]; break;
      case 13: v = redd[13]; break;
      default: break;
    }
    __hip_atomic_store(a.part + ((size_t)b * a.part_ld + tile) * PART_N + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

