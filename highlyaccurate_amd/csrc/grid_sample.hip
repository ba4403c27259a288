// Stand-alone bilinear sampler with analytic Jacobian: jacobian.py:138-205.
// (The LM loop uses the fused kernel in lm_solve.hip; this is the operator-level entry point that
// mirrors the reference's `grid_sample(image, optical, jac)` for callers that want the maps.)
#include "common.h"

__global__ __launch_bounds__(256) void grid_sample_kernel(const float* __restrict__ img, const float* __restrict__ opt,
                                                          const float* __restrict__ jac, float* __restrict__ out,
                                                          float* __restrict__ jout, int N, int C, int IH, int IW,
                                                          int HW, int M) {
  const size_t total = (size_t)N * HW * C;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const size_t pix = e / C;              // n*HW + p
    const int n = (int)(pix / HW);
    const float ix = opt[pix * 2 + 0], iy = opt[pix * 2 + 1];
    const float lx = (float)(IW - 1), ly = (float)(IH - 1);
    const bool inb = (ix >= 0.f) && (ix <= lx) && (iy >= 0.f) && (iy <= ly);
    float v = 0.f, ddx = 0.f, ddy = 0.f;
    if (inb) {
      const float x0 = floorf(ix), y0 = floorf(iy);
      const float x1 = fminf(x0 + 1.f, lx), y1 = fminf(y0 + 1.f, ly);
      const float wx0 = x1 - ix, wx1 = ix - x0, wy0 = y1 - iy, wy1 = iy - y0;
      const float* b = img + (size_t)n * IH * IW * C + c;
      const float nw = b[((size_t)y0 * IW + (size_t)x0) * C], ne = b[((size_t)y0 * IW + (size_t)x1) * C];
      const float sw = b[((size_t)y1 * IW + (size_t)x0) * C], se = b[((size_t)y1 * IW + (size_t)x1) * C];
      v = nw * (wx0 * wy0) + ne * (wx1 * wy0) + sw * (wx0 * wy1) + se * (wx1 * wy1);
      ddx = -wy0 * nw + wy0 * ne - wy1 * sw + wy1 * se;
      ddy = -wx0 * nw - wx1 * ne + wx0 * sw + wx1 * se;
    }
    out[e] = v;
    if (jout) {
      for (int m = 0; m < M; ++m) {
        const float* j = jac + ((size_t)m * N * HW + pix) * 2;
        jout[(size_t)m * total + e] = ddx * j[0] + ddy * j[1];
      }
    }
  }
}

extern "C" int hla_grid_sample(const float* image, const float* optical, const float* jac, float* out, float* jac_out,
                               int N, int C, int IH, int IW, int H, int W, int M, hla_stream_t stream) {
  HLA_REQUIRE(image && optical && out, "hla_grid_sample: null argument");
  HLA_REQUIRE(N > 0 && C > 0 && IH > 0 && IW > 0 && H > 0 && W > 0, "hla_grid_sample: bad sizes");
  HLA_REQUIRE((jac == nullptr) == (jac_out == nullptr), "hla_grid_sample: jac and jac_out go together");
  const size_t total = (size_t)N * H * W * C;
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(grid_sample_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, image, optical, jac, out,
                     jac_out, N, C, IH, IW, H * W, jac ? M : 0);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Backward of the operator (include/hla.h, hla_grid_sample_bwd).  A group of LPP lanes owns one sample; a lane holds
// channels cl + e*LPP (e < EPL) of a chunk of LPP*EPL channels, so that one atomic wave-instruction covers a contiguous run
// of a texel's channels (256 B at C >= 64) and the tap loads are coalesced.  EXACT: C == LPP*EPL, one chunk, no channel
// masks; otherwise the chunk loop covers any C.  The 2 + 2M per-sample sums are reduced inside the lane group with
// __shfl_xor and stored by its first lane (one owner per sample, no atomics); d_image is accumulated with fp32 atomicAdd
// (one hardware add under -munsafe-fp-atomics), so its last bits depend on arrival order.  W_IMG / W_OPT / W_JAC: which
// outputs are wanted; an unwanted one removes its loads, arithmetic and reductions.
struct GsBwdArgs {
  const float *img, *opt, *jac, *d_out, *d_jac_out;
  float *d_img, *d_opt, *d_jac;
  int N, C, IH, IW, HW, M;
};

template <int LPP, int EPL, bool EXACT, bool W_IMG, bool W_OPT, bool W_JAC>
__global__ __launch_bounds__(256) void grid_sample_bwd_kernel(const GsBwdArgs a) {
  constexpr int PPB = 256 / LPP;                     // samples per block
  constexpr bool TAPS = W_OPT || W_JAC;              // d_image alone needs no image values
  const int cl = threadIdx.x % LPP, sub = threadIdx.x / LPP;
  const int C = EXACT ? LPP * EPL : a.C;
  const size_t npix = (size_t)a.N * a.HW;
  const float lx = (float)(a.IW - 1), ly = (float)(a.IH - 1);
  const bool has_g = a.d_out != nullptr;
  const int M = a.d_jac_out ? a.M : 0;
  for (size_t base = (size_t)blockIdx.x * PPB; base < npix; base += (size_t)gridDim.x * PPB) {   // uniform per block
    const size_t pix = base + sub;
    const bool live = pix < npix;
    float ix = -1.f, iy = -1.f;
    if (live) { ix = a.opt[pix * 2 + 0]; iy = a.opt[pix * 2 + 1]; }
    const bool inb = (ix >= 0.f) && (ix <= lx) && (iy >= 0.f) && (iy <= ly);
    float wx0 = 0.f, wx1 = 0.f, wy0 = 0.f, wy1 = 0.f;
    size_t o_nw = 0, o_ne = 0, o_sw = 0, o_se = 0;
    if (inb) {
      const float x0 = floorf(ix), y0 = floorf(iy);
      const float x1 = fminf(x0 + 1.f, lx), y1 = fminf(y0 + 1.f, ly);
      wx0 = x1 - ix; wx1 = ix - x0; wy0 = y1 - iy; wy1 = iy - y0;
      const size_t ib = (pix / a.HW) * (size_t)a.IH * a.IW;
      o_nw = (ib + (size_t)y0 * a.IW + (size_t)x0) * C; o_ne = (ib + (size_t)y0 * a.IW + (size_t)x1) * C;
      o_sw = (ib + (size_t)y1 * a.IW + (size_t)x0) * C; o_se = (ib + (size_t)y1 * a.IW + (size_t)x1) * C;
    }
    float sox = 0.f, soy = 0.f;
    for (int cb = 0; cb < C; cb += LPP * EPL) {
      float g[EPL], av[EPL], bv[EPL], ddx[EPL], ddy[EPL], crs[EPL];
      bool ok[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const int c = cb + cl + e * LPP;
        ok[e] = inb && (EXACT || c < C);
        g[e] = (ok[e] && has_g) ? a.d_out[pix * C + c] : 0.f;
        av[e] = bv[e] = ddx[e] = ddy[e] = crs[e] = 0.f;
        if (TAPS && ok[e]) {
          const float nw = a.img[o_nw + c], ne = a.img[o_ne + c], sw = a.img[o_sw + c], se = a.img[o_se + c];
          ddx[e] = wy0 * (ne - nw) + wy1 * (se - sw);
          ddy[e] = wx0 * (sw - nw) + wx1 * (se - ne);
          crs[e] = nw - ne - sw + se;
        }
      }
      for (int m = 0; m < M; ++m) {                  // uniform: every lane of the wave takes part in the reductions
        const size_t mp = (size_t)m * npix + pix;
        float jx = 0.f, jy = 0.f, sx = 0.f, sy = 0.f;
        if (inb) { jx = a.jac[mp * 2 + 0]; jy = a.jac[mp * 2 + 1]; }
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const float dj = ok[e] ? a.d_jac_out[mp * C + (cb + cl + e * LPP)] : 0.f;
          if (W_IMG || W_OPT) { av[e] += dj * jx; bv[e] += dj * jy; }
          if (W_JAC) { sx += dj * ddx[e]; sy += dj * ddy[e]; }
        }
        if (W_JAC) {
#pragma unroll
          for (int o = LPP >> 1; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
          if (live && cl == 0) {
            float* p = a.d_jac + mp * 2;
            if (EXACT || cb == 0) { p[0] = sx; p[1] = sy; } else { p[0] += sx; p[1] += sy; }   // same lane wrote chunk 0
          }
        }
      }
      if (W_OPT) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) { sox += g[e] * ddx[e] + bv[e] * crs[e]; soy += g[e] * ddy[e] + av[e] * crs[e]; }
      }
      if (W_IMG) {
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (ok[e]) atomicAdd(a.d_img + o_nw + (cb + cl + e * LPP), g[e] * (wx0 * wy0) - av[e] * wy0 - bv[e] * wx0);
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (ok[e]) atomicAdd(a.d_img + o_ne + (cb + cl + e * LPP), g[e] * (wx1 * wy0) + av[e] * wy0 - bv[e] * wx1);
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (ok[e]) atomicAdd(a.d_img + o_sw + (cb + cl + e * LPP), g[e] * (wx0 * wy1) - av[e] * wy1 + bv[e] * wx0);
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (ok[e]) atomicAdd(a.d_img + o_se + (cb + cl + e * LPP), g[e] * (wx1 * wy1) + av[e] * wy1 + bv[e] * wx1);
      }
    }
    if (W_OPT) {
#pragma unroll
      for (int o = LPP >> 1; o > 0; o >>= 1) { sox += __shfl_xor(sox, o, 64); soy += __shfl_xor(soy, o, 64); }
      if (live && cl == 0) { a.d_opt[pix * 2 + 0] = sox; a.d_opt[pix * 2 + 1] = soy; }
    }
  }
}

template <int LPP, int EPL, bool EXACT>
static void gs_bwd_launch(const GsBwdArgs& a, hipStream_t st) {
  const size_t npix = (size_t)a.N * a.HW, ppb = 256 / LPP;
  const size_t nb = (npix + ppb - 1) / ppb;
  const dim3 grid((unsigned)(nb < 8192 ? nb : 8192)), block(256);
  const int want = (a.d_img ? 1 : 0) | (a.d_opt ? 2 : 0) | (a.d_jac ? 4 : 0);
  switch (want) {
#define GS_BWD_CASE(k) \
    case k: hipLaunchKernelGGL((grid_sample_bwd_kernel<LPP, EPL, EXACT, ((k) & 1) != 0, ((k) & 2) != 0, ((k) & 4) != 0>), grid, block, 0, st, a); break;
    GS_BWD_CASE(1) GS_BWD_CASE(2) GS_BWD_CASE(3) GS_BWD_CASE(4) GS_BWD_CASE(5) GS_BWD_CASE(6) GS_BWD_CASE(7)
#undef GS_BWD_CASE
    default: break;
  }
}

extern "C" int hla_grid_sample_bwd(const float* image, const float* optical, const float* jac, const float* d_out,
                                   const float* d_jac_out, float* d_image, float* d_optical, float* d_jac, int N, int C,
                                   int IH, int IW, int H, int W, int M, hla_stream_t stream) {
  HLA_REQUIRE(image && optical, "hla_grid_sample_bwd: image and optical must not be NULL");
  HLA_REQUIRE(N > 0 && C > 0 && IH > 0 && IW > 0 && H > 0 && W > 0, "hla_grid_sample_bwd: bad sizes");
  HLA_REQUIRE(!d_jac_out || jac, "hla_grid_sample_bwd: d_jac_out given without jac");
  HLA_REQUIRE(!d_jac || jac, "hla_grid_sample_bwd: d_jac wanted without jac");
  HLA_REQUIRE(!(d_jac_out || d_jac) || M > 0, "hla_grid_sample_bwd: d_jac_out / d_jac need M > 0 (got %d)", M);
  if (!d_image && !d_optical && !d_jac) return HLA_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t npix = (size_t)N * H * W;
  // a NULL cotangent stands for zeros: the outputs that depend on it alone are zero-filled and leave the launch
  if (d_jac && !d_jac_out) {
    HLA_CHECK_HIP(hipMemsetAsync(d_jac, 0, (size_t)M * npix * 2 * sizeof(float), st));
    d_jac = nullptr;
  }
  if (!d_out && !d_jac_out) {          // every gradient is zero; d_image is accumulated into, so it stays as it is
    if (d_optical) HLA_CHECK_HIP(hipMemsetAsync(d_optical, 0, npix * 2 * sizeof(float), st));
    return HLA_OK;
  }
  if (!d_image && !d_optical && !d_jac) return HLA_OK;
  const GsBwdArgs a{image, optical, jac, d_out, d_jac_out, d_image, d_optical, d_jac, N, C, IH, IW, H * W, d_jac_out ? M : 0};
  switch (C) {
    case 16: gs_bwd_launch<16, 1, true>(a, st); break;       // four samples per wave
    case 32: gs_bwd_launch<32, 1, true>(a, st); break;
    case 64: gs_bwd_launch<64, 1, true>(a, st); break;
    case 128: gs_bwd_launch<64, 2, true>(a, st); break;
    case 256: gs_bwd_launch<64, 4, true>(a, st); break;
    default:                                                  // any other C: masked channel chunks
      if (C == 1) gs_bwd_launch<1, 1, false>(a, st);          // confidence maps: one lane per sample
      else if (C <= 8) gs_bwd_launch<8, 1, false>(a, st);
      else gs_bwd_launch<64, 1, false>(a, st);
  }
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}
