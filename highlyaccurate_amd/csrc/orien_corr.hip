// LM_S2GP.orien_corr (models_kitti.py:1543-1624): the sliding correlation of the ground map against the polar-resampled satellite
// map along the heading axis, its normalisation, the triplet loss, and their gradients.
//   P1   [B,H,W+S-1,C] the window of the polar satellite map the S shifts read (the reference's polar_sat1: columns -n .. W+n-1 of
//                      polar_grids[l] modulo its width, S = 2n+1, where its slices do not clamp), sampled by hla_grid_sample from
//                      the RAW satellite map; P1n = p1_inv_norm[b] * P1 is what the reference correlates
//   f    [B,H,W,C]     the ground map (raw * grd_inv_norm[b]);  g = f / max(||f||, 1e-12)           (F.normalize, 1572)
//   dot[b,s] = sum_{h,w,c} P1n[b,h,w+s,c] g[b,h,w,c]        the grouped conv2d, row 0               (1588-1589)
//   E[b,s]   = sum_{h,w<W,c} P1n[b,h,w+s,c]^2               avg_pool2d(.., divisor_override=1)      (1591-1592)
//   corr     = 2 - 2 dot / max(sqrt(E), 1e-6)                                                       (1593-1594)
// The contraction is a Hankel matrix-vector product per (sample, row, channel) -- no operand is shared across rows or channels, so
// it has no MFMA shape: fp32 VALU work on LDS-staged strips, every P1 element reused across shifts from registers.  Per-block
// partials are fp32, written to the workspace and reduced in a FIXED order in fp64 by a closing launch (so is E, from per-column
// energies and a sliding sum): the result does not depend on the order in which blocks finish.  The backward writes both
// gradients in gather form (no atomics): bitwise reproducible.  d_P1 goes on to the satellite map through hla_orien_window_bwd.
#include "common.h"

constexpr int OC_TW = 128, OC_TS = 64, OC_CC = 16, OC_CS = 20, OC_PC = OC_TW + OC_TS - 1;

// e[b,x] = sum_{h,c} src[b,h,x,c]^2 (fp64; a thread's <= H*C/256 terms in fp32, then a fixed-order fp64 tree).  grid (Wd, B)
__global__ __launch_bounds__(256) void oc_col_energy(const float* __restrict__ src, double* __restrict__ e, int H, int Wd, int C) {
  __shared__ double sh[4];
  const int x = blockIdx.x, b = blockIdx.y, t = threadIdx.x, C4 = C >> 2;
  const size_t row = (size_t)Wd * C;
  const float* base = src + ((size_t)b * H * Wd + x) * C;
  double acc = 0.0;
  for (int i = t; i < H * C4; i += 256) {
    const int h = i / C4, q = i % C4;
    const float4 v = *(const float4*)(base + (size_t)h * row + q * 4);
    acc += (double)(v.x * v.x + v.y * v.y) + (double)(v.z * v.z + v.w * v.w);
  }
  acc = wave_sum_f64(acc);
  if ((t & 63) == 0) sh[t >> 6] = acc;
  __syncthreads();
  if (t == 0) e[(size_t)b * Wd + x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// part[b][h * nWT + wt][s] = sum_{w in tile wt, c} P1[b,h,w+s,c] G[b,h,w,c] for the shifts of tile st.  grid (nWT * nST, H, B).
// A thread owns 8 columns x 4 shifts: per channel quad 11 + 8 LDS vectors feed 32 four-channel dot products.
__global__ __launch_bounds__(256) void oc_dot(const float* __restrict__ P1, const float* __restrict__ G, float* __restrict__ part,
                                              int H, int W, int Wp, int C, int nWT, int S) {
  __shared__ float sP[OC_PC * OC_CS];
  __shared__ float sG[OC_TW * OC_CS];
  __shared__ float red[16][OC_TS];
  const int wt = blockIdx.x % nWT, st = blockIdx.x / nWT, h = blockIdx.y, b = blockIdx.z;
  const int w0 = wt * OC_TW, s0 = st * OC_TS;
  const float* prow = P1 + ((size_t)b * H + h) * (size_t)Wp * C;
  const float* grow = G + ((size_t)b * H + h) * (size_t)W * C;
  const int t = threadIdx.x, i = t >> 4, j = t & 15;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < C; c0 += OC_CC) {
    __syncthreads();
    for (int e = t; e < OC_PC * 4; e += 256) {
      const int col = e >> 2, q = e & 3, x = w0 + s0 + col;
      *(float4*)(sP + col * OC_CS + q * 4) = x < Wp ? *(const float4*)(prow + (size_t)x * C + c0 + q * 4) : zero;
    }
    for (int e = t; e < OC_TW * 4; e += 256) {
      const int col = e >> 2, q = e & 3, w = w0 + col;
      *(float4*)(sG + col * OC_CS + q * 4) = w < W ? *(const float4*)(grow + (size_t)w * C + c0 + q * 4) : zero;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 g[8], p[11];
#pragma unroll
      for (int wi = 0; wi < 8; ++wi) g[wi] = *(const float4*)(sG + (8 * i + wi) * OC_CS + q * 4);
#pragma unroll
      for (int k = 0; k < 11; ++k) p[k] = *(const float4*)(sP + (8 * i + 4 * j + k) * OC_CS + q * 4);
#pragma unroll
      for (int wi = 0; wi < 8; ++wi)
#pragma unroll
        for (int si = 0; si < 4; ++si) {
          const float4 a = p[wi + si], c = g[wi];
          acc[si] += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
        }
    }
  }
#pragma unroll
  for (int si = 0; si < 4; ++si) red[i][4 * j + si] = acc[si];
  __syncthreads();
  if (t < OC_TS && s0 + t < S) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][t];
    part[((size_t)b * H * nWT + (size_t)h * nWT + wt) * S + s0 + t] = s;
  }
}

// fixed-order fp64 block sum of one value per thread (every thread gets the total)
__device__ __forceinline__ double oc_block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  return sh[0];
}

// grid B: the closing launch of the forward
__global__ __launch_bounds__(256) void oc_close(const float* __restrict__ part, const double* __restrict__ eP, const double* __restrict__ eG,
                                                const double* __restrict__ a_s, const double* __restrict__ a_g, double* __restrict__ dot,
                                                double* __restrict__ E, double* __restrict__ gnorm, float* __restrict__ corr, int NP, int S,
                                                int W, int Wp) {
  __shared__ double sh[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const double as = a_s ? a_s[b] : 1.0, ag = a_g ? a_g[b] : 1.0;
  double g2 = 0.0;
  for (int w = t; w < W; w += 256) g2 += eG[(size_t)b * W + w];
  g2 = oc_block_sum(g2, sh);
  const double nf = ag * sqrt(g2), N = fmax(nf, 1e-12);
  if (t == 0) gnorm[b] = nf;
  for (int s = t; s < S; s += 256) {
    double d = 0.0, e = 0.0;
    for (int p = 0; p < NP; ++p) d += (double)part[((size_t)b * NP + p) * S + s];
    for (int w = 0; w < W; ++w) e += eP[(size_t)b * Wp + s + w];
    d *= as * ag / N;
    e *= as * as;
    dot[(size_t)b * S + s] = d;
    E[(size_t)b * S + s] = e;
    corr[(size_t)b * S + s] = (float)(2.0 - 2.0 * d / fmax(sqrt(e), 1e-6));
  }
}

// grid B: the per-sample scalars of the backward.  With D = max(sqrt(E), 1e-6):
//   ddot[s] = -2 d_corr[s] / D,   dE[s] = d_corr[s] dot[s] / D^3 where sqrt(E) > 1e-6, else 0 (no gradient through a clamped E)
//   kappa = sum_s ddot[s] dot[s] = g . d_g   (the projection of the second normalisation)
//   d_f   = (a_s / N) sum_s ddot[s] P1[., w+s] - (a_g kappa / N^2) G           kf = ddot,            alpha[0], coefA
//   d_P1n = (a_g / N) sum_s ddot[s] G[., x-s]  + 2 a_s beta[x] P1              kr = ddot reversed,   alpha[1], coefB[x]
//   beta[x] = sum of dE[s] over the shifts whose window covers column x: max(0, x-W+1) <= s <= min(S-1, x)
__global__ __launch_bounds__(256) void oc_bwd_prep(const double* __restrict__ dot, const double* __restrict__ E, const double* __restrict__ gnorm,
                                                   const double* __restrict__ a_s, const double* __restrict__ a_g,
                                                   const float* __restrict__ d_corr, double* __restrict__ dE, double* __restrict__ kf,
                                                   double* __restrict__ kr, double* __restrict__ alpha, double* __restrict__ coefA,
                                                   double* __restrict__ coefB, int B, int S, int W, int Wp) {
  __shared__ double sh[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const double as = a_s ? a_s[b] : 1.0, ag = a_g ? a_g[b] : 1.0;
  const double nf = gnorm[b], N = fmax(nf, 1e-12);
  double kap = 0.0;
  for (int s = t; s < S; s += 256) {
    const double e = E[(size_t)b * S + s], sq = sqrt(e), D = fmax(sq, 1e-6), d = dot[(size_t)b * S + s];
    const double gc = (double)d_corr[(size_t)b * S + s];
    const double dd = -2.0 * gc / D;
    dE[(size_t)b * S + s] = sq > 1e-6 ? gc * d / (D * D * D) : 0.0;
    kf[(size_t)b * S + s] = dd;
    kr[(size_t)b * S + (S - 1 - s)] = dd;
    kap += dd * d;
  }
  kap = oc_block_sum(kap, sh);          // (its barriers also publish dE to the block)
  if (t == 0) {
    alpha[b] = as / N;
    alpha[B + b] = ag / N;
    coefA[b] = nf >= 1e-12 ? -ag * kap / (N * N) : 0.0;      // (a clamped norm is a constant: no projection)
  }
  for (int x = t; x < Wp; x += 256) {
    const int lo = max(0, x - W + 1), hi = min(S - 1, x);
    double be = 0.0;
    for (int s = lo; s <= hi; ++s) be += dE[(size_t)b * S + s];
    coefB[(size_t)b * Wp + x] = 2.0 * as * be;
  }
}

// out[b,h,x,c] = alpha[b] sum_s kern[b,s] src[b,h,x+off+s,c] + coef[b,x] self[b,h,x,c]   (src is zero outside [0,srcW))
// grid (nXT * C / CCH, H, B); a thread owns 4 columns x 4 channels and walks the shifts in tiles of 64 through an LDS strip.
// The sums are fp64: the triplet loss's cotangent sums to zero over the shifts, so each output is what is left of S cancelling
// terms, and fp32 accumulation showed in the parameter gradients (measured: EXPERIMENTS.md, "proj='polar' and orien_corr").
template <int NC4>
__global__ __launch_bounds__(256) void oc_corr1d(const float* __restrict__ src, int srcW, const float* __restrict__ self,
                                                 float* __restrict__ out, int outW, const double* __restrict__ kern,
                                                 const double* __restrict__ alpha, const double* __restrict__ coef, int coef_sb, int coef_sx,
                                                 int H, int C, int S, int off, int nXT) {
  constexpr int NWG = 256 / NC4, TW = 4 * NWG, TS = 64, PC = TW + TS - 1, CCH = NC4 * 4, CS = CCH + 4;
  __shared__ float sS[PC * CS];
  __shared__ double sK[TS];
  const int xt = blockIdx.x % nXT, c0 = (blockIdx.x / nXT) * CCH, h = blockIdx.y, b = blockIdx.z;
  const int x0 = xt * TW, t = threadIdx.x, c4 = t % NC4, wg = t / NC4;
  const float* srow = src + ((size_t)b * H + h) * (size_t)srcW * C + c0;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  double acc[4][4] = {};
  for (int s0 = 0; s0 < S; s0 += TS) {
    __syncthreads();
    for (int e = t; e < PC * NC4; e += 256) {
      const int col = e / NC4, q = e % NC4, xs = x0 + off + s0 + col;
      *(float4*)(sS + col * CS + q * 4) = (xs >= 0 && xs < srcW) ? *(const float4*)(srow + (size_t)xs * C + q * 4) : zero;
    }
    if (t < TS) sK[t] = s0 + t < S ? kern[(size_t)b * S + s0 + t] : 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TS + 3; ++k) {
      const float4 vf = *(const float4*)(sS + (4 * wg + k) * CS + c4 * 4);
      const double v[4] = {(double)vf.x, (double)vf.y, (double)vf.z, (double)vf.w};
#pragma unroll
      for (int xi = 0; xi < 4; ++xi) {
        const int sl = k - xi;
        if (sl >= 0 && sl < TS) {
          const double kk = sK[sl];
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[xi][c] += kk * v[c];
        }
      }
    }
  }
  const double al = alpha[b];
#pragma unroll
  for (int xi = 0; xi < 4; ++xi) {
    const int x = x0 + 4 * wg + xi;
    if (x < outW) {
      const size_t idx = (((size_t)b * H + h) * (size_t)outW + x) * C + c0 + c4 * 4;
      const float4 sv = *(const float4*)(self + idx);
      const double cf = coef[(size_t)b * coef_sb + (size_t)x * coef_sx];
      float4 o;
      o.x = (float)(al * acc[xi][0] + cf * sv.x); o.y = (float)(al * acc[xi][1] + cf * sv.y);
      o.z = (float)(al * acc[xi][2] + cf * sv.z); o.w = (float)(al * acc[xi][3] + cf * sv.w);
      *(float4*)(out + idx) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Backward of the window sampling (hla_grid_sample on the polar window) to the satellite map, summed in fp64.  Near the centre of
// the polar fan every column of a row lands on the same four texels, so a texel collects about a thousand terms that largely
// cancel (the cotangent sums to zero over the shifts): summed with fp32 atomics (hla_grid_sample_bwd) the result carried 7-10
// fp32 ulps of the map's maximum and changed from run to run.  Here the terms -- d_P1 times the exact bilinear weights, the forward's
// rules (grid_sample.hip: hard in-bounds mask, far corner clamped) -- are added to an fp64 image with hardware fp64 atomics (their
// order moves the sum by 1e-16 relative) and rounded to fp32 once by a second launch.
__global__ __launch_bounds__(256) void oc_window_bwd(const float* __restrict__ opt, const float* __restrict__ d_out, double* __restrict__ acc,
                                                     int N, int C, int IH, int IW, int HW) {
  const size_t total = (size_t)N * HW * C;
  const float lx = (float)(IW - 1), ly = (float)(IH - 1);
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const size_t pix = e / C;              // n*HW + p
    const int n = (int)(pix / HW);
    const float ix = opt[pix * 2 + 0], iy = opt[pix * 2 + 1];
    if (!((ix >= 0.f) && (ix <= lx) && (iy >= 0.f) && (iy <= ly))) continue;
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float x1 = fminf(x0 + 1.f, lx), y1 = fminf(y0 + 1.f, ly);
    const double wx0 = (double)(x1 - ix), wx1 = (double)(ix - x0), wy0 = (double)(y1 - iy), wy1 = (double)(iy - y0);
    const double g = (double)d_out[e];
    double* b = acc + (size_t)n * IH * IW * C + c;
    atomicAdd(b + ((size_t)y0 * IW + (size_t)x0) * C, g * (wx0 * wy0));
    atomicAdd(b + ((size_t)y0 * IW + (size_t)x1) * C, g * (wx1 * wy0));
    atomicAdd(b + ((size_t)y1 * IW + (size_t)x0) * C, g * (wx0 * wy1));
    atomicAdd(b + ((size_t)y1 * IW + (size_t)x1) * C, g * (wx1 * wy1));
  }
}

__global__ __launch_bounds__(256) void oc_round_f32(const double* __restrict__ acc, float* __restrict__ out, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) out[e] = (float)acc[e];
}

extern "C" int hla_orien_window_bwd(const float* optical, const float* d_out, double* acc, float* d_image, int N, int C, int IH,
                                    int IW, int H, int W, hla_stream_t stream) {
  HLA_REQUIRE(optical && d_out && acc && d_image, "hla_orien_window_bwd: null argument");
  HLA_REQUIRE(N > 0 && C > 0 && IH > 0 && IW > 0 && H > 0 && W > 0, "hla_orien_window_bwd: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const size_t img = (size_t)N * IH * IW * C, total = (size_t)N * H * W * C;
  HLA_CHECK_HIP(hipMemsetAsync(acc, 0, img * sizeof(double), st));
  const int g1 = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  hipLaunchKernelGGL(oc_window_bwd, dim3(g1), dim3(256), 0, st, optical, d_out, acc, N, C, IH, IW, H * W);
  const int g2 = (int)((img + 255) / 256 < 16384 ? (img + 255) / 256 : 16384);
  hipLaunchKernelGGL(oc_round_f32, dim3(g2), dim3(256), 0, st, (const double*)acc, d_image, img);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

// ---------------------------------------------------------------------------------------------
// triplet_loss (models_kitti.py:1607-1624), one level: sum_{b,s} log(1 + exp(10 (corr[b,gt_b] - corr[b,s]))) / (B (S - 1)),
// gt_b = (S-1)/2 + round(gt_heading[b] * rotation_range / degree_per_pixel) (fp32 like the reference's tensors, half to even;
// a negative index counts from the end like a Python index; one outside [-S,S) -- the reference raises -- gives NaN).
__device__ __forceinline__ int oc_gt_index(const float* gt, long long gs, int b, float rr, float deg, int S) {
  const float r = rintf(gt[(long long)b * gs] * rr / deg);
  const float fi = (float)(S - 1) / 2.f + r;
  if (!(fi >= -(float)S && fi < (float)S)) return -1;
  const int i = (int)fi;
  return i < 0 ? i + S : i;
}

__global__ __launch_bounds__(256) void oc_triplet(const float* __restrict__ corr, const float* __restrict__ gt, long long gs, float rr,
                                                  float deg, float* __restrict__ loss, int accumulate, int B, int S) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  double acc = 0.0;
  bool bad = false;
  for (int b = 0; b < B; ++b) {
    const int gi = oc_gt_index(gt, gs, b, rr, deg, S);
    if (gi < 0) { bad = true; continue; }
    const float pos = corr[(size_t)b * S + gi];
    for (int s = t; s < S; s += 256) acc += (double)log1pf(expf((pos - corr[(size_t)b * S + s]) * 10.f));
  }
  acc = oc_block_sum(acc, sh);
  if (t == 0) {
    const float v = bad ? __builtin_nanf("") : (float)acc / (float)((long long)B * (S - 1));
    loss[0] = accumulate ? loss[0] + v : v;
  }
}

// d_corr[b,s] = g/(B(S-1)) * 10 * ( [s == gt_b] sum_s' sig(z_s') - sig(z_s) ),  z_s = 10 (pos - corr[b,s]).   grid B
__global__ __launch_bounds__(256) void oc_triplet_bwd(const float* __restrict__ corr, const float* __restrict__ gt, long long gs, float rr,
                                                      float deg, const float* __restrict__ g_loss, float* __restrict__ d_corr, int B, int S) {
  __shared__ double sh[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int gi = oc_gt_index(gt, gs, b, rr, deg, S);
  const float sc = g_loss[0] * 10.f / (float)((long long)B * (S - 1));
  const float pos = gi >= 0 ? corr[(size_t)b * S + gi] : __builtin_nanf("");
  double tot = 0.0;
  for (int s = t; s < S; s += 256) {
    const float z = (pos - corr[(size_t)b * S + s]) * 10.f;
    const float sg = 1.f / (1.f + expf(-z));
    tot += (double)sg;
    d_corr[(size_t)b * S + s] = -sc * sg;
  }
  tot = oc_block_sum(tot, sh);          // (its barriers order the stores above before the update of the gt column)
  if (t == 0 && gi >= 0) d_corr[(size_t)b * S + gi] += sc * (float)tot;
}

// ---------------------------------------------------------------------------------------------
struct OcLayout { size_t eP, eG, part, dE, kf, kr, alpha, coefA, coefB, total; int nWT, nST, NP; };

static OcLayout oc_layout(int B, int H, int W, int Sn) {
  OcLayout L{};
  const size_t S = (size_t)Sn, Wp = (size_t)W + S - 1;
  L.nWT = (W + OC_TW - 1) / OC_TW;
  L.nST = (int)((S + OC_TS - 1) / OC_TS);
  L.NP = H * L.nWT;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += hla_align_up(bytes, 256); return at; };
  L.eP = take((size_t)B * Wp * 8);
  L.eG = take((size_t)B * W * 8);
  L.part = take((size_t)B * L.NP * S * 4);
  L.dE = take((size_t)B * S * 8);
  L.kf = take((size_t)B * S * 8);
  L.kr = take((size_t)B * S * 8);
  L.alpha = take((size_t)B * 2 * 8);
  L.coefA = take((size_t)B * 8);
  L.coefB = take((size_t)B * Wp * 8);
  L.total = o;
  return L;
}

static int oc_check(const char* who, int B, int H, int W, int C, int S) {
  HLA_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && W > 0 && S >= 1, "%s: need 0 < B, H <= 65535, W > 0, S >= 1", who);
  HLA_REQUIRE(C == 16 || C == 64 || C == 128 || C == 256, "%s: unsupported channel count %d (16, 64, 128, 256)", who, C);
  HLA_REQUIRE((long long)W + S < (1LL << 24), "%s: W + S must be below 2^24", who);
  return HLA_OK;
}

extern "C" size_t hla_orien_corr_workspace_bytes(int B, int H, int W, int C, int S) {
  if (oc_check("hla_orien_corr_workspace_bytes", B, H, W, C, S)) return 0;
  return oc_layout(B, H, W, S).total;
}

extern "C" int hla_orien_corr(const float* P1, const float* grd_feat, const double* p1_inv_norm, const double* grd_inv_norm,
                              double* dot, double* E, double* gnorm, float* corr, void* workspace, size_t workspace_bytes,
                              int B, int H, int W, int C, int S, hla_stream_t stream) {
  const int rc = oc_check("hla_orien_corr", B, H, W, C, S);
  if (rc) return rc;
  HLA_REQUIRE(P1 && grd_feat && dot && E && gnorm && corr && workspace, "hla_orien_corr: null argument");
  const OcLayout L = oc_layout(B, H, W, S);
  if (workspace_bytes < L.total) {
    hla_set_error("hla_orien_corr: workspace of %zu bytes, need %zu", workspace_bytes, L.total);
    return HLA_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int Wp = W + S - 1;
  double* eP = (double*)(ws + L.eP);
  double* eG = (double*)(ws + L.eG);
  float* part = (float*)(ws + L.part);
  hipLaunchKernelGGL(oc_col_energy, dim3(Wp, B), dim3(256), 0, st, P1, eP, H, Wp, C);
  hipLaunchKernelGGL(oc_col_energy, dim3(W, B), dim3(256), 0, st, grd_feat, eG, H, W, C);
  hipLaunchKernelGGL(oc_dot, dim3(L.nWT * L.nST, H, B), dim3(256), 0, st, P1, grd_feat, part, H, W, Wp, C, L.nWT, S);
  hipLaunchKernelGGL(oc_close, dim3(B), dim3(256), 0, st, (const float*)part, (const double*)eP, (const double*)eG, p1_inv_norm,
                     grd_inv_norm, dot, E, gnorm, corr, L.NP, S, W, Wp);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

template <int NC4>
static void oc_launch_corr1d(hipStream_t st, const float* src, int srcW, const float* self, float* out, int outW, const double* kern,
                             const double* alpha, const double* coef, int coef_sb, int coef_sx, int B, int H, int C, int S, int off) {
  constexpr int TW = 4 * (256 / NC4), CCH = NC4 * 4;
  const int nXT = (outW + TW - 1) / TW;
  hipLaunchKernelGGL((oc_corr1d<NC4>), dim3(nXT * (C / CCH), H, B), dim3(256), 0, st, src, srcW, self, out, outW, kern, alpha, coef,
                     coef_sb, coef_sx, H, C, S, off, nXT);
}

extern "C" int hla_orien_corr_bwd(const float* P1, const float* grd_feat, const double* p1_inv_norm, const double* grd_inv_norm,
                                  const double* dot, const double* E, const double* gnorm, const float* d_corr, float* d_P1,
                                  float* d_grd_feat, void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int S,
                                  hla_stream_t stream) {
  const int rc = oc_check("hla_orien_corr_bwd", B, H, W, C, S);
  if (rc) return rc;
  HLA_REQUIRE(P1 && grd_feat && dot && E && gnorm && d_corr && d_P1 && d_grd_feat && workspace, "hla_orien_corr_bwd: null argument");
  const OcLayout L = oc_layout(B, H, W, S);
  if (workspace_bytes < L.total) {
    hla_set_error("hla_orien_corr_bwd: workspace of %zu bytes, need %zu", workspace_bytes, L.total);
    return HLA_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int Wp = W + S - 1;
  double* dE = (double*)(ws + L.dE);
  double *kf = (double*)(ws + L.kf), *kr = (double*)(ws + L.kr), *alpha = (double*)(ws + L.alpha), *coefA = (double*)(ws + L.coefA),
         *coefB = (double*)(ws + L.coefB);
  hipLaunchKernelGGL(oc_bwd_prep, dim3(B), dim3(256), 0, st, dot, E, gnorm, p1_inv_norm, grd_inv_norm, d_corr, dE, kf, kr, alpha, coefA,
                     coefB, B, S, W, Wp);
  if (C == 16) {
    oc_launch_corr1d<4>(st, P1, Wp, grd_feat, d_grd_feat, W, kf, alpha, coefA, 1, 0, B, H, C, S, 0);
    oc_launch_corr1d<4>(st, grd_feat, W, P1, d_P1, Wp, kr, alpha + B, coefB, Wp, 1, B, H, C, S, -(S - 1));
  } else {
    oc_launch_corr1d<16>(st, P1, Wp, grd_feat, d_grd_feat, W, kf, alpha, coefA, 1, 0, B, H, C, S, 0);
    oc_launch_corr1d<16>(st, grd_feat, W, P1, d_P1, Wp, kr, alpha + B, coefB, Wp, 1, B, H, C, S, -(S - 1));
  }
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

static int oc_triplet_check(const char* who, const float* corr, const float* gt, double deg, int B, int S) {
  HLA_REQUIRE(corr && gt, "%s: null argument", who);
  HLA_REQUIRE(B > 0 && S > 0 && deg > 0.0, "%s: need B, S > 0 and degree_per_pixel > 0", who);
  return HLA_OK;
}

extern "C" int hla_orien_triplet_loss(const float* corr, const float* gt_heading, long long gt_stride, double rotation_range,
                                      double degree_per_pixel, float* loss, int accumulate, int B, int S, hla_stream_t stream) {
  const int rc = oc_triplet_check("hla_orien_triplet_loss", corr, gt_heading, degree_per_pixel, B, S);
  if (rc) return rc;
  HLA_REQUIRE(loss, "hla_orien_triplet_loss: null output");
  hipLaunchKernelGGL(oc_triplet, dim3(1), dim3(256), 0, (hipStream_t)stream, corr, gt_heading, gt_stride, (float)rotation_range,
                     (float)degree_per_pixel, loss, accumulate, B, S);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

extern "C" int hla_orien_triplet_loss_bwd(const float* corr, const float* gt_heading, long long gt_stride, double rotation_range,
                                          double degree_per_pixel, const float* g_loss, float* d_corr, int B, int S,
                                          hla_stream_t stream) {
  const int rc = oc_triplet_check("hla_orien_triplet_loss_bwd", corr, gt_heading, degree_per_pixel, B, S);
  if (rc) return rc;
  HLA_REQUIRE(g_loss && d_corr, "hla_orien_triplet_loss_bwd: null argument");
  hipLaunchKernelGGL(oc_triplet_bwd, dim3(B), dim3(256), 0, (hipStream_t)stream, corr, gt_heading, gt_stride, (float)rotation_range,
                     (float)degree_per_pixel, g_loss, d_corr, B, S);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}
