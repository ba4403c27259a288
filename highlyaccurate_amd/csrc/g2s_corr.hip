// LM_G2SP.corr (models_kitti.py:501-577) and its triplet_loss (579-595): the dense translation search.  The ground map, projected
// onto the satellite plane at the zero pose and centre-cropped (the caller samples the crop with hla_grid_sample), slides over the
// satellite map in both axes:
//   s    [B,A,A,C]    the satellite map (raw * sat_inv_norm[b])
//   f    [B,Hc,Wc,C]  the crop (raw * g2s_inv_norm[b]);  g = f / max(||f||, 1e-12)                    (F.normalize, 549)
//   dot[b,dy,dx] = sum_{y<Hc,x<Wc,c} g[b,y,x,c] s[b,y+dy,x+dx,c]     the grouped conv2d              (551-552)
//   E[b,dy,dx]   = sum_{y<Hc,x<Wc,c} s[b,y+dy,x+dx,c]^2              avg_pool2d(.., divisor_override=1), channel sum  (554-555)
//   corr         = 2 - 2 dot / max(sqrt(E), 1e-6)                                                     (556-557)
// FORWARD.  Per sample the contraction is a GEMM, M = dx, N = dy, K = (satellite row r, x, c), on v_mfma_f32_32x32x2_f32 (exact
// fp32 products).  For one satellite row r the A operand is a Toeplitz view of an LDS-staged row strip (lane dx reads column
// x + dx), the B operand the crop rows r - dy of the tile's 32 dy.  Operand reuse: a workgroup walks r for ONE K column (16 x by
// 16 channels) at a time and keeps that column of the 32 live crop rows as a RING in LDS (row y in slot y mod 32): every r step
// fetches one new crop row (1 KB) and one satellite strip (3 KB) for 128 MFMAs, instead of the tile's whole [32,Wc,C] slab.  The
// K columns of a tile, not its rows, are split over up to 16 workgroups (a column split needs no ring warm-up; the split depends on
// the shape only, never on B).  Numerics: an accumulator element collects 64 products per r step and is flushed into an fp64
// register sum every 64 steps (4096 products); the four waves' sums are added in fp64 in a fixed order, the workgroups' partials
// are stored plainly and added in fp64 in split order by the closing launch.  Nothing depends on B, the grid or the run.
// E: per-pixel channel energies in fp64, then separable window sums (rows, then columns), every sum in a fixed order.
// BACKWARD.  Both gradients are 2-D correlations of the shift plane ddot with a map, in gather form (no atomics, bitwise
// reproducible).  They run on the vector ALU, LDS-tiled, fp32 operands with fp64 accumulators (orien_corr's oc_corr1d with an
// outer loop over dy); the MFMA form is not built (EXPERIMENTS.md, "LM_G2SP.corr").
#include "common.h"
#include "g2s_corr_tile.h"

typedef float gc_f32x16 __attribute__((ext_vector_type(16)));

// e[pix] = sum_c src[pix,c]^2 in fp64; four lanes share a pixel (lane q takes float4 q, q+4, ..), added in a fixed order
__global__ __launch_bounds__(256) void gc_energy(const float* __restrict__ src, double* __restrict__ e, size_t npix, int C) {
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, pix = gid >> 2;
  const int l4 = (int)(gid & 3), C4 = C >> 2;
  double acc = 0.0;
  if (pix < npix)
    for (int q = l4; q < C4; q += 4) {
      const float4 v = *(const float4*)(src + pix * C + q * 4);
      acc += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  if (pix < npix && l4 == 0) e[pix] = acc;
}

// h[b,r,dx] = sum_{x<Wc} e[b,r,dx+x]
__global__ __launch_bounds__(256) void gc_row_sums(const double* __restrict__ e, double* __restrict__ h, size_t total, int A, int Nx, int Wc) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int dx = (int)(i % Nx);
  const size_t br = i / Nx;
  const double* p = e + br * A + dx;
  double s = 0.0;
  for (int x = 0; x < Wc; ++x) s += p[x];
  h[i] = s;
}

// part[b][split][dy][dx] = sum over the split's K columns and every r of the tile.  grid (nTx * nTy, nsplit, B)
__global__ __launch_bounds__(256) void gc_dot(const float* __restrict__ sat, const float* __restrict__ g2s, double* __restrict__ part,
                                              int A, int Hc, int Wc, int C, int Ny, int Nx, int nTx, int ncol, int nsplit) {
  __shared__ __attribute__((aligned(16))) float sm[GC_LDS_FLOATS];
  float* ring = sm;
  float* strip = sm + GC_RING_FLOATS;
  const int tx = blockIdx.x % nTx, ty = blockIdx.x / nTx, split = blockIdx.y, b = blockIdx.z;
  const int dx0 = tx * GC_T, dy0 = ty * GC_T;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i = lane & 31, kk = lane >> 5;
  const int r0 = gc_r_begin(dy0), r1 = gc_r_end(dy0, Ny, Hc);
  const float* sb = sat + (size_t)b * A * A * C;
  const float* gb = g2s + (size_t)b * Hc * Wc * C;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  gc_f32x16 acc;
  double sum[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) { acc[v] = 0.f; sum[v] = 0.0; }
  int steps = 0;
  // this thread's staging duty: one float4 of the strip (t < 188) or of the new crop row (t >= 192)
  const bool ld_strip = t < GC_STRIP_LOADERS, ld_ring = t >= GC_RING_LOADER0;
  const int scol = t >> 2, sq = t & 3, rxl = (t - GC_RING_LOADER0) >> 2, rq = t & 3;
  for (int col = gc_split_begin(split, ncol); col < gc_split_end(split, ncol); ++col) {
    const int x0 = gc_col_x0(col, Wc), c0 = gc_col_c0(col, Wc);
    __syncthreads();                                  // the previous column's last reads are done
    for (int e = t; e < GC_RING_FLOATS; e += 256) ring[e] = 0.f;        // rows y < 0 of the first steps are zero
    auto fetch = [&](int r) -> float4 {
      if (ld_strip) {
        const int x = x0 + dx0 + scol;
        return x < A ? *(const float4*)(sb + ((size_t)r * A + x) * C + c0 + sq * 4) : zero;
      }
      if (ld_ring) {
        const int y = r - dy0, x = x0 + rxl;
        return (y < Hc && x < Wc) ? *(const float4*)(gb + ((size_t)y * Wc + x) * C + c0 + rq * 4) : zero;
      }
      return zero;
    };
    float4 nxt = fetch(r0);
    for (int r = r0; r < r1; ++r) {
      __syncthreads();                                // the previous step's reads (and the zero fill) are done
      if (ld_strip) {
        float* p = strip + gc_strip_index(scol, sq * 4);
        p[0] = nxt.x; p[1] = nxt.y; p[2] = nxt.z; p[3] = nxt.w;
      } else if (ld_ring) {
        float* p = ring + gc_ring_index(r - dy0, rxl, rq * 4);
        p[0] = nxt.x; p[1] = nxt.y; p[2] = nxt.z; p[3] = nxt.w;
      }
      __syncthreads();
      if (r + 1 < r1) nxt = fetch(r + 1);             // in flight under the MFMAs
      const float* rrow = ring + gc_ring_slot(r - dy0 - i) * GC_RS;
#pragma unroll
      for (int u = 0; u < GC_XW; ++u) {
        const int xl = wave * GC_XW + u;
#pragma unroll
        for (int cp = 0; cp < GC_CC / 2; ++cp) {
          const int c = 2 * cp + kk;
          const float a = strip[gc_strip_index(xl + i, c)];      // A[dx = i][k]: s[r, x0 + xl + dx0 + i, c0 + c]
          const float w = rrow[xl * GC_CC + c];                  // B[k][dy = i]: g[r - dy0 - i, x0 + xl, c0 + c]
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w, acc, 0, 0, 0);
        }
      }
      if (++steps == GC_FLUSH_STEPS) {
#pragma unroll
        for (int v = 0; v < 16; ++v) { sum[v] += (double)acc[v]; acc[v] = 0.f; }
        steps = 0;
      }
    }
  }
#pragma unroll
  for (int v = 0; v < 16; ++v) sum[v] += (double)acc[v];
  __syncthreads();
  double* red = (double*)sm;                          // 4 waves x 1024 doubles = 32768 bytes, inside the ring's 32896
#pragma unroll
  for (int v = 0; v < 16; ++v) red[wave * 1024 + v * 64 + lane] = sum[v];
  __syncthreads();
  for (int e = t; e < 1024; e += 256) {
    const int v = e >> 6, ln = e & 63;
    const int dx = dx0 + gc_acc_dx(v, ln), dy = dy0 + gc_acc_dy(ln);
    if (dx < Nx && dy < Ny)
      part[gc_part_index(b, split, dy, dx, nsplit, Ny, Nx)] = ((red[e] + red[1024 + e]) + red[2048 + e]) + red[3072 + e];
  }
}

// fixed-order fp64 block sum of one value per thread (every thread gets the total)
__device__ __forceinline__ double gc_block_sum(double v, double* sh) {
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

// the closing launch of the forward.  grid (ceil(Ny Nx / 256), B); every block forms the sample's ||f|| in the same order
__global__ __launch_bounds__(256) void gc_close(const double* __restrict__ part, const double* __restrict__ h, const double* __restrict__ eg,
                                                const double* __restrict__ a_s, const double* __restrict__ a_g, double* __restrict__ dot,
                                                double* __restrict__ E, double* __restrict__ gnorm, float* __restrict__ corr, int A, int Hc,
                                                int Wc, int Ny, int Nx, int nsplit) {
  __shared__ double sh[256];
  const int b = blockIdx.y, t = threadIdx.x;
  const double as = a_s ? a_s[b] : 1.0, ag = a_g ? a_g[b] : 1.0;
  double g2 = 0.0;
  const size_t npg = (size_t)Hc * Wc;
  for (size_t p = t; p < npg; p += 256) g2 += eg[(size_t)b * npg + p];
  g2 = gc_block_sum(g2, sh);
  const double nf = ag * sqrt(g2), N = fmax(nf, 1e-12);
  if (blockIdx.x == 0 && t == 0) gnorm[b] = nf;
  const int s = blockIdx.x * 256 + t;
  if (s >= Ny * Nx) return;
  const int dy = s / Nx, dx = s % Nx;
  double d = 0.0, e = 0.0;
  for (int k = 0; k < nsplit; ++k) d += part[gc_part_index(b, k, dy, dx, nsplit, Ny, Nx)];
  for (int y = 0; y < Hc; ++y) e += h[((size_t)b * A + dy + y) * Nx + dx];
  d *= as * ag / N;
  e *= as * as;
  const size_t o = (size_t)b * Ny * Nx + s;
  dot[o] = d;
  E[o] = e;
  corr[o] = (float)(2.0 - 2.0 * d / fmax(sqrt(e), 1e-6));
}

// grid B: the per-sample scalars of the backward (orien_corr.hip: oc_bwd_prep, over the Ny x Nx plane).  With D = max(sqrt(E), 1e-6):
//   ddot = -2 d_corr / D,  beta = d_corr dot / D^3 where sqrt(E) > 1e-6, else 0;  kappa = sum ddot dot = g . d_g
//   d_f   = (a_s / N) sum ddot[dy,dx] S[y+dy, x+dx] - (a_g kappa / N^2) F        kf = ddot,                      alpha[0], coefA
//   d_sat = (a_g / N) sum ddot[dy,dx] F[r-dy, x-dx] + 2 a_s Bsum[r,x] S         kr = ddot reversed along dx,    alpha[1], coefB
__global__ __launch_bounds__(256) void gc_bwd_prep(const double* __restrict__ dot, const double* __restrict__ E, const double* __restrict__ gnorm,
                                                   const double* __restrict__ a_s, const double* __restrict__ a_g,
                                                   const float* __restrict__ d_corr, double* __restrict__ beta, double* __restrict__ kf,
                                                   double* __restrict__ kr, double* __restrict__ alpha, double* __restrict__ coefA, int B,
                                                   int Ny, int Nx) {
  __shared__ double sh[256];
  const int b = blockIdx.x, t = threadIdx.x, S = Ny * Nx;
  const double as = a_s ? a_s[b] : 1.0, ag = a_g ? a_g[b] : 1.0;
  const double nf = gnorm[b], N = fmax(nf, 1e-12);
  double kap = 0.0;
  for (int s = t; s < S; s += 256) {
    const size_t o = (size_t)b * S + s;
    const double e = E[o], sq = sqrt(e), D = fmax(sq, 1e-6), d = dot[o], gc = (double)d_corr[o];
    const double dd = -2.0 * gc / D;
    const int dy = s / Nx, dx = s % Nx;
    beta[o] = sq > 1e-6 ? gc * d / (D * D * D) : 0.0;
    kf[o] = dd;
    kr[(size_t)b * S + (size_t)dy * Nx + (Nx - 1 - dx)] = dd;
    kap += dd * d;
  }
  kap = gc_block_sum(kap, sh);
  if (t == 0) {
    alpha[b] = as / N;
    alpha[B + b] = ag / N;
    coefA[b] = nf >= 1e-12 ? -ag * kap / (N * N) : 0.0;      // (a clamped norm is a constant: no projection)
  }
}

// hb[b,dy,x] = sum of beta[b,dy,dx] over the dx whose window covers column x: max(0, x-Wc+1) <= dx <= min(Nx-1, x)
__global__ __launch_bounds__(256) void gc_beta_rows(const double* __restrict__ beta, double* __restrict__ hb, size_t total, int A, int Nx, int Wc) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % A);
  const size_t bdy = i / A;
  const int lo = max(0, x - Wc + 1), hi = min(Nx - 1, x);
  double s = 0.0;
  for (int dx = lo; dx <= hi; ++dx) s += beta[bdy * Nx + dx];
  hb[i] = s;
}

// coefB[b,r,x] = 2 a_s sum of hb[b,dy,x] over max(0, r-Hc+1) <= dy <= min(Ny-1, r)
__global__ __launch_bounds__(256) void gc_beta_cols(const double* __restrict__ hb, const double* __restrict__ a_s, double* __restrict__ coefB,
                                                    size_t total, int A, int Ny, int Hc) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % A), r = (int)((i / A) % A), b = (int)(i / ((size_t)A * A));
  const int lo = max(0, r - Hc + 1), hi = min(Ny - 1, r);
  double s = 0.0;
  for (int dy = lo; dy <= hi; ++dy) s += hb[((size_t)b * Ny + dy) * A + x];
  coefB[i] = 2.0 * (a_s ? a_s[b] : 1.0) * s;
}

// out[b,Y,x,c] = alpha[b] sum_{dy,s} kern[b,dy,s] src[b, Y + sgn dy, x + off + s, c] + coef[b,Y,x] self[b,Y,x,c]   (src zero outside)
// grid (nXT * C / CCH, outH, B); a thread owns 4 columns x 4 channels and walks the shifts of a row in tiles of 64 through an LDS
// strip, row after row.  fp64 sums: the triplet loss's cotangent sums to zero over the shifts, so an output is what is left of
// Ny Nx cancelling terms.  One template serves both directions: sgn = +1, off = 0 for d_g;  sgn = -1, off = -(Nx-1) and the
// dx-reversed plane for d_sat.
template <int NC4>
__global__ __launch_bounds__(256) void gc_corr2d(const float* __restrict__ src, int srcH, int srcW, const float* __restrict__ self,
                                                 float* __restrict__ out, int outH, int outW, const double* __restrict__ kern,
                                                 const double* __restrict__ alpha, const double* __restrict__ coef, size_t coef_sb,
                                                 int coef_sy, int coef_sx, int C, int Ny, int Nx, int sgn, int off, int nXT) {
  constexpr int NWG = 256 / NC4, TW = 4 * NWG, TS = 64, PC = TW + TS - 1, CCH = NC4 * 4, CS = CCH + 4;
  __shared__ float sS[PC * CS];
  __shared__ double sK[TS];
  const int xt = blockIdx.x % nXT, c0 = (blockIdx.x / nXT) * CCH, Y = blockIdx.y, b = blockIdx.z;
  const int x0 = xt * TW, t = threadIdx.x, c4 = t % NC4, wg = t / NC4;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  double acc[4][4] = {};
  for (int dy = 0; dy < Ny; ++dy) {
    const int yr = Y + sgn * dy;
    if (yr < 0 || yr >= srcH) continue;
    const float* srow = src + ((size_t)b * srcH + yr) * (size_t)srcW * C + c0;
    const double* krow = kern + ((size_t)b * Ny + dy) * Nx;
    for (int s0 = 0; s0 < Nx; s0 += TS) {
      const int xlo = x0 + off + s0;
      if (xlo + PC <= 0 || xlo >= srcW) continue;     // the whole strip lies off the source row
      __syncthreads();
      for (int e = t; e < PC * NC4; e += 256) {
        const int col = e / NC4, q = e % NC4, xs = xlo + col;
        *(float4*)(sS + col * CS + q * 4) = (xs >= 0 && xs < srcW) ? *(const float4*)(srow + (size_t)xs * C + q * 4) : zero;
      }
      if (t < TS) sK[t] = s0 + t < Nx ? krow[s0 + t] : 0.0;
      __syncthreads();
#pragma unroll
      for (int k = 0; k < TS + 3; ++k) {
        const float4 vf = *(const float4*)(sS + (4 * wg + k) * CS + c4 * 4);
        const double v[4] = {(double)vf.x, (double)vf.y, (double)vf.z, (double)vf.w};
#pragma unroll
        for (int xi = 0; xi < 4; ++xi) {
          const int sl = k - xi;
          if (sl >= 0 && sl < TS) {
            const double kv = sK[sl];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[xi][c] += kv * v[c];
          }
        }
      }
    }
  }
  const double al = alpha[b];
#pragma unroll
  for (int xi = 0; xi < 4; ++xi) {
    const int x = x0 + 4 * wg + xi;
    if (x < outW) {
      const size_t idx = (((size_t)b * outH + Y) * (size_t)outW + x) * C + c0 + c4 * 4;
      const float4 sv = *(const float4*)(self + idx);
      const double cf = coef[(size_t)b * coef_sb + (size_t)Y * coef_sy + (size_t)x * coef_sx];
      float4 o;
      o.x = (float)(al * acc[xi][0] + cf * sv.x); o.y = (float)(al * acc[xi][1] + cf * sv.y);
      o.z = (float)(al * acc[xi][2] + cf * sv.z); o.w = (float)(al * acc[xi][3] + cf * sv.w);
      *(float4*)(out + idx) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// triplet_loss (models_kitti.py:579-595), one level: sum_{b,dy,dx} log(1 + exp(10 (corr[b,h_b,w_b] - corr[b,dy,dx]))) / (B (Ny Nx - 1)),
//   w_b = round(Nx/2 + gt_shift_u[b] shift_range_lon / mpp),  h_b = round(Ny/2 - gt_shift_v[b] shift_range_lat / mpp)
// in fp32 like the reference's tensors, half to even, Nx/2 a true division; a negative index counts from the end like a Python index;
// one outside [-N,N) -- the reference raises -- gives NaN.  Returns the flat index h Nx + w, or -1.
__device__ __forceinline__ int gc_wrap(float fi, int N) {
  if (!(fi >= -(float)N && fi < (float)N)) return -1;
  const int i = (int)fi;
  return i < 0 ? i + N : i;
}
__device__ __forceinline__ int gc_gt_index(const float* gu, long long us, const float* gv, long long vs, int b, float lat, float lon,
                                           float mpp, int Ny, int Nx) {
  const int w = gc_wrap(rintf((float)Nx / 2.f + gu[(long long)b * us] * lon / mpp), Nx);
  const int h = gc_wrap(rintf((float)Ny / 2.f - gv[(long long)b * vs] * lat / mpp), Ny);
  return (w < 0 || h < 0) ? -1 : h * Nx + w;
}

__global__ __launch_bounds__(256) void gc_triplet(const float* __restrict__ corr, const float* __restrict__ gu, long long us,
                                                  const float* __restrict__ gv, long long vs, float lat, float lon, float mpp,
                                                  float* __restrict__ loss, int accumulate, int B, int Ny, int Nx) {
  __shared__ double sh[256];
  const int t = threadIdx.x, S = Ny * Nx;
  double acc = 0.0;
  bool bad = false;
  for (int b = 0; b < B; ++b) {
    const int gi = gc_gt_index(gu, us, gv, vs, b, lat, lon, mpp, Ny, Nx);
    if (gi < 0) { bad = true; continue; }
    const float pos = corr[(size_t)b * S + gi];
    for (int s = t; s < S; s += 256) acc += (double)log1pf(expf((pos - corr[(size_t)b * S + s]) * 10.f));
  }
  acc = gc_block_sum(acc, sh);
  if (t == 0) {
    const float v = bad ? __builtin_nanf("") : (float)acc / (float)((long long)B * (S - 1));
    loss[0] = accumulate ? loss[0] + v : v;
  }
}

// d_corr[b,s] = g/(B(S-1)) * 10 * ( [s == gt_b] sum_s' sig(z_s') - sig(z_s) ),  z_s = 10 (pos - corr[b,s]).   grid B
__global__ __launch_bounds__(256) void gc_triplet_bwd(const float* __restrict__ corr, const float* __restrict__ gu, long long us,
                                                      const float* __restrict__ gv, long long vs, float lat, float lon, float mpp,
                                                      const float* __restrict__ g_loss, float* __restrict__ d_corr, int B, int Ny, int Nx) {
  __shared__ double sh[256];
  const int b = blockIdx.x, t = threadIdx.x, S = Ny * Nx;
  const int gi = gc_gt_index(gu, us, gv, vs, b, lat, lon, mpp, Ny, Nx);
  const float sc = g_loss[0] * 10.f / (float)((long long)B * (S - 1));
  const float pos = gi >= 0 ? corr[(size_t)b * S + gi] : __builtin_nanf("");
  double tot = 0.0;
  for (int s = t; s < S; s += 256) {
    const float z = (pos - corr[(size_t)b * S + s]) * 10.f;
    const float sg = 1.f / (1.f + expf(-z));
    tot += (double)sg;
    d_corr[(size_t)b * S + s] = -sc * sg;
  }
  tot = gc_block_sum(tot, sh);          // (its barriers order the stores above before the update of the gt entry)
  if (t == 0 && gi >= 0) d_corr[(size_t)b * S + gi] += sc * (float)tot;
}

// ---------------------------------------------------------------------------------------------
static int gc_check(const char* who, int B, int A, int Hc, int Wc, int C) {
  HLA_REQUIRE(B > 0 && B <= 65535 && A > 0 && A <= 16384, "%s: need 0 < B <= 65535 and 0 < A <= 16384", who);
  HLA_REQUIRE(Hc >= 1 && Hc <= A && Wc >= 1 && Wc <= A, "%s: the crop %d x %d must lie inside the %d x %d map", who, Hc, Wc, A, A);
  HLA_REQUIRE(C == 16 || C == 64 || C == 128 || C == 256, "%s: unsupported channel count %d (16, 64, 128, 256)", who, C);
  const long long Ny = A - Hc + 1, Nx = A - Wc + 1;
  HLA_REQUIRE((long long)gc_tiles((int)Ny) * gc_tiles((int)Nx) < (1LL << 31) && (Ny * Nx + 255) / 256 < (1LL << 31),
              "%s: too many shifts for one launch", who);
  HLA_REQUIRE(((long long)B * A * A * 4 + 255) / 256 < (1LL << 31), "%s: B A A overflows a launch", who);
  return HLA_OK;
}

extern "C" size_t hla_g2s_corr_workspace_bytes(int B, int A, int Hc, int Wc, int C) {
  if (gc_check("hla_g2s_corr_workspace_bytes", B, A, Hc, Wc, C)) return 0;
  return gc_layout(B, A, Hc, Wc, C).total;
}

static inline unsigned gc_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

extern "C" int hla_g2s_corr(const float* sat, const float* g2s, const double* sat_inv_norm, const double* g2s_inv_norm, double* dot,
                            double* E, double* gnorm, float* corr, void* workspace, size_t workspace_bytes, int B, int A, int Hc,
                            int Wc, int C, hla_stream_t stream) {
  const int rc = gc_check("hla_g2s_corr", B, A, Hc, Wc, C);
  if (rc) return rc;
  HLA_REQUIRE(sat && g2s && dot && E && gnorm && corr && workspace, "hla_g2s_corr: null argument");
  const GcLayout L = gc_layout(B, A, Hc, Wc, C);
  if (workspace_bytes < L.total) {
    hla_set_error("hla_g2s_corr: workspace of %zu bytes, need %zu", workspace_bytes, L.total);
    return HLA_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double *e = (double*)(ws + L.e), *eg = (double*)(ws + L.eg), *h = (double*)(ws + L.h), *part = (double*)(ws + L.part);
  const int Ny = L.Ny, Nx = L.Nx, nTx = gc_tiles(Nx), nTy = gc_tiles(Ny);
  const size_t npix = (size_t)B * A * A, npg = (size_t)B * Hc * Wc, nh = (size_t)B * A * Nx;
  hipLaunchKernelGGL(gc_energy, dim3(gc_blocks(npix * 4)), dim3(256), 0, st, sat, e, npix, C);
  hipLaunchKernelGGL(gc_energy, dim3(gc_blocks(npg * 4)), dim3(256), 0, st, g2s, eg, npg, C);
  hipLaunchKernelGGL(gc_row_sums, dim3(gc_blocks(nh)), dim3(256), 0, st, (const double*)e, h, nh, A, Nx, Wc);
  // executed FLOPs: every tile walks whole 32 x 32 blocks of shifts
  double steps = 0.0;
  for (int ty = 0; ty < nTy; ++ty) steps += gc_r_end(ty * GC_T, Ny, Hc) - gc_r_begin(ty * GC_T);
  hla_prof_begin(K_G2SCORR, 2.0 * GC_T * GC_T * GC_XC * GC_CC * steps * nTx * L.ncol * B,
                 4.0 * ((double)npix + (double)npg) * C, st);
  hipLaunchKernelGGL(gc_dot, dim3(nTx * nTy, L.nsplit, B), dim3(256), 0, st, sat, g2s, part, A, Hc, Wc, C, Ny, Nx, nTx, L.ncol, L.nsplit);
  hla_prof_end(st);
  hipLaunchKernelGGL(gc_close, dim3(gc_blocks((size_t)Ny * Nx), B), dim3(256), 0, st, (const double*)part, (const double*)h,
                     (const double*)eg, sat_inv_norm, g2s_inv_norm, dot, E, gnorm, corr, A, Hc, Wc, Ny, Nx, L.nsplit);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

template <int NC4>
static void gc_launch_corr2d(hipStream_t st, const float* src, int srcH, int srcW, const float* self, float* out, int outH, int outW,
                             const double* kern, const double* alpha, const double* coef, size_t coef_sb, int coef_sy, int coef_sx,
                             int B, int C, int Ny, int Nx, int sgn, int off) {
  constexpr int TW = 4 * (256 / NC4), CCH = NC4 * 4;
  const int nXT = (outW + TW - 1) / TW;
  hipLaunchKernelGGL((gc_corr2d<NC4>), dim3(nXT * (C / CCH), outH, B), dim3(256), 0, st, src, srcH, srcW, self, out, outH, outW, kern,
                     alpha, coef, coef_sb, coef_sy, coef_sx, C, Ny, Nx, sgn, off, nXT);
}

extern "C" int hla_g2s_corr_bwd(const float* sat, const float* g2s, const double* sat_inv_norm, const double* g2s_inv_norm,
                                const double* dot, const double* E, const double* gnorm, const float* d_corr, float* d_sat,
                                float* d_g2s, void* workspace, size_t workspace_bytes, int B, int A, int Hc, int Wc, int C,
                                hla_stream_t stream) {
  const int rc = gc_check("hla_g2s_corr_bwd", B, A, Hc, Wc, C);
  if (rc) return rc;
  HLA_REQUIRE(sat && g2s && dot && E && gnorm && d_corr && d_sat && d_g2s && workspace, "hla_g2s_corr_bwd: null argument");
  const GcLayout L = gc_layout(B, A, Hc, Wc, C);
  if (workspace_bytes < L.total) {
    hla_set_error("hla_g2s_corr_bwd: workspace of %zu bytes, need %zu", workspace_bytes, L.total);
    return HLA_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double *kf = (double*)(ws + L.kf), *kr = (double*)(ws + L.kr), *beta = (double*)(ws + L.beta), *hb = (double*)(ws + L.hb),
         *coefB = (double*)(ws + L.coefB), *alpha = (double*)(ws + L.alpha), *coefA = (double*)(ws + L.coefA);
  const int Ny = L.Ny, Nx = L.Nx;
  const size_t nhb = (size_t)B * Ny * A, nsat = (size_t)B * A * A;
  hipLaunchKernelGGL(gc_bwd_prep, dim3(B), dim3(256), 0, st, dot, E, gnorm, sat_inv_norm, g2s_inv_norm, d_corr, beta, kf, kr, alpha, coefA,
                     B, Ny, Nx);
  hipLaunchKernelGGL(gc_beta_rows, dim3(gc_blocks(nhb)), dim3(256), 0, st, (const double*)beta, hb, nhb, A, Nx, Wc);
  hipLaunchKernelGGL(gc_beta_cols, dim3(gc_blocks(nsat)), dim3(256), 0, st, (const double*)hb, sat_inv_norm, coefB, nsat, A, Ny, Hc);
  const double flops = 2.0 * 2.0 * (double)B * Hc * Wc * C * Ny * Nx;        // algorithmic: both gradients
  hla_prof_begin(K_G2SCORR_BWD, flops, 8.0 * ((double)nsat + (double)B * Hc * Wc) * C, st);
  if (C == 16) {
    gc_launch_corr2d<4>(st, sat, A, A, g2s, d_g2s, Hc, Wc, kf, alpha, coefA, 1, 0, 0, B, C, Ny, Nx, 1, 0);
    gc_launch_corr2d<4>(st, g2s, Hc, Wc, sat, d_sat, A, A, kr, alpha + B, coefB, (size_t)A * A, A, 1, B, C, Ny, Nx, -1, -(Nx - 1));
  } else {
    gc_launch_corr2d<16>(st, sat, A, A, g2s, d_g2s, Hc, Wc, kf, alpha, coefA, 1, 0, 0, B, C, Ny, Nx, 1, 0);
    gc_launch_corr2d<16>(st, g2s, Hc, Wc, sat, d_sat, A, A, kr, alpha + B, coefB, (size_t)A * A, A, 1, B, C, Ny, Nx, -1, -(Nx - 1));
  }
  hla_prof_end(st);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

static int gc_triplet_check(const char* who, const float* corr, const float* gu, const float* gv, double mpp, int B, int Ny, int Nx) {
  HLA_REQUIRE(corr && gu && gv, "%s: null argument", who);
  HLA_REQUIRE(B > 0 && Ny > 0 && Nx > 0 && (long long)Ny * Nx < (1LL << 31) && mpp > 0.0, "%s: need B, Ny, Nx > 0, Ny Nx < 2^31 and meters_per_pixel > 0", who);
  return HLA_OK;
}

extern "C" int hla_g2s_corr_triplet_loss(const float* corr, const float* gt_shift_u, long long gt_u_stride, const float* gt_shift_v,
                                         long long gt_v_stride, double shift_range_lat, double shift_range_lon, double meters_per_pixel,
                                         float* loss, int accumulate, int B, int Ny, int Nx, hla_stream_t stream) {
  const int rc = gc_triplet_check("hla_g2s_corr_triplet_loss", corr, gt_shift_u, gt_shift_v, meters_per_pixel, B, Ny, Nx);
  if (rc) return rc;
  HLA_REQUIRE(loss, "hla_g2s_corr_triplet_loss: null output");
  hipLaunchKernelGGL(gc_triplet, dim3(1), dim3(256), 0, (hipStream_t)stream, corr, gt_shift_u, gt_u_stride, gt_shift_v, gt_v_stride,
                     (float)shift_range_lat, (float)shift_range_lon, (float)meters_per_pixel, loss, accumulate, B, Ny, Nx);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

extern "C" int hla_g2s_corr_triplet_loss_bwd(const float* corr, const float* gt_shift_u, long long gt_u_stride, const float* gt_shift_v,
                                             long long gt_v_stride, double shift_range_lat, double shift_range_lon,
                                             double meters_per_pixel, const float* g_loss, float* d_corr, int B, int Ny, int Nx,
                                             hla_stream_t stream) {
  const int rc = gc_triplet_check("hla_g2s_corr_triplet_loss_bwd", corr, gt_shift_u, gt_shift_v, meters_per_pixel, B, Ny, Nx);
  if (rc) return rc;
  HLA_REQUIRE(g_loss && d_corr, "hla_g2s_corr_triplet_loss_bwd: null argument");
  HLA_REQUIRE(B <= 65535 * 32768, "hla_g2s_corr_triplet_loss_bwd: B overflows a launch");
  hipLaunchKernelGGL(gc_triplet_bwd, dim3(B), dim3(256), 0, (hipStream_t)stream, corr, gt_shift_u, gt_u_stride, gt_shift_v, gt_v_stride,
                     (float)shift_range_lat, (float)shift_range_lon, (float)meters_per_pixel, g_loss, d_corr, B, Ny, Nx);
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}
