// Backward of the VGG16-U-Net extractor (what autograd does in the reference through VGG.py:121-203):
//   * L2_norm backward (VGG.py:511-514)
//   * data gradients: every conv's dgrad is the SAME MFMA implicit-GEMM kernel as the forward pass, run on
//     transposed + tap-flipped packed weights, with the ReLU mask / gradient fan-in / "sum 2x2" (nearest-upsample
//     backward) fused into its epilogue and the max-pool routing (argmax) fused into its loader
//   * weight gradients: MFMA GEMMs that contract over PIXELS (the kernels: wgrad_kernels.h; planned and launched here)
#include <vector>
#include <stdlib.h>
#include "wgrad_kernels.h"
#include "vgg_layers.h"

// per-sample max |x| of an fp32 map (fp32 bit pattern, atomicMax into a zeroed word): the scale of a gradient map that no
// convolution epilogue produced (the L2-norm backward's outputs, with the confidence heads' contribution added)
static __global__ __launch_bounds__(256) void absmax_map_kernel(const float* __restrict__ x, size_t per_sample, size_t skip, int nblk,
                                                                unsigned* __restrict__ amax) {
  const int b = blockIdx.x / nblk, k = blockIdx.x % nblk;
  const float4* p = (const float4*)(x + (size_t)b * per_sample);
  float m = 0.f;
  for (size_t i = skip / 4 + (size_t)k * 256 + threadIdx.x; i < per_sample / 4; i += (size_t)nblk * 256) {
    const float4 v = p[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  m = wave_max_f32(m);
  if ((threadIdx.x & 63) == 0 && __float_as_uint(m) > __hip_atomic_load(amax + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(amax + b, __float_as_uint(m));
}

// out[i] = sum_k part[k][i]  (fixed order: deterministic).  Generic 2-D gather: element i = (row, col) with col < out_inner,
// input row pitch in_inner (conv0: 32 -> 27).  16 columns x 16 k-lanes per block: the bias / conv0 / conf-head reductions
// have few columns and up to 2048 partial rows, so the parallelism has to come from k (a single thread walking all of
// K costs one load latency per row: 0.5 ms for K = 512).  Launch with (n + 15) / 16 blocks.
static __global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                              size_t n, int K, int in_stride_inner, int out_inner, int in_inner) {
  __shared__ float sh[16][17];
  const int col = threadIdx.x & 15, kl = threadIdx.x >> 4;
  const size_t i = (size_t)blockIdx.x * 16 + col;
  float s = 0.f;
  if (i < n) {
    const size_t src = (i / out_inner) * in_inner + i % out_inner;
#pragma unroll 8
    for (int k = kl; k < K; k += 16) s += part[(size_t)k * in_stride_inner + src];
  }
  sh[kl][col] = s;
  __syncthreads();
  if (kl == 0 && i < n) {
#pragma unroll
    for (int k = 1; k < 16; ++k) s += sh[k][col];
    out[i] = s;
  }
}

// contiguous case, n % 4 == 0: 32 float4 columns x 8 k-lanes per block; each k-lane sums its rows in order, the 8 lane
// sums are then added in order (deterministic), with 8x more loads in flight than the generic kernel
static __global__ __launch_bounds__(256) void reduce_partials4_kernel(const float4* __restrict__ part, float4* __restrict__ out,
                                                                      size_t n4, int K) {
  __shared__ float4 sh[8][32];
  const int col = threadIdx.x & 31, kl = threadIdx.x >> 5;
  const size_t i = (size_t)blockIdx.x * 32 + col;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n4) {
#pragma unroll 4
    for (int k = kl; k < K; k += 8) {
      const float4 v = part[(size_t)k * n4 + i];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  sh[kl][col] = s;
  __syncthreads();
  if (kl == 0 && i < n4) {
#pragma unroll
    for (int k = 1; k < 8; ++k) { const float4 v = sh[k][col]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    out[i] = s;
  }
}

// first level of a two-level fixed-order reduction over MANY partial rows (the fused conv0 weight gradient: one [64][32] row per
// data-gradient workgroup, up to 32768 of them): slab s = blockIdx.x sums rows s, s + gridDim.x, ... in that order into out2[s].
// K on the device for a data-dependent launch: n_live (the first int of its ConvDyn) x B workgroups wrote a row.
static __global__ __launch_bounds__(256) void reduce_rows_kernel(const float4* __restrict__ part, float4* __restrict__ out2, int n4, int K,
                                                                 const int* __restrict__ dyn_nlive, int B) {
  const int Kd = dyn_nlive ? *dyn_nlive * B : K, s = blockIdx.x, ns = gridDim.x;
  for (int c = threadIdx.x; c < n4; c += 256) {
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int k = s; k < Kd; k += ns) {
      const float4 v = part[(size_t)k * n4 + c];
      sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
    }
    out2[(size_t)s * n4 + c] = sum;
  }
}

// ---------------------------------------------------------------------------------------------
// L2_norm backward: y = a*x with a = 1/||x||  =>  dx = a*dy - a^3 * (x . dy) * x      (per sample)
static __global__ __launch_bounds__(256) void l2bwd_dot_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        double* __restrict__ part, size_t per_sample, int nblk) {
  __shared__ double sh[4];
  const int b = blockIdx.x / nblk, k = blockIdx.x % nblk;
  const float4* px = (const float4*)(x + (size_t)b * per_sample);
  const float4* pd = (const float4*)(dy + (size_t)b * per_sample);
  float s = 0.f;
  double sd = 0.0;
  int cnt = 0;
  for (size_t i = (size_t)k * 256 + threadIdx.x; i < per_sample / 4; i += (size_t)nblk * 256) {
    const float4 u = px[i], v = pd[i];
    s += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
    if (++cnt == 64) { sd += (double)s; s = 0.f; cnt = 0; }
  }
  sd += (double)s;
  sd = wave_sum_f64(sd);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sd;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)b * nblk + k] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// `rowiv` (optional, ORTHO only): per map row the column interval of the pixels where dy is not exactly zero, over the whole
// batch, kept as atomicMax targets {-lo, hi} (memset to 0x80 bytes = "nothing yet") -- the seed of the data-dependent trimming.
template <typename T, bool ORTHO>
__global__ __launch_bounds__(256) void l2bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          const double* __restrict__ part, const double* __restrict__ inv,
                                                          T* __restrict__ out, size_t per_sample, int nblk,
                                                          int* __restrict__ rowiv = nullptr, int C = 1, int Wl = 1,
                                                          size_t skip = 0,        // floats at the start of a sample that are neither
                                                                                 // read nor written (the caller's static first rows)
                                                          unsigned* __restrict__ amax = nullptr) {   // split mode: [B] atomicMax target
                                                                                 // for max |out| per sample (the scale the map's consumer
                                                                                 // uses), instead of a separate pass over the map
  const int b = blockIdx.x / nblk, k = blockIdx.x % nblk;
  float mx = 0.f;
  double dot = 0.0;
  if (!ORTHO)
    for (int i = 0; i < nblk; ++i) dot += part[(size_t)b * nblk + i];
  const double al = inv[b];
  const float c1 = (float)al, c3 = (float)(al * al * al * dot);
  const float4* px = (const float4*)(x + (size_t)b * per_sample);
  const float4* pd = (const float4*)(dy + (size_t)b * per_sample);
  T* po = out + (size_t)b * per_sample;
  if (ORTHO && rowiv) {
    // Row tracking: the block takes a CONTIGUOUS slice of the sample (a few map rows), collects their intervals in LDS and
    // touches the global counters once per row at the end.  (History: one filter read + atomic per non-zero vector made the
    // counters an L2 hot spot -- 0.18 -> 2.6 ms for the three maps; one per wave and iteration still cost +0.45 ms.)
    constexpr int MAXR = 64;
    __shared__ int siv[2 * MAXR];
    const size_t n4 = per_sample / 4, c = (n4 + nblk - 1) / nblk, start = (size_t)k * c, end = start + c < n4 ? start + c : n4;
    const int r0 = (int)(start * 4 / (unsigned)C) / Wl, r1 = end > start ? (int)((end * 4 - 1) / (unsigned)C) / Wl : r0;
    const bool local = r1 - r0 < MAXR;                                    // block-uniform
    for (int e = threadIdx.x; e < 2 * MAXR; e += 256) siv[e] = INT_MIN;
    __syncthreads();
    for (size_t i = start + threadIdx.x; i < end; i += 256) {
      const float4 v = pd[i];
      store4(po + i * 4, c1 * v.x, c1 * v.y, c1 * v.z, c1 * v.w);
      mx = fmaxf(fmaxf(mx, fmaxf(fabsf(c1 * v.x), fabsf(c1 * v.y))), fmaxf(fabsf(c1 * v.z), fabsf(c1 * v.w)));
      const bool nz = v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f;
      const unsigned long long m = __ballot(nz);
      if (m) {
        // a wave's 64 vectors are consecutive in memory (1-4 pixels), so they almost always lie in ONE row: reduce the columns
        // across the wave and let one lane update that row
        const int pix = (int)(i * 4 / (unsigned)C), py = pix / Wl, pxx = pix - py * Wl;
        const int first = __ffsll((long long)m) - 1;
        const int py0 = __shfl(py, first, 64);
        int nlo = nz ? -pxx : INT_MIN, hi = nz ? pxx + 1 : INT_MIN, row = py;
        if (__ballot(nz && py != py0) == 0) {
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) { nlo = max(nlo, __shfl_xor(nlo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
          if ((int)(threadIdx.x & 63) != first) nlo = hi = INT_MIN;
          row = py0;
        }
        if (nlo != INT_MIN) {
          if (local) { atomicMax(&siv[2 * (row - r0)], nlo); atomicMax(&siv[2 * (row - r0) + 1], hi); }
          else { atomicMax(rowiv + 2 * row, nlo); atomicMax(rowiv + 2 * row + 1, hi); }
        }
      }
    }
    __syncthreads();
    if (local && (int)threadIdx.x <= r1 - r0 && siv[2 * threadIdx.x + 1] != INT_MIN) {
      int* r = rowiv + 2 * (r0 + threadIdx.x);
      // (the plain reads only filter: a stale value costs one redundant atomic, never a missed one)
      if (siv[2 * threadIdx.x] > __hip_atomic_load(r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(r, siv[2 * threadIdx.x]);
      if (siv[2 * threadIdx.x + 1] > __hip_atomic_load(r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(r + 1, siv[2 * threadIdx.x + 1]);
    }
    if (amax) {
      mx = wave_max_f32(mx);
      if ((threadIdx.x & 63) == 0 && mx > 0.f && __float_as_uint(mx) > __hip_atomic_load(amax + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(amax + b, __float_as_uint(mx));      // (the plain read only filters)
    }
    return;
  }
  for (size_t i = skip / 4 + (size_t)k * 256 + threadIdx.x; i < per_sample / 4; i += (size_t)nblk * 256) {
    const float4 v = pd[i];
    if (ORTHO) {       // HLA_VGG_BWD_SCALE_INVARIANT: x . dy = 0 analytically, dx = dy / ||x||; x is not read
      store4(po + i * 4, c1 * v.x, c1 * v.y, c1 * v.z, c1 * v.w);
      mx = fmaxf(fmaxf(mx, fmaxf(fabsf(c1 * v.x), fabsf(c1 * v.y))), fmaxf(fabsf(c1 * v.z), fabsf(c1 * v.w)));
    } else {
      const float4 u = px[i];
      store4(po + i * 4, c1 * v.x - c3 * u.x, c1 * v.y - c3 * u.y, c1 * v.z - c3 * u.z, c1 * v.w - c3 * u.w);
    }
  }
  if (ORTHO && amax) {
    mx = wave_max_f32(mx);
    if ((threadIdx.x & 63) == 0 && mx > 0.f && __float_as_uint(mx) > __hip_atomic_load(amax + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(amax + b, __float_as_uint(mx));
  }
}

// level 4: gradient w.r.t. the conv2 output = unpool(gradient of the pooled map, forward argmax) + gradient arriving through
// the conv_dec3 skip connection (already ReLU-masked).  One pass at full resolution, 16 B per thread.
template <typename T>
__global__ __launch_bounds__(256) void unpool_add_kernel(const T* __restrict__ gp, const unsigned char* __restrict__ idx,
                                                         const T* __restrict__ skip, T* __restrict__ out, int B, int H, int W) {
  constexpr int EPL = 16 / sizeof(T), C = 64, PPX = C / EPL;
  const size_t n = (size_t)B * H * W * PPX;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int part = (int)(i % PPX);
    const size_t pix = i / PPX;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const size_t b = pix / ((size_t)W * H);
    const size_t e0 = ((b * (H / 2) + (y >> 1)) * (W / 2) + (x >> 1)) * C + part * EPL;
    const unsigned pos = ((y & 1) << 1) | (x & 1);
    uint4 g = *(const uint4*)(gp + e0), sk = *(const uint4*)(skip + pix * C + part * EPL);
    T ge[EPL], se[EPL];
    unsigned char id[EPL];
    __builtin_memcpy(ge, &g, 16); __builtin_memcpy(se, &sk, 16); __builtin_memcpy(id, idx + e0, EPL);
#pragma unroll
    for (int k = 0; k < EPL; ++k) ge[k] = (T)((id[k] == pos ? to_f32(ge[k]) : 0.f) + to_f32(se[k]));
    __builtin_memcpy(&g, ge, 16);
    *(uint4*)(out + pix * C + part * EPL) = g;
  }
}

// ---------------------------------------------------------------------------------------------
// Confidence head backward (VGG.py:62-76,160-162):  conf = sigmoid(-s),  s = sigmoid(z),  z = conv3x3(relu(x), w)
//   dz = -d_conf * conf*(1-conf) * s*(1-s)   with s recovered from conf:  e^s = (1-conf)/conf
static __global__ __launch_bounds__(256) void conf_dz_kernel(const float* __restrict__ conf, const float* __restrict__ d_conf,
                                                      float* __restrict__ dz, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float c = conf[i];
    const float s = logf((1.f - c) / c);
    dz[i] = -d_conf[i] * c * (1.f - c) * s * (1.f - s);
  }
}

// One pass over relu(x) [B,H,W,C]:  gx[q,c] += (x>0) * sum_tap w[c,tap]*dz[q-off(tap)]   (data gradient, added into the
// gradient of the raw map) and per-block partial sums of  dw[c,tap] = sum_q relu(x)[q,c]*dz[q-off(tap)].
// G = C/EPL lanes share a pixel; the 256/G pixel slots of a block are folded with shuffles + LDS at the end.
template <typename T>
__global__ __launch_bounds__(256) void conf_bwd_kernel(const T* __restrict__ act, const float* __restrict__ w,
                                                       const float* __restrict__ dz, T* __restrict__ gx,
                                                       float* __restrict__ part, int B, int H, int W, int C) {
  constexpr int EPL = 16 / sizeof(T);
  extern __shared__ float sh[];   // [4][9*C]
  const int G = C / EPL, ppb = 256 / G, gi = threadIdx.x % G;
  float wr[9][EPL], acc[9][EPL];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int k = 0; k < EPL; ++k) { wr[t][k] = w[(gi * EPL + k) * 9 + t]; acc[t][k] = 0.f; }
  const size_t npix = (size_t)B * H * W;
  for (size_t pix = (size_t)blockIdx.x * ppb + threadIdx.x / G; pix < npix; pix += (size_t)gridDim.x * ppb) {
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    float dzm[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int yy = y - (t / 3 - 1), xx = x - (t % 3 - 1);
      dzm[t] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? dz[(long)pix - ((long)(t / 3 - 1) * W + (t % 3 - 1))] : 0.f;
    }
    const uint4 raw = *(const uint4*)(act + pix * C + gi * EPL);
    uint4 graw = *(const uint4*)(gx + pix * C + gi * EPL);
    T a[EPL], g[EPL];
    __builtin_memcpy(a, &raw, 16);
    __builtin_memcpy(g, &graw, 16);
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const float av = to_f32(a[k]);
      float d = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) { acc[t][k] += av * dzm[t]; d += wr[t][k] * dzm[t]; }
      g[k] = (T)(to_f32(g[k]) + (av > 0.f ? d : 0.f));
    }
    __builtin_memcpy(&graw, g, 16);
    *(uint4*)(gx + pix * C + gi * EPL) = graw;
  }
  // fold the pixel slots: lanes with equal gi inside a wave, then the 4 waves
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      float v = acc[t][k];
      for (int o = G; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
      acc[t][k] = v;
    }
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  if (G >= 64 ? true : ln < G) {
    // G == 64 (fp32, C = 256): every lane of the wave owns distinct channels
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int k = 0; k < EPL; ++k) sh[wv * 9 * C + ((ln % G) * EPL + k) * 9 + t] = acc[t][k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 9 * C; e += 256)
    part[(size_t)blockIdx.x * 9 * C + e] = (sh[e] + sh[9 * C + e]) + (sh[2 * 9 * C + e] + sh[3 * 9 * C + e]);
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// Data-dependent trimming.  The satellite branch's incoming gradient is what the LM loop's bilinear taps scattered: for KITTI
// geometry ~10 % of the texels, inside the fan the camera sees (apex at the map centre, opening towards +u).  l2bwd_apply
// records, per ROW of each returned map, the column interval of its non-zero gradient (over the batch); bwd_fan_kernel pushes
// the three interval sets through the layer graph exactly -- a 3x3 conv: union of the three neighbouring rows, one pixel wider;
// the 2x upsample's sum-pool: rows pairwise, halved; an unpool: doubled; a fan-in: union -- and derives, for every gradient map,
// the part its producer WRITES: per band of 8 rows one column interval rounded out to the 32-px tiles (DYN_BANDS).  From those
// it builds the list of live tiles of every data- and weight-gradient launch.  A launch visits only its live tiles and reads a
// source as zero outside the part its producer wrote.  Nothing is promised by the caller and nothing is approximated: outside
// its support a gradient is exactly zero, so no value changes (only the weight-gradient summation order).
// (the maps M_*, the launches DC_* / DW_* and what each reads and writes: vgg_graph.h)
// What bwd_fan_kernel needs to list the live tiles of one launch: the launch's resolution divisor and tile height, sh = 1 where it
// runs at twice the resolution of the map whose bands bound it (a pool_sum data gradient, a weight gradient through an unpool),
// and its descriptor's words 2 and 3 (band offsets of the maps it reads, -1: dense)
struct FanJob { int div, th, sh, bands, list, desc, d2, d3; };
struct DynLayout {
  int seed[3];              // per-row {-lo, hi} atomicMax targets of d_feat[l] (memset to 0x80 bytes = "nothing yet")
  int seed_ints;
  int bands[M_N];           // per map: [ceil(rows / 8)] x {lo, hi}
  int conv_desc[DC_N];      // ConvDyn
  int conv_list[DC_N];
  int wg_desc[DW_N];        // {n_live, list offset, band offset of g or -1}
  int wg_list[DW_N];
  int used;
  int total;                // ints
  FanJob fan[DC_N + DW_N];
};
// tiles per sample of the dense walk of a data-gradient (8 rows) / weight-gradient (WG_TH rows) launch of layer l
static inline int bwd_tiles(int l, int H, int W, int th) {
  const int div = vgg_layer_div(l);
  return ((H / div + th - 1) / th) * ((W / div + 31) / 32);
}
static DynLayout dyn_layout(int H, int W) {
  DynLayout L{};
  int o = 0;
  auto take = [&](int n) { const int r = o; o += (n + 3) & ~3; return r; };
  for (int l = 0; l < 3; ++l) L.seed[l] = take(2 * (H / kActMaps[kLevelMap[l]].div));
  L.seed_ints = o;
  for (int m = 0; m < M_N; ++m) L.bands[m] = take(2 * ((H / kGradMaps[m].m.div + 7) / 8));
  for (int i = 0; i < DC_N; ++i) {
    L.conv_desc[i] = take(4);
    L.conv_list[i] = take(bwd_tiles(kDgrad[i].layer, H, W, 8));
  }
  for (int i = 0; i < DW_N; ++i) {
    L.wg_desc[i] = take(4);
    L.wg_list[i] = take(bwd_tiles(kWgrad[i].layer, H, W, WG_TH));
  }
  L.used = take(4);         // [0] = 1 when the last call trimmed
  L.total = o;
  // g_x21 (l2bwd_apply writes every element) and the L2 side buffers are dense
  auto band_of = [&](int m) { return (m < 0 || m >= M_N || m == M_X21) ? -1 : L.bands[m]; };
  for (int i = 0; i < DC_N; ++i) {
    const VggDgradLaunch& d = kDgrad[i];
    L.fan[i] = FanJob{vgg_layer_div(d.layer), 8, d.pool_sum, L.bands[d.out], L.conv_list[i], L.conv_desc[i], band_of(d.src), band_of(d.add)};
  }
  for (int i = 0; i < DW_N; ++i) {
    const VggWgradLaunch& w = kWgrad[i];
    L.fan[DC_N + i] = FanJob{vgg_layer_div(w.layer), WG_TH, w.unpool >= 0 ? 1 : 0, L.bands[w.g], L.wg_list[i], L.wg_desc[i], band_of(w.g), 0};
  }
  return L;
}

typedef int2 IV;                                    // column interval [x, y); empty = {1 << 29, 0}
__device__ __forceinline__ IV iv_empty() { return make_int2(1 << 29, 0); }
__device__ __forceinline__ bool iv_none(const IV& a) { return a.x >= a.y; }
__device__ __forceinline__ IV iv_union(const IV& a, const IV& b) { return make_int2(min(a.x, b.x), max(a.y, b.y)); }

// one block of 1024 threads, thread = row.  H <= 1024 (the host falls back to the dense walk otherwise).
static __global__ __launch_bounds__(1024) void bwd_fan_kernel(int* __restrict__ dyn, DynLayout L, int H, int W) {
  __shared__ IV A[1024], Bv[1024], C9[512], C7[256];
  const int t = threadIdx.x;
  const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, H8 = H / 8, W8 = W / 8;
  auto seed = [&](int l, int row, int Wn) {
    const int* r = dyn + L.seed[l] + 2 * row;
    if (r[1] < 0) return iv_empty();
    const IV v = make_int2(max(-r[0], 0), min(r[1], Wn));
    return iv_none(v) ? iv_empty() : v;
  };
  auto at = [&](const IV* src, int row, int n) { return (row >= 0 && row < n) ? src[row] : iv_empty(); };
  auto grow = [&](const IV* src, int row, int n, int Wn) {
    IV v = iv_union(iv_union(at(src, row - 1, n), at(src, row, n)), at(src, row + 1, n));
    if (iv_none(v)) return iv_empty();
    return make_int2(max(v.x - 1, 0), min(v.y + 1, Wn));
  };
  auto down2 = [&](const IV* src, int row, int n) {
    const IV v = iv_union(at(src, 2 * row, n), at(src, 2 * row + 1, n));
    return iv_none(v) ? iv_empty() : make_int2(v.x >> 1, (v.y + 1) >> 1);
  };
  auto up2 = [&](const IV* src, int row, int n) {
    const IV v = at(src, row >> 1, n);
    return iv_none(v) ? iv_empty() : make_int2(2 * v.x, 2 * v.y);
  };
  // what the producer of map m writes: per band of 8 rows the support rounded out to 32-px tiles
  auto bands = [&](int m, const IV* src, int n, int Wn) {
    __syncthreads();
    if (t < (n + 7) / 8) {
      IV v = iv_empty();
      for (int r = 0; r < 8; ++r) v = iv_union(v, at(src, 8 * t + r, n));
      if (iv_none(v)) v = make_int2(0, 0);
      else v = make_int2(v.x & ~31, min((v.y + 31) & ~31, Wn));
      dyn[L.bands[m] + 2 * t] = v.x;
      dyn[L.bands[m] + 2 * t + 1] = v.y;
    }
    __syncthreads();
  };
  if (t < H2) A[t] = seed(2, t, W2);                          bands(M_X21, A, H2, W2);
  if (t < H2) Bv[t] = grow(A, t, H2, W2);                     bands(M_D2A, Bv, H2, W2);
  if (t < H2) C9[t] = grow(Bv, t, H2, W2);                    bands(M_X3P, C9, H2, W2);     // conv_dec2.1^T of g_d2a, still at H/2
  if (t < H4) A[t] = iv_union(seed(1, t, W4), down2(C9, t, H2));   bands(M_X18, A, H4, W4);
  if (t < H4) Bv[t] = grow(A, t, H4, W4);                     bands(M_D1A, Bv, H4, W4);
  if (t < H4) C7[t] = grow(Bv, t, H4, W4);                    bands(M_X8P, C7, H4, W4);
  if (t < H8) A[t] = iv_union(seed(0, t, W8), down2(C7, t, H4));   bands(M_X15, A, H8, W8);
  if (t < H4) Bv[t] = up2(A, t, H8);                          __syncthreads();               // virtual unpool of g_x15
  if (t < H4) A[t] = grow(Bv, t, H4, W4);                     bands(M_A12, A, H4, W4);
  if (t < H4) Bv[t] = grow(A, t, H4, W4);                     bands(M_A10, Bv, H4, W4);
  if (t < H4) A[t] = iv_union(grow(Bv, t, H4, W4), C7[t]);    bands(M_X8, A, H4, W4);        // + the x8 skip branch
  if (t < H2) Bv[t] = up2(A, t, H4);                          __syncthreads();
  if (t < H2) A[t] = grow(Bv, t, H2, W2);                     bands(M_A5, A, H2, W2);
  if (t < H2) Bv[t] = iv_union(grow(A, t, H2, W2), C9[t]);    bands(M_X3, Bv, H2, W2);       // + the x3 skip branch
  if (t < H) A[t] = up2(Bv, t, H2);                           __syncthreads();
  if (t < H) Bv[t] = grow(A, t, H, W);                        bands(M_A0, Bv, H, W);
  __threadfence_block();
  __syncthreads();

  // ---- live-tile lists: one wave per launch (L.fan: the data gradients, then the weight gradients).  entry = (tile row << 16) | tile column
  const int lane = t & 63, wv = t >> 6;
  for (int job = wv; job < DC_N + DW_N; job += 16) {
    const FanJob& J = L.fan[job];
    const int Hl = H / J.div, Wl = W / J.div, tiles_y = (Hl + J.th - 1) / J.th, tiles_x = (Wl + 31) / 32;
    const int* bd = dyn + J.bands;
    int* list = dyn + J.list;
    int base = 0;
    for (int ty0 = 0; ty0 < tiles_y; ty0 += 64) {
      const int ty = ty0 + lane;
      int tx0 = 0, tx1 = 0;
      if (ty < tiles_y) {
        // band of the map this tile row belongs to; map columns -> launch columns: << sh
        const int band = ((ty * J.th) >> J.sh) >> 3;
        const int lo = bd[2 * band], hi = bd[2 * band + 1];
        tx0 = (lo << J.sh) / 32;
        tx1 = min(((hi << J.sh) + 31) / 32, tiles_x);
      }
      const int cnt = max(tx1 - tx0, 0);
      int inc = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
      int w = base + inc - cnt;
      for (int tx = tx0; tx < tx1; ++tx) list[w++] = (ty << 16) | tx;
      base += __shfl(inc, 63, 64);
    }
    if (lane == 0) {
      int* d = dyn + J.desc;
      d[0] = base; d[1] = J.list; d[2] = J.d2; d[3] = J.d3;
    }
  }
}

struct BwdPlan {
  size_t g[M_ALL];                              // the gradient maps (vgg_graph.h); the level-4 ones 0 at level 3
  size_t dot, part, bpart, dz, dyn;
  size_t gamax;                                 // split mode: [kGradAmaxSlots][B] per-sample max |gradient map| (fp32 bits)
  size_t total;
};

// per device (bit = device id; ids >= 64 never set a bit and take the fallback kernels): the wave-specialised weight-gradient
// kernel's LDS request was accepted.  One word per kernel -- wgrad_split_ws_kernel asks for 115 KB, wgrad_ws_kernel<T> for 96 KB:
// a device or partition mode may grant one and refuse the other.
static std::atomic<unsigned long long> g_wgrad_split_ws_ok{0};
static std::atomic<unsigned long long> g_wgrad_ws_ok{0};
static inline unsigned long long dev_bit(int d) { return (d >= 0 && d < 64) ? 1ull << d : 0ull; }
static int wgrad_ksplit(int Cout, int Cin, int ntile, int resident = 512) {
  const int pairs = (Cout / 64) * (Cin / 64);
  int ks = resident / (pairs > 0 ? pairs : 1);     // 512 workgroups = one resident generation (2 per CU)
  if (ks < 1) ks = 1;
  if (ks > ntile) ks = ntile;
  return ks;
}

static void bwd_plan(int B, int H, int W, int dtype, BwdPlan* p, bool level4 = false, bool fold = false) {
  const size_t es = hla_elem_bytes(dtype);
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += hla_align_up(bytes, 256); return r; };
  const size_t P = (size_t)B * H * W;
  *p = BwdPlan{};
  for (int m : kBwdPlanOrder) p->g[m] = take((size_t)B * vgg_map_elems(kGradMaps[m].m, H, W) * es);
  p->dot = take((size_t)B * 64 * sizeof(double));
  size_t maxpart = (size_t)1024 * 2 * 64 * 32 * 4;      // conv0
  for (int l = 1; l < (level4 ? kAllLayers : kPackedLayers); ++l) {
    const VggHW g = vgg_layer_hw(l, H, W, fold);
    const int ntile = B * ((g.h + WG_TH - 1) / WG_TH) * ((g.w + 31) / 32);
    const size_t sz = (size_t)wgrad_ksplit(kLayers[l].cout, kLayers[l].cin, ntile) * kLayers[l].cout * kLayers[l].cin * 9 * 4;
    if (sz > maxpart) maxpart = sz;
  }
  p->part = take(maxpart);
  p->bpart = take((size_t)2048 * 256 * 4);
  p->dz = take((level4 ? P : P / 4) * sizeof(float));
  p->dyn = take((size_t)dyn_layout(H, W).total * sizeof(int));
  p->gamax = take((size_t)kGradAmaxSlots * B * sizeof(unsigned));
  if (level4)
    for (int m : kBwdPlanOrder4) p->g[m] = take((size_t)B * vgg_map_elems(kGradMaps[m].m, H, W) * es);
  p->total = o;
}

template <typename T>
void vgg_pack_all_T(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st) {
  std::conditional_t<Prec<T>::SPLIT, SplitPackTable, PackTable> tb{};
  int n = 0;
  for (int l = 1; l < kAllLayers; ++l) {          // conv0 needs no data gradient
    if (l >= kPackedLayers && !prm->w[l]) continue;
    // transposed conv: Cout' = cin, Cin' = cout (pack mode 2 transposes and flips the taps)
    tb.w[n] = prm->w[l]; tb.off[n] = packed_offset(l, dtype); tb.cout[n] = kLayers[l].cin; tb.cin[n] = kLayers[l].cout;
    tb.first[n] = 2;
    if constexpr (Prec<T>::SPLIT) tb.slot[n] = l;
    ++n;
  }
  if constexpr (Prec<T>::SPLIT) {
    // split mode: (hi, lo) fp16 fragments of s_w * w, transposed; the tail behind the last layer holds the per-layer scales
    // (float[16]) and 32 scratch words for the |w| maxima, as in the forward packing (vgg.hip)
    float* tail = (float*)(packed + packed_offset(kAllLayers, dtype));
    unsigned* scratch = (unsigned*)tail + 32;
    (void)hipMemsetAsync(tail, 0, kPackTailBytes, st);
    hipLaunchKernelGGL(absmax_multi_kernel, dim3(64, n), dim3(256), 0, st, tb, scratch, (unsigned*)nullptr);
    hipLaunchKernelGGL(pack_weights_split_multi_kernel, dim3(256, n), dim3(256), 0, st, tb, packed, (const unsigned*)scratch, tail);
  } else
    hipLaunchKernelGGL((pack_weights_multi_kernel<T>), dim3(256, n), dim3(256), 0, st, tb, packed);
}

// One backward call: what hla_vgg_backward was given, checked, with its plan
struct VggBwdCall {
  const float* x; size_t x_plane; const hla_vgg_params* prm; const char* packedT; const char* fw;
  const float* const* feat; const double* inv_norm; const float* const* d_feat; const float* const* conf; const float* const* d_conf;
  const hla_vgg_grads* gr; char* bw;
  int B, H, W, level, dtype, flags, first_row8;
  hipStream_t st;
  BwdPlan bp;
};

template <typename T>
int vgg_backward_t(const VggBwdCall& c) {
  const char *packedT = c.packedT, *fw = c.fw;
  const float* const *conf = c.conf, *const *d_conf = c.d_conf;
  const hla_vgg_grads* gr = c.gr;
  char* bw = c.bw;
  const BwdPlan& bp = c.bp;
  const int B = c.B, H = c.H, W = c.W, flags = c.flags;
  hipStream_t st = c.st;
  const bool level4 = c.level == 4;
  // conv0's weight gradient inside the epilogue of conv2's data gradient (conv_epilogue_wg0); the two-phase flag keeps the
  // stored map + wgrad0_kernel (A/B and tests; level 4 reads conv2's gradient from a materialised map anyway)
  const bool fuse0 = !level4 && !(flags & (HLA_VGG_BWD_WGRAD_TWO_PHASE | HLA_VGG_BWD_WGRAD0_UNFUSED));
  const int NL = level4 ? 4 : 3;
  // HLA_VGG_BWD_FOLD_DECODER: the decoder's launches run on the folded geometry [2h, w/2] (vgg_layer_hw; same buffers)
  const bool fold = (flags & HLA_VGG_BWD_FOLD_DECODER) != 0;
  VggPlan fp;
  vgg_plan(B, H, W, c.dtype, true, &fp, level4, fold);
  constexpr int KC = SB / (int)sizeof(T);
  constexpr bool SPLIT = Prec<T>::SPLIT;
  using ET = std::conditional_t<SPLIT, float, T>;      // element type of the stored maps (split mode: fp32): the elementwise kernels
  static HlaPerDeviceOnce attr_once;
  HLA_CHECK_HIP(attr_once.run([] {
    if constexpr (SPLIT) {
      // (the wave-specialised form needs 115 KB of dynamic LDS: where the device refuses it, the launches below fall back to
      //  wgrad_split_kernel -- ws_ok, per device)
      int d = 0;
      (void)hipGetDevice(&d);
      const bool ok = hipFuncSetAttribute((const void*)wgrad_split_ws_kernel<f16>, hipFuncAttributeMaxDynamicSharedMemorySize, wgs_ws_lds_bytes()) == hipSuccess;
      if (ok) g_wgrad_split_ws_ok.fetch_or(dev_bit(d)); else (void)hipGetLastError();
      return hipFuncSetAttribute((const void*)wgrad_split_kernel<f16>, hipFuncAttributeMaxDynamicSharedMemorySize, wgs_lds_bytes());
    }
    else {
      if constexpr (sizeof(T) == 2) {
        int d = 0;
        (void)hipGetDevice(&d);
        // 96 KB of dynamic LDS: refused -> the launches fall back to wgrad_kernel<T> (g_wgrad_ws_ok)
        const bool ws = hipFuncSetAttribute((const void*)wgrad_ws_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, wg_ws_lds_bytes<T>()) == hipSuccess;
        if (ws) g_wgrad_ws_ok.fetch_or(dev_bit(d)); else (void)hipGetLastError();
      }
      return hipFuncSetAttribute((const void*)wgrad_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, wg_lds_bytes<T>());
    }
  }));
  auto F = [&](int m) { return m >= 0 ? (const void*)(fw + fp.act[m]) : (const void*)nullptr; };      // forward activation
  auto G = [&](int m) { return m >= 0 ? (void*)(bw + bp.g[m]) : (void*)nullptr; };                    // gradient map
  auto IDX = [&](int i) { return i >= 0 ? (const unsigned char*)(fw + fp.idx[i]) : (const unsigned char*)nullptr; };
  // split mode: per-sample maxima of the forward's activations (recorded by its epilogues) and of this pass's gradient maps
  // (recorded by the data-gradient epilogues, or by absmax_map_kernel for the maps no convolution produced); the transposed
  // packing's per-layer weight scales sit behind the last packed layer
  const unsigned* fam = (const unsigned*)(fw + fp.amax);
  unsigned* gam = (unsigned*)(bw + bp.gamax);
  auto FA = [&](int slot) { return (SPLIT && slot >= 0) ? fam + (size_t)slot * B : (const unsigned*)nullptr; };
  auto GA = [&](int slot) { return (SPLIT && slot >= 0) ? gam + (size_t)slot * B : (unsigned*)nullptr; };
  const float* wtailT = (const float*)(packedT + packed_offset(kAllLayers, c.dtype));
  if (SPLIT) HLA_CHECK_HIP(hipMemsetAsync(gam, 0, (size_t)kGradAmaxSlots * B * sizeof(unsigned), st));

  // ---- L2_norm backward of the returned maps
  // at level 4 x21 also feeds conv_dec3, so its L2-norm gradient goes to a side buffer and is merged by that dgrad's epilogue
  const int l2map[4] = {M_L2_15, M_L2_18, level4 ? M_L2_21 : M_X21, M_X24};
  // data-dependent trimming (see bwd_fan_kernel): needs exact zeros outside the support, i.e. the one-pass L2 backward, and no
  // confidence-head gradient (which is dense).  Not combined with the caller's static first rows (the ground branch: every
  // column of its bottom half carries gradient, so there is nothing to gain).  The trimming tables describe the unfolded layer
  // graph, so the folded decoder takes the dense walk.
  const bool with_conf = conf && d_conf;
  const bool dynamic = !level4 && (flags & HLA_VGG_BWD_SCALE_INVARIANT) && !(flags & HLA_VGG_BWD_DENSE) && !with_conf &&
                       c.first_row8 == 0 && H <= 1024 && !fold;
  const DynLayout dl = dyn_layout(H, W);
  int* dynp = (int*)(bw + bp.dyn);
  if (dynamic) HLA_CHECK_HIP(hipMemsetAsync(dynp, 0x80, (size_t)dl.seed_ints * sizeof(int), st));
  HLA_CHECK_HIP(hipMemsetAsync(dynp + dl.used, dynamic ? 1 : 0, sizeof(int), st));
  // the first row of every gradient map and launch (all zero = no trimming when first_row8 == 0)
  const VggBwdRows rows = vgg_bwd_rows(c.first_row8, level4, (flags & HLA_VGG_BWD_SCALE_INVARIANT) != 0, with_conf);
  const int l2_row0[4] = {rows.n[M_X15], rows.n[M_X18], rows.n[M_X21], 0};
  size_t per[4];
  for (int l = 0; l < 4; ++l) per[l] = vgg_map_elems(kActMaps[kLevelMap[l]], H, W);
  bool l2_recorded_amax = false;
  for (int l = 0; l < NL; ++l) {
    const VggMapDef& m = kActMaps[kLevelMap[l]];
    int nblk = (int)(per[l] / 4 / 256 / 8);
    nblk = nblk < 1 ? 1 : (nblk > 64 ? 64 : nblk);
    double* part = (double*)(bw + bp.dot);
    if (flags & HLA_VGG_BWD_SCALE_INVARIANT) {
      const size_t skip = (size_t)l2_row0[l] * (W / m.div) * m.C;
      hla_prof_begin(K_ELEMWISE, 0, (double)B * (per[l] - skip) * (4 + sizeof(T)), st);
      // split mode: the finest map's gradient (g_x21 / g_x24) is READ by a convolution, which needs its per-sample maximum; the
      // pass that writes it records it, unless the confidence heads still add into it (then absmax_map below does)
      unsigned* am = (SPLIT && l == NL - 1 && !with_conf) ? GA(level4 ? GA_X24 : GA_X21) : (unsigned*)nullptr;
      l2_recorded_amax = l2_recorded_amax || am != nullptr;
      hipLaunchKernelGGL((l2bwd_apply_kernel<ET, true>), dim3(B * nblk), dim3(256), 0, st, c.feat[l], c.d_feat[l], part,
                         c.inv_norm + (size_t)l * B, (ET*)G(l2map[l]), per[l], nblk, dynamic ? dynp + dl.seed[l] : (int*)nullptr,
                         m.C, W / m.div, skip, am);
    } else {
      hla_prof_begin(K_ELEMWISE, 0, (double)B * per[l] * (16 + sizeof(T)), st);
      hipLaunchKernelGGL(l2bwd_dot_kernel, dim3(B * nblk), dim3(256), 0, st, c.feat[l], c.d_feat[l], part, per[l], nblk);
      hipLaunchKernelGGL((l2bwd_apply_kernel<ET, false>), dim3(B * nblk), dim3(256), 0, st, c.feat[l], c.d_feat[l], part,
                         c.inv_norm + (size_t)l * B, (ET*)G(l2map[l]), per[l], nblk);
    }
    hla_prof_end(st);
  }

  if (dynamic) hipLaunchKernelGGL(bwd_fan_kernel, dim3(1), dim3(1024), 0, st, dynp, dl, H, W);

  // ---- confidence heads (only the ground branch with using_weight=1 ever has d_conf): adds into the raw-map gradients
  if (with_conf) {
    for (int l = 0; l < NL; ++l) {
      if (!d_conf[l]) continue;
      const VggMapDef& m = kActMaps[kLevelMap[l]];
      const VggHW g = vgg_map_hw(m, H, W, fold);
      constexpr int EPL = 16 / (int)sizeof(ET);
      const int ppb = 256 / (m.C / EPL);
      const size_t npix = (size_t)B * g.h * g.w;
      const int grid = (int)((npix + ppb - 1) / ppb < 1024 ? (npix + ppb - 1) / ppb : 1024);
      float* dz = (float*)(bw + bp.dz);
      hla_prof_begin(K_ELEMWISE, 4.0 * 9 * m.C * (double)npix, (double)npix * (3 * m.C * sizeof(ET) + 12), st);
      hipLaunchKernelGGL(conf_dz_kernel, dim3((unsigned)((npix + 255) / 256 < 2048 ? (npix + 255) / 256 : 2048)), dim3(256), 0, st,
                         conf[l], d_conf[l], dz, npix);
      hipLaunchKernelGGL((conf_bwd_kernel<ET>), dim3(grid), dim3(256), 4 * 9 * m.C * sizeof(float), st, (const ET*)F(kLevelMap[l]),
                         c.prm->w[13 + l], (const float*)dz, (ET*)G(l2map[l]), (float*)(bw + bp.part), B, g.h, g.w, m.C);
      const size_t n = (size_t)9 * m.C;
      hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, (const float*)(bw + bp.part),
                         gr->dw[13 + l], n, grid, (int)n, 1, 1);
      hla_prof_end(st);
    }
  }

  // split mode: the scale of the two gradient maps that convolutions READ but no convolution wrote (at level 3: g_x21; l2_18 /
  // l2_15 are only ever added in an epilogue, in fp32)
  auto absmax_map = [&](int m, size_t skip) {
    const size_t per_sample = vgg_map_elems(kGradMaps[m].m, H, W);
    int nblk = (int)(per_sample / 4 / 256 / 8);
    nblk = nblk < 1 ? 1 : (nblk > 64 ? 64 : nblk);
    hla_prof_begin(K_ELEMWISE, 0, (double)B * (per_sample - skip) * 4, st);
    hipLaunchKernelGGL(absmax_map_kernel, dim3(B * nblk), dim3(256), 0, st, (const float*)G(m), per_sample, skip, nblk, GA(kGradMaps[m].ga));
    hla_prof_end(st);
  };
  if (SPLIT && !l2_recorded_amax) {
    if (level4) absmax_map(M_X24, 0);
    else absmax_map(M_X21, (size_t)rows.n[M_X21] * (W / kGradMaps[M_X21].m.div) * kGradMaps[M_X21].m.C);
  }

  // ---- the launches of the walk, by their row in kDgrad / kWgrad (vgg_graph.h); rows below DC_N / DW_N have a live-tile list
  bool launch_ok = true;
  auto dgrad = [&](int i) {
    const VggDgradLaunch& d = kDgrad[i];
    const bool fuse_wg0 = i == DC_1 && fuse0;
    const VggHW g = vgg_layer_hw(d.layer, H, W, fold);
    ConvArgs a{};
    if (fuse_wg0) {      // conv2's data gradient contracted into conv0's weight gradient in its epilogue; g_a0 receives the partials
      a.wg0_x = c.x; a.wg0_x_plane = c.x_plane ? c.x_plane : (size_t)H * W; a.wg0_part = (float*)G(d.out);
    }
    a.amax1 = GA(kGradMaps[d.src].ga); a.amax_out = GA(fuse_wg0 ? -1 : kGradMaps[d.out].ga); a.wscale = SPLIT ? wtailT + d.layer : nullptr;
    if (i < DC_N) {
      a.dyn = dynamic ? dynp : nullptr; a.dyn_desc = dl.conv_desc[i];
      a.row_begin = rows.dc_row[i]; a.src_row_lo = rows.dc_src_lo[i]; a.add_row_lo = rows.dc_add_lo[i];
    }
    a.src1 = G(d.src); a.C1 = kLayers[d.layer].cout; a.unpool_idx = IDX(d.unpool);
    const int nstage = kLayers[d.layer].cout / KC;
    a.wpk = (const uint4*)(packedT + packed_offset(d.layer, c.dtype)) + (size_t)(d.c0 / 32) * nstage * 18 * 64;
    a.out_act = fuse_wg0 ? nullptr : G(d.out); a.mask_act = F(d.mask); a.add_src = G(d.add); a.pool_sum = d.pool_sum;
    a.B = B; a.H = g.h; a.W = g.w; a.Cout = kGradMaps[d.out].m.C; a.relu_act = 0;
    if (!launch_conv<T, true>(st, a, d.pool_sum != 0)) launch_ok = false;
  };
  auto wgrad = [&](int i) {
    const VggWgradLaunch& wl = kWgrad[i];
    const int l = wl.layer;
    const VggHW g = vgg_layer_hw(l, H, W, fold);
    WgradArgs a{};
    if (i < DW_N) { a.dyn = dynamic ? dynp : nullptr; a.dyn_desc = dl.wg_desc[i]; a.row_begin = rows.dw_row[i]; }
    a.x1 = F(wl.x1); a.x2 = F(wl.x2); a.C1 = kActMaps[wl.x1].C; a.C2 = wl.x2 >= 0 ? kActMaps[wl.x2].C : 0; a.up1 = wl.x2 >= 0 ? 1 : 0;
    a.g = G(wl.g); a.g_unpool = IDX(wl.unpool);
    a.B = B; a.H = g.h; a.W = g.w; a.Cout = kLayers[l].cout; a.Cin = kLayers[l].cin;
    a.tiles_x = (g.w + 31) / 32; a.tiles_y = (g.h - a.row_begin + WG_TH - 1) / WG_TH; a.ntile = B * a.tiles_x * a.tiles_y;
    // wave-specialised kernels (split and 16-bit, unless the device refused their LDS or the caller asks for the two-phase ones):
    // one 8-wave workgroup per CU -> 256 workgroups are one resident generation; two-phase: two 4-wave workgroups -> 512
    bool ws = false;
    if constexpr (SPLIT || sizeof(T) == 2) {
      int d = 0;
      (void)hipGetDevice(&d);
      ws = ((SPLIT ? g_wgrad_split_ws_ok : g_wgrad_ws_ok).load() & dev_bit(d)) != 0 && !(flags & HLA_VGG_BWD_WGRAD_TWO_PHASE);
    }
    a.KS = wgrad_ksplit(a.Cout, a.Cin, a.ntile, ws ? 256 : 512);
    a.part = (float*)(bw + bp.part);
    a.bpart = (kLayers[l].has_bias && gr->db[l]) ? (float*)(bw + bp.bpart) : nullptr;
    const double P = (double)B * (g.h - a.row_begin) * g.w;
    hla_prof_begin_dyn(K_WGRAD, 2.0 * 9 * a.Cin * a.Cout * P, P * (a.Cin + a.Cout) * sizeof(T), st,
                       a.dyn ? a.dyn + a.dyn_desc : nullptr, a.tiles_x * a.tiles_y);
    const dim3 grid(a.KS, a.Cin / 64, a.Cout / 64), block(ws ? 512 : 256);
    if constexpr (SPLIT) {      // (the amax slots of its input activation(s) and of the gradient map)
      const WgradSplitExtra ex{FA(wl.x1), FA(wl.x2), GA(kGradMaps[wl.g].ga)};
      if (ws) hipLaunchKernelGGL(wgrad_split_ws_kernel<f16>, grid, block, wgs_ws_lds_bytes(), st, a, ex);
      else hipLaunchKernelGGL(wgrad_split_kernel<f16>, grid, block, wgs_lds_bytes(), st, a, ex);
    } else {
      if constexpr (sizeof(T) == 2) {
        if (ws) hipLaunchKernelGGL((wgrad_ws_kernel<T>), grid, block, wg_ws_lds_bytes<T>(), st, a);
      }
      if (!ws) hipLaunchKernelGGL((wgrad_kernel<T>), grid, block, wg_lds_bytes<T>(), st, a);
    }
    hla_prof_end(st);
    const size_t n = (size_t)a.Cout * a.Cin * 9;
    hla_prof_begin(K_ELEMWISE, 0, (double)n * 4 * (a.KS + 1), st);
    hipLaunchKernelGGL(reduce_partials4_kernel, dim3((unsigned)((n / 4 + 31) / 32)), dim3(256), 0, st, (const float4*)a.part,
                       (float4*)gr->dw[l], n / 4, a.KS);
    hla_prof_end(st);
    if (a.bpart)
      hipLaunchKernelGGL(reduce_partials_kernel, dim3((a.Cout + 15) / 16), dim3(256), 0, st, a.bpart, gr->db[l], (size_t)a.Cout, a.KS, a.Cout, 1, 1);
  };
  // ---- the walk, from the last layer down: a layer's data gradient(s), then its weight gradient.  (Level 4: conv_dec3 is
  // zero-padded to 64 channels, the host slices its weight gradients.)
  for (int l = (level4 ? kAllLayers : kPackedLayers) - 1; l >= 1; --l) {
    if (l == 1 && level4) {      // the conv2 output also fed conv_dec3: materialise unpool(g_x3) + skip gradient once
      const size_t n = (size_t)B * H * W * (64 * sizeof(ET) / 16);
      hla_prof_begin(K_ELEMWISE, 0, (double)B * H * W * 64 * sizeof(ET) * 2.25, st);
      hipLaunchKernelGGL((unpool_add_kernel<ET>), dim3((unsigned)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535)), dim3(256), 0, st,
                         (const ET*)G(M_X3), IDX(IDX_3), (const ET*)G(M_X2P), (ET*)G(M_C2), B, H, W);
      hla_prof_end(st);
      if (SPLIT) absmax_map(M_C2, 0);
    }
    for (int i = 0; i < DC_ALL; ++i)
      if (kDgrad[i].layer == l && vgg_level_runs(kDgrad[i].level, level4)) dgrad(i);
    for (int i = 0; i < DW_ALL; ++i)
      if (kWgrad[i].layer == l && vgg_level_runs(kWgrad[i].level, level4)) wgrad(i);
  }
  // ---- conv0's weight gradient
  const int n_a0 = rows.dw_row[DW_0];
  if (fuse0) {
    // it left the data gradient's epilogue as one [64][32] partial per workgroup, in the place of the map (8 KB per 8 x 32-pixel
    // tile against the map's 32 / 64 KB): 1024 slabs, then the generic gather (k < 27: dW0, column 27: db0)
    const int tiles = ((W + 31) / 32) * ((H - n_a0 + 7) / 8) * B, NS = 1024;
    float* slab = (float*)(bw + bp.part);
    hla_prof_begin(K_ELEMWISE, 0, (double)tiles * 8192.0 * (dynamic ? 0.5 : 1.0), st);
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(NS), dim3(256), 0, st, (const float4*)G(M_A0), (float4*)slab, 512, tiles,
                       dynamic ? dynp + dl.conv_desc[DC_1] : (const int*)nullptr, B);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((64 * 27 + 15) / 16), dim3(256), 0, st, (const float*)slab, gr->dw[0], (size_t)64 * 27, NS, 64 * 32, 27, 32);
    if (gr->db[0]) hipLaunchKernelGGL(reduce_partials_kernel, dim3(4), dim3(256), 0, st, (const float*)slab + 27, gr->db[0], (size_t)64, NS, 64 * 32, 1, 32);
    hla_prof_end(st);
  } else {
    Wgrad0Args a{};
    a.x = c.x; a.x_plane = c.x_plane ? c.x_plane : (size_t)H * W; a.g = G(M_A0); a.B = B; a.H = H; a.W = W;
    a.row_begin = n_a0;
    a.dyn = dynamic ? dynp : nullptr; a.dyn_desc = dl.wg_desc[DW_0];
    a.tiles_x = (W + 31) / 32; a.tiles_y = (H - a.row_begin + WG_TH - 1) / WG_TH; a.ntile = B * a.tiles_x * a.tiles_y;
    a.KS = a.ntile < 1024 ? a.ntile : 1024;
    a.part = (float*)(bw + bp.part); a.bpart = (float*)(bw + bp.bpart);
    // (split mode: conv0's weight gradient -- K = pixels, N = 27 -- runs on the exact-fp32 kernel: 34 GFLOP, 0.2 ms at B = 32)
    const int lds = WG_TH * 32 * wg_stride<ET>() + 3 * (WG_TH + 2) * 48 * 4;
    const double P = (double)B * (H - a.row_begin) * W;
    hla_prof_begin_dyn(K_WGRAD, 2.0 * 27 * 64 * P, P * (12 + 64 * sizeof(ET)), st, a.dyn ? a.dyn + a.dyn_desc : nullptr,
                       a.tiles_x * a.tiles_y);
    hipLaunchKernelGGL((wgrad0_kernel<ET>), dim3(a.KS), dim3(256), lds, st, a);
    hla_prof_end(st);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((64 * 27 + 15) / 16), dim3(256), 0, st, a.part, gr->dw[0], (size_t)64 * 27, a.KS * 2, 64 * 32, 27, 32);
    if (gr->db[0]) hipLaunchKernelGGL(reduce_partials_kernel, dim3(4), dim3(256), 0, st, a.bpart, gr->db[0], (size_t)64, a.KS * 2, 64, 1, 1);
  }
  HLA_CHECK_HIP(hipGetLastError());
  return launch_ok ? HLA_OK : HLA_ERR_ARG;
}

#if HLA_TU_DTYPE >= 0
template void vgg_pack_all_T<TuT>(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st);
template int vgg_backward_t<TuT>(const VggBwdCall& c);
#else
#define HLA_EXTERN_T(T) \
  extern template void vgg_pack_all_T<T>(const hla_vgg_params* prm, char* packed, int dtype, hipStream_t st); \
  extern template int vgg_backward_t<T>(const VggBwdCall& c);
HLA_EXTERN_T(float) HLA_EXTERN_T(bf16) HLA_EXTERN_T(f16) HLA_EXTERN_T(split32)

extern "C" size_t hla_vgg_bwd_workspace_bytes(int B, int H, int W, int level, int dtype) {
  BwdPlan p;
  bwd_plan(B, H, W, dtype, &p, level == 4);
  return p.total;
}

extern "C" size_t hla_vgg_bwd_workspace_bytes_flags(int B, int H, int W, int level, int dtype, int flags) {
  BwdPlan p;
  bwd_plan(B, H, W, dtype, &p, level == 4, (flags & HLA_VGG_BWD_FOLD_DECODER) != 0);
  return p.total;
}

// (HLA_F16X3: fp32 storage in the HLA_F32 workspace layout; data and weight gradients on split-fp16 kernels, conv0's weight
// gradient and the elementwise passes on the fp32 ones)
extern "C" size_t hla_vgg_packed_weight_T_bytes(int dtype) {
  return packed_offset(kAllLayers, dtype) + (dtype == HLA_F16X3 ? kPackTailBytes : 0);
}

extern "C" int hla_vgg_pack_weights_T(const hla_vgg_params* params, void* packed, int dtype, hla_stream_t stream) {
  HLA_REQUIRE(params && packed, "hla_vgg_pack_weights_T: null argument");
  HLA_REQUIRE(hla_dtype_ok(dtype), "hla_vgg_pack_weights_T: bad dtype %d", dtype);
  hla_dispatch_dtype(dtype, [&](auto t) { vgg_pack_all_T<typename decltype(t)::type>(params, (char*)packed, dtype, (hipStream_t)stream); });
  HLA_CHECK_HIP(hipGetLastError());
  return HLA_OK;
}

extern "C" int hla_vgg_backward(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights_T,
                                const void* fwd_workspace, const float* const feat[4], const double* inv_norm,
                                const float* const d_feat[4], const float* const conf[4], const float* const d_conf[4],
                                const hla_vgg_grads* grads, void* workspace, size_t workspace_bytes, int B, int H, int W,
                                int level, int dtype, int flags, int first_row8, hla_stream_t stream) {
  HLA_REQUIRE(x && params && packed_weights_T && fwd_workspace && feat && inv_norm && d_feat && grads && workspace,
              "hla_vgg_backward: null argument");
  HLA_REQUIRE(hla_dtype_ok(dtype), "hla_vgg_backward: bad dtype %d", dtype);
  HLA_REQUIRE(level == 3 || level == 4, "hla_vgg_backward: level must be 3 or 4");
  HLA_REQUIRE((size_t)H * W * 64 * 4 < ((size_t)1 << 31), "hla_vgg_backward: image too large (H*W must be below 2^23 pixels)");
  HLA_REQUIRE(x_plane == 0 || x_plane >= (size_t)H * W, "hla_vgg_backward: x_plane (%zu) must be 0 or >= H*W", x_plane);
  HLA_REQUIRE(first_row8 == 0 || (first_row8 >= 4 && first_row8 < H / 8), "hla_vgg_backward: first_row8 must be 0 or in [4, H/8)");
  const int NLc = level == 4 ? 4 : 3;
  HLA_REQUIRE(B > 0 && H % 8 == 0 && W % 8 == 0, "hla_vgg_backward: H and W must be multiples of 8");
  HLA_REQUIRE(!(flags & HLA_VGG_BWD_FOLD_DECODER) || (W % 16 == 0 && first_row8 == 0),
              "hla_vgg_backward: HLA_VGG_BWD_FOLD_DECODER needs W %% 16 == 0 and first_row8 == 0 (got W = %d, first_row8 = %d)", W, first_row8);
  for (int l = 0; l < kPackedLayers; ++l) HLA_REQUIRE(grads->dw[l], "hla_vgg_backward: dw[%d] missing", l);
  HLA_REQUIRE(!d_conf || conf, "hla_vgg_backward: d_conf given without conf");
  if (d_conf)
    for (int l = 0; l < NLc; ++l)
      HLA_REQUIRE(!d_conf[l] || (conf[l] && grads->dw[13 + l]), "hla_vgg_backward: d_conf[%d] needs conf[%d] and dw[%d]", l, l, 13 + l);
  if (level == 4)
    HLA_REQUIRE(feat[3] && d_feat[3] && params->w[11] && params->w[12] && grads->dw[11] && grads->dw[12],
                "hla_vgg_backward: level 4 needs feat[3], d_feat[3], the padded conv_dec3 weights and dw[11], dw[12] ([64,128,3,3], [64,64,3,3])");
  VggBwdCall c{x, x_plane, params, (const char*)packed_weights_T, (const char*)fwd_workspace, feat, inv_norm, d_feat, conf, d_conf, grads,
               (char*)workspace, B, H, W, level, dtype, flags, first_row8, (hipStream_t)stream, {}};
  bwd_plan(B, H, W, dtype, &c.bp, level == 4, (flags & HLA_VGG_BWD_FOLD_DECODER) != 0);
  if (workspace_bytes < c.bp.total) {
    hla_set_error("hla_vgg_backward: workspace %zu < %zu", workspace_bytes, c.bp.total);
    return HLA_ERR_WORKSPACE;
  }
  return hla_dispatch_dtype(dtype, [&](auto t) { return vgg_backward_t<typename decltype(t)::type>(c); });
}
extern "C" int hla_vgg_backward_live_tiles(const void* workspace, int B, int H, int W, int level, int dtype, long long* live,
                                           long long* total) {
  HLA_REQUIRE(workspace && live && total, "hla_vgg_backward_live_tiles: null argument");
  HLA_REQUIRE(hla_dtype_ok(dtype), "hla_vgg_backward_live_tiles: bad dtype %d", dtype);
  BwdPlan bp;
  bwd_plan(B, H, W, dtype, &bp, level == 4);
  const DynLayout L = dyn_layout(H, W);
  std::vector<int> h(L.total);
  HLA_CHECK_HIP(hipMemcpy(h.data(), (const char*)workspace + bp.dyn, (size_t)L.total * sizeof(int), hipMemcpyDeviceToHost));
  *live = *total = 0;
  if ((h[L.used] & 0xff) != 1) return HLA_OK;
  for (int i = 0; i < DC_N; ++i) {
    *live += h[L.conv_desc[i]];
    *total += bwd_tiles(kDgrad[i].layer, H, W, 8);
  }
  for (int i = 0; i < DW_N; ++i) {
    *live += h[L.wg_desc[i]];
    *total += bwd_tiles(kWgrad[i].layer, H, W, WG_TH);
  }
  return HLA_OK;
}
#endif
