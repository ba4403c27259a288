// Weight-gradient kernels of the VGG16-U-Net backward (planning and launches: vgg_backward.hip).
// Every kernel computes the same contraction: a 64 x 64 (Cout x Cin) tile of dW, 9 taps, summed over the pixels of a k-slice
// of 4 x 32 pixel tiles, as an MFMA GEMM whose K dimension is PIXELS.  Both operands are "k-major" in NHWC (pixels are rows);
// for the 16-bit types the fragments come from gfx950's transposing read ds_read_b64_tr_b16 out of [pixel][channel] LDS tiles
// (tools/probes/tr16_probe.hip documents the lane semantics), for fp32 a lane needs one element per MFMA and plain ds_read_b32
// suffices.  Bias gradients ride along as one extra MFMA against an all-ones fragment.
//   wgrad_kernel<T>          two-phase (load -> barrier -> MFMA in every wave): fp32, and the 16-bit fallback / test reference
//   wgrad_ws_kernel<T>       wave-specialised, 16-bit (the default)
//   wgrad_split_kernel<H>    two-phase, precision 'fp16x3' (fallback / test reference)
//   wgrad_split_ws_kernel<H> wave-specialised, precision 'fp16x3' (the default)
//   wgrad0_kernel<T>         conv0 from a stored gradient map
// The kernels share the building blocks below -- block decode, accumulators + epilogue, buffer descriptors, the two loaders, the
// inner tap loop -- and differ in role, loader, fragment walk and what happens to a piece on its way into LDS.
#pragma once
#include "conv_kernels.h"

// (frag_kmajor / frag_ones / KStep: conv_kernels.h -- the fused conv0 weight gradient in the data-gradient epilogue uses them too)

constexpr int WG_TH = 4;                                  // pixel tile of the weight-gradient kernels: 4 rows x 32 px
struct WgradArgs {
  const void* x1; const void* x2;      // conv input (stored post-ReLU activations); virtual upsample+concat as forward
  const void* g;                       // d(loss)/d(conv output) NHWC T [B,H,W,Cout], or the pooled map's gradient
  const unsigned char* g_unpool;       //   [B,H/2,W/2,Cout] + forward argmax (virtual unpool) when non-null
  float* part;                         // [KS][Cout][Cin][9] partial sums
  float* bpart;                        // [KS][Cout] partial bias gradients, or null
  int C1, C2, up1, B, H, W, Cout, Cin, tiles_x, tiles_y, ntile, KS;
  int row_begin;                       // first pixel row that carries gradient (even with g_unpool); rows above are skipped
  const int* dyn;                      // data-dependent launch (bwd_fan_kernel): base of the device-side tables, or null
  int dyn_desc;                        //   int offset of {live tiles per sample, list offset, band table of g or -1}: only the
                                       //   listed tiles are visited, and g reads as zero outside the part its producer wrote
};

// tile enumeration of the weight-gradient kernels
struct WgTiles {
  const int* dyn; int nl, list, gb, ntile, tiles_x, tiles_y, row_begin, H, W, gsh;
  __device__ __forceinline__ WgTiles(const int* dyn_, int desc, int H_, int W_, int row_begin_, int tiles_x_, int tiles_y_,
                                     int ntile_all, int B, int gsh_)
      : dyn(dyn_), nl(0), list(0), gb(-1), ntile(ntile_all), tiles_x(tiles_x_), tiles_y(tiles_y_), row_begin(row_begin_),
        H(H_), W(W_), gsh(gsh_) {
    if (!dyn) return;
    nl = dyn[desc]; list = dyn[desc + 1]; gb = dyn[desc + 2];
    ntile = nl * B;
  }
  // origin of a tile and the column interval [gx0, gx1) of this launch's coordinates in which g may be read
  __device__ __forceinline__ void origin(int tile, int& b, int& y0, int& x0, int& gx0, int& gx1) const {
    gx0 = 0; gx1 = W;
    if (dyn) {
      b = tile / nl;
      const int e = dyn[list + tile % nl];
      y0 = (e >> 16) * WG_TH; x0 = (e & 0xffff) * 32;
      if (gb >= 0) {
        const int band = (y0 >> gsh) >> 3;
        gx0 = dyn[gb + 2 * band] << gsh;
        gx1 = min(dyn[gb + 2 * band + 1] << gsh, W);
      }
    } else {
      int q = tile;
      x0 = (q % tiles_x) * 32; q /= tiles_x;
      y0 = row_begin + (q % tiles_y) * WG_TH;
      b = q / tiles_y;
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Building blocks

// What a workgroup computes -- k-slice ks of the tile (co0, ci0) -- and where its operands live: the input channels come from x1
// or x2 (the forward's virtual concat), x1 possibly at half resolution (virtual nearest upsample: sh), g possibly as the pooled
// map's gradient (virtual unpool: gsh).
struct WgBlock {
  int ks, ci0, co0, Cs, coff, sh, Hs, Ws, gsh, Hg, Wg;
  bool first;
  const char* xsrc;
  __device__ __forceinline__ explicit WgBlock(const WgradArgs& a) {
    ks = blockIdx.x; ci0 = blockIdx.y * 64; co0 = blockIdx.z * 64;
    first = ci0 < a.C1;
    xsrc = (const char*)(first ? a.x1 : a.x2);
    Cs = first ? a.C1 : a.C2; coff = first ? ci0 : ci0 - a.C1; sh = (first && a.up1) ? 1 : 0;
    Hs = a.H >> sh; Ws = a.W >> sh;
    gsh = a.g_unpool ? 1 : 0; Hg = a.H >> gsh; Wg = a.W >> gsh;
  }
  // (it: which 32 input channels of the tile a wave multiplies -- the bias needs one of the two)
  __device__ __forceinline__ bool want_bias(const WgradArgs& a, int it) const { return a.bpart && blockIdx.y == 0 && it == 0; }
  __device__ __forceinline__ WgTiles tiles(const WgradArgs& a) const {
    return WgTiles(a.dyn, a.dyn_desc, a.H, a.W, a.row_begin, a.tiles_x, a.tiles_y, a.ntile, a.B, a.g_unpool ? 1 : 0);
  }
};

// A wave's accumulators -- 32 x 32 (co x ci) per tap, and the bias column -- and the partial-sum epilogue.
struct WgAcc {
  f32x16 acc[9], accb;
  __device__ __forceinline__ WgAcc() {
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) accb[r] = 0.f;
  }
  // D[i = co][j = ci]: lane -> ci = ci0 + it*32 + (lane&31); reg r -> co = co0 + ct*32 + (r&3) + 8(r>>2) + 4(lane>>5)
  // (inv / invg: split mode undoes its operand scales here)
  __device__ __forceinline__ void store(const WgradArgs& a, const WgBlock& k, int ct, int it, int lane, bool want_bias,
                                        float inv = 1.f, float invg = 1.f) const {
    const int ks = k.ks, ci0 = k.ci0, co0 = k.co0;
    const int ci = ci0 + it * 32 + (lane & 31), g5 = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * g5;
      float* o = a.part + (((size_t)ks * a.Cout + co) * a.Cin + ci) * 9;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) o[tap] = acc[tap][r] * inv;
      if (want_bias && (lane & 31) == 0) a.bpart[(size_t)ks * a.Cout + co] = accb[r] * invg;
    }
  }
};

// The inner tap loop: the X fragment(s) of halo row rho and column shift kx feed the up to three taps ky whose output row
// r = rho - ky lies inside the TH-row tile.  One product, or split mode's hi hi + lo hi + hi lo (in that order per accumulator).
template <typename T, int TH>
__device__ __forceinline__ void wg_taps(f32x16 (&acc)[9], int rho, int kx, const uint4 (&A)[TH], const uint4& B) {
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int r = rho - ky;
    if (r >= 0 && r < TH) mma16<T>(acc[ky * 3 + kx], A[r], B);
  }
}
template <typename T, int TH>
__device__ __forceinline__ void wg_taps(f32x16 (&acc)[9], int rho, int kx, const uint4 (&Ah)[TH], const uint4 (&Al)[TH],
                                        const uint4& Bh, const uint4& Bl) {
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int r = rho - ky;
    if (r >= 0 && r < TH) {
      mma16<T>(acc[ky * 3 + kx], Ah[r], Bh);
      mma16<T>(acc[ky * 3 + kx], Al[r], Bh);
      mma16<T>(acc[ky * 3 + kx], Ah[r], Bl);
    }
  }
}

typedef unsigned wg_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned wg_u32x2 __attribute__((ext_vector_type(2)));
constexpr int WG_OOB = (int)0x80000000;                  // an offset beyond every descriptor's range: the load returns zeros

// raw buffer descriptor over [base, base + bytes) (wave-uniform)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wg_rsrc(const void* base, size_t bytes) {
  const unsigned long long p = (unsigned long long)base;
  const void* pu = (const void*)(((unsigned long long)__builtin_amdgcn_readfirstlane((int)(unsigned)(p >> 32)) << 32) |
                                 (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)p));
  return __builtin_amdgcn_make_buffer_rsrc((void*)pu, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}

// Tile loads are raw buffer loads through one descriptor per operand and sample (base = the sample's map, range = its bytes).  A
// piece outside the image / the written part of g gets an offset beyond the range and reads as ZERO: no branch around a load, so
// all of a tile's loads are in flight together.  (With `if (inside) v = *p` hipcc puts each load into its own exec-masked block
// that ends with an s_waitcnt vmcnt(0): the exact-fp32 kernel's 29 loads per tile were 29 dependent round trips, and the split
// kernel ran at 0.37 of its MFMA ceiling where the forward kernels reach 0.55.)
// ES: bytes per stored element.  ri: the forward argmax bytes of the pooled map, one per element of g; without unpool a
// zero-sized descriptor, which reads 0.
template <int ES>
struct WgSampleRsrc {
  __amdgpu_buffer_rsrc_t rx, rg, ri;
  __device__ __forceinline__ WgSampleRsrc(const WgradArgs& a, const WgBlock& k, int b) {
    const size_t xs_bytes = (size_t)k.Hs * k.Ws * k.Cs * ES, gs_bytes = (size_t)k.Hg * k.Wg * a.Cout * ES;
    rx = wg_rsrc(k.xsrc + (size_t)b * xs_bytes, xs_bytes);
    rg = wg_rsrc((const char*)a.g + (size_t)b * gs_bytes, gs_bytes);
    ri = wg_rsrc(a.g_unpool ? a.g_unpool + (size_t)b * (gs_bytes / ES) : (const unsigned char*)a.g, a.g_unpool ? gs_bytes / ES : 0);
  }
};

// How a TH-row tile's 16-B pieces are dealt to 256 loading threads: thread t holds piece `part` of pixels pix0 + i * PSTEP.
template <int ES, int TH>
struct WgPieces {
  static constexpr int EPL = 16 / ES, PPX = 64 * ES / 16;                       // elements per piece, pieces per 64-channel pixel
  static constexpr int XPIX = (TH + 2) * HWID, GPIX = TH * 32;
  static constexpr int NX = (XPIX * PPX + 255) / 256, NG = GPIX * PPX / 256, PSTEP = 256 / PPX;
  static_assert(GPIX * PPX % 256 == 0, "gradient tile pieces per thread");
  typedef std::conditional_t<EPL == 8, wg_u32x2, unsigned> Idx;                 // the argmax bytes of a piece's elements
  static __device__ __forceinline__ Idx load_idx(__amdgpu_buffer_rsrc_t ri, int e0) {
    if constexpr (EPL == 8) return __builtin_amdgcn_raw_buffer_load_b64(ri, e0, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b32(ri, e0, 0, 0);
  }
};

// The virtual unpool keeps the elements of a piece of g whose forward argmax is the pixel's own (y & 1, x & 1).  Three forms,
// each measured in the kernel that uses it:
// generic compare, element by element (wgrad_kernel<T>)
template <typename T, typename Idx>
__device__ __forceinline__ void wg_unpool_mask_generic(wg_u32x4& v, Idx idx, unsigned pos) {
  constexpr int EPL = 16 / sizeof(T);
  T ev[EPL];
  unsigned char id[sizeof(Idx)];
  __builtin_memcpy(ev, &v, 16);
  __builtin_memcpy(id, &idx, sizeof(Idx));
#pragma unroll
  for (int k = 0; k < EPL; ++k) if (id[k] != pos) ev[k] = (T)0.f;
  __builtin_memcpy(&v, ev, 16);
}
// packed, 16-bit elements (wgrad_ws_kernel): a byte of idx ^ pos spread into a 16-bit lane is zero only for a match, so
// (lane - 1) >> 15 is the lane's keep mask
__device__ __forceinline__ void wg_unpool_mask_perm(wg_u32x4& v, wg_u32x2 idx, unsigned pos) {
  typedef short s16x2 __attribute__((ext_vector_type(2)));
  const unsigned m0 = idx.x ^ (pos * 0x01010101u), m1 = idx.y ^ (pos * 0x01010101u);
  auto keep = [](unsigned m, unsigned sel) {
    s16x2 w2 = __builtin_bit_cast(s16x2, __builtin_amdgcn_perm(0u, m, sel));
    w2 = (w2 - (short)1) >> 15;
    return __builtin_bit_cast(unsigned, w2);
  };
  v.x &= keep(m0, 0x0c010c00u); v.y &= keep(m0, 0x0c030c02u);
  v.z &= keep(m1, 0x0c010c00u); v.w &= keep(m1, 0x0c030c02u);
}
// byte compares on four fp32 elements, ahead of the hi / lo split (wgrad_split_kernel, wgrad_split_ws_kernel)
__device__ __forceinline__ void wg_unpool_mask_bytes(float& e0, float& e1, float& e2, float& e3, unsigned idx, unsigned pos) {
  if ((idx & 0xff) != pos) e0 = 0.f;
  if (((idx >> 8) & 0xff) != pos) e1 = 0.f;
  if (((idx >> 16) & 0xff) != pos) e2 = 0.f;
  if ((idx >> 24) != pos) e3 = 0.f;
}

// The two-phase loader: every thread of a 256-thread workgroup requests its pieces of one tile into staging registers, all of
// them back to back (memory-level parallelism); the kernel writes them to LDS behind a barrier.  [lo, hi): a window of the
// thread's pieces (fp32 stages a tile in batches).
template <int ES, int TH>
struct WgStagedTile : WgPieces<ES, TH> {
  typedef WgPieces<ES, TH> P;
  wg_u32x4 xr[P::NX], gr[P::NG];
  typename P::Idx gid[P::NG];
  int part, pix0;
  __device__ __forceinline__ explicit WgStagedTile(int t) : part(t % P::PPX), pix0(t / P::PPX) {}
  // input halo tile with origin (y0, x0) of sample b, zero outside the image
  __device__ __forceinline__ void load_x(const WgradArgs& a, const WgBlock& k, int b, int y0, int x0, int lo = 0, int hi = P::NX) {
    const WgSampleRsrc<ES> rs(a, k, b);
#pragma unroll
    for (int i = 0; i < P::NX; ++i) {
      if (i < lo || i >= hi) continue;
      const int pix = pix0 + i * P::PSTEP;
      const int hy = pix / HWID, hx = pix - hy * HWID, y = y0 - 1 + hy, x = x0 - 1 + hx;
      const bool ok = pix < P::XPIX && y >= 0 && y < a.H && x >= 0 && x < a.W;
      xr[i] = __builtin_amdgcn_raw_buffer_load_b128(rs.rx, ok ? (((y >> k.sh) * k.Ws + (x >> k.sh)) * k.Cs + k.coff + part * P::EPL) * ES : WG_OOB, 0, 0);
    }
  }
  // output-gradient tile, columns [gx0, gx1) (virtual unpool: + the forward argmax)
  __device__ __forceinline__ void load_g(const WgradArgs& a, const WgBlock& k, int b, int y0, int x0, int gx0, int gx1, int lo = 0, int hi = P::NG) {
    const WgSampleRsrc<ES> rs(a, k, b);
#pragma unroll
    for (int i = 0; i < P::NG; ++i) {
      if (i < lo || i >= hi) continue;
      const int pix = pix0 + i * P::PSTEP;
      const int y = y0 + pix / 32, x = x0 + pix % 32;
      const bool ok = y < a.H && x >= gx0 && x < gx1;
      const int e0 = ok ? ((y >> k.gsh) * k.Wg + (x >> k.gsh)) * a.Cout + k.co0 + part * P::EPL : WG_OOB;
      gr[i] = __builtin_amdgcn_raw_buffer_load_b128(rs.rg, ok ? e0 * ES : WG_OOB, 0, 0);
      gid[i] = P::load_idx(rs.ri, e0);
    }
  }
};

// The steps of a k-slice: whole tiles (TH == WG_TH), or a tile's two halves of TH = WG_TH / 2 rows -- (tile, half 0), (tile,
// half 1), next tile; the lower half of a tile at the image's last rows may be empty and is skipped.  -1 ends the walk.  Both
// roles of a wave-specialised kernel step through it identically (they meet at one barrier per step).
template <int TH>
struct WgWalk {
  static constexpr int PER = WG_TH / TH;
  static_assert(PER == 1 || PER == 2, "whole or half tiles");
  const WgTiles tl;
  const int KS, H, n;
  __device__ __forceinline__ WgWalk(const WgradArgs& a, const WgBlock& k) : tl(k.tiles(a)), KS(a.KS), H(a.H), n(PER * tl.ntile) {}
  __device__ __forceinline__ int first(int ks) const { return PER * ks < n ? PER * ks : -1; }    // (the upper half of a listed tile is never empty)
  __device__ __forceinline__ void origin(int s, int& b, int& y0, int& x0, int& gx0, int& gx1) const {
    tl.origin(s / PER, b, y0, x0, gx0, gx1);
    y0 += (s % PER) * TH;
  }
  __device__ __forceinline__ int next(int s) const {
    if constexpr (PER == 1) {
      s += KS;
      return s < n ? s : -1;
    } else {
      for (;;) {                                             // the next non-empty half tile after s
        s += (s & 1) ? 2 * KS - 1 : 1;
        if (s >= n) return -1;
        int b, y0, x0, g0, g1;
        origin(s, b, y0, x0, g0, g1);
        if (y0 < H) return s;
      }
    }
  }
};

// The loader role of the wave-specialised kernels (waves 4-7): global -> registers, two steps of the walk in flight -> the idle
// one of the two LDS buffers (`commit`: the kernel's way of writing a Stage into buffer 0 / 1).
// A piece's place in the tile is fixed for the thread's life: its halo row / column (hy, hx) and, relative to the tile's origin,
// the COLUMN part of its byte offset in the source map (the origin's column is a multiple of 32 and splits off exactly, also
// through the nearest-upsample shift; its row may be odd and does not).  Per step a piece then costs a shift-multiply-add, the
// bounds compares and a select.
template <int ES, int TH>
struct WgWsLoader : WgPieces<ES, TH> {
  typedef WgPieces<ES, TH> P;
  struct Stage { wg_u32x4 xr[P::NX]; wg_u32x4 gr[P::NG]; typename P::Idx gid[P::NG]; int ypar, xpar; };
  const WgradArgs& a;
  const WgBlock& k;
  const WgWalk<TH>& walk;
  int part, pix0, xrel[P::NX], xhyx[P::NX], grel[P::NG];
  __device__ __forceinline__ WgWsLoader(const WgradArgs& a_, const WgBlock& k_, const WgWalk<TH>& walk_, int t)
      : a(a_), k(k_), walk(walk_), part(t % P::PPX), pix0(t / P::PPX) {
#pragma unroll
    for (int i = 0; i < P::NX; ++i) {
      const int pix = pix0 + i * P::PSTEP, hy = pix / HWID, hx = pix - hy * HWID;
      xhyx[i] = pix < P::XPIX ? (hy << 8) | hx : (200 << 8);                          // (a row no image has: never valid)
      xrel[i] = (((hx - 1) >> k.sh) * k.Cs + k.coff + part * P::EPL) * ES;      // column part (arithmetic shift: floor; x0 is a multiple of 32)
    }
#pragma unroll
    for (int i = 0; i < P::NG; ++i) {
      const int pix = pix0 + i * P::PSTEP;
      grel[i] = (((pix / 32) >> k.gsh) * k.Wg + ((pix % 32) >> k.gsh)) * a.Cout + k.co0 + part * P::EPL;
    }
  }
  // Every load is issued unconditionally (a step that does not exist, s < 0, gets out-of-range offsets everywhere and reads
  // zeros): straight-line code, so the compiler can COUNT the loads in flight and wait for one stage while the next one's are
  // still outstanding.  (A branch around the loads makes the wait a vmcnt(0).)
  __device__ __forceinline__ void issue(int s, Stage& S) const {
    int b = 0, x0 = 0, gx0 = 0, gx1 = 0, y0 = 0;
    const bool live = s >= 0;
    if (live) walk.origin(s, b, y0, x0, gx0, gx1);
    S.ypar = y0; S.xpar = x0;
    const WgSampleRsrc<ES> rs(a, k, b);
    // uniform: the tile origin's offset and the valid ranges of hy / hx (input halo) and of the gradient tile's rows / columns.
    // Source row of halo row hy: (y0 - 1 + hy) >> sh = ((y0 - 1) >> sh) + ((hy + ((y0 - 1) & sh)) >> sh) -- the static first row of
    // a trimmed ground launch may be odd, so the tile origin's parity under the upsample shift is carried (ypar); columns split
    // off exactly (x0 is a multiple of 32), and so does the unpool shift (y0 is even where g is the pooled map's gradient)
    const int sh = k.sh, gsh = k.gsh;
    const int ylo = y0 - 1, ypar = ylo & sh, rowb = k.Ws * k.Cs * ES;
    const int xbase = __builtin_amdgcn_readfirstlane(((ylo >> sh) * k.Ws + (x0 >> sh)) * k.Cs * ES);
    const int gbase = __builtin_amdgcn_readfirstlane(((y0 >> gsh) * k.Wg + (x0 >> gsh)) * a.Cout);
    const int hy_lo = live ? max(0, 1 - y0) : 255, hy_hi = a.H - y0 + 1, hx_lo = max(0, 1 - x0), hx_hi = a.W - x0 + 1;
    const int gy_hi = live ? a.H - y0 : 0, gx_lo = gx0 - x0, gx_hi = gx1 - x0;
#pragma unroll
    for (int i = 0; i < P::NX; ++i) {                  // input halo tile, zero outside the image
      const int hy = xhyx[i] >> 8, hx = xhyx[i] & 255;
      const bool ok = hy >= hy_lo && hy < hy_hi && hx >= hx_lo && hx < hx_hi;
      S.xr[i] = __builtin_amdgcn_raw_buffer_load_b128(rs.rx, ok ? xbase + ((hy + ypar) >> sh) * rowb + xrel[i] : WG_OOB, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < P::NG; ++i) {                  // output-gradient tile (virtual unpool: + the forward argmax)
      const int pix = pix0 + i * P::PSTEP, py = pix / 32, px = pix % 32;
      const bool ok = py < gy_hi && px >= gx_lo && px < gx_hi;
      const int e0 = ok ? gbase + grel[i] : WG_OOB;
      S.gr[i] = __builtin_amdgcn_raw_buffer_load_b128(rs.rg, ok ? e0 * ES : WG_OOB, 0, 0);
      S.gid[i] = P::load_idx(rs.ri, e0);
    }
  }
  // position (2 * (y & 1) + (x & 1)) of piece i's pixel inside its 2 x 2 pool window
  __device__ __forceinline__ unsigned pool_pos(const Stage& S, int i) const {
    const int pix = pix0 + i * P::PSTEP;
    return (((S.ypar + pix / 32) & 1) << 1) | ((S.xpar + pix % 32) & 1);
  }
  template <typename Commit>
  __device__ __forceinline__ void run(int s_first, Commit commit) const {
    Stage A, Bq;
    int ta = s_first, tb = ta >= 0 ? walk.next(ta) : -1;
    issue(ta, A);
    issue(tb, Bq);
    commit(A, 0);
    __syncthreads();                                     // barrier 0: buffer 0 holds the first step
    int cur = 0;
    // at the top: the matrix waves work on step `ta` in buffer `cur`; Bq holds (in flight) the loads of `tb`; A is free
    while (ta >= 0) {
      int tc = tb >= 0 ? walk.next(tb) : -1;
      issue(tc, A);
      commit(Bq, cur ^ 1);
      __syncthreads();
      ta = tb; tb = tc; cur ^= 1;
      if (ta < 0) break;
      tc = tb >= 0 ? walk.next(tb) : -1;
      issue(tc, Bq);
      commit(A, cur ^ 1);
      __syncthreads();
      ta = tb; tb = tc; cur ^= 1;
    }
  }
};

template <typename T> constexpr int wg_stride() { return 64 * (int)sizeof(T) + 16; }
template <typename T> constexpr int wg_lds_bytes() { return ((WG_TH + 2) * HWID + WG_TH * 32) * wg_stride<T>(); }   // one tile: X halo + G
template <typename T> constexpr int wg_ws_lds_bytes() { return 2 * wg_lds_bytes<T>(); }                             // two buffers

// ---------------------------------------------------------------------------------------------
// wgrad_kernel: two-phase.  Every wave loads, then every wave multiplies, with nothing but the co-resident workgroup to overlap
// the phases.  fp32 (parity mode) runs on it; for the 16-bit types it is the fallback (a device that refuses wgrad_ws_kernel's
// LDS) and the tests' reference (HLA_VGG_BWD_WGRAD_TWO_PHASE).
template <typename T>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(WgradArgs a) {
  typedef WgStagedTile<(int)sizeof(T), WG_TH> Ld;
  constexpr int STR = wg_stride<T>(), NX = Ld::NX, NG = Ld::NG, XPIX = Ld::XPIX, KPX = KStep<T>::PX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Xs = smem;
  char* Gs = smem + XPIX * STR;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, ct = wv >> 1, it = wv & 1;
  const WgBlock k(a);
  const bool want_bias = k.want_bias(a, it);
  WgAcc acc;
  const uint4 ones = frag_ones<T>();

  // Register-staged tile loads.  (Issuing the NEXT tile's requests before the current tile's MFMA phase needs the staging
  // registers live across it: one workgroup per CU, measured slower.)
  Ld ld(t);
  const WgTiles tl = k.tiles(a);
  // (the origin is derived again wherever it is needed rather than kept: fp32 sits at 256 registers, and values held across the
  //  barrier cost it two more spills)
  auto load_x = [&](int tile, int lo, int hi) {
    int b, y0, x0, gx0, gx1;
    tl.origin(tile, b, y0, x0, gx0, gx1);
    ld.load_x(a, k, b, y0, x0, lo, hi);
  };
  auto load_g = [&](int tile, int lo, int hi) {
    int b, y0, x0, gx0, gx1;
    tl.origin(tile, b, y0, x0, gx0, gx1);
    ld.load_g(a, k, b, y0, x0, gx0, gx1, lo, hi);
  };
  auto store_x = [&](int lo, int hi) {
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      if (i < lo || i >= hi) continue;
      const int pix = ld.pix0 + i * Ld::PSTEP;
      if (pix < XPIX) *(wg_u32x4*)(Xs + pix * STR + ld.part * 16) = ld.xr[i];
    }
  };
  auto store_g = [&](int tile, int lo, int hi) {
    int b, y0, x0, gx0, gx1;
    tl.origin(tile, b, y0, x0, gx0, gx1);
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      if (i < lo || i >= hi) continue;
      const int pix = ld.pix0 + i * Ld::PSTEP;
      wg_u32x4 v = ld.gr[i];
      if (a.g_unpool) wg_unpool_mask_generic<T>(v, ld.gid[i], (((y0 + pix / 32) & 1) << 1) | ((x0 + pix % 32) & 1));
      *(wg_u32x4*)(Gs + pix * STR + ld.part * 16) = v;
    }
  };

  for (int tile = k.ks; tile < tl.ntile; tile += a.KS) {
    if (sizeof(T) == 2) {
      load_x(tile, 0, NX); load_g(tile, 0, NG);
      __syncthreads();                                 // previous tile fully consumed
      store_x(0, NX);
      store_g(tile, 0, NG);
    } else {                                           // fp32 (parity mode): batches of 4 pieces = 16 staging registers
      __syncthreads();
#pragma unroll
      for (int lo = 0; lo < NX; lo += 4) { load_x(tile, lo, lo + 4); store_x(lo, lo + 4); }
#pragma unroll
      for (int lo = 0; lo < NG; lo += 4) { load_g(tile, lo, lo + 4); store_g(tile, lo, lo + 4); }
    }
    __syncthreads();
    // G fragments of the whole tile stay in registers; every X fragment (halo row rho, column shift kx, K-step kk) is
    // fetched ONCE and feeds the up to three taps ky with r = rho - ky inside the tile  (halves the LDS reads per MFMA)
    // (K-steps are taken two at a time so that the resident G fragments cost 32 VGPRs for every dtype)
#pragma unroll 1
    for (int kk0 = 0; kk0 < 32 / KPX; kk0 += 2) {
      uint4 Af[2][WG_TH];
#pragma unroll
      for (int r = 0; r < WG_TH; ++r)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          Af[kk][r] = frag_kmajor<T>(Gs, STR, r * 32 + (kk0 + kk) * KPX, ct * 32, lane);
          if (want_bias) mma16<T>(acc.accb, Af[kk][r], ones);
        }
#pragma unroll
      for (int rho = 0; rho < WG_TH + 2; ++rho) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const uint4 Bf = frag_kmajor<T>(Xs, STR, rho * HWID + kx + (kk0 + kk) * KPX, it * 32, lane);
            wg_taps<T, WG_TH>(acc.acc, rho, kx, Af[kk], Bf);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  acc.store(a, k, ct, it, lane, want_bias);
}

// ---------------------------------------------------------------------------------------------
// wgrad_ws_kernel: the 16-bit weight gradient, WAVE-SPECIALISED (round 5; the split-mode twin is wgrad_split_ws_kernel below, which
// explains the scheme).  One 8-wave workgroup per CU: waves 4-7 fetch a 4-row tile's pieces two tiles ahead through registers
// (raw buffer loads, zero fill by the descriptors' range check, the virtual unpool's argmax mask applied on the way into LDS) and
// write them into the idle one of two LDS buffers; waves 0-3 -- one per SIMD -- only read fragments and multiply, the next halo
// row's fragments requested ahead of the current row's MFMAs.  One barrier per tile.  Plain AND un-pooling launches (the two-phase
// kernels run load -> barrier -> MFMA phases in every wave: 0.30 of the MFMA peak where the forward reaches 0.48).
template <typename T>
__global__ __launch_bounds__(512, 1) void wgrad_ws_kernel(WgradArgs a) {
  static_assert(sizeof(T) == 2, "16-bit types");
  typedef WgWsLoader<2, WG_TH> Ld;
  constexpr int STR = wg_stride<T>(), KPX = 16, BUFB = wg_lds_bytes<T>();
  constexpr int oX = 0, oG = Ld::XPIX * STR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const WgBlock k(a);
  const WgWalk<WG_TH> walk(a, k);
  const int t_first = walk.first(k.ks);

  if (wv >= 4) {                                         // ---------------- loader waves
    const Ld ld(a, k, walk, t - 256);
    ld.run(t_first, [&](const typename Ld::Stage& S, int buf) __attribute__((always_inline)) {
      char* base = smem + buf * BUFB;
#pragma unroll
      for (int i = 0; i < Ld::NX; ++i) {
        const int pix = ld.pix0 + i * Ld::PSTEP;
        if (pix < Ld::XPIX) *(wg_u32x4*)(base + oX + pix * STR + ld.part * 16) = S.xr[i];
      }
#pragma unroll
      for (int i = 0; i < Ld::NG; ++i) {
        const int pix = ld.pix0 + i * Ld::PSTEP;
        wg_u32x4 v = S.gr[i];
        if (a.g_unpool) wg_unpool_mask_perm(v, S.gid[i], ld.pool_pos(S, i));
        *(wg_u32x4*)(base + oG + pix * STR + ld.part * 16) = v;
      }
    });
    return;
  }

  // ---------------- matrix waves
  const int ct = wv >> 1, it = wv & 1;
  const bool want_bias = k.want_bias(a, it);
  WgAcc acc;
  const uint4 ones = frag_ones<T>();
  __syncthreads();                                       // barrier 0
  int cur = 0;
  for (int tile = t_first; tile >= 0; tile = walk.next(tile)) {
    const char* Xs = smem + cur * BUFB + oX;
    const char* Gs = smem + cur * BUFB + oG;
    // the G fragments of the whole tile (4 rows x 2 K-steps) stay in registers; halo row rho's X fragments (3 column shifts x 2
    // K-steps) are requested one row ahead of the MFMAs that consume them and feed the up to three taps ky with r = rho - ky
    uint4 Af[2][WG_TH], Bf[2][3][2];
#pragma unroll
    for (int r = 0; r < WG_TH; ++r)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) Af[kk][r] = frag_kmajor<T>(Gs, STR, r * 32 + kk * KPX, ct * 32, lane);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) Bf[0][kx][kk] = frag_kmajor<T>(Xs, STR, kx + kk * KPX, it * 32, lane);
#pragma unroll
    for (int rho = 0; rho < WG_TH + 2; ++rho) {
      if (rho + 1 < WG_TH + 2) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) Bf[(rho + 1) & 1][kx][kk] = frag_kmajor<T>(Xs, STR, (rho + 1) * HWID + kx + kk * KPX, it * 32, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (rho == 0 && want_bias) {
#pragma unroll
        for (int r = 0; r < WG_TH; ++r)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) mma16<T>(acc.accb, Af[kk][r], ones);
      }
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) wg_taps<T, WG_TH>(acc.acc, rho, kx, Af[kk], Bf[rho & 1][kx][kk]);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                     // the loaders have filled the other buffer; this one is free
    cur ^= 1;
  }
  acc.store(a, k, ct, it, lane, want_bias);
}

// ---------------------------------------------------------------------------------------------
// Split-fp16 weight gradient (precision 'fp16x3'): the same contraction over pixels with both operands fed to the matrix cores
// as hi + lo = fp16(s v) + fp16(s v - hi): G X ~= Ghi Xhi + Glo Xhi + Ghi Xlo, three v_mfma_f32_32x32x16_f16 per product, fp32
// accumulate -- fp32-class gradients at a third of the fp16 MFMA rate instead of the exact-fp32 kernels' sixteenth.
// Storage stays fp32 (the maps a split-mode forward / backward keep); a tile's 16-B pieces are split where they enter LDS, into
// an fp16 hi plane and an fp16 lo plane per operand, each laid out like the f16 kernel's tile, so the k-major fragments come
// from the same transpose reads.  Scales: ONE power of two per operand for the whole launch, from the maximum over the batch
// of the per-sample maxima their producers recorded (the gradient is a sum over the batch, so a batch-wide scale costs no
// accuracy where it matters: elements below 2^-17 of the batch maximum keep an absolute error of 2^-39 of it); exact to undo.
// (The kernels are templates on the plane type H = f16 so that only the translation unit that launches them compiles them.)
struct WgradSplitExtra {
  const unsigned* amax_x1; const unsigned* amax_x2; const unsigned* amax_g;   // [B] fp32 bit patterns of max |.| per sample
};
constexpr int WGS_STR = 64 * 2 + 16;                       // fp16 plane row stride (as wg_stride<f16>)
// A tile of the (shared) tile lists is WG_TH = 4 rows x 32 pixels; with two fp16 planes per operand that is 96 KB of LDS and one
// workgroup per CU, whose load and MFMA phases then run strictly one after the other (measured: 1.9 ms per launch, 6x the bf16
// kernel for 3x its MFMAs).  The tile is therefore walked as two HALVES of WGS_TH = 2 rows: 58 KB, two workgroups per CU.
constexpr int WGS_TH = 2;
constexpr int wgs_lds_bytes() { return 2 * ((WGS_TH + 2) * HWID + WGS_TH * 32) * WGS_STR; }      // one half tile: {Xh, Xl, Gh, Gl}
constexpr int wgs_ws_lds_bytes() { return 2 * wgs_lds_bytes(); }                                 // two buffers

// launch-wide scales (uniform)
__device__ __forceinline__ void wgs_scales(const WgradArgs& a, const WgradSplitExtra& sx, bool first, float& s_x, float& s_g) {
  unsigned mx = 0, mg = 0;
  const unsigned* ax = first ? sx.amax_x1 : sx.amax_x2;
  for (int b = 0; b < a.B; ++b) { mx = max(mx, ax[b]); mg = max(mg, sx.amax_g[b]); }
  s_x = split_scale(mx); s_g = split_scale(mg);
}
// a piece of four fp32 values, scaled, as hi and lo fp16 quads
__device__ __forceinline__ void wgs_split_piece(const wg_u32x4& v, float s, uint2& hi, uint2& lw) {
  split4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w), s, hi, lw);
}
// a piece of g: the virtual unpool's mask (pos: the pixel's place in its pool window), then the split
__device__ __forceinline__ void wgs_split_g_piece(const WgradArgs& a, const wg_u32x4& v, unsigned idx, unsigned pos, float s, uint2& hi, uint2& lw) {
  float e0 = __uint_as_float(v.x), e1 = __uint_as_float(v.y), e2 = __uint_as_float(v.z), e3 = __uint_as_float(v.w);
  if (a.g_unpool) wg_unpool_mask_bytes(e0, e1, e2, e3, idx, pos);
  split4(e0, e1, e2, e3, s, hi, lw);
}

template <typename H>
__global__ __launch_bounds__(256, 2) void wgrad_split_kernel(WgradArgs a, WgradSplitExtra sx) {
  typedef WgStagedTile<4, WGS_TH> Ld;                      // 16-B fp32 pieces, 16 per pixel (64 channels)
  constexpr int STR = WGS_STR, XPIX = Ld::XPIX, GPIX = Ld::GPIX, KPX = 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Xh = smem;
  char* Xl = Xh + XPIX * STR;
  char* Gh = Xl + XPIX * STR;
  char* Gl = Gh + GPIX * STR;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, ct = wv >> 1, it = wv & 1;
  const WgBlock k(a);
  const bool want_bias = k.want_bias(a, it);
  float s_x, s_g;
  wgs_scales(a, sx, k.first, s_x, s_g);
  WgAcc acc;
  const uint4 ones = frag_ones<H>();

  const WgTiles tl = k.tiles(a);
  for (int tile2 = 2 * k.ks; tile2 < 2 * tl.ntile; tile2 += (tile2 & 1) ? 2 * a.KS - 1 : 1) {      // (tile, half 0), (tile, half 1), next tile
    int b, y0, x0, gx0, gx1;
    tl.origin(tile2 >> 1, b, y0, x0, gx0, gx1);
    y0 += (tile2 & 1) * WGS_TH;
    if (y0 >= a.H) continue;                           // (uniform: the lower half of a tile at the image's last rows)
    Ld ld(t);                                          // a half tile's 13 (+ 4 argmax) loads, all in flight together
    ld.load_x(a, k, b, y0, x0);
    ld.load_g(a, k, b, y0, x0, gx0, gx1);
    __syncthreads();                                   // previous half tile fully consumed (the loads above are in flight across it)
#pragma unroll
    for (int i = 0; i < Ld::NX; ++i) {
      const int pix = ld.pix0 + i * Ld::PSTEP;
      uint2 hi, lw;
      wgs_split_piece(ld.xr[i], s_x, hi, lw);
      if (pix < XPIX) { *(uint2*)(Xh + pix * STR + ld.part * 8) = hi; *(uint2*)(Xl + pix * STR + ld.part * 8) = lw; }
    }
#pragma unroll
    for (int i = 0; i < Ld::NG; ++i) {
      const int pix = ld.pix0 + i * Ld::PSTEP;
      uint2 hi, lw;
      wgs_split_g_piece(a, ld.gr[i], ld.gid[i], (((y0 + pix / 32) & 1) << 1) | ((x0 + pix % 32) & 1), s_g, hi, lw);
      *(uint2*)(Gh + pix * STR + ld.part * 8) = hi; *(uint2*)(Gl + pix * STR + ld.part * 8) = lw;
    }
    __syncthreads();
    // one K-step (16 pixels) at a time: the G fragments of the half tile's rows (hi and lo) stay resident while
    // every X fragment (halo row rho, column shift kx) is fetched once and feeds the up to three taps ky that use it
#pragma unroll 1
    for (int kk = 0; kk < 32 / KPX; ++kk) {
      uint4 Ah[WGS_TH], Al[WGS_TH];
#pragma unroll
      for (int r = 0; r < WGS_TH; ++r) {
        Ah[r] = frag_kmajor<H>(Gh, STR, r * 32 + kk * KPX, ct * 32, lane);
        Al[r] = frag_kmajor<H>(Gl, STR, r * 32 + kk * KPX, ct * 32, lane);
        if (want_bias) { mma16<H>(acc.accb, Ah[r], ones); mma16<H>(acc.accb, Al[r], ones); }
      }
#pragma unroll
      for (int rho = 0; rho < WGS_TH + 2; ++rho) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const uint4 Bh = frag_kmajor<H>(Xh, STR, rho * HWID + kx + kk * KPX, it * 32, lane);
          const uint4 Bl = frag_kmajor<H>(Xl, STR, rho * HWID + kx + kk * KPX, it * 32, lane);
          wg_taps<H, WGS_TH>(acc.acc, rho, kx, Ah, Al, Bh, Bl);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  acc.store(a, k, ct, it, lane, want_bias, 1.f / (s_x * s_g), 1.f / s_g);
}

// ---------------------------------------------------------------------------------------------
// wgrad_split_ws_kernel: the same contraction, WAVE-SPECIALISED (round 5).  wgrad_split_kernel runs load -> split -> barrier ->
// MFMA in every wave, with nothing but the second resident workgroup to overlap the phases: 0.47 of its MFMA ceiling where the
// forward kernels reach 0.55.  Here a workgroup is EIGHT waves on one CU: waves 4-7 are LOADERS (they fetch a half tile's fp32
// pieces two half tiles ahead, split them into the fp16 hi / lo planes and write them into the idle LDS buffer -- the ~400 VALU
// instructions per half tile that used to sit between two MFMA phases), waves 0-3 are the MATRIX waves (one per SIMD: transposing
// LDS reads and MFMAs only, fragments requested one halo row ahead of the MFMAs that consume them).  A matrix wave and a loader
// share each SIMD, so the split's VALU work and the global-load latency run under the MFMAs instead of between them.  One
// workgroup barrier per half tile; LDS: two buffers of {Xh, Xl, Gh, Gl} = 115 KB, one workgroup per CU, 256 registers per wave.
// Same tile lists, same order of every partial sum's terms as wgrad_split_kernel (bit-identical partials for the same KS).
template <typename H>
__global__ __launch_bounds__(512, 1) void wgrad_split_ws_kernel(WgradArgs a, WgradSplitExtra sx) {
  typedef WgWsLoader<4, WGS_TH> Ld;                        // 16-B fp32 pieces, 16 per pixel (64 channels)
  constexpr int STR = WGS_STR, XPIX = Ld::XPIX, GPIX = Ld::GPIX, KPX = 16, BUFB = wgs_lds_bytes();
  constexpr int oXh = 0, oXl = XPIX * STR, oGh = 2 * XPIX * STR, oGl = 2 * XPIX * STR + GPIX * STR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const WgBlock k(a);
  const WgWalk<WGS_TH> walk(a, k);
  const int t_first = walk.first(k.ks);
  float s_x, s_g;

  if (wv >= 4) {                                           // wave-uniform role
    // ---------------- loader waves: global -> registers (two half tiles in flight) -> split -> LDS planes of the idle buffer
    wgs_scales(a, sx, k.first, s_x, s_g);
    const Ld ld(a, k, walk, t - 256);
    ld.run(t_first, [&](const typename Ld::Stage& S, int buf) __attribute__((always_inline)) {
      char* base = smem + buf * BUFB;
#pragma unroll
      for (int i = 0; i < Ld::NX; ++i) {
        const int pix = ld.pix0 + i * Ld::PSTEP;
        uint2 hi, lw;
        wgs_split_piece(S.xr[i], s_x, hi, lw);
        if (pix < XPIX) { *(uint2*)(base + oXh + pix * STR + ld.part * 8) = hi; *(uint2*)(base + oXl + pix * STR + ld.part * 8) = lw; }
      }
#pragma unroll
      for (int i = 0; i < Ld::NG; ++i) {
        const int pix = ld.pix0 + i * Ld::PSTEP;
        uint2 hi, lw;
        wgs_split_g_piece(a, S.gr[i], S.gid[i], ld.pool_pos(S, i), s_g, hi, lw);
        *(uint2*)(base + oGh + pix * STR + ld.part * 8) = hi; *(uint2*)(base + oGl + pix * STR + ld.part * 8) = lw;
      }
    });
    return;
  }

  // ---------------- matrix waves
  const int ct = wv >> 1, it = wv & 1;
  const bool want_bias = k.want_bias(a, it);
  wgs_scales(a, sx, k.first, s_x, s_g);
  WgAcc acc;
  const uint4 ones = frag_ones<H>();
  __syncthreads();                                       // barrier 0
  int cur = 0;
  for (int t2 = t_first; t2 >= 0; t2 = walk.next(t2)) {
    const char* base = smem + cur * BUFB;
    const char *Xh = base + oXh, *Xl = base + oXl, *Gh = base + oGh, *Gl = base + oGl;
    // A flat walk over the half tile's 8 steps (K-step kk = 16 pixels, halo row rho): the G fragments of a K-step (two rows, hi and
    // lo) stay resident while its four halo rows pass; the X fragments of step s + 1 -- and, in a K-step's last row, the G
    // fragments of the next one -- are REQUESTED AT THE TOP of step s, ahead of its 9-18 MFMAs (this wave has the SIMD's matrix pipe
    // to itself: nothing else covers the LDS latency; left to the scheduler the requests sank to just before the step's last MFMA
    // and every step started with an LDS round trip: 0.77 of the pipe with the loaders idle).  A fragment feeds the up to two taps
    // ky that use it.  Term order per accumulator as in wgrad_split_kernel: (hi hi, lo hi, hi lo) per (kk, rho, kx, ky).
    constexpr int NSTEP = (32 / KPX) * (WGS_TH + 2);
    uint4 Ah[2][WGS_TH], Al[2][WGS_TH], Bh[2][3], Bl[2][3];
#pragma unroll
    for (int r = 0; r < WGS_TH; ++r) {
      Ah[0][r] = frag_kmajor<H>(Gh, STR, r * 32, ct * 32, lane);
      Al[0][r] = frag_kmajor<H>(Gl, STR, r * 32, ct * 32, lane);
    }
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      Bh[0][kx] = frag_kmajor<H>(Xh, STR, kx, it * 32, lane);
      Bl[0][kx] = frag_kmajor<H>(Xl, STR, kx, it * 32, lane);
    }
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
      const int kk = st / (WGS_TH + 2), rho = st % (WGS_TH + 2);
      if (st + 1 < NSTEP) {
        const int kn = (st + 1) / (WGS_TH + 2), rn = (st + 1) % (WGS_TH + 2);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          Bh[(st + 1) & 1][kx] = frag_kmajor<H>(Xh, STR, rn * HWID + kx + kn * KPX, it * 32, lane);
          Bl[(st + 1) & 1][kx] = frag_kmajor<H>(Xl, STR, rn * HWID + kx + kn * KPX, it * 32, lane);
        }
        if (rn == 0) {
#pragma unroll
          for (int r = 0; r < WGS_TH; ++r) {
            Ah[kn & 1][r] = frag_kmajor<H>(Gh, STR, r * 32 + kn * KPX, ct * 32, lane);
            Al[kn & 1][r] = frag_kmajor<H>(Gl, STR, r * 32 + kn * KPX, ct * 32, lane);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (rho == 0 && want_bias) {
#pragma unroll
        for (int r = 0; r < WGS_TH; ++r) { mma16<H>(acc.accb, Ah[kk & 1][r], ones); mma16<H>(acc.accb, Al[kk & 1][r], ones); }
      }
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) wg_taps<H, WGS_TH>(acc.acc, rho, kx, Ah[kk & 1], Al[kk & 1], Bh[st & 1][kx], Bl[st & 1][kx]);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                     // the loaders have filled the other buffer; this one is free
    cur ^= 1;
  }
  acc.store(a, k, ct, it, lane, want_bias, 1.f / (s_x * s_g), 1.f / s_g);
}

// ---------------------------------------------------------------------------------------------
// conv0: dW0[co][k = c*9+tap] over the NCHW fp32 input (k padded to 32 as one "ci tile").
struct Wgrad0Args {
  const float* x;        // [B,3,H,W], channel planes x_plane elements apart
  size_t x_plane;
  const void* g;         // d(loss)/d(conv0 pre-activation) NHWC T [B,H,W,64]
  float* part;           // [KS][2 row-halves][64][32]
  float* bpart;          // [KS][2][64]
  int B, H, W, tiles_x, tiles_y, ntile, KS;
  int row_begin;         // first pixel row that carries gradient
  const int* dyn;        // as WgradArgs::dyn / dyn_desc
  int dyn_desc;
};

template <typename T>
__global__ __launch_bounds__(256) void wgrad0_kernel(Wgrad0Args a) {
  constexpr int EPL = 16 / sizeof(T), STR = wg_stride<T>(), PPX = 64 * (int)sizeof(T) / 16, KPX = KStep<T>::PX;
  constexpr int IW = 48;   // plane row pitch (32 + 2 halo + K-step overrun)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Gs = smem;
  float* in = (float*)(smem + WG_TH * 32 * STR);     // [3][WG_TH+2][IW]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, ct = wv & 1, half = wv >> 1;
  const int ks = blockIdx.x;
  f32x16 acc, accb;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; accb[r] = 0.f; }
  const uint4 ones = frag_ones<T>();
  const int j = lane & 31, g5 = lane >> 5;            // B operand: column j = k index (c, ky, kx)
  const int jc = j < 27 ? j / 9 : 0, jky = (j % 9) / 3, jkx = j % 3;
  const WgTiles tl(a.dyn, a.dyn_desc, a.H, a.W, a.row_begin, a.tiles_x, a.tiles_y, a.ntile, a.B, 0);
  for (int tile = ks; tile < tl.ntile; tile += a.KS) {
    int b, y0, x0, gx0, gx1;
    tl.origin(tile, b, y0, x0, gx0, gx1);
    __syncthreads();
    // (every load of a tile is requested before the first LDS write: as two rolled loops this was 14 dependent
    //  load -> wait -> write round trips per tile against a few microseconds of MFMA work -- the kernel ran at 68 TF)
    constexpr int NI = (3 * (WG_TH + 2) * IW + 255) / 256, NG = WG_TH * 32 * PPX / 256;
    static_assert(WG_TH * 32 * PPX % 256 == 0, "gradient tile pieces per thread");
    float vi[NI];
    uint4 vg[NG];
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const int e = t + it * 256;
      const int c = e / ((WG_TH + 2) * IW), r = e % ((WG_TH + 2) * IW), iy = r / IW, ix = r % IW;
      const int y = y0 - 1 + iy, x = x0 - 1 + ix;
      vi[it] = 0.f;
      if (e < 3 * (WG_TH + 2) * IW && ix < HWID && y >= 0 && y < a.H && x >= 0 && x < a.W)
        vi[it] = a.x[((size_t)b * 3 + c) * a.x_plane + (size_t)y * a.W + x];
    }
#pragma unroll
    for (int it = 0; it < NG; ++it) {
      const int e = t + it * 256;
      const int pix = e / PPX, part = e % PPX;
      const int y = y0 + pix / 32, x = x0 + pix % 32;
      vg[it] = make_uint4(0, 0, 0, 0);
      if (y < a.H && x >= gx0 && x < gx1)
        vg[it] = *(const uint4*)((const T*)a.g + (((size_t)b * a.H + y) * a.W + x) * 64 + part * EPL);
    }
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const int e = t + it * 256;
      if (e < 3 * (WG_TH + 2) * IW) in[e] = vi[it];
    }
#pragma unroll
    for (int it = 0; it < NG; ++it) {
      const int e = t + it * 256;
      *(uint4*)(Gs + (e / PPX) * STR + (e % PPX) * 16) = vg[it];
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < WG_TH / 2; ++rr) {
      const int r = half * (WG_TH / 2) + rr;
#pragma unroll
      for (int kk = 0; kk < 32 / KPX; ++kk) {
        const uint4 A = frag_kmajor<T>(Gs, STR, r * 32 + kk * KPX, ct * 32, lane);
        T e[EPL];
        const float* row = in + (jc * (WG_TH + 2) + r + jky) * IW + jkx + kk * KPX;
#pragma unroll
        for (int jj = 0; jj < EPL; ++jj) {
          // bf16: k = 8*g5 + jj ; fp32: k = 2*jj + g5   (pixel offset inside the K-step, see KStep)
          const int k = sizeof(T) == 2 ? 8 * g5 + jj : 2 * jj + g5;
          e[jj] = (T)(j < 27 ? row[k] : 0.f);
        }
        mma16<T>(acc, A, __builtin_bit_cast(uint4, e));
        mma16<T>(accb, A, ones);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * g5;
    a.part[(((size_t)ks * 2 + half) * 64 + co) * 32 + j] = acc[r];
    if (j == 0) a.bpart[((size_t)ks * 2 + half) * 64 + co] = accb[r];
  }
}
