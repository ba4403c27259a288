// Tile, ring, split and workspace arithmetic of g2s_corr.hip, in plain C++: the kernels include it, and so does the host sweep of
// tests/test_g2s_corr_ref_cpu.py, which walks every index the kernels form (the pattern of conv_block_map.h).
//
// The forward contraction per sample is a GEMM with M = dx, N = dy and K = (satellite row r, x, c):
//   acc[dx][dy] += sum_{r,x,c} s[r, x + dx, c] g[r - dy, x, c]        (g = 0 outside 0 <= r - dy < Hc)
// A workgroup owns one GC_T x GC_T tile of shifts and a range of K COLUMNS, a column being one (x-chunk of GC_XC, c-chunk of GC_CC)
// pair walked over every r of the tile.  Its four waves split a column's GC_XC x positions; each holds one 32x32 accumulator.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define GC_HD __host__ __device__ inline
#else
#define GC_HD inline
#endif

constexpr int GC_T = 32;                              // shifts per tile side (the MFMA's M and N)
constexpr int GC_XC = 16, GC_CC = 16;                 // a K column: 16 x positions by 16 channels
constexpr int GC_WAVES = 4;                           // waves per workgroup; wave w takes x positions 4w .. 4w+3 of the column
constexpr int GC_XW = GC_XC / GC_WAVES;
constexpr int GC_SW = GC_T + GC_XC - 1;               // satellite strip: the columns one r step reads (Toeplitz view)
constexpr int GC_CS = GC_CC + 1;                      // strip column stride in floats (odd: 32 lanes, 32 banks)
constexpr int GC_STRIP_FLOATS = GC_SW * GC_CS;
constexpr int GC_SLOTS = 32;                          // ring of g rows: row y lives in slot y mod 32 while r - dy0 - 31 <= y <= r - dy0
constexpr int GC_RS = GC_XC * GC_CC + 1;              // ring slot stride in floats (odd)
constexpr int GC_RING_FLOATS = GC_SLOTS * GC_RS;
constexpr int GC_LDS_FLOATS = GC_RING_FLOATS + GC_STRIP_FLOATS;
constexpr int GC_STEP_PRODUCTS = GC_XW * GC_CC;       // products one accumulator element collects per r step
constexpr int GC_FLUSH_LIMIT = 4096;                  // products an fp32 accumulator may collect before it goes to fp64
constexpr int GC_FLUSH_STEPS = GC_FLUSH_LIMIT / GC_STEP_PRODUCTS;
constexpr int GC_MAX_SPLITS = 16;                     // workgroups that share a tile's K columns (fixed by the shape, never by B)
constexpr int GC_STRIP_LOADERS = GC_SW * (GC_CC / 4); // threads 0 .. 187 fetch one float4 of the strip each
constexpr int GC_RING_LOADER0 = 192;                  // threads 192 .. 255 fetch one float4 of the new g row each

GC_HD int gc_tiles(int n) { return (n + GC_T - 1) / GC_T; }
GC_HD int gc_xchunks(int Wc) { return (Wc + GC_XC - 1) / GC_XC; }
GC_HD int gc_columns(int Wc, int C) { return gc_xchunks(Wc) * (C / GC_CC); }
GC_HD int gc_cols_per_split(int ncol) { return (ncol + GC_MAX_SPLITS - 1) / GC_MAX_SPLITS; }
GC_HD int gc_splits(int ncol) { const int cps = gc_cols_per_split(ncol); return (ncol + cps - 1) / cps; }
GC_HD int gc_split_begin(int split, int ncol) { return split * gc_cols_per_split(ncol); }
GC_HD int gc_split_end(int split, int ncol) { const int e = (split + 1) * gc_cols_per_split(ncol); return e < ncol ? e : ncol; }
GC_HD int gc_col_x0(int col, int Wc) { return (col % gc_xchunks(Wc)) * GC_XC; }
GC_HD int gc_col_c0(int col, int Wc) { return (col / gc_xchunks(Wc)) * GC_CC; }

// the satellite rows a tile with first shift dy0 walks: [begin, end)
GC_HD int gc_r_begin(int dy0) { return dy0; }
GC_HD int gc_r_end(int dy0, int Ny, int Hc) { const int last = dy0 + GC_T - 1 < Ny - 1 ? dy0 + GC_T - 1 : Ny - 1; return last + Hc; }

GC_HD int gc_ring_slot(int y) { return y & (GC_SLOTS - 1); }               // (two's complement: also for y < 0)
GC_HD int gc_ring_index(int y, int xl, int c) { return gc_ring_slot(y) * GC_RS + xl * GC_CC + c; }
GC_HD int gc_strip_index(int col, int c) { return col * GC_CS + c; }

// element v (0..15) of lane l of the 32x32 accumulator: M index (dx) and N index (dy) within the tile
GC_HD int gc_acc_dx(int v, int lane) { return 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }
GC_HD int gc_acc_dy(int lane) { return lane & 31; }

GC_HD size_t gc_align(size_t x) { return (x + 255) / 256 * 256; }

// byte offsets into the workspace (one size serves the forward and the backward)
struct GcLayout {
  size_t e, eg, h, part;                    // forward: pixel energies of sat [B,A,A] and g2s [B,Hc,Wc], row window sums [B,A,Nx], partials
  size_t kf, kr, beta, hb, coefB, alpha, coefA;   // backward
  size_t total;
  int Ny, Nx, ncol, nsplit;
};

GC_HD GcLayout gc_layout(int B, int A, int Hc, int Wc, int C) {
  GcLayout L{};
  L.Ny = A - Hc + 1;
  L.Nx = A - Wc + 1;
  L.ncol = gc_columns(Wc, C);
  L.nsplit = gc_splits(L.ncol);
  const size_t b = (size_t)B, S = (size_t)L.Ny * L.Nx, AA = (size_t)A * A;
  size_t o = 0;
  L.e = o;     o += gc_align(b * AA * 8);
  L.eg = o;    o += gc_align(b * Hc * Wc * 8);
  L.h = o;     o += gc_align(b * A * L.Nx * 8);
  L.part = o;  o += gc_align(b * L.nsplit * S * 8);
  L.kf = o;    o += gc_align(b * S * 8);
  L.kr = o;    o += gc_align(b * S * 8);
  L.beta = o;  o += gc_align(b * S * 8);
  L.hb = o;    o += gc_align(b * L.Ny * A * 8);
  L.coefB = o; o += gc_align(b * AA * 8);
  L.alpha = o; o += gc_align(b * 2 * 8);
  L.coefA = o; o += gc_align(b * 8);
  L.total = o;
  return L;
}

GC_HD size_t gc_part_index(int b, int split, int dy, int dx, int nsplit, int Ny, int Nx) {
  return (((size_t)b * nsplit + split) * Ny + dy) * Nx + dx;
}
