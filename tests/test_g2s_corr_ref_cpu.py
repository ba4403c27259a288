"""``LM_G2SP.corr`` without a GPU: the CPU restatement (tests/g2s_corr_ref.py) against plain loops, the crop plan and the loss's
index rule, the package's surface (method, exported symbols, crop_plan), and a host sweep of the forward kernel's tile, ring, split
and workspace arithmetic (highlyaccurate_amd/csrc/g2s_corr_tile.h is plain C++: a stand-alone program includes the very functions
the kernel calls and walks every index it would form)."""
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

import g2s_corr_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'highlyaccurate_amd', 'csrc')
F64 = torch.float64


def test_crop_plan_kitti_and_the_small_fixture():
    # KITTI: 512-pixel satellite image, ranges 20 m / 20 m
    assert [GR.crop_plan(A, l, 20.0, 20.0) for l, A in enumerate((64, 128, 256))] == [(38, 38, 13, 13), (76, 76, 26, 26), (153, 153, 52, 52)]
    # 128-pixel image, ranges 4 m / 6 m: offsets 10 from 10.5 at level 2 (half to even)
    plans = [GR.crop_plan(A, l, 4.0, 6.0) for l, A in enumerate((16, 32, 64))]
    assert [p[:2] for p in plans] == [(10, 8), (21, 16), (43, 33)]
    assert [p[2:] for p in plans] == [(3, 4), (6, 8), (10, 16)]
    assert [(A - p[0] + 1, A - p[1] + 1) for A, p in zip((16, 32, 64), plans)] == [(7, 9), (12, 17), (22, 32)]
    with pytest.raises(ValueError):
        GR.crop_plan(16, 0, 20.0, 20.0)


def test_restatement_equals_four_nested_loops():
    g = torch.Generator().manual_seed(3)
    B, C, A, Hc, Wc = 2, 2, 6, 3, 4
    s = torch.randn(B, C, A, A, generator=g, dtype=F64)
    s = s / s.reshape(B, -1).norm(dim=1).view(B, 1, 1, 1)
    f = torch.randn(B, C, Hc, Wc, generator=g, dtype=F64)
    want = GR.corr_loops(s, f)
    for safe in (False, True):
        got, dot, E = GR.corr_from_crop(s, f, safe)
        assert tuple(got.shape) == (B, A - Hc + 1, A - Wc + 1)
        assert (got - want).abs().max() < 1e-12
    # a zero satellite map: corr == 2 exactly, and the safe clamp keeps autograd finite with no gradient through E
    z = torch.zeros(1, C, A, A, dtype=F64, requires_grad=True)
    c, _, _ = GR.corr_from_crop(z, f[:1], True)
    assert (c == 2).all()
    c.sum().backward()
    assert torch.isfinite(z.grad).all()


def test_index_rule_half_to_even_wrap_and_nan():
    mpp = 0.5
    one = lambda u, v, Ny=9, Nx=8: GR.gt_index(torch.tensor([u]), torch.tensor([v]), 1.0, 1.0, mpp, Ny, Nx)[0]
    assert one(0.0, 0.0) == (4, 4)                       # round(4.5) = 4 (half to even), round(4.0) = 4
    assert one(0.25, -0.5) == (6, 4)                     # h = round(4.5 + 1) = round(5.5) = 6,  w = round(4 + 0.5) = 4
    assert one(0.75, 0.0) == (4, 6)                      # w = round(5.5) = 6
    assert one(-2.5, 3.0) == (7, 7)                      # w = -1 -> 7,  h = round(-1.5) = -2 -> 7
    assert one(-6.0, 0.0) == (4, 0)                      # w = -8 = -Nx: still a Python index
    assert one(-6.5, 0.0) is None and one(2.0, 0.0) is None and one(0.0, -2.5) is None       # w = -9; w = 8; h = 9.5 -> 10
    corr = torch.rand(2, 9, 8, dtype=F64)
    ok = GR.triplet_level(corr, torch.tensor([[0.0], [0.25]]), torch.tensor([[0.0], [-0.5]]), 1.0, 1.0, mpp)
    pos = torch.stack([corr[0, 4, 4], corr[1, 6, 4]]).view(2, 1, 1)
    assert abs(float(ok) - float(torch.log(1 + torch.exp(10 * (pos - corr))).sum() / (2 * 71))) < 1e-12
    assert math.isnan(float(GR.triplet_level(corr, torch.tensor([[0.0], [2.0]]), torch.tensor([[0.0], [0.0]]), 1.0, 1.0, mpp)))


def test_package_surface_and_crop_plan():
    from highlyaccurate_amd import _g2s_corr, _lib
    from highlyaccurate_amd.models_kitti import LM_G2SP
    assert hasattr(LM_G2SP, 'corr')
    lib = _lib.load()
    for name in ('hla_g2s_corr_workspace_bytes', 'hla_g2s_corr', 'hla_g2s_corr_bwd', 'hla_g2s_corr_triplet_loss',
                 'hla_g2s_corr_triplet_loss_bwd', 'hla_grid_sample', 'hla_orien_window_bwd'):
        assert getattr(lib, name).argtypes is not None, name
    assert abs(_g2s_corr.level_mpp(1) - GR.level_mpp(1)) < 1e-15
    for lat, lon in ((20.0, 20.0), (4.0, 6.0), (0.0, 0.0), (1.3, 7.9), (12.5, 3.1)):
        a = SimpleNamespace(shift_range_lat=lat, shift_range_lon=lon)
        for level in range(4):
            for A in range(8, 257):
                try:
                    want = GR.crop_plan(A, level, lat, lon)
                except ValueError:
                    with pytest.raises(ValueError, match='too large'):
                        _g2s_corr.crop_plan(A, level, a)
                    continue
                assert _g2s_corr.crop_plan(A, level, a) == want, (A, level, lat, lon)
    # sizes that are refused come back as 0 with a message, not a crash (no GPU is touched)
    assert lib.hla_g2s_corr_workspace_bytes(2, 32, 8, 8, 32) == 0 and b'channel' in lib.hla_last_error()
    assert lib.hla_g2s_corr_workspace_bytes(2, 32, 33, 8, 64) == 0 and b'crop' in lib.hla_last_error()
    assert lib.hla_g2s_corr_workspace_bytes(1, 256, 153, 153, 64) > 0


def test_zero_pose_grid_is_the_oracles_uv_of_the_crop():
    """``zero_pose_grid`` (the package's own fp64 restatement, on the CPU here) against oracle.ref_cpu.g2s_pose_to_uv in fp64."""
    from highlyaccurate_amd import _g2s_corr
    from oracle import ref_cpu as O
    from test_g2s_pose_search_gpu import CAMERA_K, GRD_HW
    K = torch.tensor(CAMERA_K, dtype=torch.float32)
    args = O.default_args(shift_range_lat=4.0, shift_range_lon=6.0, rotation_range=10.0)
    z = torch.zeros(K.shape[0], 1, dtype=F64)
    for level, (A, hw) in enumerate(((16, (8, 32)), (32, (16, 64)), (64, (32, 128)))):
        plan = Hc, Wc, top, left = _g2s_corr.crop_plan(A, level, args)
        got = _g2s_corr.zero_pose_grid(K, A, hw, GRD_HW, plan)
        uv, _, _ = O.g2s_pose_to_uv(args, A, z, z, z, K, hw[0], hw[1], GRD_HW[0], GRD_HW[1], require_jac=False)
        want = uv[:, top:top + Hc, left:left + Wc]
        assert got.dtype == torch.float32 and tuple(got.shape) == (K.shape[0], Hc, Wc, 2)
        err = ((got.double() - want).abs() / want.abs().clamp_min(1.0)).max()
        assert err < 2.0 ** -23, (level, float(err))


SWEEP = r'''
#include "g2s_corr_tile.h"
#include <cstdio>
#include <vector>

static long fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
  long shapes = 0;
  // ---- constants
  CHECK(GC_FLUSH_STEPS >= 1 && GC_FLUSH_STEPS * GC_STEP_PRODUCTS <= GC_FLUSH_LIMIT, "flush: %d steps x %d products", GC_FLUSH_STEPS, GC_STEP_PRODUCTS);
  CHECK(GC_WAVES * 1024 * 8 <= GC_RING_FLOATS * 4, "the closing reduction does not fit the ring");
  CHECK(GC_STRIP_LOADERS <= GC_RING_LOADER0 && GC_RING_LOADER0 + GC_XC * (GC_CC / 4) == 256, "loader threads");
  CHECK((GC_CS & 1) && (GC_RS & 1), "odd LDS strides");
  {  // the accumulator map is a bijection onto the tile
    std::vector<int> seen(GC_T * GC_T, 0);
    for (int v = 0; v < 16; ++v) for (int l = 0; l < 64; ++l) {
      const int dx = gc_acc_dx(v, l), dy = gc_acc_dy(l);
      CHECK(dx >= 0 && dx < GC_T && dy >= 0 && dy < GC_T, "acc map range v %d lane %d", v, l);
      if (dx >= 0 && dx < GC_T && dy >= 0 && dy < GC_T) ++seen[dy * GC_T + dx];
    }
    for (int i = 0; i < GC_T * GC_T; ++i) CHECK(seen[i] == 1, "acc map: element %d owned %d times", i, seen[i]);
  }
  {  // staging: every strip and ring-row element is written once, inside its buffer; every operand read is inside and was written
    std::vector<int> st(GC_STRIP_FLOATS, 0), rg(GC_RING_FLOATS, 0);
    for (int t = 0; t < 256; ++t) {
      if (t < GC_STRIP_LOADERS) for (int k = 0; k < 4; ++k) {
        const int i = gc_strip_index(t >> 2, (t & 3) * 4 + k);
        CHECK(i >= 0 && i < GC_STRIP_FLOATS, "strip write %d", i);
        if (i >= 0 && i < GC_STRIP_FLOATS) ++st[i];
      } else if (t >= GC_RING_LOADER0) for (int k = 0; k < 4; ++k) {
        const int i = gc_ring_index(5, (t - GC_RING_LOADER0) >> 2, (t & 3) * 4 + k);
        CHECK(i >= 0 && i < GC_RING_FLOATS, "ring write %d", i);
        if (i >= 0 && i < GC_RING_FLOATS) ++rg[i];
      }
    }
    for (int w = 0; w < GC_WAVES; ++w) for (int u = 0; u < GC_XW; ++u) for (int i = 0; i < GC_T; ++i) for (int c = 0; c < GC_CC; ++c) {
      const int xl = w * GC_XW + u, a = gc_strip_index(xl + i, c), b = gc_ring_index(5, xl, c);
      CHECK(a >= 0 && a < GC_STRIP_FLOATS && st[a] == 1, "strip read %d", a);
      CHECK(b >= 0 && b < GC_RING_FLOATS && rg[b] == 1, "ring read %d", b);
    }
    for (int y = -40; y < 400; ++y) CHECK(gc_ring_slot(y) >= 0 && gc_ring_slot(y) < GC_SLOTS && gc_ring_slot(y) == gc_ring_slot(y + GC_SLOTS), "slot of row %d", y);
  }
  const int Cs[4] = {16, 64, 128, 256};
  for (int A = 1; A <= 70; ++A) {
    for (int Hc = 1; Hc <= A; ++Hc) {
      const int Ny = A - Hc + 1, nTy = gc_tiles(Ny);
      // every dy is owned by one (tile, lane) pair; the r range of a tile stays on the map; the ring holds the row each lane reads
      std::vector<int> own(Ny, 0);
      for (int ty = 0; ty < nTy; ++ty) {
        const int dy0 = ty * GC_T, r0 = gc_r_begin(dy0), r1 = gc_r_end(dy0, Ny, Hc);
        for (int j = 0; j < GC_T; ++j) if (dy0 + j < Ny) ++own[dy0 + j];
        CHECK(r0 >= 0 && r1 <= A && r0 < r1, "r range A %d Hc %d tile %d: [%d,%d)", A, Hc, ty, r0, r1);
        int held[GC_SLOTS];                       // the crop row a slot holds; -1: zeros
        for (int s = 0; s < GC_SLOTS; ++s) held[s] = -1;
        std::vector<int> used((size_t)GC_T * Hc, 0);
        for (int r = r0; r < r1; ++r) {
          const int ynew = r - dy0;
          held[gc_ring_slot(ynew)] = ynew < Hc ? ynew : -1;
          for (int j = 0; j < GC_T; ++j) {
            const int y = r - dy0 - j, want = (y >= 0 && y < Hc) ? y : -1;
            CHECK(held[gc_ring_slot(y)] == want, "ring A %d Hc %d tile %d r %d lane %d: slot holds %d, row %d wanted", A, Hc, ty, r, j, held[gc_ring_slot(y)], want);
            if (want >= 0) ++used[(size_t)j * Hc + y];
          }
        }
        // every (dy, y) product row of the tile's real shifts is met exactly once
        for (int j = 0; j < GC_T && dy0 + j < Ny; ++j) for (int y = 0; y < Hc; ++y) CHECK(used[(size_t)j * Hc + y] == 1, "A %d Hc %d dy %d crop row %d met %d times", A, Hc, dy0 + j, y, used[(size_t)j * Hc + y]);
      }
      for (int dy = 0; dy < Ny; ++dy) CHECK(own[dy] == 1, "A %d Hc %d: dy %d owned %d times", A, Hc, dy, own[dy]);
      for (int Wc = 1; Wc <= A; ++Wc) {
        const int Nx = A - Wc + 1, nTx = gc_tiles(Nx), nxc = gc_xchunks(Wc);
        if (Hc == 1) {                            // the x axis does not depend on Hc
          std::vector<int> ownx(Nx, 0);
          for (int tx = 0; tx < nTx; ++tx) for (int i = 0; i < GC_T; ++i) if (tx * GC_T + i < Nx) ++ownx[tx * GC_T + i];
          for (int dx = 0; dx < Nx; ++dx) CHECK(ownx[dx] == 1, "A %d Wc %d: dx %d owned %d times", A, Wc, dx, ownx[dx]);
          // every (dx, x) pair of a real shift reads satellite column x + dx < A through the strip, once over the x-chunks
          for (int tx = 0; tx < nTx; ++tx) {
            std::vector<int> met((size_t)GC_T * Wc, 0);
            for (int xc = 0; xc < nxc; ++xc) for (int xl = 0; xl < GC_XC; ++xl) for (int i = 0; i < GC_T; ++i) {
              const int x = xc * GC_XC + xl, dx = tx * GC_T + i, col = xl + i, sx = xc * GC_XC + tx * GC_T + col;
              CHECK(col < GC_SW, "strip column %d", col);
              if (x < Wc && dx < Nx) { CHECK(sx == x + dx && sx < A, "A %d Wc %d: strip column %d is map column %d", A, Wc, col, sx); ++met[(size_t)i * Wc + x]; }
            }
            for (int i = 0; i < GC_T && tx * GC_T + i < Nx; ++i) for (int x = 0; x < Wc; ++x) CHECK(met[(size_t)i * Wc + x] == 1, "A %d Wc %d dx %d x %d met %d times", A, Wc, tx * GC_T + i, x, met[(size_t)i * Wc + x]);
          }
        }
        for (int ci = 0; ci < 4; ++ci, ++shapes) {
          const int C = Cs[ci], ncol = gc_columns(Wc, C), nsplit = gc_splits(ncol);
          // the splits tile the K columns; the columns tile (x-chunk, c-chunk)
          CHECK(nsplit >= 1 && nsplit <= GC_MAX_SPLITS, "A %d Wc %d C %d: %d splits", A, Wc, C, nsplit);
          int next = 0;
          for (int s = 0; s < nsplit; ++s) {
            CHECK(gc_split_begin(s, ncol) == next && gc_split_end(s, ncol) > next, "A %d Wc %d C %d split %d: [%d,%d) after %d", A, Wc, C, s, gc_split_begin(s, ncol), gc_split_end(s, ncol), next);
            next = gc_split_end(s, ncol);
          }
          CHECK(next == ncol, "A %d Wc %d C %d: the splits end at %d of %d", A, Wc, C, next, ncol);
          std::vector<int> cm(ncol, 0);
          for (int col = 0; col < ncol; ++col) {
            const int x0 = gc_col_x0(col, Wc), c0 = gc_col_c0(col, Wc);
            CHECK(x0 >= 0 && x0 < Wc && x0 % GC_XC == 0 && c0 >= 0 && c0 + GC_CC <= C && c0 % GC_CC == 0, "column %d -> x0 %d c0 %d", col, x0, c0);
            const int id = (c0 / GC_CC) * nxc + x0 / GC_XC;
            if (id >= 0 && id < ncol) ++cm[id];
            // the last float4 a loader may fetch lies inside its map
            const int xs = x0 + GC_XC - 1 < Wc - 1 ? x0 + GC_XC - 1 : Wc - 1;
            CHECK(((size_t)(Hc - 1) * Wc + xs) * C + c0 + GC_CC <= (size_t)Hc * Wc * C, "g2s fetch past the end");
            CHECK(((size_t)(A - 1) * A + (A - 1)) * C + c0 + GC_CC <= (size_t)A * A * C, "sat fetch past the end");
          }
          for (int col = 0; col < ncol; ++col) CHECK(cm[col] == 1, "column id %d made %d times", col, cm[col]);
          // the chain of an accumulator: products collected between two flushes, over a split's whole walk
          if (Wc == 1 || Wc == A)
            for (int ty = 0; ty < nTy; ++ty) for (int s = 0; s < nsplit; ++s) {
              int steps = 0, chain = 0;
              const int n = (gc_split_end(s, ncol) - gc_split_begin(s, ncol)) * (gc_r_end(ty * GC_T, Ny, Hc) - gc_r_begin(ty * GC_T));
              for (int k = 0; k < n; ++k) {
                chain += GC_STEP_PRODUCTS;
                CHECK(chain <= GC_FLUSH_LIMIT, "chain of %d products", chain);
                if (++steps == GC_FLUSH_STEPS) { steps = 0; chain = 0; }
              }
            }
          // workspace: sections in order, none overlapping, the largest index of each inside it
          const int B = 3;
          const GcLayout L = gc_layout(B, A, Hc, Wc, C);
          CHECK(L.Ny == Ny && L.Nx == Nx && L.ncol == ncol && L.nsplit == nsplit, "layout sizes");
          const size_t off[12] = {L.e, L.eg, L.h, L.part, L.kf, L.kr, L.beta, L.hb, L.coefB, L.alpha, L.coefA, L.total};
          const size_t S = (size_t)Ny * Nx;
          const size_t need[11] = {(size_t)B * A * A, (size_t)B * Hc * Wc, (size_t)B * A * Nx, gc_part_index(B - 1, nsplit - 1, Ny - 1, Nx - 1, nsplit, Ny, Nx) + 1,
                                   B * S, B * S, B * S, (size_t)B * Ny * A, (size_t)B * A * A, (size_t)2 * B, (size_t)B};
          for (int k = 0; k < 11; ++k) CHECK(off[k] % 256 == 0 && off[k] + need[k] * 8 <= off[k + 1], "A %d Hc %d Wc %d C %d: workspace section %d", A, Hc, Wc, C, k);
          CHECK(gc_part_index(B - 1, nsplit - 1, Ny - 1, Nx - 1, nsplit, Ny, Nx) + 1 == (size_t)B * nsplit * S, "part index");
        }
      }
    }
  }
  std::printf("%s: %ld shapes, %ld failures\n", fails ? "FAILED" : "ok", shapes, fails);
  return fails ? 1 : 0;
}
'''


def _cxx():
    for name in ('g++', 'c++', 'clang++'):
        path = shutil.which(name)
        if path:
            return path
    for path in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++'):
        if os.path.exists(path):
            return path
    return None


def test_tile_ring_split_and_workspace_arithmetic_on_the_host(tmp_path):
    cxx = _cxx()
    assert cxx is not None, 'no host C++ compiler'
    src = tmp_path / 'g2s_corr_sweep.cpp'
    src.write_text(SWEEP)
    exe = tmp_path / 'g2s_corr_sweep'
    base = [cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)]
    # a stand-alone program: the sanitizers go in where the toolchain has their runtimes, else it is built plain
    if subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    n = sum(A * A for A in range(1, 71)) * 4
    assert r.stdout.strip().endswith(f'{n} shapes, 0 failures')
