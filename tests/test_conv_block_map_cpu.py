"""The workgroup -> (tile, output-channel block) map of the conv3x3 launches (highlyaccurate_amd/csrc/conv_block_map.h), checked on
the host: the header is plain C++, so a stand-alone program includes the very functions the kernels call.

The kernels launch a 1-D grid of nblk * gy workgroups (nblk tiles, gy blocks of output channels).  The hardware deals workgroups
round-robin to the 8 XCDs by their linear id, so the workgroups one XCD receives, in order, are blk = x, x + 8, x + 16, ...
What the map promises:
  * it is a bijection from [0, nblk * gy) onto tiles x channel blocks (every output is computed exactly once);
  * along each of the 8 residue sequences a tile's gy blocks follow one another directly, channel block 0 first (so blocks
    1.. find the tile's input in the L2 the first one filled), except for the tiles that straddle one of the at most 7 seams
    between the XCDs' contiguous chunks;
  * with one channel block it is xcd_contiguous itself, which gives every residue a contiguous ascending run of tiles.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'highlyaccurate_amd', 'csrc')

PROGRAM = r'''
#include "conv_block_map.h"
#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
  long grids = 0;
  for (int gy = 1; gy <= 4; ++gy)
    for (int nblk = 1; nblk <= 300; ++nblk, ++grids) {
      const int nwg = nblk * gy;
      // bijection, and the range of both parts
      std::vector<int> seen(nwg, 0);
      for (int blk = 0; blk < nwg; ++blk) {
        const ConvBlock m = conv_block_map(blk, nwg, gy);
        CHECK(m.tile >= 0 && m.tile < nblk && m.cb >= 0 && m.cb < gy, "range: nblk %d gy %d blk %d -> tile %d cb %d", nblk, gy, blk, m.tile, m.cb);
        if (m.tile >= 0 && m.tile < nblk && m.cb >= 0 && m.cb < gy) ++seen[m.tile * gy + m.cb];
      }
      for (int i = 0; i < nwg; ++i) CHECK(seen[i] == 1, "bijection: nblk %d gy %d: (tile %d, cb %d) is produced %d times", nblk, gy, i / gy, i % gy, seen[i]);
      // per residue: a tile's blocks are one run cb = 0, 1, ..., gy - 1; count the tiles of which that is not true
      std::vector<int> whole(nblk, 0);
      for (int x = 0; x < 8; ++x) {
        int run_tile = -1, run_len = 0;
        for (int blk = x; blk < nwg; blk += 8) {
          const ConvBlock m = conv_block_map(blk, nwg, gy);
          if (m.tile == run_tile && m.cb == run_len) ++run_len;
          else { run_tile = m.tile; run_len = m.cb == 0 ? 1 : -1000000; }
          if (run_len == gy && m.tile >= 0 && m.tile < nblk) ++whole[m.tile];
        }
      }
      int broken = 0;
      for (int t = 0; t < nblk; ++t) broken += whole[t] != 1;
      CHECK(broken <= 7, "locality: nblk %d gy %d: %d tiles are not visited as one run of their blocks", nblk, gy, broken);
      if (gy == 1) {
        for (int blk = 0; blk < nwg; ++blk) {
          const ConvBlock m = conv_block_map(blk, nwg, 1);
          CHECK(m.tile == xcd_contiguous(blk, nblk) && m.cb == 0, "gy == 1: nblk %d blk %d -> tile %d cb %d, xcd_contiguous %d", nblk, blk, m.tile, m.cb, xcd_contiguous(blk, nblk));
        }
        // xcd_contiguous itself: every residue walks a contiguous ascending run, and the runs tile [0, nblk) in residue order
        int next = 0;
        for (int x = 0; x < 8; ++x)
          for (int blk = x; blk < nblk; blk += 8) { CHECK(xcd_contiguous(blk, nblk) == next, "xcd_contiguous: nblk %d blk %d -> %d, expected %d", nblk, blk, xcd_contiguous(blk, nblk), next); ++next; }
        CHECK(next == nblk, "xcd_contiguous: nblk %d: %d ids walked", nblk, next);
      }
    }
  std::printf("%s: %ld grids, %d failures\n", fails ? "FAILED" : "ok", grids, fails);
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


def test_block_map_is_a_bijection_that_keeps_a_tiles_channel_blocks_together(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'block_map_check.cpp'
    src.write_text(PROGRAM)
    exe = tmp_path / 'block_map_check'
    # plain host C++: no HIP headers, no -x hip -- the header must stand on its own
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith('1200 grids, 0 failures')
