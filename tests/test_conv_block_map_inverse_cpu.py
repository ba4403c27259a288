"""xcd_contiguous_inv (highlyaccurate_amd/csrc/conv_block_map.h), checked on the host like the map itself
(tests/test_conv_block_map_cpu.py): vgg_fixup_loop walks one sample's positions of a conv launch in order and needs, for each, the
workgroup id whose conv_block_map is that position.  For every grid size 1..2500 and every position v the inverse returns an id in
range that xcd_contiguous maps back to v.
"""
import subprocess

import pytest

from test_conv_block_map_cpu import CSRC, _cxx

PROGRAM = r'''
#include "conv_block_map.h"
#include <cstdio>

int main() {
  long fails = 0, n = 0;
  for (int nb = 1; nb <= 2500; ++nb)
    for (int v = 0; v < nb; ++v, ++n) {
      const int bid = xcd_contiguous_inv(v, nb);
      if (bid < 0 || bid >= nb || xcd_contiguous(bid, nb) != v) {
        if (fails++ < 20) std::printf("nb %d v %d -> bid %d -> %d\n", nb, v, bid, bid >= 0 && bid < nb ? xcd_contiguous(bid, nb) : -1);
      }
    }
  std::printf("%s: %ld positions, %ld failures\n", fails ? "FAILED" : "ok", n, fails);
  return fails ? 1 : 0;
}
'''


def test_inverse_of_the_xcd_contiguous_order(tmp_path):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'block_map_inverse_check.cpp'
    src.write_text(PROGRAM)
    exe = tmp_path / 'block_map_inverse_check'
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith('3126250 positions, 0 failures')
