// Workgroup id -> (tile, output-channel block) of the conv3x3 launches.  Plain C++: conv_kernels.h includes it for the kernels,
// a host program can include it as it is (tests/test_conv_block_map_cpu.py checks the properties stated below).
#pragma once

#if defined(__HIPCC__)
#define HLA_MAP_FN __host__ __device__ __forceinline__
#else
#define HLA_MAP_FN inline
#endif

// Workgroups are dealt round-robin to the 8 XCDs (each with its own L2).  Remap the linear id so that every XCD works on
// a CONTIGUOUS run of tiles: vertically adjacent tiles, which share two halo rows, then hit the same L2.  Bijective for
// any grid size (cdna_hip_programming.md "XCD swizzle must be bijective").  Measured: +1 % in one A/B, within noise in the next.
// (`bid & 7` labels the workgroups that share an XCD; the dispatcher deals by the LINEAR id, which is why the launches are 1-D.)
HLA_MAP_FN int xcd_contiguous(int bid, int nb) {
  const int q = nb >> 3, r = nb & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
// The inverse: the workgroup id that xcd_contiguous maps to position v (vgg_fixup_loop walks one sample's positions in order and
// hands each body the id the launch over the whole batch would have given it; tests/test_conv_block_map_inverse_cpu.py).
HLA_MAP_FN int xcd_contiguous_inv(int v, int nb) {
  const int q = nb >> 3, r = nb & 7, split = r * (q + 1);      // (v >= split implies q > 0: with q == 0, split == nb)
  const int xcd = v < split ? v / (q + 1) : r + (v - split) / q;
  return ((v < split ? v - xcd * (q + 1) : v - split - (xcd - r) * q) << 3) + xcd;
}

// A launch with `gy` output-channel blocks per tile is a 1-D grid of nwg = tiles * gy workgroups, the channel block innermost in
// the XCD-contiguous order: the workgroups an XCD receives one after the other (bid, bid + 8, ...) are the gy blocks of one tile,
// then the next tile's, so all but the first find the tile's halo in that XCD's L2.  (With the channel block as the grid's y the
// second pass over the tiles started when the first had ended, the input long gone from every cache.)  A tile's blocks are split
// between two XCDs at most at the 7 seams of xcd_contiguous' chunks; that costs those tiles their locality, nothing else.
// gy == 1: tile = xcd_contiguous(bid, nwg), cb = 0.
struct ConvBlock { int tile, cb; };
HLA_MAP_FN ConvBlock conv_block_map(int bid, int nwg, int gy) {
  const int v = xcd_contiguous(bid, nwg);
  return ConvBlock{v / gy, v % gy};
}
