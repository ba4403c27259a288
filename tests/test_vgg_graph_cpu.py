"""The layer graph and the row / column plans of the VGG extractor (highlyaccurate_amd/csrc/vgg_graph.h), checked on the host: the
header is plain C++, so a stand-alone program includes the very tables and functions vgg.hip and vgg_backward.hip walk, and prints
them for every first_row8 in {0, 4..23}, with and without confidence heads, level 4, training, scale_invariant, and first_col32
in {0, 1, 2} with and without the fix-up pass.

Compared here with
  * the forward row and column formulas as the host code stated them before the header existed, restated below;
  * ``vgg_bwd16_ref._n_rows`` (the backward's first rows) and the per-launch src_row_lo / add_row_lo / weight-gradient rows of
    the walk as it was written out, restated below;
  * the maps' divisors and channel counts of ``vgg_bwd16_ref`` (FWD_MAPS, FWD_IDX, BWD_MAPS, BWD_MAPS4) and the order of its
    ``bwd_plan`` regions, which ``test_vgg_bwd16_ref_cpu`` pins to the library's workspace sizes.
Soundness, by propagation over the printed tables themselves: every launch starts at or above the first row its consumers
read (a 3x3 conv reads one row above, a 2x upsample halves, a 2x2 pool doubles, the confidence heads read one row above),
and in the backward every launch reads a gradient map from exactly the first row its producer wrote.
The same program is built once more with -fsanitize=address,undefined and run.
"""
import os
import subprocess

import pytest

import vgg_bwd16_ref as BR
from test_conv_block_map_cpu import _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'highlyaccurate_amd', 'csrc')

PROGRAM = r'''
#include "vgg_graph.h"
#include <cstdio>

int main() {
  for (int m = 0; m < AM_N; ++m) std::printf("act %d %d %d %d\n", m, kActMaps[m].div, kActMaps[m].C, kActMaps[m].fold);
  for (int i = 0; i < IDX_N; ++i) std::printf("idx %d %d\n", i, kIdxOf[i]);
  for (int l = 0; l < 4; ++l) std::printf("level %d %d\n", l, kLevelMap[l]);
  for (int m = 0; m < M_ALL; ++m) std::printf("grad %d %d %d %d %d\n", m, kGradMaps[m].m.div, kGradMaps[m].m.C, kGradMaps[m].m.fold, kGradMaps[m].ga);
  std::printf("order3");
  for (int m : kBwdPlanOrder) std::printf(" %d", m);
  std::printf("\norder4");
  for (int m : kBwdPlanOrder4) std::printf(" %d", m);
  std::printf("\n");
  for (int l = 0; l < kAllLayers; ++l) {
    const VggFwdLaunch& f = kFwd[l];
    const VggHW g = vgg_layer_hw(l, 64, 160, false), gf = vgg_layer_hw(l, 64, 160, true);
    std::printf("fwd %d %d %d %d %d %d %d %d %d %d %d %d\n", l, f.src, f.skip, f.out, f.level, f.idx, vgg_layer_pools(l) ? 1 : 0, vgg_layer_div(l),
                g.h, g.w, gf.h, gf.w);
  }
  for (int i = 0; i < DC_ALL; ++i) {
    const VggDgradLaunch& d = kDgrad[i];
    std::printf("dgrad %d %d %d %d %d %d %d %d %d %d\n", i, d.layer, d.c0, d.src, d.unpool, d.out, d.mask, d.add, d.pool_sum, d.level);
  }
  for (int i = 0; i < DW_ALL; ++i) {
    const VggWgradLaunch& w = kWgrad[i];
    std::printf("wgrad %d %d %d %d %d %d %d\n", i, w.layer, w.x1, w.x2, w.g, w.unpool, w.level);
  }
  for (int f = 0; f < 24; f = f ? f + 1 : 4)
    for (int wc = 0; wc < 2; ++wc)
      for (int mode = 0; mode < 4; ++mode) {      // bit 0: level 4; bit 1: training / not scale_invariant
        const VggFwdRows r = vgg_fwd_rows(f, mode & 1, (mode & 2) != 0, wc != 0);
        std::printf("fwdrows %d %d %d %d", f, wc, mode & 1, mode >> 1);
        for (int l = 0; l < kAllLayers; ++l) std::printf(" %d", r.row[l]);
        const VggBwdRows b = vgg_bwd_rows(f, mode & 1, !(mode & 2), wc != 0);
        std::printf("\nbwdrows %d %d %d %d", f, wc, mode & 1, (mode & 2) ? 0 : 1);
        for (int m = 0; m < M_N; ++m) std::printf(" %d", b.n[m]);
        for (int i = 0; i < DC_N; ++i) std::printf(" %d %d %d", b.dc_row[i], b.dc_src_lo[i], b.dc_add_lo[i]);
        for (int i = 0; i < DW_N; ++i) std::printf(" %d", b.dw_row[i]);
        std::printf("\n");
      }
  for (int c = 0; c < 3; ++c)
    for (int fix = 0; fix < 2; ++fix)
      for (int l = 1; l < kAllLayers; ++l) {
        const VggCols v = vgg_cols(l, c, fix != 0);
        std::printf("cols %d %d %d %d %d\n", c, fix, l, v.begin, v.tiles);
      }
  return 0;
}
'''

# the ids, in the order of the header's enums
ACT = ['x3', 'a5', 'x8', 'a10', 'a12', 'x15r', 'd1a', 'x18r', 'd2a', 'x21r', 'x2r', 'd3a', 'x24r', 'a0']
IDX = ['idx3', 'idx8', 'idx15']
GRAD = ['g_x21', 'g_d2a', 'g_x3p', 'g_x18', 'g_d1a', 'g_x8p', 'g_x15', 'g_a12', 'g_a10', 'g_x8', 'g_a5', 'g_x3', 'g_a0',
        'g_x24', 'g_d3a', 'g_x2p', 'g_c2', 'l2_15', 'l2_18', 'l2_21']
M = {n: i for i, n in enumerate(GRAD)}
A = {n: i for i, n in enumerate(ACT)}
DC = ['10', '9U', '9S', '8', '7U', '7S', '6', '5', '4', '3', '2', '1']
DW = ['10', '9', '8', '7', '6', '5', '4', '3', '2', '1', '0']
F_VALUES = [0] + list(range(4, 24))


@pytest.fixture(scope='module')
def printed(tmp_path_factory):
    cxx = _cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('vgg_graph')
    src = d / 'vgg_graph_print.cpp'
    src.write_text(PROGRAM)
    outs = []
    # plain host C++: no HIP headers, no -x hip -- the header must stand on its own; then the same program under the sanitizers
    for name, extra in (('plain', ['-O1']), ('san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = d / f'vgg_graph_print_{name}'
        subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', *extra, '-I', CSRC, str(src), '-o', str(exe)], check=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-4000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    rows = {}
    for line in outs[0].splitlines():
        key, *v = line.split()
        rows.setdefault(key, []).append([int(x) for x in v])
    return rows


def test_maps_have_the_divisors_and_channels_the_workspace_sizes_pin(printed):
    assert len(printed['act']) == len(ACT) and len(printed['grad']) == len(GRAD)
    for m, div, C, fold in printed['act']:
        assert (div, C) == (BR.FWD_MAPS[ACT[m]] if ACT[m] != 'a0' else (1, 64)), ACT[m]
        assert fold == (1 if ACT[m] in ('d1a', 'x18r', 'd2a', 'x21r', 'd3a', 'x24r') else 0), ACT[m]      # the decoder's outputs
    for i, m in printed['idx']:
        assert BR.FWD_IDX[IDX[i]] == BR.FWD_MAPS[ACT[m]] and IDX[i][3:] == ACT[m].rstrip('r')[1:]
    assert [ACT[m] for _, m in printed['level']] == ['x15r', 'x18r', 'x21r', 'x24r']
    both = dict(BR.BWD_MAPS, **BR.BWD_MAPS4)
    assert sorted(both) == sorted(GRAD)
    for m, div, C, fold, ga in printed['grad']:
        assert (div, C) == both[GRAD[m]], GRAD[m]
    # every map a convolution reads has its own amax slot; the L2 side buffers (only added in an epilogue) have none
    ga = [r[4] for r in printed['grad']]
    assert ga[17:] == [-1, -1, -1] and sorted(ga[:17]) == list(range(17))
    # the order of the regions in the backward workspace: vgg_bwd16_ref.bwd_plan's, pinned to the library's totals
    names = [k for k in BR.bwd_plan(1, 8, 8, True)[0] if k in both]
    assert [GRAD[m] for m in printed['order3'][0] + printed['order4'][0]] == names


# resolution divisor of each layer's launch and the geometry [H/div, W/div] or, for the decoder under the fold, [2H/div, W/div/2]
LAUNCH_DIV = [1, 1, 2, 2, 4, 4, 4, 4, 4, 2, 2, 1, 1]


def test_forward_launch_table(printed):
    H, W = 64, 160
    chans = {m: C for m, _, C, _ in printed['act']}
    cin = [c for c, _ in BR.LAYERS]
    cout = [c for _, c in BR.LAYERS]
    for l, src, skip, out, level, idx, pools, div, h, w, hf, wf in printed['fwd']:
        assert div == LAUNCH_DIV[l] and (h, w) == (H // div, W // div)
        assert (hf, wf) == ((2 * h, w // 2) if l >= 7 else (h, w))
        assert pools == (1 if l in (1, 3, 6) else 0) == (1 if idx >= 0 else 0)
        assert chans[out] == cout[l] and (3 if l == 0 else chans[src] + (chans[skip] if skip >= 0 else 0)) == cin[l], l
        assert level == {6: 0, 8: 1, 10: 2, 12: 3}.get(l, -1)
        if l >= 2:      # the source is what the layer before wrote; the skips are the encoder maps of the same resolution
            assert src == printed['fwd'][l - 1][3]
        assert skip == {7: A['x8'], 9: A['x3'], 11: A['x2r']}.get(l, -1)


def _parent_fwd_rows(f8, level4, train, want_conf):
    """first rows of conv0 + conv2 and of layers 2..12, as vgg_build_convs computed them"""
    f = 0 if (level4 or train) else f8
    wc = 1 if want_conf else 0
    if not f:
        return [0] * 13
    return [0, 8 * f - 32, 4 * f - 15, 4 * f - 14, 2 * f - 6, 2 * f - 5, 2 * f - 4, 2 * f - 2 - wc, 2 * f - 1 - wc, 4 * f - 1 - wc,
            4 * f - wc, 0, 0]


def test_forward_rows_are_the_parents_and_sound(printed):
    fwd = {r[0]: r for r in printed['fwd']}
    seen = set()
    for f8, wc, level4, train, *rows in printed['fwdrows']:
        seen.add((f8, wc, level4, train))
        assert rows == _parent_fwd_rows(f8, level4, train, wc), (f8, wc, level4, train)
        assert all(r >= 0 for r in rows)
        if level4 or train:
            assert not any(rows)
            continue
        # first row of every stored map that its producer writes, in the map's resolution (a pooling layer: whole 2x2 rows)
        first = {fwd[l][3]: (-(-rows[l] // 2) if fwd[l][6] else rows[l]) for l in range(1, 11)}
        for l in range(2, 11):
            _, src, skip = fwd[l][:3]
            need = max(rows[l] - 1, 0)            # a 3x3 conv reads one row above its first output row
            if skip >= 0:                         # the 2x upsampled source halves
                assert first[src] <= need // 2 and first[skip] <= need, (f8, wc, l)
            else:
                assert first[src] <= need, (f8, wc, l)
        # what the caller reads: rows f / 2f / 4f of x15 / x18 / x21, the confidence heads one row above
        for m, r in ((A['x15r'], f8), (A['x18r'], 2 * f8), (A['x21r'], 4 * f8)):
            assert first[m] <= max(r - wc, 0), (f8, wc, ACT[m])
    assert seen == {(f, wc, a, b) for f in F_VALUES for wc in (0, 1) for a in (0, 1) for b in (0, 1)}


def test_columns_are_the_parents(printed):
    assert len(printed['cols']) == 3 * 2 * 12
    for c, fix, l, begin, tiles in printed['cols']:
        scale = 4 // LAUNCH_DIV[l]                 # W_l / (W / 4)
        exact = l == 1                             # conv0 + conv2 computes conv0's halo itself
        assert begin == (0 if fix else c * scale), (c, fix, l)
        assert tiles == ((c * scale + (0 if exact else 1)) if fix else 0), (c, fix, l)


def test_backward_tables(printed):
    dg = {tuple(r[:1])[0]: r[1:] for r in printed['dgrad']}
    want = {  # launch: (layer, c0, src, unpool, out, mask, add, pool_sum), as the walk of vgg_backward_t passed them
        '10': (10, 0, 'g_x21', None, 'g_d2a', 'd2a', None, 0), '9U': (9, 0, 'g_d2a', None, 'g_x18', 'x18r', 'l2_18', 1),
        '9S': (9, 128, 'g_d2a', None, 'g_x3p', 'x3', None, 0), '8': (8, 0, 'g_x18', None, 'g_d1a', 'd1a', None, 0),
        '7U': (7, 0, 'g_d1a', None, 'g_x15', 'x15r', 'l2_15', 1), '7S': (7, 256, 'g_d1a', None, 'g_x8p', 'x8', None, 0),
        '6': (6, 0, 'g_x15', 'idx15', 'g_a12', 'a12', None, 0), '5': (5, 0, 'g_a12', None, 'g_a10', 'a10', None, 0),
        '4': (4, 0, 'g_a10', None, 'g_x8', 'x8', 'g_x8p', 0), '3': (3, 0, 'g_x8', 'idx8', 'g_a5', 'a5', None, 0),
        '2': (2, 0, 'g_a5', None, 'g_x3', 'x3', 'g_x3p', 0), '1': (1, 0, 'g_x3', 'idx3', 'g_a0', 'a0', None, 0)}
    four = [(12, 0, 'g_x24', None, 'g_d3a', 'd3a', None, 0), (11, 0, 'g_d3a', None, 'g_x21', 'x21r', 'l2_21', 1),
            (11, 64, 'g_d3a', None, 'g_x2p', 'x2r', None, 0), (1, 0, 'g_c2', None, 'g_a0', 'a0', None, 0)]
    enc = lambda t: [t[0], t[1], M[t[2]], -1 if t[3] is None else IDX.index(t[3]), M[t[4]], A[t[5]], -1 if t[6] is None else M[t[6]], t[7]]
    for i, name in enumerate(DC):
        assert dg[i] == enc(want[name]) + [3 if name == '1' else 0], name
    for k, t in enumerate(four):
        assert dg[len(DC) + k] == enc(t) + [4], t
    wg = {r[0]: r[1:] for r in printed['wgrad']}
    wantw = [(10, 'd2a', None, 'g_x21', None, 0), (9, 'x18r', 'x3', 'g_d2a', None, 0), (8, 'd1a', None, 'g_x18', None, 0),
             (7, 'x15r', 'x8', 'g_d1a', None, 0), (6, 'a12', None, 'g_x15', 'idx15', 0), (5, 'a10', None, 'g_a12', None, 0),
             (4, 'x8', None, 'g_a10', None, 0), (3, 'a5', None, 'g_x8', 'idx8', 0), (2, 'x3', None, 'g_a5', None, 0),
             (1, 'a0', None, 'g_x3', 'idx3', 3), (0, None, None, 'g_a0', None, 0),
             (12, 'd3a', None, 'g_x24', None, 4), (11, 'x21r', 'x2r', 'g_d3a', None, 4), (1, 'a0', None, 'g_c2', None, 4)]
    for i, (l, x1, x2, g, up, level) in enumerate(wantw):
        assert wg[i] == [l, -1 if x1 is None else A[x1], -1 if x2 is None else A[x2], M[g], -1 if up is None else IDX.index(up), level], i


def test_backward_rows_are_the_parents_and_sound(printed):
    dgrad = [r[1:] for r in printed['dgrad']][:len(DC)]
    wgrad = [r[1:] for r in printed['wgrad']][:len(DW)]
    seen = set()
    for f8, wc, level4, si, *v in printed['bwdrows']:
        seen.add((f8, wc, level4, si))
        n, v = dict(zip(GRAD, v[:13])), v[13:]
        dc = {name: tuple(v[3 * i:3 * i + 3]) for i, name in enumerate(DC)}
        dw = dict(zip(DW, v[36:]))
        assert len(v) == 36 + 11
        p = BR._n_rows(f8, bool(wc), bool(si), bool(level4))
        assert {k[2:]: r for k, r in n.items()} == {k: r for k, r in p.items() if not k.startswith('rb_')}, (f8, wc, level4, si)
        # (row_begin, src_row_lo, add_row_lo) of every data gradient and row_begin of every weight gradient, as the walk passed them
        assert dc == {'10': (p['d2a'], p['x21'], 0), '9U': (p['rb_up18'], p['d2a'], 0), '9S': (p['x3p'], p['d2a'], 0),
                      '8': (p['d1a'], p['x18'], 0), '7U': (p['rb_up15'], p['d1a'], 0), '7S': (p['x8p'], p['d1a'], 0),
                      '6': (p['a12'], 2 * p['x15'], 0), '5': (p['a10'], p['a12'], 0), '4': (p['x8'], p['a10'], p['x8p']),
                      '3': (p['a5'], 2 * p['x8'], 0), '2': (p['x3'], p['a5'], p['x3p']), '1': (p['a0'], 2 * p['x3'], 0)}
        assert dw == {'10': p['x21'], '9': p['d2a'], '8': p['x18'], '7': p['d1a'], '6': 2 * p['x15'], '5': p['a12'], '4': p['a10'],
                      '3': 2 * p['x8'], '2': p['a5'], '1': 2 * p['x3'], '0': p['a0']}
        f = f8 if (si and not level4) else 0
        if not f:
            assert not any(n.values()) and not any(v)
            continue
        # the caller's promise: d_feat[l] (and with the heads the confidence gradient, one row higher) is zero above f * 2^l
        assert n['g_x21'] <= 4 * f - wc and n['g_x18'] <= 2 * f - wc and n['g_x15'] <= f - wc
        for i, (layer, c0, src, unpool, out, mask, add, pool_sum, level) in enumerate(dgrad):
            row, src_lo, add_lo = dc[DC[i]]
            scale = 2 if unpool >= 0 else 1               # an unpool doubles the rows
            assert src_lo == scale * n[GRAD[src]]          # read from exactly the first row the producer wrote
            assert row <= max(src_lo - 1, 0)              # a 3x3 conv widens the support by one row
            if pool_sum:                                  # the 2x2 sum halves: whole pairs of rows
                assert row % 2 == 0 and n[GRAD[out]] == row // 2
            else:
                assert n[GRAD[out]] == row
            if add >= 0 and add < 13:                     # a fan-in: the added map is zero above ITS first row, which the launch covers
                assert add_lo == n[GRAD[add]] >= row
            else:
                assert add_lo == 0
        for i, (layer, x1, x2, g, unpool, level) in enumerate(wgrad):
            assert dw[DW[i]] == (2 if unpool >= 0 else 1) * n[GRAD[g]]
    assert seen == {(f, wc, a, b) for f in F_VALUES for wc in (0, 1) for a in (0, 1) for b in (0, 1)}
