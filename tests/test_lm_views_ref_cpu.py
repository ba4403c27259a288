"""CPU checks of the multi-view LM reference (tests/lm_views_ref.py) -- the semantics ``hla_s2g_lm_solve_views`` is built to: one
``LM_update`` on the union of the views' pixels -- and a host sweep of the index and workspace arithmetic of the kernels
(highlyaccurate_amd/csrc/lm_views.h is plain C++: a stand-alone program includes the very functions the kernels call)."""
import os
import shutil
import subprocess

import numpy as np
import torch

import lm_kernel_ref as R
import lm_views_ref as VR

F64, F32 = torch.float64, torch.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'highlyaccurate_amd', 'csrc')
B, V, SEED = 2, 3, 11
TOL_POSE = 1e-6      # the GPU pose gate: max(TOL_POSE, 2 |ref32 - ref64|)


def _case(dt=F64, shape='ragged', Cn=64):
    geom = VR.make_views_geom(B, V)
    lv = VR.make_views_level(shape, Cn, 16, B, V, R.case_seed('views_cpu', shape, Cn, SEED))
    p0 = VR.random_pose(B, SEED)
    ruv = VR.random_draws(1, B, SEED + 1)
    return VR.cast_views_geom(geom, dt), R.cast_level(lv, dt), R.pose_cols(p0, dt), tuple(ruv[0, i][:, None].to(dt) for i in range(2))


def _cat(p):
    return torch.cat(p, 1).double().numpy()


def _single_level(l1):
    """A one-view level as lm_kernel_ref takes it: table [h,w,3]."""
    o = R.SimpleNamespace(**vars(l1))
    o.table = l1.table[0]
    return o


def test_one_view_is_todays_step_exactly():
    geom, lv, pose, ruv = _case()
    args = R.update_args()
    for v in range(V):
        g1, l1 = VR.select_views(geom, lv, [v])
        one = _single_level(l1)
        gs = R.SimpleNamespace(ford=1, ranges=geom.ranges, R_FL=g1.R_FL[:, 0], T_FL=g1.T_FL[:, 0])
        for w in (0, 1):
            a = VR.views_step(args, g1, l1, pose, w, ruv)
            b = R.level_step(args, gs, one, pose, w, ruv)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (v, w)
            sa, ma = VR.views_sums(g1, l1, pose, w)
            sb, mb, _ = R.level_sums(gs, one, pose, w)
            assert torch.equal(sa, sb) and torch.equal(ma, mb), (v, w)


def test_per_view_sums_add_up_to_the_unions():
    geom, lv, pose, _ = _case()
    for w in (0, 1):
        tot, mags = VR.views_sums(geom, lv, pose, w)
        parts = [VR.one_view_sums(geom, lv, pose, v, w)[0] for v in range(V)]
        acc = torch.zeros_like(tot)
        for p in parts:
            acc = acc + p
        assert bool(((acc - tot).abs() <= 1e-12 * mags).all()), (w, ((acc - tot).abs() / mags).max())
        assert bool((parts[0][:, 0] > 0).all() and (parts[1][:, 2] > 0).all())      # every view sees something


def test_duplicate_and_permuted_views():
    geom, lv, pose, ruv = _case()
    args = R.update_args()
    base = _cat(VR.views_step(args, geom, lv, pose, 1, ruv))
    g1, l1 = VR.select_views(geom, lv, [0])
    one = _cat(VR.views_step(args, g1, l1, pose, 1, ruv))
    g2, l2 = VR.select_views(geom, lv, [0, 0])
    assert np.abs(_cat(VR.views_step(args, g2, l2, pose, 1, ruv)) - one).max() <= 1e-12
    gp, lp = VR.select_views(geom, lv, [2, 0, 1])
    assert np.abs(_cat(VR.views_step(args, gp, lp, pose, 1, ruv)) - base).max() <= 1e-12
    assert np.abs(base - one).max() > 1e-4      # (the other views do matter)


def test_masked_out_view_is_exactly_absent():
    geom, lv, pose, ruv = _case()
    args = R.update_args()
    lm = R.SimpleNamespace(**vars(lv))
    lm.table = lv.table.clone()
    lm.table[1] = VR.masked_table(lv.table[1])
    s1, _ = VR.one_view_sums(geom, lm, pose, 1, 1)
    assert not bool(s1.any())
    gw, lw = VR.select_views(geom, lv, [0, 2])
    a, b = VR.views_step(args, geom, lm, pose, 1, ruv), VR.views_step(args, gw, lw, pose, 1, ruv)
    # the union's sums run over more (zero) terms: the same values up to the order torch adds them in; the solve from
    # explicitly added per-view sums is exact
    assert np.abs(_cat(a) - _cat(b)).max() <= 1e-12
    tot = sum(VR.one_view_sums(geom, lm, pose, v, 1)[0] for v in (0, 2))
    with_zero = (VR.one_view_sums(geom, lm, pose, 0, 1)[0] + s1) + VR.one_view_sums(geom, lm, pose, 2, 1)[0]
    assert torch.equal(tot, with_zero)
    assert np.array_equal(VR.step_from_sums(tot, _cat(pose)), VR.step_from_sums(with_zero, _cat(pose)))


def test_solve_from_summed_view_sums_is_the_unions_step():
    """What the closing kernel does -- add the views' sums, solve once -- is ``O.lm_update`` on the union."""
    geom, lv, pose, ruv = _case()
    args = R.update_args()
    tot = sum(VR.one_view_sums(geom, lv, pose, v, 1)[0] for v in range(V))
    assert np.abs(VR.step_from_sums(tot, _cat(pose)) - _cat(VR.views_step(args, geom, lv, pose, 1, ruv))).max() <= 1e-12


def test_per_view_normalisation_is_told_apart():
    """The planted variant (sum_v H_v / ns_v^2) moves the pose by more than the GPU pose gate."""
    g64, l64, p64, r64 = _case(F64)
    g32, l32, p32, r32 = _case(F32)
    args = R.update_args()
    ref64, ref32 = _cat(VR.views_step(args, g64, l64, p64, 1, r64)), _cat(VR.views_step(args, g32, l32, p32, 1, r32))
    allow = np.maximum(TOL_POSE, 2 * np.abs(ref32 - ref64))
    planted = VR.step_per_view_normalised([VR.one_view_sums(g64, l64, p64, v, 1)[0] for v in range(V)], _cat(p64))
    moved = np.abs(planted - ref64)
    print('planted variant moves the pose by', moved.max(1), 'gate', allow.max(1))
    assert bool(((moved > 10 * allow).any(1)).all()), (moved, allow)


SWEEP = r'''
#include <cstdio>
#include <vector>
#include "lm_views.h"
int main() {
  long fails = 0, cases = 0;
  const int shapes[][5] = {{7, 37, 5, 0, 64}, {9, 20, 4, 3, 128}, {33, 131, 1, 0, 16}, {129, 257, 0, 0, 256}};   // h, w, row0, skip, C
  for (int B = 1; B <= 9; ++B)
    for (int V = 1; V <= LMV_MAX_VIEWS; ++V)
      for (auto& s : shapes) {
        const int h = s[0], w = s[1], hs = h - s[3], C = s[4], A = 16, part_ld = 65, J = B * V;
        ++cases;
        const LmvLayout L = lmv_layout(B, V, part_ld);
        // regions in order, aligned, large enough, inside the total
        if (L.coef != 0 || L.pose < L.coef + (size_t)J * LMV_COEF_N * 8 || L.part < L.pose + (size_t)B * 12 ||
            L.total < L.part + (size_t)J * part_ld * LMV_PART_N * 8 || L.pose % 256 || L.part % 256 || L.total % 256) ++fails;
        std::vector<char> seen(J, 0);
        for (int b = 0; b < B; ++b)
          for (int v = 0; v < V; ++v) {
            const int j = lmv_pseudo(b, v, V);
            if (j < 0 || j >= J || seen[j]++) ++fails;
            if (lmv_sample(j, V) != b || lmv_view(j, V) != v) ++fails;
            // the last element a kernel touches of each array lies inside it
            if (lmv_sat_offset(j, V, A, C) + (size_t)A * A * C > (size_t)B * A * A * C) ++fails;
            if (lmv_grd_offset(j, hs, w, C) + (size_t)hs * w * C > (size_t)J * hs * w * C) ++fails;
            if (lmv_conf_offset(j, hs, w) + (size_t)hs * w > (size_t)J * hs * w) ++fails;
            if (lmv_table_offset(j, V, h, w) + (size_t)h * w * 3 > (size_t)V * h * w * 3) ++fails;
            if ((lmv_coef_offset(j) + LMV_COEF_N) * 8 > L.pose - L.coef) ++fails;
            if ((lmv_part_offset(j, part_ld - 1, part_ld) + LMV_PART_N) * 8 > L.total - L.part) ++fails;
            if (j + 1 < J && lmv_part_offset(j, part_ld - 1, part_ld) + LMV_PART_N > lmv_part_offset(j + 1, 0, part_ld)) ++fails;
            if (lmv_view_sums_offset(b, v, V) != (size_t)j * 16) ++fails;
          }
      }
  std::printf("%s: %ld cases, %ld failures\n", fails ? "FAILED" : "ok", cases, fails);
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


def test_index_and_workspace_arithmetic_on_the_host(tmp_path):
    cxx = _cxx()
    assert cxx is not None, 'no host C++ compiler'
    src = tmp_path / 'lm_views_sweep.cpp'
    src.write_text(SWEEP)
    exe = tmp_path / 'lm_views_sweep'
    base = [cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, str(src), '-o', str(exe)]
    # a stand-alone program: the sanitizers go in where the toolchain has their runtimes, else it is built plain
    if subprocess.run(base + ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(f'{9 * 8 * 4} cases, 0 failures')
