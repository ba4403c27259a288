"""CPU checks of the closed-form reference of ``hla_g2s_pose_score_bwd`` (tests/g2s_pose_score_bwd_ref.py).

1. In fp64 it equals ``torch.autograd.grad`` of the cost of ``g2s_pose_score_ref.score`` to 1e-10 * T on every case the GPU test
   runs.  The cost is taken through ``pose_score_bwd_ref.cost_clamp_const`` (the same values, and a finite autograd where nothing
   is in view and both sums are zero).
2. The fp32 run of the reference against its fp64 run on the scale T, on every case: its worst ratio per output is printed, the
   overall worst is ``REF32_WORST`` of the reference module, and the GPU gate is twice that.  Never derived from the kernel.
3. The conditions on the inputs: the out-of-view hypothesis sees nothing, every other one sees something in every sample, and in
   the 'crowded' case most neighbouring pixel pairs share a texel cell while some in every sample do not.
4. The library exports the two new symbols, and the workspace query refuses a Ford config and K = 0 without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import g2s_geo_ref as R
import g2s_pose_score_bwd_ref as GB
import g2s_pose_score_ref as GP

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('d_sat', 'd_grd', 'd_conf')


@pytest.mark.parametrize('case', GB.CASES, ids=GB.case_id)
def test_closed_form_equals_autograd_fp64(case):
    r = GB.reference(case)
    sat, grd, conf = R.cast(r.c, F64, requires_grad=True)
    sums, _, counts, cost, _ = GP.score(r.c, r.l, r.poses, r.w, F64, maps=(sat, grd, conf))
    safe = GB.cost_clamp_const(sums)
    seen = counts > 0
    assert torch.allclose(safe[seen], cost[seen], rtol=1e-14, atol=0) and bool((safe[~seen] == 0).all())
    loss = (r.d_cost.double() * safe).sum()
    wrt = [sat[r.l], grd[r.l]] + ([conf[r.l]] if r.w else [])
    want = list(torch.autograd.grad(loss, wrt)) + ([] if r.w else [torch.zeros_like(conf[r.l])])
    for name, a, b, t in zip(NAMES, r.grads, want, r.T):
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), name
        ratio, zeros = GB.worst_ratio(a, b, t)
        assert zeros and bool((b[t == 0] == 0).all()), name
        assert ratio <= 1e-10, (name, ratio)
    if not r.w:
        assert bool((r.grads[2] == 0).all()) and bool((r.T[2] == 0).all())


def _ref32(case):
    r = GB.reference(case)
    sums32 = GP.score(r.c, r.l, r.poses, r.w, F32)[0]
    got, _ = GB.grads(r.c, r.l, r.poses, r.w, sums32, r.d_cost, F32)
    return [GB.worst_ratio(a, b, t) for a, b, t in zip(got, r.grads, r.T)]


def test_fp32_reference_sizes_the_gpu_gate():
    """What sizes the gate of tests/test_g2s_pose_score_bwd_gpu.py: the reference's own fp32 run (maps, coordinates, sums and
    arithmetic in fp32) against its fp64 run, on the scale T, over all cases."""
    worst = [0.0, 0.0, 0.0]
    for case in GB.CASES:
        res = _ref32(case)
        print(f'GPSB ref32 {GB.case_id(case)}: worst |ref32 - ref64| / T = ' + ', '.join(f'{n} {r[0]:.2e}' for n, r in zip(NAMES, res)))
        for i, (ratio, zeros) in enumerate(res):
            assert zeros, (case, NAMES[i])
            assert ratio <= GB.TOL, (case, NAMES[i], ratio)
            worst[i] = max(worst[i], ratio)
    print('GPSB ref32 worst over all cases: ' + ', '.join(f'{n} {r:.2e}' for n, r in zip(NAMES, worst)) +
          f' (REF32_WORST {GB.REF32_WORST:.2e}, gate {GB.TOL:.2e})')
    # the constant is this measurement (fp32 sums may differ in the last digits from one CPU to another)
    assert 0.5 * GB.REF32_WORST <= max(worst) <= 1.05 * GB.REF32_WORST, worst


@pytest.mark.parametrize('case', GB.CASES, ids=GB.case_id)
def test_conditions_on_the_inputs(case):
    r = GB.reference(case)
    K = r.poses.shape[1]
    if r.out_k is not None:
        rows = GP.far_out_rows(r.c)
        assert bool((r.sums[rows, r.out_k, 6] == 0).all())
        only = torch.zeros_like(r.d_cost)
        only[:, r.out_k] = 1.5
        g, T = GB.grads(r.c, r.l, r.poses, r.w, r.sums, only)
        for a, t in zip(g, T):
            assert bool((a[rows] == 0).all()) and bool((t[rows] == 0).all())
    ordinary = [b for b in range(r.c.B) if b != getattr(r.c, 'out', None)]
    for k in range(K):
        if k != r.out_k:
            assert bool((r.counts[ordinary, k] > 0).all()), k
    assert bool((r.d_cost == 0).any()) or K == 1
    assert bool((r.d_cost > 0).any() and (r.d_cost < 0).any()) or K == 1


def test_crowded_case_shares_cells():
    r = GB.reference(GB.CROWDED)
    assert r.c.levels[r.l] == GB.CROWDED_LEVEL and r.w == 1
    for k in range(r.poses.shape[1]):
        if k == r.out_k:
            continue
        same, diff = GB.shared_cells(r.c, r.l, r.poses[:, k])
        print(f'GPSB crowded hypothesis {k}: neighbouring in-view pairs in one cell {same.tolist()}, in two {diff.tolist()}')
        assert bool((same >= diff).all()) and bool((diff >= 1).all()), (k, same, diff)


def test_scale_invariance():
    """The cost does not depend on the scale of either map, so each sample's gradient is orthogonal to its map."""
    for case in (GB.CASES[4], GB.CASES[5], GB.CROWDED):
        r = GB.reference(case)
        sat, grd, _ = R.cast(r.c, F64)
        for name, x, d in (('sat', sat[r.l], r.grads[0]), ('grd', grd[r.l], r.grads[1])):
            dot, mag = (x * d).flatten(1).sum(1), (x * d).abs().flatten(1).sum(1)
            assert bool((mag > 0).all()) and bool((dot.abs() <= 1e-12 * mag).all()), (case, name, (dot.abs() / mag).max())


def test_header_declares_and_library_exports_g2s_pose_score_bwd():
    from highlyaccurate_amd import _lib
    from highlyaccurate_amd import build as B
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hla.h')).read(), flags=re.S)
    names = ('hla_g2s_pose_score_bwd', 'hla_g2s_pose_score_bwd_workspace_bytes')
    for name in names:
        assert re.search(r'\b%s\s*\(' % name, text), name
    lib = C.CDLL(B.build())
    assert all(hasattr(lib, n) for n in names)
    bound = _lib.load()
    assert len(bound.hla_g2s_pose_score_bwd.argtypes) == 14 and len(bound.hla_g2s_pose_score_bwd_workspace_bytes.argtypes) == 4


def test_workspace_query_refuses_ford_and_k0_without_a_gpu():
    from highlyaccurate_amd import _lib
    lib = _lib.load()
    cfg, lv = _lib.S2GConfig(), _lib.S2GLevel()
    cfg.n_levels, cfg.n_iters, cfg.dof = 1, 1, 3
    cfg.shift_range_lat = cfg.shift_range_lon = 20.0
    cfg.rotation_range = 10.0
    lv.A, lv.h, lv.w, lv.C, lv.meter_per_pixel, lv.feat_dtype = 16, 4, 8, 64, 0.5, _lib.HLA_F32
    dummy = (C.c_float * 4)()
    lv.sat_feat = lv.grd_feat = C.addressof(dummy)           # never read by a workspace query
    query = lambda B, K: lib.hla_g2s_pose_score_bwd_workspace_bytes(C.byref(cfg), C.byref(lv), B, K)
    assert query(2, 5) >= 2 * 5 * 8 * 4
    assert query(2, 0) == 0 and 'K >= 1' in lib.hla_last_error().decode()
    cfg.ford = 1
    assert query(2, 5) == 0 and 'KITTI-only' in lib.hla_last_error().decode()
    cfg.ford = 0
    assert query(2, 5) > 0
