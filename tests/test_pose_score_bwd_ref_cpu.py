"""CPU checks of the closed-form reference of ``hla_s2g_pose_score_bwd`` (tests/pose_score_bwd_ref.py).

1. In fp64 it equals ``torch.autograd.grad`` of the cost of ``pose_score_ref.score`` to 1e-10 * T on every case of
   ``pose_score_ref.GPU_CASES`` with and without weights (the out-of-view hypothesis included) and on a level with deferred norms.
   Autograd of the header's formula is NaN where sum s^2 = 0 (0 x the infinite slope of sqrt at 0), so it is taken twice: of
   ``score``'s own cost over the hypotheses that see something, and over ALL hypotheses of the same formula with the clamped norm
   written as the constant it is (``_cost_clamp_const``; its values equal ``score``'s cost).
2. The fp32 run of the reference against its fp64 run on the scale T, on every case tests/test_pose_score_bwd_gpu.py runs.  It
   does NOT stay inside the project's TOL_SUM = 2e-6: the worst ratio is 3.06e-4 (d_sat at K = 33; d_grd 5.7e-5, d_conf 1.8e-6 --
   T takes |s| of the sampled value and the fp32 run forms its bilinear weights from fp32 coordinates).  The gate of the GPU test
   is therefore twice that worst ratio, 6.12e-4 (``pose_score_bwd_ref.TOL``), and this test holds the fp32 run inside it.
3. Scale invariance: sum sat x d_sat and sum grd x d_grd vanish per sample, to 1e-12 of the sum of the absolute products."""
import os
import re

import pytest
import torch

import lm_kernel_ref as R
import pose_score_bwd_ref as PB
import pose_score_ref as PS

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_cost_clamp_const = PB.cost_clamp_const


def _autograd(geom64, lv, poses, w, dc, cols=None):
    """d(sum d_cost x cost)/d(sat, grd, conf) by autograd on fresh fp64 leaves; cols: the hypotheses to take (score's own cost),
    None: all of them through ``_cost_clamp_const``."""
    leaf = R.cast_level(lv, F64, requires_grad=True)
    if cols is None:
        sums, _, _, cost, _ = PS.score(geom64, leaf, poses, w)
        safe = _cost_clamp_const(sums)
        assert torch.allclose(safe, cost, rtol=1e-14, atol=0)
        loss = (dc.double() * safe).sum()
    else:
        _, _, _, cost, _ = PS.score(geom64, leaf, poses[:, cols], w)
        loss = (dc.double()[:, cols] * cost).sum()
    wrt = [leaf.sat, leaf.grd] + ([leaf.conf] if w else [])
    g = list(torch.autograd.grad(loss, wrt))
    return g + ([torch.zeros_like(leaf.conf)] if not w else [])


def _check_autograd(tag, geom, ref_lv, poses, w, dc):
    g64 = R.cast_geom(geom, F64)
    sums, _, counts, _, _ = PS.score(g64, ref_lv, poses, w)
    seen = [k for k in range(poses.shape[1]) if bool((sums[:, k, 0] > 0).all())]
    assert len(seen) < poses.shape[1] or poses.shape[1] == 1, 'the case has no out-of-view hypothesis'
    for cols in (None, seen):
        dck = dc if cols is None else dc.clone()
        if cols is not None:
            dck[:, [k for k in range(poses.shape[1]) if k not in seen]] = 0
        got, T = PB.grads(g64, ref_lv, poses, w, sums, dck)
        want = _autograd(g64, ref_lv, poses, w, dc, cols)
        for name, a, b, t in zip(('d_sat', 'd_grd', 'd_conf'), got, want, T):
            assert torch.isfinite(a).all() and torch.isfinite(b).all(), (tag, name)
            ratio, zeros = PB.worst_ratio(a, b, t)
            assert zeros and bool((b[t == 0] == 0).all()), (tag, name)
            assert ratio <= 1e-10, (tag, name, 'all' if cols is None else 'seen', ratio)
        assert (got[1][:, :, :ref_lv.row0] == 0).all() and (got[2][:, :, :ref_lv.row0] == 0).all()


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('case', PS.GPU_CASES, ids=str)
def test_closed_form_equals_autograd_fp64(case, using_weight):
    ford, shape, Cn, A, B, _ = case
    geom, run_lv, inv, ref_lv, poses, dc = PB.case_inputs((ford, shape, Cn, A, B, using_weight, PS.K_CASE, PS.OUT_K, False))
    _check_autograd(f'{case} w{using_weight}', geom, ref_lv, poses, using_weight, dc)


@pytest.mark.parametrize('using_weight', [0, 1])
def test_closed_form_equals_autograd_with_deferred_norms(using_weight):
    """The reference reads raw map x inverse norm; the gradient is the one with respect to that product."""
    geom, run_lv, inv, ref_lv, poses, dc = PB.case_inputs((0, 'ragged', 128, 16, 3, using_weight, PS.K_CASE, PS.OUT_K, True))
    assert inv is not None and not torch.equal(run_lv.sat.double(), ref_lv.sat)
    _check_autograd(f'deferred w{using_weight}', geom, ref_lv, poses, using_weight, dc)


@pytest.mark.parametrize('case', PB.CASES, ids=str)
def test_fp32_reference_is_inside_the_gpu_gate(case):
    """What sizes the gate of tests/test_pose_score_bwd_gpu.py: the reference's own fp32 run (maps, sums and arithmetic in fp32)
    against its fp64 run, on the scale T.  Never derived from the kernel."""
    c = PB.reference(case)
    w = case[5]
    lv32, g32 = R.cast_level(c['ref_lv'], F32), R.cast_geom(c['geom'], F32)
    sums32 = PS.score(g32, lv32, c['poses'], w)[0]
    got, _ = PB.grads(g32, lv32, c['poses'], w, sums32, c['d_cost'])
    seen = []
    for name, a, b, t in zip(('d_sat', 'd_grd', 'd_conf'), got, c['grads'], c['T']):
        ratio, zeros = PB.worst_ratio(a, b, t)
        print(f'PSB ref32 {case} {name}: worst |ref32 - ref64| / T = {ratio:.2e} (gate {PB.TOL:.1e})')
        seen.append((name, ratio, zeros))
    for name, ratio, zeros in seen:
        assert zeros, (case, name)
        assert ratio <= PB.TOL, (case, name, ratio)


@pytest.mark.parametrize('case', [PB.CASES[2], PB.CASES[3], PB.CASES[8], PB.CASES[-1]], ids=str)
def test_scale_invariance(case):
    """The cost does not depend on the scale of either map, so each sample's gradient is orthogonal to its map."""
    c = PB.reference(case)
    lv = c['ref_lv']
    d_sat, d_grd, _ = c['grads']
    for name, x, d in (('sat', lv.sat, d_sat), ('grd', lv.grd, d_grd)):
        dot, mag = (x * d).flatten(1).sum(1), (x * d).abs().flatten(1).sum(1)
        assert bool((mag > 0).all()) and bool((dot.abs() <= 1e-12 * mag).all()), (case, name, (dot.abs() / mag).max())


def test_out_of_view_hypothesis_gives_the_satellite_map_nothing():
    case = PB.CASES[2]
    c = PB.reference(case)
    only = torch.zeros_like(c['d_cost'])
    only[:, PS.OUT_K] = 1.5
    g, T = PB.grads(R.cast_geom(c['geom'], F64), c['ref_lv'], c['poses'], case[5], c['sums'], only)
    assert (c['counts'][:, PS.OUT_K, 0] == 0).all() and (g[0] == 0).all() and (T[0] == 0).all()
    assert (g[1] != 0).any()                      # the ground map still feels its own norm


def test_header_declares_and_library_exports_pose_score_bwd():
    from highlyaccurate_amd import _lib
    from highlyaccurate_amd import build as B
    import ctypes
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hla.h')).read(), flags=re.S)
    names = ('hla_s2g_pose_score_bwd', 'hla_s2g_pose_score_bwd_workspace_bytes')
    for name in names:
        assert re.search(r'\b%s\s*\(' % name, text), name
    lib = ctypes.CDLL(B.build())
    assert all(hasattr(lib, n) for n in names)
    bound = _lib.load()
    assert len(bound.hla_s2g_pose_score_bwd.argtypes) == 13 and len(bound.hla_s2g_pose_score_bwd_workspace_bytes.argtypes) == 4
