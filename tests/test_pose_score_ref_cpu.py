"""CPU checks of the pose-search layer: the fp64 reference of ``hla_s2g_pose_score`` (tests/pose_score_ref.py) against the LM
loop's own reference, the gate its fp32 run leaves room for on every case tests/test_pose_score_gpu.py runs, and the host logic of
``forward_search`` (``pose_grid``, the eligibility rule, argument errors, the ABI surface)."""
import os
import re

import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import pose_score_ref as PS

F64, F32 = torch.float64, torch.float32
TOL_SUM = 2e-6           # the gate of tests/test_pose_score_gpu.py (tests/test_lm_kernels_vs_fp64.py's TOL_SUM)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRID = [(0, 'ragged', C, 16, 3, w) for C in (16, 64, 128, 256) for w in (0, 1)]

_CACHE = {}


def _run(ford, shape, C, A, B, w):
    """(geom, level, poses, fp64 result, fp32 result) of one case, computed once."""
    key = (ford, shape, C, A, B, w)
    if key not in _CACHE:
        geom, lv = R.make_geom(ford, B), R.make_level(ford, shape, C, A, B, R.case_seed(ford, shape, C, A, B))
        poses = PS.hypotheses(B, PS.K_CASE, R.case_seed('ps', *key), out_of_view=PS.OUT_K)
        r64 = PS.score(R.cast_geom(geom, F64), R.cast_level(lv, F64), poses, w)
        r32 = PS.score(R.cast_geom(geom, F32), R.cast_level(lv, F32), poses, w)
        _CACHE[key] = (geom, lv, poses, r64, r32)
    return _CACHE[key]


@pytest.mark.parametrize('case', [(0, 'ragged', 128, 16, 3, 1), (1, 'ragged', 64, 13, 3, 0), (0, 'skip', 128, 16, 2, 1)], ids=str)
def test_norm_sums_are_the_lm_references(case):
    """Slots 0 and 1 are the ||s||^2 and ||g||^2 of lm_kernel_ref.step_sums at the same pose, exactly."""
    ford, shape, C, A, B, w = case
    geom, lv, poses, r64, _ = _run(*case)
    g64, l64 = R.cast_geom(geom, F64), R.cast_level(lv, F64)
    for k in (0, 1, 5):          # in-view hypotheses (step_sums evaluates the batch alone)
        sums, _, _ = R.level_sums(g64, l64, R.pose_cols(poses[:, k], F64), w)
        assert torch.equal(r64[0][:, k, :2], sums[:, :2]), (case, k)


@pytest.mark.parametrize('case', GRID + PS.GPU_CASES, ids=str)
def test_cost_formula_counts_and_fp32_headroom(case):
    geom, lv, poses, r64, r32 = _run(*case)
    sums, mags, counts, cost, direct = r64
    # the closing formula equals sum w (s/ns - g/ng)^2 formed directly
    err = (cost - direct).abs().max().item()
    print(f'PSREF {case}: |formula - direct| = {err:.2e}')
    assert err <= 1e-14
    # the fp32 run of the same code stays inside the GPU gate
    ratio = ((r32[0].double() - sums).abs() / torch.where(mags > 0, mags, torch.ones_like(mags))).max().item()
    print(f'PSREF {case}: fp32 reference |ref32 - ref64| / T_k = {ratio:.2e} (gate {TOL_SUM:.0e})')
    assert ((r32[0].double() - sums).abs() <= TOL_SUM * mags).all()
    assert torch.equal(r32[2], counts)
    # counts: the zero pose sees a good part of the border table; in view implies ground mask
    assert (counts[:, 0, 0] >= 0.2 * counts[:, 0, 1]).all() and (counts[..., 0] <= counts[..., 1]).all()
    # the out-of-view hypothesis: nothing sampled, cost 1 without weights
    k = PS.OUT_K
    assert (sums[:, k, [0, 2, 3, 5]] == 0).all() and (counts[:, k, 0] == 0).all() and (counts[:, k, 1] > 0).all()
    if not case[5]:
        assert (cost[:, k].float() == 1).all(), cost[:, k]
        assert torch.equal(sums[..., 3:6], sums[..., 0:3])
    assert (cost >= -1e-12).all() and (cost <= 4 + 1e-12).all()


@pytest.mark.parametrize('ford', [0, 1])
@pytest.mark.parametrize('shape,C', [('ragged', 128), ('mid', 16)])
def test_planted_minimum_separates(ford, shape, C):
    """The ground map sampled from the satellite map at hypothesis 2's pose: that hypothesis scores ~0, every other one >= 1
    (the margins tests/test_pose_score_gpu.py relies on)."""
    B, K = 2, 7
    poses = PS.planted_poses(B)
    geom, lv = PS.planted_level(ford, shape, C, 16, B, R.case_seed('planted-level', ford, shape, C), 2, poses)
    _, _, _, cost, _ = PS.score(R.cast_geom(geom, F64), R.cast_level(lv, F64), poses, 0)
    cost = cost.float()          # the kernel's output type: the out-of-view hypothesis' 1 - 1e-16 is 1
    others = cost[:, [k for k in range(K) if k != 2]]
    print(f'PSREF planted ford{ford} {shape} C{C}: cost[2] = {cost[:, 2].max():.2e}, min other = {others.min():.3f}')
    assert (cost[:, 2] <= 1e-5).all() and (others >= 1).all()


# ----------------------------------------------------------------------------------------------------------------------
# host logic
# ----------------------------------------------------------------------------------------------------------------------
def test_pose_grid_values_and_order():
    from highlyaccurate_amd._s2gp import pose_grid
    from highlyaccurate_amd import models_kitti, models_ford
    assert models_kitti.pose_grid is pose_grid and models_ford.pose_grid is pose_grid
    g = pose_grid(3, 1, 3, span=(1.0, 1.0, 0.5))
    assert g.dtype == torch.float32 and tuple(g.shape) == (9, 3)
    want = [[0, 0, 0], [-1, 0, -.5], [-1, 0, 0], [-1, 0, .5], [0, 0, -.5], [0, 0, .5], [1, 0, -.5], [1, 0, 0], [1, 0, .5]]
    assert torch.equal(g, torch.tensor(want, dtype=torch.float32))
    g = pose_grid(5, 3, 1)
    assert tuple(g.shape) == (15, 3) and torch.equal(g[0], torch.zeros(3))
    assert sorted(set(g[:, 0].tolist())) == [-1.0, -0.5, 0.0, 0.5, 1.0] and sorted(set(g[:, 1].tolist())) == [-1.0, 0.0, 1.0]
    assert len({tuple(r) for r in g.tolist()}) == 15
    assert torch.equal(pose_grid(1, 1, 1), torch.zeros(1, 3))
    for bad in ((2, 1, 1), (1, 0, 1), (1, 1, 4)):
        with pytest.raises(ValueError):
            pose_grid(*bad)


def test_eligibility_rule_and_fallback():
    from highlyaccurate_amd._s2gp import eligible_cost
    inf = float('inf')
    cost = torch.tensor([[1.9, 1.0, 0.5, 1.2], [0.7, 0.6, 0.5, 0.4], [1.5, 1.0, 1.0, 1.0]])
    sums = torch.zeros(3, 4, 8, dtype=F64)
    sums[0, :, 6] = torch.tensor([100., 0., 49., 50.])          # nothing / too little in view loses its low cost
    sums[1, :, 6] = torch.tensor([10., 20., 30., 40.])
    sums[2, :, 6] = float('nan')                                  # no candidate is eligible: candidate 0 stands
    out = eligible_cost(cost, sums, 0.5)
    assert out.dtype == cost.dtype
    assert out[0].tolist() == [pytest.approx(1.9), inf, inf, pytest.approx(1.2)]
    assert out[1].tolist() == [inf, pytest.approx(0.6), pytest.approx(0.5), pytest.approx(0.4)]
    assert out[2, 1:].tolist() == [inf] * 3 and torch.isfinite(out[2, 0])
    idx = torch.topk(out, 2, dim=1, largest=False).indices
    assert idx[0].tolist() == [3, 0] and idx[1].tolist() == [3, 2] and idx[2, 0].item() == 0
    assert torch.equal(cost[0], torch.tensor([1.9, 1.0, 0.5, 1.2]))      # the input is left as it was
    # min_in_view = 0: every candidate is eligible
    assert torch.equal(eligible_cost(cost[:2], sums[:2], 0.0), cost[:2])


def test_poses_shape_errors():
    from types import SimpleNamespace
    from highlyaccurate_amd._s2gp import S2GPBase, _poses_arg
    assert tuple(_poses_arg(torch.zeros(5, 3), 2).shape) == (2, 5, 3)
    assert tuple(_poses_arg(torch.zeros(2, 5, 3), 2).shape) == (2, 5, 3)
    assert tuple(_poses_arg([[0, 0, 0]], 4).shape) == (4, 1, 3)
    feats = [torch.zeros(2, 4, 4, 16)]
    for bad in (torch.zeros(3), torch.zeros(5, 2), torch.zeros(3, 5, 3), torch.zeros(0, 3), torch.zeros(2, 0, 3), torch.zeros(2, 5, 3, 1)):
        with pytest.raises(ValueError, match='poses'):
            _poses_arg(bad, 2)
        with pytest.raises(ValueError, match='poses'):
            S2GPBase.score_poses(SimpleNamespace(), feats, feats, [None], (32, 32), bad, 0)


def test_models_have_forward_search():
    from highlyaccurate_amd.models_kitti import LM_S2GP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    assert hasattr(LM_S2GP, 'forward_search') and hasattr(LM_S2GP_Ford, 'forward_search')
    assert hasattr(LM_S2GP, 'score_poses') and hasattr(LM_S2GP_Ford, 'score_poses')


def test_header_declares_and_library_exports_pose_score():
    import ctypes
    from highlyaccurate_amd import _lib, build as B
    hdr = open(os.path.join(ROOT, 'include', 'hla.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('hla_s2g_pose_score', 'hla_s2g_pose_score_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, code), name
    assert 'models_kitti.py:982-996' in hdr and 'models_ford.py:414-430' in hdr
    lib = ctypes.CDLL(B.build())
    assert hasattr(lib, 'hla_s2g_pose_score') and hasattr(lib, 'hla_s2g_pose_score_workspace_bytes')
    bound = _lib.load()
    assert bound.hla_s2g_pose_score.argtypes is not None and bound.hla_s2g_pose_score_workspace_bytes.argtypes is not None
