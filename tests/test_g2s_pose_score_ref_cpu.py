"""CPU checks of LM_G2SP's pose-search layer: the fp64 reference of ``hla_g2s_pose_score`` (tests/g2s_pose_score_ref.py) and its
inputs on every case tests/test_g2s_pose_score_gpu.py runs -- the closing formula against the cost formed directly, the headroom
the reference's own fp32 run leaves inside the GPU gate, the far-out hypothesis, the planted minimum's margins -- and the host
layer: the methods, the header's declarations and citations, the library's exports, the binding, the argument errors."""
import os
import re

import pytest
import torch

import g2s_geo_ref as R
import g2s_pose_score_ref as GP

F64, F32 = torch.float64, torch.float32
TOL_SUM = 2e-6           # the gate of tests/test_g2s_pose_score_gpu.py (TOL_SUM of every LM kernel suite)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(tag, c, l, w, poses, out_k):
    hw = c.levels[l][2]
    # the inputs: no (hypothesis, pixel) within GUARD of a texel line or a border
    for k in range(poses.shape[1]):
        d = GP.min_dist(GP.uv_of(c, l, poses[:, k], F64), hw)
        assert float(d.min()) > R.GUARD, (tag, k, d)
    sums, mags, counts, cost, direct = GP.score(c, l, poses, w, F64)
    s32, _, n32, _, _ = GP.score(c, l, poses, w, F32)
    seen = counts > 0
    # the closing formula equals sum w (f/nf - s/ns)^2 formed directly
    err = (cost[seen] - direct[seen]).abs().max().item()
    print(f'GPSREF {tag}: |formula - direct| = {err:.2e}, in view {counts.min().item()}..{counts.max().item()} of {hw}')
    assert err <= 1e-14 and torch.equal(torch.isinf(cost), ~seen) and torch.equal(torch.isinf(direct), ~seen)
    # the fp32 run of the same code stays inside the GPU gate, with the same pixels in view
    ratio = ((s32.double() - sums).abs() / torch.where(mags > 0, mags, torch.ones_like(mags))).max().item()
    print(f'GPSREF {tag}: fp32 reference |ref32 - ref64| / T_k = {ratio:.2e} (gate {TOL_SUM:.0e})')
    assert ((s32.double() - sums).abs() <= TOL_SUM * mags).all()
    assert torch.equal(n32, counts) and torch.equal(sums[..., 6], counts.double())
    # the far-out hypothesis: nothing in view, zero sums, the pose-independent slot intact, cost +inf
    # (but for the sample of the 'behind' case: its centre pixel has q0 = 0 and lands on u = 0, in bounds, at EVERY pose)
    k, rows = out_k, GP.far_out_rows(c)
    assert (counts[rows, k] == 0).all() and (sums[rows, k, :7] == 0).all() and (sums[rows, k, 7] > 0).all()
    assert (cost[rows, k] == float('inf')).all()
    assert (sums[..., 7] == sums[:, :1, 7]).all()
    # something is in view somewhere (the sample of the 'out' case never is), and the cost is in [0, 4]
    ordinary = [b for b in range(c.B) if b != getattr(c, 'out', None)]
    assert (counts[ordinary][:, 0] > 0).all(), counts
    assert (cost[seen] >= -1e-12).all() and (cost[seen] <= 4 + 1e-12).all()
    if not w:
        assert torch.equal(sums[..., 3:6], sums[..., 0:3])


@pytest.mark.parametrize('run', GP.RUNS, ids=GP.run_id)
def test_reference_formula_headroom_and_far_out_hypothesis(run):
    key, l, w = run
    c = GP.get(*key)
    _check(GP.run_id(run), c, l, w, GP.hypotheses(c, l), GP.OUT_K)


@pytest.mark.parametrize('proj', ['geo', 'nn'])
def test_the_seventy_hypotheses_meet_the_same_conditions(proj):
    c, l, w, poses = GP.k70(proj)
    _check(f'k70 {proj}', c, l, w, poses, GP.K70_OUT)


@pytest.mark.parametrize('proj', ['geo', 'nn'])
def test_planted_minimum_separates(proj):
    """The satellite map is the ground map projected at hypothesis 2's pose wherever that is in view: that hypothesis scores
    ~0, every other one that sees anything >= 1 (the margins tests/test_g2s_pose_score_gpu.py relies on)."""
    c, l, poses = GP.planted(proj)
    _, _, counts, cost, _ = GP.score(c, l, poses, 0, F64)
    cost = cost.float()
    K = poses.shape[1]
    others = cost[:, [k for k in range(K) if k != GP.PLANTED_K]]
    seen = counts[:, [k for k in range(K) if k != GP.PLANTED_K]] > 0
    print(f'GPSREF planted {proj}: cost[2] = {cost[:, GP.PLANTED_K].max():.2e}, min other = {others[seen].min():.3f}, in view {counts.tolist()}')
    assert (counts[:, GP.PLANTED_K] >= 8).all()
    assert (cost[:, GP.PLANTED_K] <= 1e-5).all() and (others[seen] >= 1).all() and (others[~seen] == float('inf')).all()
    assert seen.sum() >= 4 * c.B and (counts[:, GP.OUT_K] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# host layer
# ----------------------------------------------------------------------------------------------------------------------
def test_model_has_the_search_methods():
    from highlyaccurate_amd import models_kitti
    from highlyaccurate_amd.models_kitti import LM_G2SP
    assert callable(getattr(LM_G2SP, 'score_poses', None)) and callable(getattr(LM_G2SP, 'forward_search', None))
    assert callable(models_kitti.pose_grid)


def test_header_declares_library_exports_and_binding_binds():
    import ctypes
    from highlyaccurate_amd import _lib, build as B
    hdr = open(os.path.join(ROOT, 'include', 'hla.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    names = ('hla_g2s_pose_score', 'hla_g2s_pose_score_workspace_bytes')
    for name in names:
        assert re.search(r'\b%s\s*\(' % name, code), name
    comment = [m for m in re.findall(r'/\*.*?\*/', hdr, flags=re.S) if 'Pose scoring in the ground -> satellite direction' in m]
    assert len(comment) == 1
    for cite in ('models_kitti.py:163-303', '289-332', '333-379'):
        assert cite in comment[0], cite
    lib = ctypes.CDLL(B.build())
    bound = _lib.load()
    for name in names:
        assert hasattr(lib, name), name
        assert getattr(bound, name).argtypes is not None, name
    assert len(bound.hla_g2s_pose_score.argtypes) == 13 and len(bound.hla_g2s_pose_score_workspace_bytes.argtypes) == 4


def _model(proj='geo', **kw):
    from highlyaccurate_amd.models_kitti import LM_G2SP
    return LM_G2SP(R.make_args(N_iters=1, using_weight=0, proj=proj, **kw))


def test_score_poses_argument_errors():
    from highlyaccurate_amd._lib import HlaError
    net = _model()
    feats = [torch.zeros(2, 4, 4, 64), torch.zeros(2, 8, 8, 64)]
    K = torch.eye(3)[None].repeat(2, 1, 1)
    for bad in (torch.zeros(3), torch.zeros(5, 2), torch.zeros(3, 5, 3), torch.zeros(0, 3), torch.zeros(2, 0, 3), torch.zeros(2, 5, 3, 1)):
        with pytest.raises(ValueError, match='poses'):
            net.score_poses(feats, feats, [None, None], K, (32, 32), bad, 0)
    for level in (-1, 2):
        with pytest.raises(ValueError, match='level'):
            net.score_poses(feats, feats, [None, None], K, (32, 32), torch.zeros(5, 3), level)
    with pytest.raises(HlaError, match='HIP device'):           # CPU tensors: no CPU path, like lm_solve
        net.score_poses(feats, feats, [None, None], K, (32, 32), torch.zeros(5, 3), 1)


def test_forward_search_argument_errors():
    from highlyaccurate_amd._lib import HlaError
    from highlyaccurate_amd.models_kitti import pose_grid
    net = _model()
    K = torch.eye(3)[None].repeat(2, 1, 1)
    with pytest.raises(HlaError, match='HIP device'):
        net.forward_search(torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 32, 128), K, pose_grid(3, 1, 1))
