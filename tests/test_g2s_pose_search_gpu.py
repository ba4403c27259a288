"""``LM_G2SP.forward_search``: candidates scored on feature maps extracted once (``score_poses`` -> hla_g2s_pose_score), the LM
loop from the best few, the best final pose kept -- for proj='geo' without and with weights and for proj='nn'.

sat 128 x 128 and grd 64 x 256 (for 'nn' the folded ground maps then have the satellite maps' sizes), B = 2, N_iters = 2, seeded
random weights.  Everything the search composes is compared bit for bit with the hand composition; the finest level's scores are
held against tests/g2s_pose_score_ref.py in fp64 on the downloaded feature maps, inside the sum gate of the kernel tests."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import g2s_geo_ref as R
import g2s_pose_score_ref as GP

pytestmark = pytest.mark.gpu

GRD_HW, SAT_A, B = (64, 256), 128, 2
SEED = 1
TOL_SUM = 2e-6
F64 = torch.float64
RANGES = (20.0, 20.0, 10.0)
MODELS = {'geo': ('geo', 0), 'geo_weighted': ('geo', 1), 'nn': ('nn', 0)}
# the KITTI intrinsics (models_kitti.py:657-660) scaled from the 375 x 1242 image to GRD_HW, one sample slightly off
CAMERA_K = [[[582.9802 * 256 / 1242, 0.0, 496.2420 * 256 / 1242], [0.0, 482.7076 * 64 / 375, 125.0034 * 64 / 375], [0.0, 0.0, 1.0]],
            [[560.0 * 256 / 1242, 0.0, 510.0 * 256 / 1242], [0.0, 470.0 * 64 / 375, 120.0 * 64 / 375], [0.0, 0.0, 1.0]]]


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _net(name):
    from highlyaccurate_amd.models_kitti import LM_G2SP
    proj, uw = MODELS[name]
    torch.manual_seed(SEED)
    return LM_G2SP(R.make_args(RANGES, N_iters=2, damping=1.0, using_weight=uw, proj=proj)).to(_dev()).eval()


def _inputs():
    g = torch.Generator().manual_seed(SEED + 1)
    sat = torch.rand(B, 3, SAT_A, SAT_A, generator=g).to(_dev())
    grd = torch.rand(B, 3, *GRD_HW, generator=g).to(_dev())
    return sat, grd, torch.tensor(CAMERA_K, dtype=torch.float32).to(_dev())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _features(net, sat, grd):
    """The extraction of ``forward``'s inference branch."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc
    sat_feats, _, sat_inv = vgg_forward_nhwc(net.SatFeatureNet, sat, want_conf=False, defer_norm=True)
    grd_feats, grd_confs, grd_inv = vgg_forward_nhwc(net.GrdFeatureNet, grd, want_conf=bool(net.using_weight), defer_norm=True)
    return sat_feats, grd_feats, grd_confs, sat_inv, grd_inv


def _rule(cost, sums, min_in_view):
    """The eligibility rule, written out independently of ``_s2gp.eligible_cost``."""
    out = cost.clone()
    for b in range(cost.shape[0]):
        n = sums[b, :, 6]
        ok = n >= min_in_view * n.max()
        out[b, ~ok] = float('inf')
        if not ok.any():
            out[b, 0] = 0.0
    return out


@pytest.mark.parametrize('name', list(MODELS))
def test_single_zero_candidate_is_forward(name):
    """candidates = [[0, 0, 0]], top_m = 1: the loop from the zero pose, i.e. forward(mode='test'), bit for bit; no random draws."""
    net = _net(name)
    sat, grd, K = _inputs()
    with torch.no_grad():
        want = net(sat, grd, K, mode='test')
        state = torch.get_rng_state()
        got = net.forward_search(sat, grd, K, [[0.0, 0.0, 0.0]], top_m=1)
    assert torch.equal(torch.get_rng_state(), state)
    for a, b in zip(got, want):
        assert torch.isfinite(b).all() and _same(a, b), (name, a, b)
    ls = net.last_search
    assert tuple(ls['traces'].shape) == (B, 1, 2, 3, 3) and tuple(ls['cost'].shape) == (B, 1) and (ls['best'] == 0).all()


@pytest.mark.parametrize('name', list(MODELS))
def test_search_is_its_hand_composition_and_scores_match_fp64(name):
    from highlyaccurate_amd.models_kitti import pose_grid
    net = _net(name)
    sat, grd, K = _inputs()
    cands, M = pose_grid(3, 3, 3), 2
    got = net.forward_search(sat, grd, K, cands, top_m=M)
    ls = dict(net.last_search)
    L, Kc = 3, cands.shape[0]
    assert set(ls) == {'cost', 'sums', 'start_index', 'traces', 'final_cost', 'best'}
    assert tuple(ls['cost'].shape) == (B, Kc) and tuple(ls['sums'].shape) == (B, Kc, 8) and tuple(ls['start_index'].shape) == (B, M)
    assert tuple(ls['traces'].shape) == (B, M, 2, L, 3) and tuple(ls['final_cost'].shape) == (B, M) and tuple(ls['best'].shape) == (B,)
    assert all(tuple(t.shape) == (B,) for t in got)

    # the hand composition: score_poses -> eligible rule -> topk -> lm_solve(init_pose) -> score_poses -> argmin
    with torch.no_grad():
        sat_feats, grd_feats, grd_confs, sat_inv, grd_inv = _features(net, sat, grd)
        hw = GRD_HW
        cost, sums = net.score_poses(sat_feats, grd_feats, grd_confs, K, hw, cands, 0, sat_inv, grd_inv)
        assert _same(cost, ls['cost']) and _same(sums, ls['sums'])
        idx = torch.topk(_rule(cost, sums, 0.5), M, dim=1, largest=False, sorted=True).indices
        assert torch.equal(idx, ls['start_index'])
        finals = []
        for m in range(M):
            start = cands.to(_dev())[idx[:, m]].contiguous()
            tr = net.lm_solve(sat_feats, grd_feats, grd_confs, K, hw, start, sat_inv, grd_inv)
            assert _same(tr, ls['traces'][:, m]), m
            finals.append(tr[:, -1, -1])
        finals = torch.stack(finals, 1).contiguous()
        fcost, fsums = net.score_poses(sat_feats, grd_feats, grd_confs, K, hw, finals, L - 1, sat_inv, grd_inv)
        assert _same(fcost, ls['final_cost'])
        best = fcost.argmin(1)
        assert torch.equal(best, ls['best'])
        pose = finals[torch.arange(B), best]
        for a, b in zip(got, (pose[:, 1], pose[:, 0], pose[:, 2])):
            assert _same(a, b)
    assert torch.isfinite(finals).all() and (sums[..., 6] > 0).any(1).all()

    # the finest level's scores against fp64 on the same maps (raw maps x their inverse norms)
    nc = lambda t: t.permute(0, 3, 1, 2).double().cpu()
    inv = lambda v, l: v[l].double().cpu().view(-1, 1, 1, 1)
    s64 = [nc(t) * inv(sat_inv, l) for l, t in enumerate(sat_feats)]
    g64 = [nc(t) * inv(grd_inv, l) for l, t in enumerate(grd_feats)]
    c64 = [t.double().cpu()[:, None] if t is not None else None for t in grd_confs]
    case = SimpleNamespace(name=name, proj=MODELS[name][0], B=B, K=K.cpu(), ori_hw=GRD_HW, ranges=RANGES,
                           levels=[(t.shape[-1], t.shape[1], tuple(g.shape[-2:])) for t, g in zip(s64, g64)])
    ref, mags, counts, rcost, _ = GP.score(case, L - 1, finals.cpu(), MODELS[name][1], F64, maps=(s64, g64, c64))
    err = (fsums.cpu() - ref).abs().numpy()
    m = mags.numpy()
    print(f'GPS search {name}: finest-level sums worst |hip - ref64| / T_k = {(err / np.where(m > 0, m, 1.0)).max():.2e} (limit {TOL_SUM:.0e}); '
          f'|cost - ref64 cost| = {(fcost.cpu().double() - rcost).abs().max():.2e}; in view {counts.tolist()}')
    assert (err <= TOL_SUM * m).all() and np.array_equal(fsums[..., 6].cpu().numpy(), counts.double().numpy())
    assert (counts > 0).any(1).all()


def test_argument_errors():
    from highlyaccurate_amd.models_kitti import pose_grid
    net = _net('geo')
    sat, grd, K = _inputs()
    cands = pose_grid(3, 1, 1)
    for bad in (0, 4):
        with pytest.raises(ValueError, match='top_m'):
            net.forward_search(sat, grd, K, cands, top_m=bad)
    with pytest.raises(ValueError, match='candidates'):
        net.forward_search(sat, grd, K, torch.zeros(3, 2))
    with pytest.raises(ValueError, match='candidates'):
        net.forward_search(sat, grd, K, torch.zeros(B + 1, 3, 3))
    with pytest.raises(ValueError, match='expected sat_map'):
        net.forward_search(sat[:1], grd, K, cands)
    with pytest.raises(ValueError, match='level'):
        net.forward_search(sat, grd, K, cands, score_level=3)
    nn = _net('nn')
    with pytest.raises(ValueError, match='FOLDED'):
        nn.forward_search(sat, grd[:, :, :32], K, cands)
