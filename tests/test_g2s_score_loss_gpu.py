"""``LM_G2SP.score_loss`` / ``score_candidates``: the triplet-form loss on the ground -> satellite pose-score surface and its HIP
backward (``_G2sScoreFn``: hla_g2s_pose_score, hla_g2s_pose_score_bwd, hla_vgg_backward), for proj='geo' without and with weights
and for proj='nn'.

sat 128 x 128, grd 64 x 256, B = 2, precision 'fp32', the camera of tests/test_g2s_pose_search_gpu.py, the oracle's seeded weights
and images.  The reference is an fp64 CPU composition: the oracle's extractors (``oracle.ref_cpu``; ``g2s_nn_ref.VGGUnet_G2S`` for
'nn'), ``g2s_pose_score_ref.score`` (its cost through ``pose_score_bwd_ref.cost_clamp_const``: the same values, finite autograd
where nothing is in view), the loss written out here, and autograd.  Gates, those of tests/test_score_loss_gpu.py: loss 1e-4
relative; parameter gradients in relative L2 < 2e-4 for conv_dec2.3, < 2e-2 for the others.

The descent check runs at MAP level, as there: on ``g2s_pose_score_ref.planted`` data, where hypothesis 2 scores ~0 and hypothesis
0 is declared true, three SGD steps on the two maps along the gradients of ``hla_g2s_pose_score_bwd`` (through the C ABI) must
shrink the margin cost[true] - min_k cost[k] and the loss."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import g2s_geo_ref as R
import g2s_nn_ref as NN
import g2s_pose_score_bwd_ref as GB
import g2s_pose_score_ref as GP
from test_g2s_pose_search_gpu import CAMERA_K, GRD_HW, MODELS, RANGES, SAT_A, B

pytestmark = pytest.mark.gpu

MIN_IN_VIEW = 0.5
F64 = torch.float64
FAR_A, FAR_B = (6.0, 0.3, 0.2), (7.0, -0.4, 0.1)      # 120 m / 140 m ahead of the 100 m map: all of it behind the camera / off the map


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _args(name, **kw):
    proj, uw = MODELS[name]
    a = R.make_args(RANGES, **{'N_iters': 2, 'damping': 1.0, 'using_weight': uw, 'proj': proj, **kw})
    a.precision = 'fp32'
    return a


def _state():
    from oracle import ref_cpu as O
    return O.synth_model_state(4, bias_scale=0.02)


def _net(name, **kw):
    from highlyaccurate_amd.models_kitti import LM_G2SP
    net = LM_G2SP(_args(name, **kw))
    net.load_state_dict(_state())
    return net.to(_dev()).train()


def _inputs():
    from oracle import ref_cpu as O
    sat, grd, gu, gv, gh = O.synth_images(9, B, grd_hw=GRD_HW, sat_a=SAT_A)
    return sat, grd, torch.tensor(CAMERA_K, dtype=torch.float32), (gu, gv, gh)


def _candidates():
    from highlyaccurate_amd.models_kitti import pose_grid
    return pose_grid(3, 3, 3)[1:].contiguous()          # without the zero pose


def _loss(net, sat, grd, K, cands, gt, **kw):
    d = _dev()
    return net.score_loss(sat.to(d), grd.to(d), K.to(d), cands, *[g.to(d) for g in gt], **kw)


def _triplet(cost, in_view, K):
    """The loss of one level on [B,K+1] costs (entry 0: the true pose) and pixel counts, written out for the reference."""
    ok = (in_view >= MIN_IN_VIEW * in_view.max(dim=1, keepdim=True).values)[:, 1:]
    t = torch.log(1 + torch.exp(10 * (cost[:, :1] - cost[:, 1:])))
    return torch.where(ok, t, torch.zeros_like(t)).sum() / (cost.shape[0] * K)


_REF = {}


def _reference(name):
    """fp64 CPU: (loss, {parameter name: gradient}, per-level costs [B,K+1]) of the composition, made once."""
    if name in _REF:
        return _REF[name]
    from oracle import ref_cpu as O
    proj, uw = MODELS[name]
    args = _args(name)
    sat, grd, K, gt = _inputs()
    on = (NN.LM_G2SP_NN if proj == 'nn' else O.LM_G2SP)(args)
    on.load_state_dict(_state())
    on = on.double()
    sat_feats, _ = on.SatFeatureNet(sat.double())
    grd_feats, grd_confs = on.GrdFeatureNet(grd.double())
    cands = _candidates()
    poses = torch.cat([torch.cat(gt, 1)[:, None, :], cands[None].expand(B, -1, -1)], 1)
    case = SimpleNamespace(name=name, proj=proj, B=B, K=K, ori_hw=GRD_HW, ranges=RANGES,
                           levels=[(s.shape[-1], s.shape[1], tuple(g.shape[-2:])) for s, g in zip(sat_feats, grd_feats)])
    loss, costs = 0, []
    for l in range(3):
        sums, _, counts, _, _ = GP.score(case, l, poses, uw, F64, maps=(sat_feats, grd_feats, grd_confs))
        cost = GB.cost_clamp_const(sums)
        loss = loss + _triplet(cost, counts.double(), cands.shape[0])
        costs.append(cost.detach())
    loss.backward()
    grads = {k: p.grad for k, p in on.named_parameters() if p.grad is not None}
    _REF[name] = (float(loss.detach()), grads, costs)
    return _REF[name]


DEC = ('SatFeatureNet.conv_dec2.3.weight', 'GrdFeatureNet.conv_dec2.3.weight')
OTHERS = ('SatFeatureNet.conv0.weight', 'SatFeatureNet.conv10.weight', 'GrdFeatureNet.conv2.weight', 'GrdFeatureNet.conv_dec1.1.weight')
HEADS = ('GrdFeatureNet.conf0.1.weight', 'GrdFeatureNet.conf1.1.weight', 'GrdFeatureNet.conf2.1.weight')


@pytest.mark.parametrize('name', list(MODELS))
def test_loss_and_gradients_against_the_fp64_composition(name):
    want_loss, want, want_costs = _reference(name)
    uw = MODELS[name][1]
    net = _net(name)
    sat, grd, K, gt = _inputs()
    loss = _loss(net, sat, grd, K, _candidates(), gt)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    print(f'G2S SCORE_LOSS {name}: loss {float(loss.detach()):.8f} (ref64 {want_loss:.8f})')
    ls = net.last_score_loss
    for l, c in enumerate(ls['costs']):
        print(f'  level {l}: |cost - ref64| = {(c.cpu().double() - want_costs[l]).abs().max():.2e}')
    assert abs(float(loss.detach()) - want_loss) < 1e-4 * abs(want_loss)
    got = dict(net.named_parameters())
    worst = []
    for k in DEC + OTHERS + (HEADS if uw else ()):
        assert got[k].grad is not None, k
        a, b = got[k].grad.double().cpu().numpy(), want[k].numpy()
        e = np.linalg.norm(a - b) / np.linalg.norm(b)
        print(f'  grad {k}: rel-l2 {e:.2e}')
        worst.append((k, e))
    for k, e in worst:
        assert np.isfinite(e) and e < (2e-4 if 'conv_dec2.3' in k else 2e-2), (k, e)
    assert len(ls['costs']) == 3 and tuple(ls['costs'][0].shape) == (B, 27) and tuple(ls['sums'][2].shape) == (B, 27, 8)
    if not uw:
        assert all(p.grad is None for k, p in net.named_parameters() if '.conf' in k)       # no weights: the heads take no part


@pytest.mark.parametrize('name', list(MODELS))
def test_an_ineligible_negative_changes_nothing(name):
    """A negative with nothing in view, replaced by another one with nothing in view: the same loss bits."""
    sat, grd, K, gt = _inputs()
    net = _net(name)
    out = []
    with torch.no_grad():
        for far in (FAR_A, FAR_B):
            cands = torch.cat([_candidates(), torch.tensor([far])])
            out.append(_loss(net, sat, grd, K, cands, gt).clone())
            sums = net.last_score_loss['sums']
            assert all((s[:, -1, 6] == 0).all() and (s[:, :-1, 6] > 0).all() for s in sums)
        l26 = _loss(net, sat, grd, K, _candidates(), gt)
    assert torch.equal(out[0], out[1])
    assert abs(float(l26) * 26 / 27 - float(out[0])) <= 1e-5 * float(out[0])     # ... and it contributes exactly zero


@pytest.mark.parametrize('name', list(MODELS))
def test_score_candidates_without_grad_is_score_poses(name):
    from test_g2s_pose_search_gpu import _features
    net = _net(name)
    sat, grd, K, gt = _inputs()
    d = _dev()
    sat, grd, K = sat.to(d), grd.to(d), K.to(d)
    cands = _candidates()
    with torch.no_grad():
        costs, sums = net.score_candidates(sat, grd, K, cands)
        sf, gf, gc, si, gi = _features(net, sat, grd)
        assert len(costs) == 3 and len(sums) == 3
        for l in range(3):
            c, s = net.score_poses(sf, gf, gc, K, GRD_HW, cands, l, si, gi)
            assert torch.equal(c, costs[l]) and torch.equal(s, sums[l]) and not costs[l].requires_grad
        one, _ = net.score_candidates(sat, grd, K, cands, levels=[2])
        assert len(one) == 1 and torch.equal(one[0], costs[2])
    # under autograd: one Function, sums without gradient
    costs_g, sums_g = net.score_candidates(sat, grd, K, cands, levels=[0, 2])
    assert all(c.requires_grad for c in costs_g) and not any(s.requires_grad for s in sums_g)
    assert costs_g[0].grad_fn is costs_g[1].grad_fn or type(costs_g[0].grad_fn) is type(costs_g[1].grad_fn)
    assert 'G2sScoreFn' in type(costs_g[0].grad_fn).__name__
    assert (costs_g[1] - costs[2]).abs().max() < 1e-4


@pytest.mark.parametrize('proj', ['geo', 'nn'])
def test_sgd_on_the_maps_shrinks_the_margin_of_a_planted_wrong_minimum(proj):
    """Map level (see the module docstring): hypothesis 2 is planted (cost ~0), hypothesis 0 is declared true.  A step moves each
    sample's map by 0.05 ||map||^2 times its gradient (the cost depends on a map's direction only, where the slope is ||map|| times
    the gradient's norm)."""
    from test_g2s_pose_score_bwd_gpu import _bwd
    from test_g2s_pose_score_gpu import _Call
    base, l, poses = GP.planted(proj)
    c = SimpleNamespace(**vars(base))
    c.sat, c.grd = list(base.sat), list(base.grd)
    K = poses.shape[1] - 1

    def margin_and_grad():
        call = _Call(c, 0)
        cost, sums = call.score(l, poses)
        cc = cost.double().requires_grad_(True)
        loss = _triplet(cc, sums[..., 6], K)
        d_cost, = torch.autograd.grad(loss, cc)
        assert (d_cost[:, GP.OUT_K] == 0).all()                      # the out-of-view negative is ineligible
        d_sat, d_grd, _ = _bwd(call, l, poses, sums, d_cost.float())
        elig = cost[:, 1:].clone()
        elig[:, GP.OUT_K - 1] = float('inf')
        return (cost[:, 0] - elig.min(1).values), float(loss.detach()), d_sat, d_grd

    m0, l0, d_sat, d_grd = margin_and_grad()
    assert (m0 > 1).all()                                            # the wrong candidate wins by a wide margin
    n2 = lambda t: t.double().flatten(1).pow(2).sum(1).float().view(-1, 1, 1, 1)
    for _ in range(3):
        c.sat[l] = (c.sat[l] - 0.05 * n2(c.sat[l]) * d_sat).contiguous()
        c.grd[l] = (c.grd[l] - 0.05 * n2(c.grd[l]) * d_grd).contiguous()
        m, ls, d_sat, d_grd = margin_and_grad()
    print(f'G2S SCORE_LOSS descent {proj}: margin {m0.tolist()} -> {m.tolist()}, loss {l0:.4f} -> {ls:.4f}')
    assert (m < m0).all() and ls < l0


def test_level_4_scores_and_trains_its_finest_level():
    """args.level = 4 is accepted: the x24 level is scored and conv_dec3 receives a finite, nonzero gradient."""
    net = _net('geo', level=4)
    sat, grd, K, gt = _inputs()
    loss = _loss(net, sat, grd, K, _candidates()[:5], gt, levels=[3])
    loss.backward()
    g = net.SatFeatureNet.conv_dec3[3].weight.grad
    assert torch.isfinite(loss) and g is not None and torch.isfinite(g).all() and (g != 0).any()
    g = net.GrdFeatureNet.conv_dec3[3].weight.grad
    assert g is not None and torch.isfinite(g).all() and (g != 0).any()


def test_refusals_and_second_backward():
    from highlyaccurate_amd._lib import HlaError
    from highlyaccurate_amd.models_kitti import LM_G2SP
    sat, grd, K, gt = _inputs()
    cands = _candidates()
    with pytest.raises(NotImplementedError, match='dropout'):
        _loss(_net('geo', dropout=1), sat, grd, K, cands, gt)
    with pytest.raises(NotImplementedError, match='using_weight'):
        LM_G2SP(_args('nn', using_weight=1))
    net = _net('geo')
    with pytest.raises(HlaError):
        net.score_loss(sat, grd, K, cands, *gt)                      # CPU tensors
    with pytest.raises(ValueError, match='candidates'):
        _loss(net, sat, grd, K, torch.zeros(3, 2), gt)
    with pytest.raises(ValueError, match='levels'):
        _loss(net, sat, grd, K, cands, gt, levels=[3])
    with pytest.raises(ValueError, match='levels'):
        _loss(net, sat, grd, K, cands, gt, levels=[0, 0])
    with pytest.raises(ValueError, match='expected sat_map'):
        _loss(net, sat[:1], grd, K, cands, gt)
    loss = _loss(net, sat, grd, K, cands[:3], gt, levels=[0])
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='twice'):
        loss.backward()
