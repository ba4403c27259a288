"""``score_loss`` / ``score_candidates`` of LM_S2GP and LM_S2GP_Ford: the triplet-form loss on the pose-score surface and its HIP
backward (``_ScoreFn``: hla_s2g_pose_score, hla_s2g_pose_score_bwd, hla_vgg_backward).

grd 64 x 256, sat 128 x 128, B = 2, precision 'fp32', the oracle's seeded weights and images (the smallest shapes of
tests/test_pose_search_gpu.py).  The reference is an fp64 CPU composition: the oracle's extractors (``oracle.ref_cpu``), the level
built from the model's own table, ``pose_score_ref.score`` (its cost through ``pose_score_bwd_ref.cost_clamp_const``: the same
values, finite autograd where nothing is in view), the loss written out here, and autograd.  Gates, those of
``test_ford_train_step_vs_oracle_autograd_small``: loss 1e-4 relative; parameter gradients in relative L2 < 2e-4 for conv_dec2.3,
< 2e-2 for the others.

The descent check runs at MAP level (planting a wrong minimum through two random-weight extractors at image level is not
practical): on ``pose_score_ref.planted_level`` data, where a wrong candidate scores ~0 and the declared true pose ~2, a few SGD
steps on the two maps along the gradients of ``hla_s2g_pose_score_bwd`` (through the C ABI, as tests/test_pose_score_bwd_gpu.py
calls it) must shrink the margin cost[true] - min_k cost[k]."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import pose_score_bwd_ref as PB
import pose_score_ref as PS

pytestmark = pytest.mark.gpu

GRD_HW, SAT_A, B = (64, 256), 128, 2
FORD_SIDE_M = 112.64
MIN_IN_VIEW = 0.5
F64 = torch.float64
FAR_A, FAR_B = (6.0, 0.3, 0.2), (-7.0, -0.4, 0.1)      # 120 m / 140 m away: nothing of the 100 m map in view


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _args(**kw):
    from oracle import ref_cpu as O
    a = O.default_args(**{'N_iters': 2, **kw})
    a.precision = 'fp32'
    return a


def _state():
    from oracle import ref_cpu as O
    return O.synth_model_state(4, bias_scale=0.02)


def _net(ford, **kw):
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    from highlyaccurate_amd.models_kitti import LM_S2GP
    net = (LM_S2GP_Ford if ford else LM_S2GP)(_args(**kw))
    net.load_state_dict(_state())
    return net.to(_dev()).train()


def _inputs(ford):
    from oracle import ref_cpu as O
    sat, grd, gu, gv, gh = O.synth_images(9, B, grd_hw=GRD_HW, sat_a=SAT_A)
    extra = None
    if ford:
        R_FL = torch.tensor([[[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]]).repeat(B, 1, 1)
        T_FL = torch.tensor([[1.7, 0.3, -1.2]]).repeat(B, 1)
        extra = dict(R_FL=R_FL, T_FL=T_FL, side_m=FORD_SIDE_M)
    return sat, grd, (gu, gv, gh), extra


def _candidates():
    from highlyaccurate_amd.models_kitti import pose_grid
    return pose_grid(3, 3, 3)[1:].contiguous()          # without the zero pose


def _loss(net, ford, sat, grd, extra, cands, gt, **kw):
    d = _dev()
    gt = [g.to(d) for g in gt]
    if ford:
        return net.score_loss(sat.to(d), grd.to(d), extra['side_m'], extra['R_FL'].to(d), extra['T_FL'].to(d), cands, *gt, **kw)
    return net.score_loss(sat.to(d), grd.to(d), cands, *gt, **kw)


def _triplet(cost, in_view, K):
    """The loss of one level on [B,K+1] costs (entry 0: the true pose) and pixel counts, written out for the reference."""
    ok = (in_view >= MIN_IN_VIEW * in_view.max(dim=1, keepdim=True).values)[:, 1:]
    t = torch.log(1 + torch.exp(10 * (cost[:, :1] - cost[:, 1:])))
    return torch.where(ok, t, torch.zeros_like(t)).sum() / (cost.shape[0] * K)


_REF = {}


def _reference(ford, using_weight):
    """fp64 CPU: (loss, {parameter name: gradient}, per-level costs [B,K+1]) of the composition, made once."""
    key = (ford, using_weight)
    if key in _REF:
        return _REF[key]
    from oracle import ref_cpu as O
    from highlyaccurate_amd import utils
    args = _args(using_weight=using_weight)
    sat, grd, gt, extra = _inputs(ford)
    on = (O.LM_S2GP_Ford if ford else O.LM_S2GP)(args, grd_hw=GRD_HW)
    on.load_state_dict(_state())
    on = on.double()
    sat_feats, _ = on.SatFeatureNet(sat.double())
    grd_feats, grd_confs = on.GrdFeatureNet(grd.double())
    tables = _net(ford).xyz_tables(GRD_HW[0], GRD_HW[1], _dev())
    cands = _candidates()
    poses = torch.cat([torch.cat(gt, 1)[:, None, :], cands[None].expand(B, -1, -1)], 1)
    geom = SimpleNamespace(ford=ford, ranges=(args.shift_range_lat, args.shift_range_lon, args.rotation_range), R_FL=None, T_FL=None)
    if ford:
        geom.R_FL, geom.T_FL = extra['R_FL'].double(), extra['T_FL'].double()
    loss, costs = 0, []
    for l in range(3):
        table = tables[l].cpu()
        h, w, A = table.shape[0], table.shape[1], sat_feats[l].shape[2]
        lv = SimpleNamespace(h=h, w=w, row0=h // 2, skip=0, C=sat_feats[l].shape[1], A=A, table=table, sat=sat_feats[l],
                             grd=grd_feats[l], conf=grd_confs[l])
        if ford:
            lv.mpp, lv.centre = extra['side_m'] / A, float(A // 2)
        else:
            lv.mpp, lv.centre = utils.get_meter_per_pixel() * utils.get_process_satmap_sidelength() / A, A / 2.0
        sums, _, counts, _, _ = PS.score(geom, lv, poses, using_weight)
        cost = PB.cost_clamp_const(sums)
        loss = loss + _triplet(cost, counts[..., 0].double(), cands.shape[0])
        costs.append(cost.detach())
    loss.backward()
    grads = {k: p.grad for k, p in on.named_parameters() if p.grad is not None}
    _REF[key] = (float(loss), grads, costs)
    return _REF[key]


DEC = ('SatFeatureNet.conv_dec2.3.weight', 'GrdFeatureNet.conv_dec2.3.weight')
OTHERS = ('SatFeatureNet.conv0.weight', 'GrdFeatureNet.conv5.weight', 'SatFeatureNet.conv_dec1.1.weight', 'GrdFeatureNet.conv14.bias')
HEADS = ('GrdFeatureNet.conf0.1.weight', 'GrdFeatureNet.conf1.1.weight', 'GrdFeatureNet.conf2.1.weight')


def _check_against_reference(ford, using_weight, names):
    want_loss, want, want_costs = _reference(ford, using_weight)
    net = _net(ford, using_weight=using_weight)
    sat, grd, gt, extra = _inputs(ford)
    loss = _loss(net, ford, sat, grd, extra, _candidates(), gt)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    print(f'SCORE_LOSS ford{ford} w{using_weight}: loss {float(loss):.6f} (ref64 {want_loss:.6f})')
    for l, c in enumerate(net.last_score_loss['costs']):
        print(f'  level {l}: |cost - ref64| = {(c.cpu().double() - want_costs[l]).abs().max():.2e}')
    assert abs(float(loss) - want_loss) < 1e-4 * abs(want_loss)
    got = dict(net.named_parameters())
    worst = []
    for k in names:
        assert got[k].grad is not None, k
        a, b = got[k].grad.double().cpu().numpy(), want[k].numpy()
        e = np.linalg.norm(a - b) / np.linalg.norm(b)
        print(f'  grad {k}: rel-l2 {e:.2e}')
        worst.append((k, e))
    for k, e in worst:
        assert np.isfinite(e) and e < (2e-4 if 'conv_dec2.3' in k else 2e-2), (k, e)
    return net


@pytest.mark.parametrize('ford', [0, 1], ids=['kitti', 'ford'])
def test_loss_and_gradients_against_the_fp64_composition(ford):
    net = _check_against_reference(ford, 0, DEC + OTHERS)
    ls = net.last_score_loss
    assert len(ls['costs']) == 3 and tuple(ls['costs'][0].shape) == (B, 27) and tuple(ls['sums'][2].shape) == (B, 27, 8)
    assert all(p.grad is None for k, p in net.named_parameters() if '.conf' in k)       # no weights: the heads take no part


def test_confidence_heads_get_gradients_with_using_weight():
    _check_against_reference(0, 1, DEC + OTHERS + HEADS)


def test_an_ineligible_negative_changes_nothing():
    """A negative with nothing in view, replaced by another one with nothing in view: the same loss bits and the same bits in
    every gradient of the ground branch (the satellite branch's sums are fp32 atomics: not compared bit for bit)."""
    sat, grd, gt, extra = _inputs(0)
    out = []
    for far in (FAR_A, FAR_B):
        net = _net(0, using_weight=1)
        cands = torch.cat([_candidates(), torch.tensor([far])])
        loss = _loss(net, 0, sat, grd, extra, cands, gt)
        loss.backward()
        sums = net.last_score_loss['sums']
        assert all((s[:, -1, 6] == 0).all() and (s[:, :-1, 6] > 0).all() for s in sums)
        out.append((loss.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    (la, ga), (lb, gb) = out
    assert torch.equal(la, lb)
    grd_keys = [k for k in ga if k.startswith('GrdFeatureNet.')]
    assert len(grd_keys) >= 20 and any('.conf' in k for k in grd_keys)
    for k in grd_keys:
        assert torch.equal(ga[k], gb[k]), k
    # ... and it contributes exactly zero: the loss is that of the 26 candidates, up to the 1 / (B K) factor
    net = _net(0, using_weight=1)
    l26 = _loss(net, 0, sat, grd, extra, _candidates(), gt)
    assert abs(float(l26) * 26 / 27 - float(la)) <= 1e-5 * float(la)


@pytest.mark.parametrize('ford', [0, 1], ids=['kitti', 'ford'])
def test_score_candidates_without_grad_is_score_poses(ford):
    net = _net(ford)
    sat, grd, gt, extra = _inputs(ford)
    d = _dev()
    sat, grd = sat.to(d), grd.to(d)
    cands = _candidates()
    with torch.no_grad():
        costs, sums = net.score_candidates(sat, grd, cands, extra=extra)
        sf, si, gf, gc, gi = net._features(sat, grd, bool(net.using_weight), False)
        assert len(costs) == 3 and len(sums) == 3
        for l in range(3):
            c, s = net.score_poses(sf, gf, gc, GRD_HW, cands, l, extra, si, gi)
            assert torch.equal(c, costs[l]) and torch.equal(s, sums[l]) and not costs[l].requires_grad
        one, _ = net.score_candidates(sat, grd, cands, levels=[2], extra=extra)
        assert len(one) == 1 and torch.equal(one[0], costs[2])
    # under autograd: the same costs up to the ground extractor's row crop, one Function, sums without gradient
    costs_g, sums_g = net.score_candidates(sat, grd, cands, levels=[0, 2], extra=extra)
    assert all(c.requires_grad for c in costs_g) and not any(s.requires_grad for s in sums_g)
    assert costs_g[0].grad_fn is costs_g[1].grad_fn or type(costs_g[0].grad_fn) is type(costs_g[1].grad_fn)
    assert (costs_g[1] - costs[2]).abs().max() < 1e-4


def test_sgd_on_the_maps_shrinks_the_margin_of_a_planted_wrong_minimum():
    """Map level (see the module docstring): hypothesis 2 is planted (cost ~0), hypothesis 0 is declared true (cost ~2)."""
    from test_pose_score_bwd_gpu import _bwd
    from test_pose_score_gpu import _call, _score
    nb = 2
    poses = PS.planted_poses(nb)
    geom, lv = PS.planted_level(0, 'ragged', 128, 16, nb, R.case_seed('score-loss-descent'), 2, poses)
    K = poses.shape[1] - 1

    def margin_and_grad():
        call = _call(geom, lv, 0)
        cost, sums = _score(call, poses)
        c = cost.double().requires_grad_(True)
        loss = _triplet(c, sums[..., 6], K)
        d_cost, = torch.autograd.grad(loss, c)
        assert (d_cost[:, PS.OUT_K] == 0).all()                      # the out-of-view negative is ineligible
        d_sat, d_grd, _ = _bwd(call, poses, sums, d_cost.float())
        elig = cost[:, 1:].clone()
        elig[:, PS.OUT_K - 1] = float('inf')
        return (cost[:, 0] - elig.min(1).values), float(loss), d_sat, d_grd

    m0, l0, d_sat, d_grd = margin_and_grad()
    assert (m0 > 1).all()                                            # the wrong candidate wins by a wide margin
    for _ in range(3):
        lv.sat = (lv.sat - 0.05 * d_sat).contiguous()
        lv.grd = (lv.grd - 0.05 * d_grd).contiguous()
        m, l, d_sat, d_grd = margin_and_grad()
    print(f'SCORE_LOSS descent: margin {m0.tolist()} -> {m.tolist()}, loss {l0:.4f} -> {l:.4f}')
    assert (m < m0).all() and l < l0


def test_refusals_and_second_backward():
    from highlyaccurate_amd._lib import HlaError
    sat, grd, gt, extra = _inputs(0)
    cands = _candidates()
    with pytest.raises(NotImplementedError, match='dropout'):
        _loss(_net(0, dropout=1), 0, sat, grd, extra, cands, gt)
    with pytest.raises(NotImplementedError, match='depth'):
        _loss(_net(0, use_gt_depth=1), 0, sat, grd, extra, cands, gt, gt_depth=torch.ones(B, 8, 8))
    with pytest.raises(NotImplementedError, match='level'):
        _loss(_net(0, level=4), 0, sat, grd, extra, cands, gt)
    net = _net(0)
    with pytest.raises(HlaError):
        net.score_loss(sat, grd, cands, *gt)                         # CPU tensors
    with pytest.raises(ValueError, match='candidates'):
        _loss(net, 0, sat, grd, extra, torch.zeros(3, 2), gt)
    with pytest.raises(ValueError, match='levels'):
        _loss(net, 0, sat, grd, extra, cands, gt, levels=[3])
    loss = _loss(net, 0, sat, grd, extra, cands[:3], gt, levels=[0])
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='twice'):
        loss.backward()
