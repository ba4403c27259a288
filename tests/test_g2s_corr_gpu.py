"""``LM_G2SP.corr``: the dense translation search at model level -- both extractors, the zero-pose projection of the crop, the
correlation of every level, the triplet loss and its HIP backward into both extractors' parameters.

The fixture of tests/test_g2s_score_loss_gpu.py (sat 128 x 128, grd 64 x 256, B = 2, precision 'fp32', its camera, the oracle's
seeded weights and images) with shift ranges (4 m, 6 m): the 20 m of that file would leave no crop at this size.  The reference is
the fp64 CPU composition of tests/g2s_corr_ref.py on the oracle's extractors, with autograd; its fp32 run sets the gates' floor.
In fp64 the smallest and second-smallest entry of corr differ by >= 1.3e-4 at every level and sample, three orders above the fp32
error: argmin, pred_u and pred_v are asserted exactly."""
import numpy as np
import pytest
import torch

import g2s_corr_ref as GR
import g2s_geo_ref as R
from test_g2s_pose_search_gpu import CAMERA_K, GRD_HW, SAT_A, B

pytestmark = pytest.mark.gpu

RANGES = (4.0, 6.0, 10.0)
F64 = torch.float64
EPS32 = 2.0 ** -23
DEC = ('SatFeatureNet.conv_dec2.3.weight', 'GrdFeatureNet.conv_dec2.3.weight')
OTHERS = ('SatFeatureNet.conv0.weight', 'SatFeatureNet.conv10.weight', 'GrdFeatureNet.conv2.weight', 'GrdFeatureNet.conv_dec1.1.weight')


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _args(ranges=RANGES, **kw):
    a = R.make_args(ranges, **{'N_iters': 2, 'damping': 1.0, 'using_weight': 0, 'proj': 'geo', **kw})
    a.precision = 'fp32'
    return a


def _state():
    from oracle import ref_cpu as O
    return O.synth_model_state(4, bias_scale=0.02)


def _net(**kw):
    from highlyaccurate_amd.models_kitti import LM_G2SP
    net = LM_G2SP(_args(**kw))
    net.load_state_dict(_state())
    return net.to(_dev()).train()


def _inputs():
    from oracle import ref_cpu as O
    sat, grd, gu, gv, gh = O.synth_images(9, B, grd_hw=GRD_HW, sat_a=SAT_A)
    return sat, grd, torch.tensor(CAMERA_K, dtype=torch.float32), (gu, gv, gh)


def _corr(net, sat, grd, K, gt, mode='train'):
    d = _dev()
    return net.corr(sat.to(d), grd.to(d), K.to(d), gt[0].to(d), gt[1].to(d), gt[2].to(d), mode=mode)


_REF = {}


def _reference(dt):
    """(loss, {parameter name: gradient}, per-level corr) of the CPU composition at dtype dt, made once."""
    if dt in _REF:
        return _REF[dt]
    from oracle import ref_cpu as O
    args = _args()
    sat, grd, K, gt = _inputs()
    on = O.LM_G2SP(args)
    on.load_state_dict(_state())
    on = on.to(dt)
    sat_feats, _ = on.SatFeatureNet(sat.to(dt))
    grd_feats, _ = on.GrdFeatureNet(grd.to(dt))
    corrs = GR.compose(args, sat_feats[:3], grd_feats[:3], K, GRD_HW)
    loss = GR.triplet_loss(corrs, gt[0], gt[1], args.shift_range_lat, args.shift_range_lon)
    loss.backward()
    grads = {k: p.grad.double() for k, p in on.named_parameters() if p.grad is not None}
    _REF[dt] = (float(loss.detach()), grads, [c.detach() for c in corrs])
    return _REF[dt]


def test_corr_loss_prediction_and_gradients_against_the_fp64_composition():
    want_loss, want, want_corr = _reference(F64)
    loss32, g32, corr32 = _reference(torch.float32)
    net = _net()
    sat, grd, K, gt = _inputs()
    loss = _corr(net, sat, grd, K, gt)
    assert loss.dim() == 0 and loss.requires_grad and 'G2sCorrFn' in type(loss.grad_fn).__name__
    loss.backward()
    print(f'G2S CORR: loss {float(loss.detach()):.8f} (ref64 {want_loss:.8f}, ref32 {loss32:.8f})')
    assert len(net.last_corr) == 3
    sizes = [(7, 9), (12, 17), (22, 32)]
    for l, c in enumerate(net.last_corr):
        assert tuple(c.shape) == (B, *sizes[l]) and c.dtype == torch.float32
        got, r64, r32 = c.cpu().double().numpy(), want_corr[l].numpy(), corr32[l].double().numpy()
        gap = np.abs(r32 - r64).max()
        err, allow = np.abs(got - r64).max(), max(2 * gap, 8 * EPS32 * np.abs(r64).max())
        two = np.sort(r64.reshape(B, -1), axis=1)[:, :2]
        print(f'  level {l}: corr in [{r64.min():.4f}, {r64.max():.4f}], max err {err:.2e}, allowed {allow:.2e} (ratio {err / allow:.3f}); '
              f'gap between the two smallest {np.min(two[:, 1] - two[:, 0]):.2e}')
        assert np.isfinite(got).all() and err <= allow, (l, err, allow)
        assert np.array_equal(got.reshape(B, -1).argmin(1), r64.reshape(B, -1).argmin(1))
    assert abs(float(loss.detach()) - want_loss) < 1e-4 * abs(want_loss)
    got = dict(net.named_parameters())
    worst = []
    for k in DEC + OTHERS:
        assert got[k].grad is not None, k
        a, b, c = got[k].grad.double().cpu().numpy(), want[k].numpy(), g32[k].numpy()
        e, e32 = np.linalg.norm(a - b) / np.linalg.norm(b), np.linalg.norm(c - b) / np.linalg.norm(b)
        lim = max(2e-4 if 'conv_dec2.3' in k else 2e-2, 2 * e32)
        print(f'  grad {k}: rel-l2 {e:.2e} (fp32 CPU composition {e32:.2e}, limit {lim:.2e})')
        worst.append((k, e, lim))
    for k, e, lim in worst:
        assert np.isfinite(e) and e < lim, (k, e, lim)
    assert all(p.grad is None for k, p in net.named_parameters() if '.conf' in k or k == 'damping')


def test_mode_test_is_the_train_paths_forward_and_predicts_exactly():
    _, _, want_corr = _reference(F64)
    net = _net()
    sat, grd, K, gt = _inputs()
    loss = _corr(net, sat, grd, K, gt)
    train_corr = [c.clone() for c in net.last_corr]
    with torch.no_grad():
        pred_u, pred_v = _corr(net, sat, grd, K, gt, mode='test')
        assert all(torch.equal(a, b) for a, b in zip(train_corr, net.last_corr))
        loss_ng = _corr(net, sat, grd, K, gt)
    assert tuple(pred_u.shape) == (B,) and tuple(pred_v.shape) == (B,) and not pred_u.requires_grad
    assert torch.equal(loss_ng, loss.detach()) and not loss_ng.requires_grad
    u, v, _ = GR.predict(want_corr[2].float(), GR.level_mpp(2))
    print(f'G2S CORR prediction: u {pred_u.tolist()} v {pred_v.tolist()} (reference u {u.tolist()} v {v.tolist()})')
    assert torch.equal(pred_u.cpu(), u) and torch.equal(pred_v.cpu(), v)
    # outside autograd the test outputs of a grad-enabled call carry no graph either
    pu, _ = _corr(net, sat, grd, K, gt, mode='test')
    assert not pu.requires_grad and torch.equal(pu, pred_u)


def test_refusals_and_second_backward():
    from highlyaccurate_amd._lib import HlaError
    sat, grd, K, gt = _inputs()
    with pytest.raises(NotImplementedError, match='nn'):
        nn = _net(proj='nn')
        d = _dev()
        nn.corr(torch.zeros(B, 3, 128, 128, device=d), torch.zeros(B, 3, 64, 256, device=d), K.to(d), gt[0].to(d), gt[1].to(d))
    net = _net()
    with pytest.raises(HlaError):
        net.corr(sat, grd, K, gt[0], gt[1])                      # CPU tensors
    with pytest.raises(ValueError, match='gt_shift'):
        _dev()
        net.corr(sat.cuda(), grd.cuda(), K.cuda())
    big = _net(ranges=(20.0, 6.0, 10.0))
    with pytest.raises(ValueError, match='too large'):
        _corr(big, sat, grd, K, gt)
    loss = _corr(net, sat, grd, K, gt)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='twice'):
        loss.backward()


def test_three_sgd_steps_on_both_extractors_lower_the_loss():
    """Model level: a step moves every parameter of both extractors along its gradient, by 0.5 % of the parameters' norm in all."""
    net = _net()
    sat, grd, K, gt = _inputs()
    params = [p for k, p in net.named_parameters() if k.startswith(('SatFeatureNet.', 'GrdFeatureNet.')) and '.conf' not in k]
    losses = []
    for step in range(4):
        for p in params:
            p.grad = None
        loss = _corr(net, sat, grd, K, gt)
        losses.append(float(loss.detach()))
        if step == 3:
            break
        loss.backward()
        with torch.no_grad():
            gs = [p.grad for p in params if p.grad is not None]
            gn = torch.sqrt(sum((g.double() ** 2).sum() for g in gs))
            pn = torch.sqrt(sum((p.double() ** 2).sum() for p in params))
            assert torch.isfinite(gn) and gn > 0
            for p in params:
                if p.grad is not None:
                    p -= (0.005 * pn / gn).float() * p.grad
    print(f'G2S CORR descent: loss {losses}')
    assert losses[1] < losses[0] and losses[3] < losses[0]
