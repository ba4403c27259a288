"""``LM_S2GP_Ford.forward_views`` / ``S2GPBase.lm_solve_views``: the multi-view LM loop on the model's own feature maps, checked
step by step against the fp64 reference of tests/lm_views_ref.py (one ``LM_update`` on the union of the views' pixels), with the
gates of tests/test_lm_views_vs_fp64.py; V = 1 against ``forward(mode='test')`` (RNG state); per-view intrinsics; no gradient;
the Python refusals.  Small Ford images (those of tests/test_pose_search_gpu.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import lm_views_ref as VR
import test_lm_views_vs_fp64 as KV

pytestmark = pytest.mark.gpu

GRD_HW, SAT_A, B = (64, 256), 128, 2
SEED = 1
FORD_SIDE_M = 112.64
F64, F32 = torch.float64, torch.float32


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _net(ford=True, **kw):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    args = O.default_args(**{'N_iters': 2, 'damping': 1.0, **kw})
    args.precision = 'fp32'
    torch.manual_seed(SEED)
    return (LM_S2GP_Ford if ford else LM_S2GP)(args).to(_dev()).eval()


def _inputs(V):
    g = torch.Generator().manual_seed(SEED + 1)
    sat = torch.rand(B, 3, SAT_A, SAT_A, generator=g).to(_dev())
    grd = torch.rand(B, V, 3, *GRD_HW, generator=g).to(_dev())
    rs = np.random.RandomState(9)
    P = np.array([[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]])
    Rs = []
    for a in rs.uniform(-0.2, 0.2, size=B * V):      # every view looks a little to another side
        c, s = np.cos(a), np.sin(a)
        Rs.append(np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]]) @ P)
    T = np.array([1.7, 0.3, -1.2]) + rs.uniform(-0.3, 0.3, size=(B, V, 3))
    return sat, grd, torch.from_numpy(np.stack(Rs)).float().reshape(B, V, 3, 3), torch.from_numpy(T).float()


def _ref_levels(net, V, feats, tables, using_weight):
    """The model's own pyramid as lm_views_ref levels (maps times their inverse norms, stored rows put back in place)."""
    sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = feats
    out = []
    for l in range(len(sat_feats)):
        s = sat_feats[l].double().cpu() * sat_inv[l].double().cpu().view(-1, 1, 1, 1)
        g = grd_feats[l].double().cpu() * grd_inv[l].double().cpu().view(-1, 1, 1, 1)
        table = tables[l].cpu()
        h, w, A, Cn = table.shape[1], table.shape[2], s.shape[1], s.shape[3]
        full = torch.zeros(B * V, h, w, Cn, dtype=F64)
        full[:, h - g.shape[1]:] = g
        conf = torch.ones(B * V, 1, h, w, dtype=F64)
        if using_weight:
            conf = torch.zeros(B * V, 1, h, w, dtype=F64)
            conf[:, 0, h - grd_confs[l].shape[1]:] = grd_confs[l].double().cpu()
        out.append(SimpleNamespace(h=h, w=w, row0=h // 2, skip=h - g.shape[1], C=Cn, A=A, V=V, table=table, mpp=FORD_SIDE_M / A,
                                   centre=float(A // 2), sat=s.permute(0, 3, 1, 2).contiguous(), grd=full.permute(0, 3, 1, 2).contiguous(),
                                   conf=conf, ford=1))
    return out


def _check_trace(net, V, sat, grd, Rv, Tv, camera_k=None, using_weight=0):
    """lm_solve_views on ``_features`` output, every step against the reference restarted from the kernel's previous pose."""
    a = net.args
    dev = _dev()
    from highlyaccurate_amd._s2gp import ford_K_network_input
    K = torch.tensor(ford_K_network_input()).reshape(1, 3, 3).repeat(V, 1, 1) if camera_k is None else camera_k
    with torch.no_grad():
        tables = net.view_tables(GRD_HW[0], GRD_HW[1], K, dev)
        feats = net._features(sat, grd.reshape(B * V, 3, *GRD_HW), bool(using_weight), False, pair=False)
        torch.manual_seed(3)
        trace = net.lm_solve_views(feats[0], feats[2], feats[3], GRD_HW, V, Rv, Tv, FORD_SIDE_M, tables, 0, None, feats[1], feats[4])
        torch.cuda.synchronize()
    lv = net.last_views
    assert lv['trace'] is trace and tuple(lv['normal_eq'].shape) == (6, B, 16) and tuple(lv['view_sums'].shape) == (6, B, V, 16)
    trace, neq, vs = trace.cpu(), lv['normal_eq'].cpu(), lv['view_sums'].cpu()
    levels = _ref_levels(net, V, feats, tables, using_weight)
    geom = SimpleNamespace(ford=1, ranges=(a.shift_range_lat, a.shift_range_lon, a.rotation_range), R_FL=Rv, T_FL=Tv)
    args = R.update_args(geom.ranges, damping=1.0)
    torch.manual_seed(3)
    rand_uv = torch.rand(6, 2, B).mul_(2.0).add_(-1.0)
    prev = torch.zeros(B, 3)
    for k, (i, l) in enumerate(R.step_order(3, 2, 0)):
        KV._check_step(f'views model V{V} step {k}', geom, levels[l], prev, using_weight, KV._ruv(rand_uv, k, F32), trace[:, i, l],
                       neq[k], vs[k], args=args)
        prev = trace[:, i, l]
    assert bool((vs[:, :, :, 2] > 0).all())      # every view has pixels on the map in every step
    return trace


def test_three_views_trace_against_reference_and_forward_views():
    V = 3
    net = _net()
    sat, grd, Rv, Tv = _inputs(V)
    trace = _check_trace(net, V, sat, grd, Rv, Tv)
    torch.manual_seed(3)
    out = net.forward_views(sat, grd, FORD_SIDE_M, Rv, Tv)
    for c in range(3):
        assert tuple(out[c].shape) == (B,) and torch.equal(out[c].cpu(), trace[:, -1, -1, c])
    # the views are not interchangeable with one of them alone
    torch.manual_seed(3)
    one = net.forward_views(sat, grd[:, :1], FORD_SIDE_M, Rv[:, :1], Tv[:, :1])
    assert float((torch.stack(one) - torch.stack(out)).abs().max()) > 1e-4


def test_one_view_trace_and_rng_state_of_forward():
    V = 1
    net = _net(using_weight=1)
    sat, grd, Rv, Tv = _inputs(V)
    _check_trace(net, V, sat, grd, Rv, Tv, using_weight=1)
    with torch.no_grad():
        torch.manual_seed(5)
        want = net(sat, grd[:, 0], FORD_SIDE_M, Rv[:, 0], Tv[:, 0], mode='test')
        state = torch.get_rng_state()
        torch.manual_seed(5)
        got = net.forward_views(sat, grd, FORD_SIDE_M, Rv, Tv)
    assert torch.equal(torch.get_rng_state(), state)
    d = float((torch.stack(got) - torch.stack(want)).abs().max())
    print(f'LMV forward_views(V = 1) against forward(mode=test): max |pose difference| = {d:.2e}')
    assert all(torch.isfinite(x).all() for x in got)


def test_camera_k_per_view_changes_tables_and_result():
    from highlyaccurate_amd._s2gp import ford_K_network_input
    V = 2
    net = _net()
    sat, grd, Rv, Tv = _inputs(V)
    K = torch.tensor(ford_K_network_input()).reshape(1, 3, 3).repeat(V, 1, 1)
    K2 = K.clone()
    K2[1, 0, 0] *= 1.25          # view 1: a longer focal length in x
    K2[1, 1, 2] -= 8.0           # and a higher horizon
    ta, tb = net.view_tables(*GRD_HW, K, _dev()), net.view_tables(*GRD_HW, K2, _dev())
    for l, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x[0], y[0]) and not torch.equal(x[1], y[1])
        assert torch.equal(x[0], net.xyz_tables(*GRD_HW, _dev())[l])
    torch.manual_seed(3)
    a = net.forward_views(sat, grd, FORD_SIDE_M, Rv, Tv)
    torch.manual_seed(3)
    same = net.forward_views(sat, grd, FORD_SIDE_M, Rv, Tv, camera_k=K)
    torch.manual_seed(3)
    b = net.forward_views(sat, grd, FORD_SIDE_M, Rv, Tv, camera_k=K2)
    assert all(torch.equal(x, y) for x, y in zip(a, same))
    assert float((torch.stack(a) - torch.stack(b)).abs().max()) > 1e-5
    _check_trace(net, V, sat, grd, Rv, Tv, camera_k=K2)


def test_outputs_carry_no_gradient_under_enable_grad():
    V = 2
    net = _net()
    sat, grd, Rv, Tv = _inputs(V)
    with torch.enable_grad():
        out = net.forward_views(sat, grd.requires_grad_(True), FORD_SIDE_M, Rv, Tv)
    assert all((not t.requires_grad) and t.grad_fn is None for t in out)
    assert not net.last_views['trace'].requires_grad


def test_python_refusals():
    V = 2
    sat, grd, Rv, Tv = _inputs(V)
    with pytest.raises(NotImplementedError, match='dropout'):
        _net(dropout=1).forward_views(sat, grd, FORD_SIDE_M, Rv, Tv)
    with pytest.raises(NotImplementedError, match='polar'):
        _net(proj='polar').forward_views(sat, grd, FORD_SIDE_M, Rv, Tv, level_first=1)
    with pytest.raises(NotImplementedError):
        _net(estimate_depth=1)
    kitti = _net(ford=False)
    assert not hasattr(kitti, 'forward_views')
    with pytest.raises(NotImplementedError, match='Ford'):
        kitti.lm_solve_views([sat], [grd], [None], GRD_HW, V, Rv, Tv, FORD_SIDE_M)
    net = _net()
    with pytest.raises(ValueError):
        net.forward_views(sat, grd[:, 0], FORD_SIDE_M, Rv, Tv)                       # no view axis
    with pytest.raises(ValueError):
        net.forward_views(sat, grd, FORD_SIDE_M, Rv[:, :1], Tv)                      # R for another V
    with pytest.raises(ValueError):
        net.forward_views(sat, grd, FORD_SIDE_M, Rv, Tv, camera_k=torch.eye(3).repeat(3, 1, 1))
    with pytest.raises(ValueError, match='at most 8'):
        net.forward_views(sat, grd[:, :1].expand(-1, 9, -1, -1, -1), FORD_SIDE_M, Rv[:, :1].expand(-1, 9, -1, -1), Tv[:, :1].expand(-1, 9, -1))
    from highlyaccurate_amd import _lib
    with pytest.raises(_lib.HlaError):
        net.forward_views(sat.cpu(), grd, FORD_SIDE_M, Rv, Tv)
