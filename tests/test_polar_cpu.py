"""CPU checks of ``proj='polar'`` for ``LM_S2GP`` / ``LM_S2GP_Ford``: the fp64-capable restatement (tests/polar_ref.py) is pinned
to what the REAL reference recorded (tools/make_golden_polar.py), the product's polar table to the reference's own table bit for
bit, and the module surface to the argument rules.  Tolerances of the pins are those test_g2s_nn_cpu.py uses for the same purpose."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from make_idx import sample_idx
from oracle import ref_cpu as O
import polar_ref as R

TABLE_SALT = 31          # tools/make_golden_polar.py


def _tuple9(res):
    return np.stack([np.atleast_1d(r.detach().double().numpy()) if r.dim() else np.full(3, float(r.detach())) for r in res[:9]])


def _trace(on, B):
    lat, lon, th = on.trace
    u, v = (lat, lon) if on.ford else (lon, lat)
    return torch.stack([u, v, th], -1).detach().reshape(B, -1, 3).double().numpy()


def _ford_extra(B, dtype):
    R_FL = torch.tensor([[[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]]).repeat(B, 1, 1)
    T_FL = torch.tensor([[1.7, 0.3, -1.2]]).repeat(B, 1)
    return 112.64, R_FL.to(dtype), T_FL.to(dtype)


def test_polar_constructs_and_other_projections_raise():
    """``LM_S2GP(proj='polar')`` constructs (NotImplementedError without the feature); any other string keeps raising."""
    from highlyaccurate_amd.models_kitti import LM_S2GP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    for cls in (LM_S2GP, LM_S2GP_Ford):
        for level in (3, 4):
            net = cls(O.default_args(proj='polar', level=level))
            assert net.polar
        assert not cls(O.default_args()).polar
        for bad in ('something', 'nn', 'CrossAttn', ''):
            with pytest.raises(NotImplementedError, match="'geo' or 'polar'"):
                cls(O.default_args(proj=bad))
    with pytest.raises(NotImplementedError, match='level=2'):
        LM_S2GP_Ford(O.default_args(proj='polar', level=2))
    assert not LM_S2GP_Ford(O.default_args(level=2)).polar
    # the updaters and options of 'geo' are all accepted
    for kw in (dict(Optimizer='SGD'), dict(Optimizer='ADAM'), dict(using_weight=1, dropout=1, train_damping=1),
               dict(deterministic_backward=1)):
        LM_S2GP(O.default_args(proj='polar', **kw))
    LM_S2GP_Ford(O.default_args(proj='polar', Optimizer='GN'))
    with pytest.raises(NotImplementedError):          # (what the issue lists as fixed in place stays)
        LM_S2GP(O.default_args(proj='polar', Optimizer='NN'))


def test_state_dict_keys_are_unchanged_by_polar():
    from highlyaccurate_amd.models_kitti import LM_S2GP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    for cls in (LM_S2GP, LM_S2GP_Ford):
        geo, pol = cls(O.default_args()), cls(O.default_args(proj='polar'))
        assert [(k, tuple(v.shape), v.dtype) for k, v in geo.state_dict().items()] == \
            [(k, tuple(v.shape), v.dtype) for k, v in pol.state_dict().items()]
    sd = O.synth_model_state(1)
    LM_S2GP(O.default_args(proj='polar')).load_state_dict(sd, strict=True)
    R.build('kitti', O.default_args(proj='polar'), 1)


def test_polar_table_is_bit_identical_to_the_reference():
    """``polar_plane_table`` and the model's per-level tables against sampled entries of the reference's grd_img2cam_polar tables."""
    from highlyaccurate_amd._s2gp import polar_plane_table
    from highlyaccurate_amd.models_kitti import LM_S2GP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    g = load_golden('e2e_kitti_polar.npz')
    for cls in (LM_S2GP, LM_S2GP_Ford):            # (the two reference classes build the same table)
        tabs = cls(O.default_args(proj='polar', level=4)).xyz_tables(256, 1024, 'cpu')
        for l in range(4):
            h, w = 256 / 2 ** (3 - l), 1024 / 2 ** (3 - l)
            t = polar_plane_table(h, w)
            assert tuple(t.shape) == tuple(g[f'table_shape_l{l}']) == (int(h), int(w), 3) and t.dtype == torch.float32
            assert torch.equal(tabs[l], t)
            flat = t.reshape(-1)
            np.testing.assert_array_equal(flat[sample_idx(flat.numel(), TABLE_SALT + l)].numpy(), g[f'table_samples_l{l}'])
            assert flat.double().sum().item() == float(g[f'table_sum_l{l}'])
            assert float(t[..., 2].min()) > 0          # the all-ones mask is what the kernels' z > 0 test gives
            rt, _ = R.polar_points(h, w)
            assert torch.equal(rt[0], t)
    # 'geo' still gets the ground-plane tables
    assert not torch.equal(LM_S2GP(O.default_args()).xyz_tables(256, 1024, 'cpu')[0], tabs[0])


def test_rows_follow_the_projection():
    """What used to assume 'only the bottom half is read' follows the projection: no ground crop, no backward row trimming."""
    from types import SimpleNamespace
    from highlyaccurate_amd import _s2gp
    for proj, f8 in (('geo', 16), ('polar', 0)):
        m = SimpleNamespace(args=O.default_args(proj=proj), level=3, polar=proj == 'polar')
        assert _s2gp._bwd_first_row8(m, (256, 1024), 128) == f8


def test_restatement_matches_reference_golden_kitti():
    """Full KITTI shape, fp32: 15-step trace of every recorded seed, the final pose and the train-mode tuple."""
    g = load_golden('e2e_kitti_polar.npz')
    B = int(g['B'])
    for seed in (int(s) for s in g['seeds']):
        net = R.build('kitti', O.default_args(proj='polar'), seed)
        sat, grd, gu, gv, gh = O.synth_images(seed + 100, B)
        torch.manual_seed(seed)
        with torch.no_grad():
            res = net(sat, grd, mode='test')
        got = _trace(net, B)
        err = np.abs(got - g[f'trace32_{seed}']).max()
        print(f'restatement vs reference, kitti polar seed {seed} fp32: max pose err {err:.2e} (range {np.abs(g[f"trace32_{seed}"]).max():.2e})')
        assert err < 2e-5
        np.testing.assert_allclose(torch.stack(res, -1).double().numpy(), g[f'final32_{seed}'], rtol=0, atol=2e-5)
        torch.manual_seed(seed)
        with torch.no_grad():
            res = net(sat, grd, gu, gv, gh, mode='train')
        assert len(res) == 14
        np.testing.assert_allclose(_tuple9(res), g[f'tuple32_{seed}'], rtol=2e-3, atol=2e-4)
        assert np.abs(g[f'otrace64_{seed}'] - g[f'trace32_{seed}']).max() < 1e-3     # the seed is well conditioned in the reference


def test_restatement_matches_reference_golden_ford():
    g = load_golden('e2e_ford_polar.npz')
    seed, B = int(g['seed']), int(g['B'])
    for dtype, key, tol in ((torch.float32, 'trace32', 2e-5), (torch.float64, 'otrace64', 1e-9)):
        net = R.build('ford', O.default_args(proj='polar', N_iters=int(g['N_iters'])), seed, dtype)
        sat, grd, *_ = O.synth_images(seed + 100, B)
        torch.manual_seed(seed)
        with torch.no_grad():
            net(sat.to(dtype), grd.to(dtype), *_ford_extra(B, dtype), mode='test')
        err = np.abs(_trace(net, B) - g[key]).max()
        print(f'restatement vs fixture, ford polar {key}: max pose err {err:.2e}')
        assert err < tol
    assert np.abs(g['otrace64'] - g['trace32']).max() < 1e-3


def test_restatement_train_gradients_match_reference_and_fixture():
    """mode='train' with train_damping=1: the restatement's autograd in fp32 against the gradient samples recorded from the REAL
    reference's autograd (fp32), and in fp64 against the fp64 columns the GPU gates use (which this restatement wrote)."""
    g = load_golden('e2e_kitti_polar.npz')
    seed, B = int(g['seeds'][0]), int(g['B'])
    keys = [k[len('grad32_'):] for k in g.files if k.startswith('grad32_')]
    assert len(keys) == 7
    for dtype in (torch.float32, torch.float64):
        net = R.build('kitti', O.default_args(proj='polar', train_damping=1), seed, dtype)
        sat, grd, gu, gv, gh = (t.to(dtype) for t in O.synth_images(seed + 100, B))
        torch.manual_seed(seed)
        res = net(sat, grd, gu, gv, gh, mode='train')
        res[0].backward()
        named = dict(net.named_parameters())
        if dtype == torch.float32:
            assert set(k for k, p in named.items() if p.grad is None) == set(str(k) for k in g['nograd_32'])
            np.testing.assert_allclose(_tuple9(res), g['tuple32_td'], rtol=2e-3, atol=2e-4)
        else:
            np.testing.assert_allclose(_tuple9(res), g['otuple64_td'], rtol=1e-9, atol=1e-9)
        for k in keys:
            gr = named[k].grad.double().reshape(-1)
            got = gr[sample_idx(gr.numel(), 77)].numpy()
            if dtype == torch.float32:
                ref = g['grad32_' + k]
                e = np.abs(got - ref[2:]).max() / np.abs(ref[2:]).max()
                print(f'restatement vs reference autograd, kitti polar {k:36s} rel err {e:.2e}')
                assert e < 2e-3, (k, e)
            else:
                np.testing.assert_allclose(got, g['ograd64_' + k][2:], rtol=1e-6, atol=1e-9 * float(gr.abs().max()))


# ----------------------------------------------------------------------------------------------------------------------
# LM_S2GP.orien_corr
# ----------------------------------------------------------------------------------------------------------------------
GRID_SALT = 41           # tools/make_golden_polar.py
STUB_RANGES = (0, 40, 200, 6000)


def test_orien_corr_surface_exists():
    """``hasattr(LM_S2GP, 'orien_corr')`` fails without the feature; Ford has none (nor has the reference's Ford class)."""
    from highlyaccurate_amd.models_kitti import LM_S2GP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    from highlyaccurate_amd._lib import HlaError
    for name in ('orien_corr', 'polar_coordinates', 'polar_transform'):
        assert hasattr(LM_S2GP, name) and not hasattr(LM_S2GP_Ford, name)
    net = LM_S2GP(O.default_args())
    assert len(net.polar_grids) == 4 and net.last_orien_corr is None and len(net.state_dict()) == 49
    with pytest.raises(HlaError):                     # CPU tensors raise like everything else
        net.orien_corr(torch.zeros(1, 3, 512, 512), torch.zeros(1, 3, 256, 1024), mode='test')


def test_polar_coordinates_are_bit_identical_to_the_reference():
    from highlyaccurate_amd.models_kitti import LM_S2GP
    g = load_golden('orien_corr_kitti.npz')
    net = LM_S2GP(O.default_args(level=4))
    for l in range(4):
        for grid in (net.polar_grids[l], net.polar_coordinates(l), R.polar_grid(l)):
            assert tuple(grid.shape) == tuple(g[f'grid_shape_l{l}']) and grid.dtype == torch.float32
            flat = grid.reshape(-1)
            np.testing.assert_array_equal(flat[sample_idx(flat.numel(), GRID_SALT + l)].numpy(), g[f'grid_samples_l{l}'])
            assert flat.double().sum().item() == float(g[f'grid_sum_l{l}'])


def test_window_columns_follow_the_reference_slices():
    """The column list the product samples equals the reference's ``cat`` of slices, the clamping cases included."""
    from highlyaccurate_amd._orien import window_columns, shifts
    P = torch.arange(512.0).reshape(1, 1, 1, 512)
    for rr, n, S in ((0, 0, 513), (40, 4, 9), (200, 18, 37), (6000, 534, 1047)):
        assert shifts(rr, 8) == (90 / 8, n)
        cols = window_columns(512, 8, n)
        assert len(cols) - 8 + 1 == S
        assert R.polar_window(P, 8, n).reshape(-1).tolist() == [float(c) for c in cols]
    assert window_columns(2048, 512, 57) == [c % 2048 for c in range(-57, 512 + 57)]


def test_orien_corr_restatement_matches_the_reference_stub_fixture():
    """fp32: the reference's recorded corr, loss, heading and map gradients for all four ranges; fp64: the columns the GPU gates use."""
    g = load_golden('orien_corr_stub.npz')
    gh = torch.from_numpy(g['gt_heading'])
    for rr in STUB_RANGES:
        for dtype, pre, tol in ((torch.float32, '', 2e-5), (torch.float64, 'o', 1e-11)):
            bits = '32' if dtype == torch.float32 else '64'
            s = torch.from_numpy(g['sat_feat']).to(dtype).requires_grad_(True)
            f = torch.from_numpy(g['grd_feat']).to(dtype).requires_grad_(True)
            corr, deg, n, _, _ = R.orien_corr_level(s, f, 0, float(rr))
            loss = R.triplet_loss([(corr, deg)], gh.to(dtype), float(rr))
            loss.backward()
            assert n == int(g[f'n_{rr}']) and deg == float(g[f'deg_{rr}'])
            np.testing.assert_allclose(corr.detach().double().numpy(), g[f'{pre}corr{bits}_{rr}'], rtol=0, atol=tol)
            np.testing.assert_allclose(float(loss.detach()), float(g[f'{pre}loss{bits}_{rr}']), rtol=max(tol, 1e-9) * 100)
            for name, t in (('dsat', s), ('dgrd', f)):
                ref = g[f'{pre}{name}{bits}_{rr}']
                e = np.abs(t.grad.double().numpy() - ref).max() / np.abs(ref).max()
                assert e < (2e-3 if dtype == torch.float32 else 1e-9), (rr, name, e)
            if corr.shape[1] <= 128:                  # an unambiguous minimum (tools/make_golden_polar.py): the planted shift
                assert float(g[f'margin_{rr}']) > 1e-3
                assert int(torch.argmin(corr[1])) == n + int(g['planted_shift'])
                np.testing.assert_array_equal(((torch.argmin(corr, -1) - n) * deg).double().numpy(), g[f'{pre}orien{bits}_{rr}'])


def test_orien_corr_restatement_matches_the_reference_kitti_fixture():
    """Full KITTI shape, B = 2, fp32: per-level corr, the train loss, the test-mode heading and the gradient samples recorded from
    the REAL reference's autograd."""
    g = load_golden('orien_corr_kitti.npz')
    seed, B = int(g['seed']), int(g['B'])
    net = O.build('kitti', O.default_args(), seed)
    sat, grd, gu, gv, gh = O.synth_images(seed + 100, B)
    loss, cl = R.orien_corr(net, sat, grd, gh, mode='train')
    loss.backward()
    for l, (c, deg) in enumerate(cl):
        assert deg == float(g[f'deg_l{l}'])
        np.testing.assert_allclose(c.detach().double().numpy(), g[f'corr32_l{l}'], rtol=0, atol=2e-5)
    np.testing.assert_allclose(float(loss.detach()), float(g['loss32']), rtol=2e-3)
    named = dict(net.named_parameters())
    assert set(k for k, p in named.items() if p.grad is None) == set(str(k) for k in g['nograd_32'])
    for k in (k[len('grad32_'):] for k in g.files if k.startswith('grad32_')):
        gr = named[k].grad.double().reshape(-1)
        ref = g['grad32_' + k]
        e = np.abs(gr[sample_idx(gr.numel(), 77)].numpy() - ref[2:]).max() / np.abs(ref[2:]).max()
        print(f'restatement vs reference autograd, orien_corr {k:36s} rel err {e:.2e}')
        assert e < 2e-3, (k, e)
    last = cl[-1][0].detach()
    n = (last.shape[1] - 1) // 2
    np.testing.assert_array_equal(((torch.argmin(last, -1) - n) * cl[-1][1]).double().numpy(), g['orien32'])
