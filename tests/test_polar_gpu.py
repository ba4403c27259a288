"""GPU tests of ``proj='polar'`` for ``LM_S2GP`` / ``LM_S2GP_Ford``: the polar table and the whole-map rows through the LM loop
(hla_s2g_lm_solve / _bwd with row0 = 0) and the model surface, against the fp64 restatement (tests/polar_ref.py, pinned to the
reference's recorded fp32 results by tests/test_polar_cpu.py) and the fixtures of tools/make_golden_polar.py.  The gates are those
tests/test_gpu_parity.py applies to the same quantities for proj='geo'."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from make_idx import sample_idx
import polar_ref as R

pytestmark = pytest.mark.gpu

TOL_SHIFT, TOL_YAW = 5e-6, 5.7e-4


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def _pose_gate(got, g64, g32, what):
    """|hip - ref64| <= max(tol, 2*|ref32 - ref64|), componentwise; last axis = (u, v, theta)."""
    tol = np.array([TOL_SHIFT, TOL_SHIFT, TOL_YAW])
    allow = np.maximum(tol, 2 * np.abs(g32 - g64))
    err = np.abs(got - g64)
    worst = (err / allow).max()
    print(f'{what}: max err {err.max():.2e} (ref fp32-fp64 gap {np.abs(g32 - g64).max():.2e}), worst ratio {worst:.2f}')
    assert worst <= 1.0, (what, err.max())


def _exec_order(trace):
    B, N, L, _ = trace.shape
    return trace.reshape(B, N * L, 3).cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_e2e_kitti_polar_vs_golden(precision):
    """LM_S2GP(proj='polar'), mode='test', full KITTI shape, B = 1: the 15-step trace of both fixture seeds; args.ground_crop is
    inert (every row is read), so both settings give the same bits.  Without the feature: NotImplementedError in the constructor."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    g = load_golden('e2e_kitti_polar.npz')
    B, d = int(g['B']), _dev()
    for seed in (int(s) for s in g['seeds']):
        sat, grd, *_ = O.synth_images(seed + 100, B)
        traces = []
        for crop in (0, 1):
            net = LM_S2GP(O.default_args(proj='polar', precision=precision, ground_crop=crop))
            net.load_state_dict(O.synth_model_state(seed))
            net = net.to(d)
            torch.manual_seed(seed)
            with torch.no_grad():
                res = net(sat.to(d), grd.to(d), mode='test')
            traces.append(net.last_trace.clone())
        assert torch.equal(traces[0], traces[1])
        trace = _exec_order(traces[0])
        _pose_gate(trace, g[f'otrace64_{seed}'], g[f'trace32_{seed}'], f'kitti polar {precision} seed {seed}')
        final = torch.stack(res, -1).cpu().numpy()
        np.testing.assert_allclose(final, g[f'final32_{seed}'], atol=2e-3)          # ordering check (lat, lon, theta)
        np.testing.assert_array_equal(final[:, [1, 0, 2]], trace[:, -1].astype(np.float32))


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_e2e_ford_polar_vs_golden(precision):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    g = load_golden('e2e_ford_polar.npz')
    seed, B, d = int(g['seed']), int(g['B']), _dev()
    sat, grd, *_ = O.synth_images(seed + 100, B)
    R_FL = torch.tensor([[[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]]).repeat(B, 1, 1)
    T_FL = torch.tensor([[1.7, 0.3, -1.2]]).repeat(B, 1)
    traces = []
    for crop in (0, 1):
        net = LM_S2GP_Ford(O.default_args(proj='polar', N_iters=int(g['N_iters']), precision=precision, ground_crop=crop))
        net.load_state_dict(O.synth_model_state(seed))
        net = net.to(d)
        torch.manual_seed(seed)
        with torch.no_grad():
            res = net(sat.to(d), grd.to(d), 112.64, R_FL.to(d), T_FL.to(d), mode='test')
        traces.append(net.last_trace.clone())
        with pytest.raises(NotImplementedError, match='level_first'):
            net(sat.to(d), grd.to(d), 112.64, R_FL.to(d), T_FL.to(d), mode='test', level_first=1)
    assert torch.equal(traces[0], traces[1])
    trace = _exec_order(traces[0])
    _pose_gate(trace, g['otrace64'], g['trace32'], f'ford polar {precision}')
    np.testing.assert_array_equal(torch.stack(res, -1).cpu().numpy(), trace[:, -1].astype(np.float32))


@pytest.mark.parametrize('kw', [dict(using_weight=1, dropout=1), dict(using_weight=1), dict(level_first=1),
                                dict(Optimizer='SGD'), dict(Optimizer='ADAM')])
def test_polar_lm_solve_small_vs_restatement(kw):
    """hla_s2g_lm_solve with row0 = 0 and the polar table on a reduced pyramid: B = 2, ground maps of 9 / 18 / 36 rows (an odd
    number at the coarsest level) by 33 / 66 / 132 columns -- no multiple of the pixel tile, several tiles per sample -- computed by
    the restatement's extractors with non-zero biases.  The 14 normal-equation sums of the first step (LM_update: under the gate
    test_gpu_parity.py applies to them for 'geo', 2e-6 of each sum's scale; with dropout the restatement leaves out the pixels
    the product's recorded keep mask drops) and the whole trace against the fp64 restatement."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    d = _dev()
    kw = dict(kw)
    lf = kw.pop('level_first', 0)
    args = O.default_args(proj='polar', **{'N_iters': 3, 'damping': 1.0, **kw})
    B, grd_hw, sat_a = 2, (72, 264), 136
    onet = R.build('kitti', args, 3, torch.float64, bias_scale=0.05, grd_hw=grd_hw)
    img_s, img_g, *_ = O.synth_images(11, B, grd_hw=grd_hw, sat_a=sat_a)
    with torch.no_grad():
        sat, _ = onet.SatFeatureNet(img_s.double())
        grd, conf = onet.GrdFeatureNet(img_g.double())
    sat, grd, conf = ([t.float() for t in ts] for ts in (sat, grd, conf))        # the inputs of both sides: fp32 values
    assert [tuple(t.shape[-2:]) for t in grd] == [(9, 33), (18, 66), (36, 132)]
    p0 = T(np.random.RandomState(4).uniform(-0.3, 0.3, size=(B, 3)).astype(np.float32))
    net = LM_S2GP(args).to(d)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(d)
    torch.manual_seed(0)
    np.random.seed(0)                      # args.dropout draws its pixel subsets from numpy's global generator
    trace = net.lm_solve([nh(s) for s in sat], [nh(g) for g in grd], [c[:, 0].contiguous().to(d) for c in conf],
                         grd_hw, None, lf, init_pose=p0, keep_normal_eq=True).cpu().numpy()
    pose = [p0[:, i:i + 1].double() for i in range(3)]
    if args.Optimizer == 'LM':
        neq = net.last_normal_eq[0, :, :14].cpu().numpy()
        keep = net.last_keep[0, :9 * 33].cpu().bool() if args.dropout else None
        assert keep is None or int(keep.sum()) == (9 * 33) // 2          # half of the WHOLE map's pixels
        ref_neq = R.normal_eq(onet, sat, grd, conf, pose, 0, args.using_weight, keep=keep)
        e_neq = np.abs(neq - ref_neq).max(0) / np.abs(ref_neq).max(0).clip(1e-30)
        print('polar normal-eq rel err per sum:', np.array2string(e_neq, precision=1))
        assert e_neq.max() < 2e-6, e_neq
    torch.manual_seed(0)
    np.random.seed(0)
    onet._adam_t = 0
    su, sv, th = pose
    L, N = 3, args.N_iters
    order = [(i, l) for l in range(L) for i in range(N)] if lf else [(i, l) for i in range(N) for l in range(L)]
    ref = np.zeros((B, N, L, 3))
    for i, l in order:
        su, sv, th = onet._step(l, sat[l].double(), None, grd[l].double(), conf[l].double(), su, sv, th, None)
        ref[:, i, l] = torch.cat([su, sv, th], 1).numpy()
    err = np.abs(trace - ref).max()
    print('polar lm small', kw, 'lf', lf, 'trace max err', err, 'ref range', np.abs(ref).max())
    assert np.isfinite(trace).all()
    assert err < 1e-4 * max(1.0, np.abs(ref).max()), (kw, err)


def _train_step(net, sat, grd, gt, seed):
    net.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    res = net(sat, grd, *gt, mode='train')
    res[0].backward()
    torch.cuda.synchronize()
    return res, {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_polar_train_step_gradients_vs_golden(precision):
    """mode='train' under autograd with train_damping = 1, full KITTI shape, B = 1: the loss and parameter-gradient samples
    against the fp64 restatement's, under the gates test_gpu_parity.py applies to train_kitti.npz (the reference's own
    fp32-vs-fp64 gap from its recorded fp32 autograd); args.train_ground_crop and args.bwd_trim are inert for the rows (every row
    carries gradient); args.deterministic_backward = 1 twice over gives the same bits."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    g = load_golden('e2e_kitti_polar.npz')
    seed, B, d = int(g['seeds'][0]), int(g['B']), _dev()
    net = LM_S2GP(O.default_args(proj='polar', train_damping=1, precision=precision, train_ground_crop=1))
    net.load_state_dict(O.synth_model_state(seed))
    net = net.to(d).train()
    sat, grd, gu, gv, gh = O.synth_images(seed + 100, B)
    sat, grd, gt = sat.to(d), grd.to(d), [gu.to(d), gv.to(d), gh.to(d)]
    res, grads = _train_step(net, sat, grd, gt, seed)
    ref_t = g['otuple64_td']
    assert abs(float(res[0].detach()) - ref_t[0][0]) < 1e-3 * abs(ref_t[0][0])
    for i in range(1, 9):
        np.testing.assert_allclose(res[i].detach().cpu().numpy(), ref_t[i], rtol=1e-3, atol=2e-3)
    assert tuple(res[13][0].shape) == (B, 1, 32, 128) and bool((res[13][0][:, :, :4] != 0).all())     # whole maps, no crop
    nograd = set(str(k) for k in g['nograd_32'])
    for k, _ in net.named_parameters():
        assert (k not in grads) == (k in nograd), k
    keys = [k[len('ograd64_'):] for k in g.files if k.startswith('ograd64_')]
    assert len(keys) == 7
    for k in keys:
        ref = g['ograd64_' + k]
        gr = grads[k].double().reshape(-1).cpu()
        got = np.concatenate([[gr.abs().sum().item(), (gr * gr).sum().item()], gr[sample_idx(gr.numel(), 77)].numpy()])
        gap = np.abs(g['grad32_' + k][2:] - ref[2:]).max()
        scale = np.abs(ref[2:]).max()
        e = np.abs(got[2:] - ref[2:]).max()
        print(f'polar train grad [{precision}] {k:36s} max err {e:.2e} (ref fp32 gap {gap:.2e}, scale {scale:.2e}); l1 {got[0]:.4e} vs {ref[0]:.4e}')
        rel_tol = 2e-4 if 'conv_dec2' in k else 5e-3
        assert e <= max(rel_tol * scale, 3 * gap), (k, e, gap, scale)
        assert abs(got[0] - ref[0]) <= max(2e-3 * ref[0], 3 * abs(g['grad32_' + k][0] - ref[0]))
    net.args.deterministic_backward = 1
    _, g1 = _train_step(net, sat, grd, gt, seed)
    _, g2 = _train_step(net, sat, grd, gt, seed)
    assert len(g1) >= 36
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    rel = max(float((g1[n].double() - grads[n].double()).norm() / max(float(grads[n].double().norm()), 1e-30)) for n in g1)
    print(f'polar deterministic backward [{precision}]: 2 runs bitwise equal over {len(g1)} tensors; vs the atomics mode: worst relative L2 {rel:.2e}')
    assert rel < 1e-3


# ----------------------------------------------------------------------------------------------------------------------
# LM_S2GP.orien_corr: hla_orien_corr / _bwd, hla_orien_triplet_loss / _bwd and the model surface
# ----------------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -23
STUB_RANGES = (0, 40, 200, 6000)
# Model-level corr bounds (normalised: corr is O(1)) = 3x max |hip - restatement_fp64| over the three levels of orien_corr_kitti.npz
# measured on MI355X when the test was first run (EXPERIMENTS.md, "proj='polar' and orien_corr"); the fp32-class bound may not
# exceed 1e-4, the reference's own accuracy gate.  Measured: fp32 1.276e-07, fp16x3 1.452e-07 (half an fp32 ulp of a corr near 2 is
# 1.2e-07; the reference's own fp32 run is 3.7e-05 from the same fp64 values), bf16 1.858e-03 (the extractors' bf16 features).
CORR_BOUND = {'fp32': 3.9e-7, 'fp16x3': 4.4e-7, 'bf16': 5.6e-3}


def _gate(got, r64, r32, what):
    """max|hip - ref64| <= max(2 max|ref32 - ref64|, 8 eps_fp32 max|ref64|): the second term allows a handful of fp32 roundings
    in the final divide and square root."""
    got, r64, r32 = (np.asarray(a, dtype=np.float64) for a in (got, r64, r32))
    err, allow = np.abs(got - r64).max(), max(2 * np.abs(r32 - r64).max(), 8 * EPS32 * np.abs(r64).max())
    print(f'{what}: max err {err:.2e}, allowed {allow:.2e} (ref fp32-fp64 gap {np.abs(r32 - r64).max():.2e}, scale {np.abs(r64).max():.2e})')
    assert np.isfinite(got).all() and err <= allow, (what, err, allow)


def _nhwc16(t, d):
    """NCHW -> NHWC on the device, channels zero-padded to 16 (zero channels add nothing to any sum or gradient)."""
    t = t.permute(0, 2, 3, 1).float()
    if t.shape[-1] < 16:
        t = torch.nn.functional.pad(t, (0, 16 - t.shape[-1]))
    return t.contiguous().to(d)


def _stub_window(d, B, W, n):
    from highlyaccurate_amd import _orien
    from oracle import ref_cpu as O
    grid = _orien.polar_coordinates(O.meter_per_pixel() * 8, 0)
    cols = torch.tensor(_orien.window_columns(grid.shape[2], W, n))
    return grid[:, :, cols, :].expand(B, -1, -1, -1).contiguous().to(d)


@pytest.mark.parametrize('rr', STUB_RANGES)
def test_orien_corr_kernels_on_the_stub_fixture(rr):
    """The kernels alone -- window sampling, hla_orien_corr, the triplet loss, their backward down to d(sat map)
    (hla_orien_window_bwd) -- on the stub
    fixture recorded from the REAL reference (S = 513, 9, 37, 1047: one shift tile and several, n < W, n > W, both clamped-slice
    cases).  The fixture's 4 channels are zero-padded to 16.  Planted minimum: exact where it is unambiguous."""
    from highlyaccurate_amd import _orien
    g = load_golden('orien_corr_stub.npz')
    d = _dev()
    n, deg = int(g[f'n_{rr}']), float(g[f'deg_{rr}'])
    sat, grd = _nhwc16(T(g['sat_feat']), d), _nhwc16(T(g['grd_feat']), d)
    B, H, W, _ = grd.shape
    grid = _stub_window(d, B, W, n)
    P1 = _orien.sample_window(sat, grid)
    corr, saved = _orien.corr_forward(P1, grd, None, None)
    assert tuple(corr.shape) == g[f'ocorr64_{rr}'].shape
    _gate(corr.cpu(), g[f'ocorr64_{rr}'], g[f'corr32_{rr}'], f'stub rr {rr} corr')
    gh = T(g['gt_heading']).float().to(d)[:, 0]
    loss = torch.empty(1, device=d)
    _orien.triplet_loss(corr, gh, rr, deg, loss, False)
    _gate(loss.cpu(), g[f'oloss64_{rr}'], g[f'loss32_{rr}'], f'stub rr {rr} loss')
    d_corr = _orien.triplet_loss_bwd(corr, gh, rr, deg, torch.ones(1, device=d))
    d_P1, d_grd = _orien.corr_backward(P1, grd, None, None, saved, d_corr)
    d_sat = _orien.sample_window_bwd(sat, grid, d_P1)
    assert not bool(d_grd[..., 4:].any()) and not bool(d_sat[..., 4:].any())
    _gate(d_grd[..., :4].permute(0, 3, 1, 2).cpu(), g[f'odgrd64_{rr}'], g[f'dgrd32_{rr}'], f'stub rr {rr} d_grd_feat')
    _gate(d_sat[..., :4].permute(0, 3, 1, 2).cpu(), g[f'odsat64_{rr}'], g[f'dsat32_{rr}'], f'stub rr {rr} d_sat_feat')
    again = _orien.corr_backward(P1, grd, None, None, saved, d_corr)                 # gather form: bitwise reproducible
    assert torch.equal(again[0], d_P1) and torch.equal(again[1], d_grd)
    idx = torch.argmin(corr, -1).cpu()
    if corr.shape[1] <= 128:
        assert float(g[f'margin_{rr}']) > 1e-3 and int(idx[1]) == n + int(g['planted_shift'])
        np.testing.assert_array_equal(((idx - n) * deg).double().numpy()[1], g[f'oorien64_{rr}'][1])
    else:                       # the polar map repeats every 128 columns: the minimum is a tie, up to the grid's fp32 rounding
        assert int(idx[1]) % 128 == int(g['planted_shift'])


@pytest.mark.parametrize('C', [16, 64, 128, 256])
@pytest.mark.parametrize('H', [1, 5])
def test_orien_corr_kernels_on_random_arrays(C, H):
    """hla_orien_corr / _bwd alone on random arrays: W = 150 and S = 141 (window 290 columns) are no multiple of any column or shift
    tile (128 / 64 forward, 64 or 256 backward) and span several; two samples with different content and raw maps with inverse
    norms; a third sample whose satellite window is all zero: E is below the clamp, corr == 2 and no gradient flows through E.
    Reference: autograd through the restatement in fp64 (fp32 for the gate's reference gap)."""
    from highlyaccurate_amd import _orien
    d = _dev()
    rs = np.random.RandomState(100 + C + H)
    B, W, S = 3, 150, 141
    P1 = rs.standard_normal((B, C, H, W + S - 1))
    P1[2] = 0.0
    grd = rs.standard_normal((B, C, H, W))
    a_s, a_g = rs.uniform(0.5, 2.0, size=B), rs.uniform(0.5, 2.0, size=B)
    coef = rs.standard_normal((B, S))
    ref = {}
    for dtype in (torch.float64, torch.float32):
        p = T(P1).to(dtype).requires_grad_(True)           # gradients w.r.t. the SCALED maps, as the kernel reports them
        f = T(grd).to(dtype).requires_grad_(True)
        ps = (p * T(a_s).to(dtype).view(B, 1, 1, 1)).detach().requires_grad_(True)
        fs = (f * T(a_g).to(dtype).view(B, 1, 1, 1)).detach().requires_grad_(True)
        c = R.corr_from_window(ps, fs, safe_clamp=True)
        (c * T(coef).to(dtype)).sum().backward()
        ref[dtype] = (c.detach().double().numpy(), ps.grad.double().numpy(), fs.grad.double().numpy())
    nh = lambda a: T(a).float().permute(0, 2, 3, 1).contiguous().to(d)
    p_d, f_d = nh(P1), nh(grd)
    inv_s, inv_g = T(a_s).to(d), T(a_g).to(d)
    corr, saved = _orien.corr_forward(p_d, f_d, inv_s, inv_g)
    again, _ = _orien.corr_forward(p_d, f_d, inv_s, inv_g)
    assert torch.equal(corr, again)
    assert bool((corr[2] == 2.0).all())
    d_P1, d_grd = _orien.corr_backward(p_d, f_d, inv_s, inv_g, saved, T(coef).float().to(d))
    r64, r32 = ref[torch.float64], ref[torch.float32]
    _gate(corr.cpu(), r64[0], r32[0], f'random C {C} H {H} corr')
    _gate(d_grd.permute(0, 3, 1, 2).cpu(), r64[2], r32[2], f'random C {C} H {H} d_grd_feat')
    # d_P1 of the zero sample is ddot / 1e-6-sized (the clamped denominator): gate it on its own scale
    _gate(d_P1[:2].permute(0, 3, 1, 2).cpu(), r64[1][:2], r32[1][:2], f'random C {C} H {H} d_P1')
    _gate(d_P1[2:].permute(0, 3, 1, 2).cpu(), r64[1][2:], r32[1][2:], f'random C {C} H {H} d_P1 (clamped E)')
    assert not bool(d_grd[2].any())                       # P1 == 0: nothing reaches the ground map, and no NaN from sqrt(0)


def _orien_model(precision, seed):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    net = LM_S2GP(O.default_args(precision=precision))
    net.load_state_dict(O.synth_model_state(seed))
    return net.to(_dev())


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3', 'bf16'])
def test_orien_corr_model_vs_golden(precision):
    """LM_S2GP.orien_corr, KITTI shape, B = 2, both modes, against orien_corr_kitti.npz: per-level corr within CORR_BOUND of the fp64
    restatement; the returned heading is [B], the last level's, and its corr is within the bound of the fp64 minimum (white-noise
    features give a nearly flat corr, so indices are not compared); fp32-class modes: the train loss and parameter-gradient
    samples under the gates test_gpu_parity.py applies to train_kitti.npz."""
    from oracle import ref_cpu as O
    g = load_golden('orien_corr_kitti.npz')
    seed, B, d = int(g['seed']), int(g['B']), _dev()
    net = _orien_model(precision, seed).train()
    sat, grd, gu, gv, gh = (t.to(d) for t in O.synth_images(seed + 100, B))
    with torch.no_grad():
        orien = net.orien_corr(sat, grd, gu, gv, gh, mode='test')
    assert tuple(orien.shape) == (B,) and len(net.last_orien_corr) == 3
    worst = 0.0
    for l, (corr, deg) in enumerate(net.last_orien_corr):
        ref = g[f'ocorr64_l{l}']
        assert tuple(corr.shape) == ref.shape and corr.dtype == torch.float32 and deg == float(g[f'deg_l{l}'])
        e = np.abs(corr.double().cpu().numpy() - ref).max()
        print(f'orien_corr [{precision}] level {l}: max |corr - fp64| {e:.3e} (reference fp32 gap {np.abs(g[f"corr32_l{l}"] - ref).max():.2e})')
        worst = max(worst, e)
    print(f'orien_corr [{precision}]: worst corr deviation {worst:.3e}, bound {CORR_BOUND[precision]}')
    bound = CORR_BOUND[precision]
    assert bound is not None and worst <= bound, (precision, worst, bound)
    ref = g['ocorr64_l2']
    n = (ref.shape[1] - 1) // 2
    idx = torch.round(orien.double().cpu() / float(g['deg_l2'])).long() + n
    assert bool(((idx >= 0) & (idx < ref.shape[1])).all())
    np.testing.assert_array_equal(idx.numpy(), torch.argmin(net.last_orien_corr[-1][0], -1).cpu().numpy())
    assert (ref[np.arange(B), idx.numpy()] - ref.min(1)).max() <= bound
    if precision == 'bf16':
        return
    loss = net.orien_corr(sat, grd, gu, gv, gh, mode='train')
    assert loss.dim() == 0 and abs(float(loss.detach()) - float(g['oloss64'])) < 1e-3 * abs(float(g['oloss64']))
    loss.backward()
    named = dict(net.named_parameters())
    nograd = set(str(k) for k in g['nograd_32'])
    for k, p in named.items():
        assert (p.grad is None) == (k in nograd), k
    for k in (k[len('ograd64_'):] for k in g.files if k.startswith('ograd64_')):
        ref = g['ograd64_' + k]
        gr = named[k].grad.double().reshape(-1).cpu()
        got = np.concatenate([[gr.abs().sum().item(), (gr * gr).sum().item()], gr[sample_idx(gr.numel(), 77)].numpy()])
        gap, scale, e = np.abs(g['grad32_' + k][2:] - ref[2:]).max(), np.abs(ref[2:]).max(), np.abs(got[2:] - ref[2:]).max()
        print(f'orien_corr train grad [{precision}] {k:36s} max err {e:.2e} (ref fp32 gap {gap:.2e}, scale {scale:.2e}); l1 {got[0]:.4e} vs {ref[0]:.4e}')
        rel_tol = 2e-4 if 'conv_dec2' in k else 5e-3
        assert e <= max(rel_tol * scale, 3 * gap), (k, e, gap, scale)
        assert abs(got[0] - ref[0]) <= max(2e-3 * ref[0], 3 * abs(g['grad32_' + k][0] - ref[0]))
    with torch.no_grad():           # mode='train' without autograd: the same scalar
        assert float(net.orien_corr(sat, grd, gu, gv, gh, mode='train')) == float(loss.detach())


def test_orien_corr_model_finds_the_planted_heading(monkeypatch):
    """mode='test' end to end on the stub fixture's maps (the extractors replaced by stubs, as in the fixture's generator):
    a [B] tensor, the planted sample's degrees exact for the two ranges with an unambiguous minimum."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd import _orien
    from highlyaccurate_amd.models_kitti import LM_S2GP
    g = load_golden('orien_corr_stub.npz')
    d = _dev()
    sat, grd = _nhwc16(T(g['sat_feat']), d), _nhwc16(T(g['grd_feat']), d)
    B = sat.shape[0]

    def stub(module, x, **kw):
        return [sat if x.shape[-1] == 512 else grd], None, torch.ones(1, B, device=d, dtype=torch.float64)
    monkeypatch.setattr(_orien, 'vgg_forward_nhwc', stub)
    for rr in (40, 200):
        net = LM_S2GP(O.default_args(rotation_range=float(rr))).to(d)
        with torch.no_grad():
            orien = net.orien_corr(torch.zeros(B, 3, 512, 512, device=d), torch.zeros(B, 3, 256, 64, device=d), mode='test')
        assert tuple(orien.shape) == (B,)
        np.testing.assert_array_equal(orien.double().cpu().numpy(), g[f'oorien64_{rr}'])
        assert float(orien[1]) == int(g['planted_shift']) * float(g[f'deg_{rr}'])


def test_orien_corr_argument_errors():
    from oracle import ref_cpu as O
    from highlyaccurate_amd import _orien
    from highlyaccurate_amd._lib import HlaError
    from highlyaccurate_amd.models_kitti import LM_S2GP
    d = _dev()
    net = LM_S2GP(O.default_args()).to(d)
    with pytest.raises(HlaError, match='HIP device'):
        net.orien_corr(torch.zeros(1, 3, 512, 512), torch.zeros(1, 3, 256, 1024, device=d), mode='test')
    with pytest.raises(ValueError, match='polar grids are built'):
        net.orien_corr(torch.zeros(1, 3, 256, 256, device=d), torch.zeros(1, 3, 256, 1024, device=d), mode='test')
    with pytest.raises(ValueError, match='256 rows'):
        net.orien_corr(torch.rand(1, 3, 512, 512, device=d), torch.rand(1, 3, 128, 512, device=d), mode='test')
    with pytest.raises(ValueError, match='gt_heading'):
        net.orien_corr(torch.zeros(1, 3, 512, 512, device=d), torch.zeros(1, 3, 256, 1024, device=d), mode='train')
    for Cn in (4, 32, 20):
        with pytest.raises(HlaError, match='unsupported channel count'):
            _orien.corr_forward(torch.zeros(1, 2, 9, Cn, device=d), torch.zeros(1, 2, 8, Cn, device=d), None, None)
    with pytest.raises(ValueError, match='does not match'):
        _orien.corr_forward(torch.zeros(1, 2, 7, 16, device=d), torch.zeros(1, 2, 8, 16, device=d), None, None)
