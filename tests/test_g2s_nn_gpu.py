"""GPU tests of ``LM_G2SP(proj='nn')``: the folded ground extractor (HLA_VGG_FOLD_DECODER), the in-plane warp solver
(hla_g2s_lm_solve / _bwd with cfg->proj = 1) and the model surface, against the fp64 restatement (tests/g2s_nn_ref.py, pinned to
the real reference by tests/test_g2s_nn_cpu.py) and the reference's recorded fp32 results.  Tolerances are those of the geo
direction's tests in test_gpu_parity.py; the bf16 bound is 3x a deviation measured on the MI355X (EXPERIMENTS.md)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from make_idx import sample_idx
import g2s_nn_ref as R

pytestmark = pytest.mark.gpu

TOL_SHIFT, TOL_YAW = 5e-6, 5.7e-4          # test_gpu_parity.py
# 3x max |bf16 - restatement_fp64| over the 15 steps of both fixture seeds, measured on MI355X (EXPERIMENTS.md, "LM_G2SP proj='nn'"):
# shifts 7.35e-4, heading 1.73e-3 (normalised units)
NN_BF16_LIMITS = (2.2e-3, 5.2e-3)


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _pose_gate(got, g64, g32, what):
    """|hip - ref64| <= max(tol, 2*|ref32 - ref64|), componentwise; last axis = (u, v, theta)."""
    tol = np.array([TOL_SHIFT, TOL_SHIFT, TOL_YAW])
    allow = np.maximum(tol, 2 * np.abs(g32 - g64))
    err = np.abs(got - g64)
    worst = (err / allow).max()
    print(f'{what}: max err {err.max():.2e} (ref fp32-fp64 gap {np.abs(g32 - g64).max():.2e}), worst ratio {worst:.2f}')
    assert worst <= 1.0, (what, err.max())


def _model(seed, B, **kw):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_G2SP
    args = O.default_args(proj='nn', **kw)           # without the feature: NotImplementedError here
    net = LM_G2SP(args)
    sd = O.synth_model_state(seed)
    sd['damping'] = args.damping * torch.ones(1, 3)
    net.load_state_dict(sd)
    sat, grd, gu, gv, gh = O.synth_images(seed + 100, B)
    K = torch.tensor([O.KITTI_K], dtype=torch.float32).repeat(B, 1, 1)
    return net.to(_dev()), [t.to(_dev()) for t in (sat, grd, K, gu, gv, gh)]


@pytest.mark.parametrize('precision,tol', [('fp32', 1e-5), ('fp16x3', 1e-5), ('bf16', 3e-2), ('fp16', 4e-3)])
def test_vgg_g2s_small_vs_golden(precision, tol):
    """VGGUnet_G2S(4) with non-zero biases against the reference's fp64 maps and confidences (all four, folded; c0 unfolded)."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.VGG import VGGUnet_G2S
    g = load_golden('vgg_g2s_small.npz')
    d = _dev()
    rs = np.random.RandomState(int(g['seed']))
    sd = O.synth_vgg_state(rs, bias_scale=0.05)
    x = T(rs.random_sample(tuple(int(v) for v in g['x_shape'])).astype(np.float32))
    B, _, H, W = x.shape
    net = VGGUnet_G2S(4, precision=precision)
    net.load_state_dict(sd)
    net = net.to(d)
    with torch.no_grad():
        feats, confs = net(x.to(d))
    assert len(feats) == 4 and len(confs) == 4
    assert tuple(confs[0].shape) == (B, 1, H // 8, W // 8) and tuple(feats[0].shape) == (B, 256, H // 4, W // 16)
    assert tuple(feats[3].shape) == (B, 16, 2 * H, W // 2) and tuple(confs[3].shape) == (B, 1, 2 * H, W // 2)
    for l in range(4):
        f = feats[l].cpu().numpy()
        assert f.shape == g[f'vgg_feat64_l{l}'].shape and confs[l].shape == g[f'vgg_conf64_l{l}'].shape
        e = _rel(f, g[f'vgg_feat64_l{l}'])
        ec = _rel(confs[l].cpu().numpy(), g[f'vgg_conf64_l{l}'])
        ss = (f.astype(np.float64) ** 2).reshape(B, -1).sum(1)
        print(f'vgg g2s {precision} map {l}: feat rel {e:.2e} conf rel {ec:.2e} sum x^2 - 1 {np.abs(ss - 1).max():.1e}')
        assert e < tol and ec < max(tol, 2e-6), (precision, l, e, ec)
        assert np.abs(ss - 1.0).max() < 1e-6, (precision, l, ss)


def test_vgg_fold_argument_errors_are_reported():
    """Shapes the folded geometry cannot take are refused at the boundary with a message, not found by a fault."""
    import ctypes as C
    from highlyaccurate_amd import _lib
    from highlyaccurate_amd.VGG import VGGUnet_G2S, vgg_forward_nhwc
    d = _dev()
    net = VGGUnet_G2S(3).to(d)
    with pytest.raises(ValueError, match='multiple of 16'):
        vgg_forward_nhwc(net, torch.rand(1, 3, 16, 40, device=d))
    with pytest.raises(ValueError, match='first_row8'):
        vgg_forward_nhwc(net, torch.rand(1, 3, 64, 64, device=d), first_row8=4)
    # ... and by the C ABI itself
    lib = _lib.load()
    x = torch.rand(1, 3, 16, 40, device=d)
    prm = _lib.VggParams()
    one = torch.zeros(16, device=d)
    fp = (C.c_void_p * 4)(one.data_ptr(), one.data_ptr(), one.data_ptr(), 0)
    rc = lib.hla_vgg_forward(_lib.ptr(x), 0, C.byref(prm), _lib.ptr(one), fp, None, _lib.ptr(one), _lib.ptr(one), 64, 1, 16, 40, 3,
                             _lib.HLA_F32, _lib.HLA_VGG_FOLD_DECODER, 0, _lib.stream_ptr())
    assert rc != 0
    with pytest.raises(_lib.HlaError, match='HLA_VGG_FOLD_DECODER'):
        _lib.check(rc, 'hla_vgg_forward')


def _small_pyramid(rs, B, Cs, As, hws):
    sat = [T(rs.standard_normal((B, c, a, a)).astype(np.float32) * 0.02) for c, a in zip(Cs, As)]
    grd = [T(rs.standard_normal((B, c, h, w)).astype(np.float32) * 0.02) for c, (h, w) in zip(Cs, hws)]
    return sat, grd


# C in {16, 64, 128, 256}; A never a multiple of the 64-pixel tile (A*A % 64 != 0); ground maps both of the satellite map's size
# (pose 0 then puts the grid's last row / column exactly on the map's) and of other sizes (part of the grid falls outside)
SMALL = dict(Cs=(256, 128, 64, 16), As=(18, 27, 42, 70), hws=((18, 18), (25, 30), (42, 42), (75, 66)))


@pytest.mark.parametrize('kw', [dict(), dict(N_iters=2, damping=10.0), dict(rotation_range=40.0, shift_range_lat=60.0,
                                                                            shift_range_lon=45.0)])
def test_inplane_solve_small_vs_restatement(kw):
    """hla_g2s_lm_solve with cfg->proj = 1 on random feature pyramids: the 12 normal-equation sums of every step of the first
    iteration (one per level / channel count), evaluated by the fp64 restatement at the pose the step started from, and the
    whole trace.  Sample 0 starts at pose 0 (integer sampling positions, the last row / column hit exactly), the others at poses
    that rotate and shift part of the grid out of the map."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_G2SP
    d = _dev()
    args = O.default_args(proj='nn', **{'N_iters': 3, 'damping': 1.0, **kw})
    B, L = 3, 4
    rs = np.random.RandomState(5)
    sat, grd = _small_pyramid(rs, B, **SMALL)
    p0 = rs.uniform(-1.0, 1.0, size=(B, 3)).astype(np.float32)
    p0[0] = 0.0
    p0 = T(p0)
    net = LM_G2SP(args).to(d)
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(d)
    trace = net.lm_solve([nh(s) for s in sat], [nh(g) for g in grd], [None] * L, None, None, init_pose=p0, keep_normal_eq=True)
    trace = trace.cpu().numpy()
    neq = net.last_normal_eq.cpu().numpy()                    # [L*N, B, 16]
    assert np.isfinite(trace).all()
    assert (neq[:, :, :2] == 1.0).all()
    sat64, grd64 = [s.double() for s in sat], [g.double() for g in grd]
    lam = args.damping * torch.ones(1, 3, dtype=torch.float64)
    outside = 0
    for l in range(L):                                        # step l of iteration 0 starts from the HIP loop's own pose
        pose = p0.double() if l == 0 else T(trace[:, 0, l - 1]).double()
        su, sv, th = (pose[:, i:i + 1] for i in range(3))
        ref = R.normal_sums(args, su, sv, th, grd64[l], sat64[l]).numpy()
        e = np.abs(neq[l, :, 2:14] - ref).max(0) / np.abs(ref).max(0).clip(1e-30)
        uv, _ = R.inplane_pose_to_uv(args, SMALL['As'][l], su, sv, th)
        h, w = SMALL['hws'][l]
        outside += int(((uv[..., 0] < 0) | (uv[..., 0] > w - 1) | (uv[..., 1] < 0) | (uv[..., 1] > h - 1)).sum())
        print(f'in-plane normal eq, level {l} (C {SMALL["Cs"][l]}): rel err per sum', np.array2string(e, precision=1))
        assert e.max() < 2e-6, (l, e)
    assert outside > 0                                        # the case does push part of the grid out of the map
    ref = R.solve(args, lam, sat64, grd64, args.N_iters, p0.double()).numpy()
    err = np.abs(trace - ref).max()
    print('in-plane small', kw, 'trace max err', err, 'ref range', np.abs(ref).max())
    assert err < 1e-4 * max(1.0, np.abs(ref).max()), (kw, err)


@pytest.mark.parametrize('kw', [dict(), dict(train_damping=1)])
def test_inplane_lm_backward_small_vs_restatement_autograd(kw):
    """hla_g2s_lm_solve_bwd with cfg->proj = 1 alone, against torch autograd through the fp64 restatement's warp + LM_update
    chain (which differentiates the heading column of the Jacobian as well: a missing d2R/dtheta2 term shows here)."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_G2SP
    d = _dev()
    args = O.default_args(proj='nn', N_iters=2, damping=0.5, rotation_range=30.0, **kw)
    B, L = 2, 4
    rs = np.random.RandomState(17)
    sat, grd = _small_pyramid(rs, B, **SMALL)
    p0 = T(rs.uniform(-0.6, 0.6, size=(B, 3)).astype(np.float32))
    coef = T(rs.standard_normal((B, args.N_iters, L, 3)))
    dpar = torch.tensor([[0.4, 0.7, 0.55]])
    lam = dpar.double().requires_grad_(True)
    sat64 = [s.double().requires_grad_(True) for s in sat]
    grd64 = [g.double().requires_grad_(True) for g in grd]
    tr = R.solve(args, lam, sat64, grd64, args.N_iters, p0.double())
    (coef * tr).sum().backward()
    net = LM_G2SP(args).to(d)
    with torch.no_grad():
        net.damping.copy_(dpar.to(d))
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(d)
    feats = ([nh(s) for s in sat], [nh(g) for g in grd], [None] * L)
    trace = net.lm_solve(*feats, None, None, init_pose=p0, keep_normal_eq=True)
    assert np.abs(trace.cpu().numpy() - tr.detach().numpy()).max() < 1e-5
    d_sat, d_grd, d_conf, d_lam = net.lm_backward(*feats, None, None, trace, net.last_normal_eq, coef.float().to(d), init_pose=p0)
    for l in range(L):
        for name, got, ref in (('sat', d_sat[l], sat64[l].grad), ('grd', d_grd[l], grd64[l].grad)):
            got = got.permute(0, 3, 1, 2).cpu().double().numpy()
            e = np.abs(got - ref.numpy()).max() / max(np.abs(ref.numpy()).max(), 1e-30)
            print(f'in-plane lm bwd {kw} level {l} d_{name}: rel err {e:.2e} (max |ref| {np.abs(ref.numpy()).max():.2e})')
            assert e < 2e-4, (kw, l, name, e)
    if args.train_damping:
        ref = lam.grad.numpy()
        e = np.abs(d_lam.cpu().view(1, 3).numpy() - ref).max() / np.abs(ref).max()
        print(f'in-plane lm bwd d_damping: rel err {e:.2e}')
        assert e < 1e-5


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_e2e_nn_full_shape_vs_golden_and_restatement(precision):
    """Full KITTI shape (256 x 1024, A = 512), both recorded seeds: |hip - restatement_fp64| <= max(tol, 2 |reference_fp32 -
    restatement_fp64|) per component over the 15 steps; the returned pose is the trace's last step bit for bit; the train-mode
    tuple has the reference's shapes."""
    g = load_golden('e2e_kitti_g2s_nn.npz')
    B = int(g['B'])
    for seed in (int(s) for s in g['seeds']):
        net, (sat, grd, K, gu, gv, gh) = _model(seed, B, precision=precision)
        with torch.no_grad():
            res = net(sat, grd, K, mode='test')
        got = net.last_trace.reshape(B, -1, 3).cpu().numpy().astype(np.float64)
        _pose_gate(got, g[f'otrace64_{seed}'], g[f'trace32_{seed}'], f'g2s nn {precision} seed {seed}')
        print(f'   |hip - reference_fp32| max {np.abs(got - g[f"trace32_{seed}"]).max():.2e}')
        np.testing.assert_array_equal(torch.stack(res, -1).cpu().numpy()[:, [1, 0, 2]], got[:, -1].astype(np.float32))
        with torch.no_grad():
            tup = net(sat, grd, K, gu, gv, gh, mode='train')
        assert len(tup) == 14
        assert [list(c.shape) for c in tup[13]] == g[f'conf_shapes_{seed}'].tolist() == [[B, 1, 32, 128], [B, 1, 128, 128], [B, 1, 256, 256]]
        ref = g[f'tuple32_{seed}']
        assert abs(float(tup[0]) - ref[0][0]) < 1e-3 * abs(ref[0][0])
        for i in range(1, 9):
            assert tuple(tup[i].shape) == (3,) and np.abs(tup[i].cpu().numpy() - ref[i]).max() < 1e-3 * max(1.0, np.abs(ref[i]).max()), i


def test_e2e_nn_bf16_pose_deviation_bounded():
    """bf16 extractor, fp32 LM loop: no golden gate can be derived, so the deviation from the fp64 restatement measured once on the
    MI355X (EXPERIMENTS.md) is the yardstick and 3x it the bound, as smoke() does for its reduced-precision modes."""
    g = load_golden('e2e_kitti_g2s_nn.npz')
    B = int(g['B'])
    worst = np.zeros(2)
    for seed in (int(s) for s in g['seeds']):
        net, (sat, grd, K, *_) = _model(seed, B, precision='bf16')
        with torch.no_grad():
            res = net(sat, grd, K, mode='test')
        got = net.last_trace.reshape(B, -1, 3).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        e = np.abs(got - g[f'otrace64_{seed}'])
        worst = np.maximum(worst, [e[..., :2].max(), e[..., 2].max()])
    print(f'g2s nn bf16: max |bf16 - restatement_fp64| shifts {worst[0]:.3e} heading {worst[1]:.3e} (normalised)')
    assert worst[0] <= NN_BF16_LIMITS[0] and worst[1] <= NN_BF16_LIMITS[1], (worst, NN_BF16_LIMITS)


def test_nn_train_step_vs_reference_autograd_golden():
    """Full KITTI shape, mode='train' with train_damping=1: the loss against the reference's recorded fp32 value, and
    loss.backward() through the HIP backward (in-plane LM backward + the folded VGG backward) against the restatement's fp64
    autograd on the recorded samples, gated like the geo direction: max(1.5e-2 * scale, 3 * |reference_fp32 - restatement_fp64|).
    The parameters without a gradient are exactly the reference's."""
    g = load_golden('e2e_kitti_g2s_nn.npz')
    seed, B = int(g['seeds'][0]), int(g['B'])
    net, (sat, grd, K, gu, gv, gh) = _model(seed, B, train_damping=1)
    net.train()
    res = net(sat, grd, K, gu, gv, gh, mode='train')
    ref_loss = g[f'tuple32_{seed}'][0][0]
    print(f'g2s nn train loss {float(res[0].detach()):.4f} (reference fp32 {ref_loss:.4f})')
    assert abs(float(res[0].detach()) - ref_loss) < 1e-3 * abs(ref_loss)
    res[0].backward()
    named = dict(net.named_parameters())
    nograd = set(str(k) for k in g['nograd_32'])
    for k, p in named.items():
        assert (p.grad is None) == (k in nograd), k
    keys = [k[len('grad32_'):] for k in g.files if k.startswith('grad32_')]
    assert len(keys) >= 9
    for k in keys:
        ref = g['grad32_' + k]
        gr = named[k].grad.double().reshape(-1).cpu()
        got = gr[sample_idx(gr.numel(), 77)].numpy()
        o64 = g['ograd64_' + k][2:]
        scale = np.abs(ref[2:]).max()
        e, e64, gap = np.abs(got - ref[2:]).max(), np.abs(got - o64).max(), np.abs(ref[2:] - o64).max()
        print(f'g2s nn train grad {k:36s} |hip-ref32| {e / scale:.2e}  |hip-restatement64| {e64 / scale:.2e}  |ref32-restatement64| '
              f'{gap / scale:.2e} (scale {scale:.2e})')
        assert e64 <= max(1.5e-2 * scale, 3 * gap), (k, e64, gap, scale)


def test_nn_standalone_vgg_g2s_is_differentiable():
    """VGGUnet_G2S under autograd on its own (HLA_VGG_BWD_FOLD_DECODER), confidence heads included, vs the fp64 restatement."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.VGG import VGGUnet_G2S
    d = _dev()
    rs = np.random.RandomState(31)
    sd = O.synth_vgg_state(rs, bias_scale=0.05)
    x = T(rs.random_sample((2, 3, 32, 96)).astype(np.float32))
    on = R.VGGUnet_G2S(4)
    on.load_state_dict(sd)
    on = on.double()
    fo, co = on(x.double())
    ws = [T(rs.standard_normal(tuple(t.shape))) for t in fo + co]
    sum((w * t).sum() for w, t in zip(ws, fo + co)).backward()
    net = VGGUnet_G2S(4)
    net.load_state_dict(sd)
    net = net.to(d).train()
    f, c = net(x.to(d))
    sum((w.float().to(d) * t).sum() for w, t in zip(ws, f + c)).backward()
    for (k, p), (_, q) in zip(net.named_parameters(), on.named_parameters()):
        e = _rel(p.grad.cpu().numpy(), q.grad.numpy())
        print(f'vgg g2s backward {k:24s} rel err {e:.2e}')
        assert e < 2e-4, (k, e)


@pytest.mark.parametrize('level', [3, 4])
def test_nn_train_step_vs_restatement_autograd_small(level):
    """LM_G2SP(proj='nn') mode='train' under autograd on a reduced shape with two samples (the full-shape fixture has one): the
    loss to 1e-4 and every parameter gradient against the fp64 restatement with the gate the issue sets for this quantity,
    max(1.5e-2 * scale, 3 * gap), gap = the restatement's own fp32-vs-fp64 difference (below 3e-4 of scale here).

    This test was first written with a flat 5e-3 bound copied from the geo direction's small train-step test and missed it on the
    MI355X: SatFeatureNet.conv2.weight 5.3e-3 (level 3), SatFeatureNet.conv_dec3.1.weight 9.1e-3 (level 4), conv0.weight 2.8e-3,
    everything from conv5 on <= 1.5e-3.  Cause, measured on the same case: the LM backward is exact at the features it is given
    (<= 4e-7 against fp64 autograd on the HIP feature maps) and d(loss)/d(feature maps) moves by only 3.7e-6 between the HIP maps
    and the fp64 ones; what differs is the 2x2 max-pool routing of near-tied texels between the fp32 extractor and the fp64
    reference in the (unchanged) satellite branch -- conv2.BIAS, which does not depend on which texel of a pool window receives
    the gradient, agrees to 1.7e-4 where conv2.WEIGHT differs by 4.5e-3.  That is the effect the 1.5e-2 term of the issue's gate
    (and of test_gpu_parity.py::test_g2s_train_step_vs_reference_autograd_golden) exists for; a flat bound without it was the
    test's mistake."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_G2SP
    d = _dev()
    args = O.default_args(proj='nn', level=level, N_iters=2, train_damping=1)
    B, grd_hw, sat_a = 2, (64, 256), 128
    sd = O.synth_model_state(4, bias_scale=0.02)
    sd['damping'] = torch.tensor([[0.1, 0.2, 0.15]])
    sat, grd, gu, gv, gh = O.synth_images(9, B, grd_hw=grd_hw, sat_a=sat_a)
    ref, loss = {}, {}
    for dt in (torch.float64, torch.float32):
        on = R.LM_G2SP_NN(args)
        on.load_state_dict(sd)
        on = on.to(dt)
        ro = on(sat.to(dt), grd.to(dt), None, gu.to(dt), gv.to(dt), gh.to(dt), mode='train')
        ro[0].backward()
        ref[dt] = {k: (None if p.grad is None else p.grad.double().numpy()) for k, p in on.named_parameters()}
        loss[dt] = float(ro[0].detach())
    net = LM_G2SP(args)
    net.load_state_dict(sd)
    net = net.to(d).train()
    K = torch.tensor([O.KITTI_K], dtype=torch.float32).repeat(B, 1, 1)
    r = net(sat.to(d), grd.to(d), K.to(d), gu.to(d), gv.to(d), gh.to(d), mode='train')
    assert len(r) == 14 and len(r[13]) == level
    assert abs(float(r[0].detach()) - loss[torch.float64]) < 1e-4 * abs(loss[torch.float64])
    r[0].backward()
    for k, p in net.named_parameters():
        r64, r32 = ref[torch.float64][k], ref[torch.float32][k]
        assert (p.grad is None) == (r64 is None), k
        if p.grad is None:
            continue
        scale = np.abs(r64).max()
        e64, gap = np.abs(p.grad.cpu().double().numpy() - r64).max(), np.abs(r32 - r64).max()
        print(f'g2s nn train grad L{level} {k:36s} |hip-restatement64| {e64 / scale:.2e}  |restatement32-64| {gap / scale:.2e} (scale {scale:.2e})')
        assert e64 <= max(1.5e-2 * scale, 3 * gap), (k, e64, gap, scale)
