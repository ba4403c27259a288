"""GPU tests of ``args.use_gt_depth`` for ``LM_S2GP`` (models_kitti.py:741-748): the per-sample point source of the fused LM kernels
(ray table x depth map, mask depth != -1) through hla_s2g_lm_solve / _bwd and the model surface, against the fp64 restatement
(tests/gt_depth_ref.py, pinned to the reference's recorded fp32 results by tests/test_gt_depth_cpu.py) and the fixture of
tools/make_golden_gt_depth.py.  The gates are those tests/test_gpu_parity.py and tests/test_polar_gpu.py apply to the same
quantities.  Without the feature ``forward`` raises NotImplementedError and ``lm_solve`` has no ``gt_depth``: every test here fails."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from make_idx import sample_idx
import gt_depth_ref as R
from test_polar_gpu import _pose_gate

pytestmark = pytest.mark.gpu

GRD_HW, SAT_A = (72, 264), 136          # level maps 9x33, 18x66, 36x132 (rows 4.., 9.., 18..); satellite maps 17, 34, 68
DEPTH_HW = (23, 77)


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.asarray(a))


def _small_depth(B, seed=21, dead_last=True):
    """[B,23,77]: per sample different, 15 % holes of -1, a handful of exact zeros (mask 1, the point at the camera) and of -0.5
    (mask 1, a point behind the camera) in the rows the loop reads; ``dead_last``: the last sample is all -1."""
    d = R.depth_map(seed, B, *DEPTH_HW).clone()
    rs = np.random.RandomState(seed + 1)
    for b in range(B):
        rows, cols = rs.randint(12, DEPTH_HW[0], size=12), rs.randint(0, DEPTH_HW[1], size=12)
        d[b, rows[:6], cols[:6]] = 0.0
        d[b, rows[6:], cols[6:]] = -0.5
    if dead_last:
        d[B - 1] = -1.0
    return d


_SMALL = {}


def _small_case(bias_args):
    """The restatement's feature maps of the reduced pyramid (made once, never written to): (sat, grd, conf) lists of NCHW fp32."""
    from oracle import ref_cpu as O
    if 'maps' not in _SMALL:
        onet = R.build(O.default_args(use_gt_depth=1), 3, torch.float64, bias_scale=0.05, grd_hw=GRD_HW)
        img_s, img_g, *_ = O.synth_images(11, 3, grd_hw=GRD_HW, sat_a=SAT_A)
        with torch.no_grad():
            sat, _ = onet.SatFeatureNet(img_s.double())
            grd, conf = onet.GrdFeatureNet(img_g.double())
        _SMALL['maps'] = tuple([t.float() for t in ts] for ts in (sat, grd, conf))
        _SMALL['sd'] = onet.state_dict()
    onet = R.LM_S2GP_Depth(bias_args, grd_hw=GRD_HW)
    onet.load_state_dict(_SMALL['sd'])
    return onet.double(), _SMALL['maps']


def _nh(t, d):
    return t.permute(0, 2, 3, 1).contiguous().to(d)


@pytest.mark.parametrize('kw', [dict(), dict(using_weight=1), dict(using_weight=1, dropout=1), dict(level_first=1),
                                dict(Optimizer='SGD')])
def test_gt_depth_lm_solve_small_vs_restatement(kw):
    """hla_s2g_lm_solve with a depth map on the reduced pyramid of test_polar_lm_solve_small_vs_restatement: B = 3, ground maps of
    9 / 18 / 36 rows by 33 / 66 / 132 columns, depth 23 x 77 (no multiple of any level), the third sample all -1: its trace must
    stay at init_pose.  The 14 normal-equation sums of the first step (2e-6 of each sum's scale) and the whole trace
    (1e-4 max(1, |ref|)) against the fp64 restatement; for {} also the in-view counts of args.strict_errors, which count the lifted
    points whatever their mask."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    d = _dev()
    kw = dict(kw)
    lf = kw.pop('level_first', 0)
    args = O.default_args(use_gt_depth=1, **{'N_iters': 3, 'damping': 1.0, **kw})
    B = 3
    onet, (sat, grd, conf) = _small_case(args)
    assert [tuple(t.shape[-2:]) for t in grd] == [(9, 33), (18, 66), (36, 132)]
    depth = _small_depth(B)
    onet.gt_depth = depth
    p0 = T(np.random.RandomState(4).uniform(-0.3, 0.3, size=(B, 3)).astype(np.float32))
    if not kw:
        args.strict_errors = 1
    net = LM_S2GP(args).to(d)
    feats = ([_nh(s, d) for s in sat], [_nh(g, d) for g in grd], [c[:, 0].contiguous().to(d) for c in conf])
    torch.manual_seed(0)
    np.random.seed(0)
    trace = net.lm_solve(*feats, GRD_HW, None, lf, init_pose=p0, keep_normal_eq=True, gt_depth=depth.to(d)).cpu().numpy()
    pose = [p0[:, i:i + 1].double() for i in range(3)]
    if args.Optimizer == 'LM':
        neq = net.last_normal_eq[0, :, :14].cpu().numpy()
        npix = (9 - 4) * 33
        keep = net.last_keep[0, :npix].cpu().bool() if args.dropout else None
        assert keep is None or int(keep.sum()) == npix // 2
        ref_neq = R.normal_eq(onet, sat, grd, conf, pose, 0, args.using_weight, keep=keep)
        e_neq = np.abs(neq - ref_neq).max(0) / np.abs(ref_neq).max(0).clip(1e-30)
        print('gt_depth normal-eq rel err per sum:', np.array2string(e_neq, precision=1))
        assert e_neq.max() < 2e-6, e_neq
        assert not neq[B - 1].any()                          # every pixel of the all -1 sample is masked
    if not kw:
        uv, _, _ = onet._pose_to_uv(0, sat[0].shape[-1], *pose, None, require_jac=False)
        lim = sat[0].shape[-1] - 1
        cnt = ((uv[..., 0] >= 0) & (uv[..., 0] <= lim) & (uv[..., 1] >= 0) & (uv[..., 1] <= lim)).reshape(B, -1).sum(1)
        np.testing.assert_array_equal(net.last_normal_eq[0, :, 14].cpu().numpy(), cnt.double().numpy())
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
    print('gt_depth lm small', kw, 'lf', lf, 'trace max err', err, 'ref range', np.abs(ref).max())
    assert np.isfinite(trace).all()
    assert err < 1e-4 * max(1.0, np.abs(ref).max()), (kw, err)
    np.testing.assert_array_equal(trace[B - 1], np.broadcast_to(p0[B - 1].numpy(), (N, L, 3)))
    # the depth map is not ignored: the same call without it gives another trace
    torch.manual_seed(0)
    np.random.seed(0)
    plain = net.lm_solve(*feats, GRD_HW, None, lf, init_pose=p0).cpu().numpy()
    assert np.abs(plain[:B - 1] - trace[:B - 1]).max() > 1e-3


def test_gt_depth_batch_index():
    """Every per-sample read of the depth map uses the global sample index: B = 16 (two stream groups, XCD-affine block map), every
    sample with its own depth map, gives bit for bit the traces of the same samples run as two batches of 8 and as 16 batches of 1."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    d = _dev()
    B = 16
    g = torch.Generator(device=d)
    g.manual_seed(77)
    sat = [torch.randn(B, SAT_A >> (3 - l), SAT_A >> (3 - l), c, device=d, generator=g) for l, c in enumerate((256, 128, 64))]
    grd = [torch.randn(B, GRD_HW[0] >> (3 - l), GRD_HW[1] >> (3 - l), c, device=d, generator=g) for l, c in enumerate((256, 128, 64))]
    depth = _small_depth(B, seed=31, dead_last=False).to(d)
    p0 = T(np.random.RandomState(4).uniform(-0.3, 0.3, size=(B, 3)).astype(np.float32))
    net = LM_S2GP(O.default_args(use_gt_depth=1, N_iters=3, damping=1.0)).to(d)

    def run(lo, hi):
        torch.manual_seed(0)
        return net.lm_solve([t[lo:hi].contiguous() for t in sat], [t[lo:hi].contiguous() for t in grd], [None] * 3, GRD_HW, None, 0,
                            init_pose=p0[lo:hi], gt_depth=depth[lo:hi]).clone()
    whole = run(0, B)
    assert torch.isfinite(whole).all() and bool((whole.abs() < 2.5).all())       # (no re-initialisation draw took part)
    assert len({whole[b].cpu().numpy().tobytes() for b in range(B)}) == B
    halves = torch.cat([run(0, 8), run(8, 16)])
    singles = torch.cat([run(b, b + 1) for b in range(B)])
    assert torch.equal(whole, halves), (whole != halves).nonzero()[:4]
    assert torch.equal(whole, singles), (whole != singles).nonzero()[:4]
    # a depth map that belongs to another sample changes the trace: the index is really read per sample
    torch.manual_seed(0)
    rolled = net.lm_solve(sat, grd, [None] * 3, GRD_HW, None, 0, init_pose=p0, gt_depth=depth.roll(1, 0))
    assert all(not torch.equal(rolled[b], whole[b]) for b in range(B))


@pytest.mark.parametrize('kw', [dict(), dict(using_weight=1)])
def test_gt_depth_lm_backward_small_vs_restatement_autograd(kw):
    """hla_s2g_lm_solve_bwd with a depth map on the case of the small forward test: d_sat, d_grd, d_conf against fp64 autograd through
    the restatement's unrolled loop, under test_lm_backward_small_vs_oracle_autograd's gate (2e-4 of the largest reference entry);
    with args.deterministic_backward two runs are bitwise equal."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    d = _dev()
    args = O.default_args(use_gt_depth=1, **{'N_iters': 3, 'damping': 1.0, **kw})
    B, L, N = 3, 3, 3
    onet, (sat, grd, conf) = _small_case(args)
    depth = _small_depth(B)
    onet.gt_depth = depth
    p0 = T(np.random.RandomState(4).uniform(-0.3, 0.3, size=(B, 3)).astype(np.float32))
    coef = T(np.random.RandomState(6).standard_normal((B, N, L, 3)))
    sat64 = [s.double().requires_grad_(True) for s in sat]
    grd64 = [g.double().requires_grad_(True) for g in grd]
    conf64 = [c.double().requires_grad_(True) for c in conf]
    su, sv, th = [p0[:, i:i + 1].double() for i in range(3)]
    torch.manual_seed(0)
    loss = 0
    for i in range(N):
        for l in range(L):
            su, sv, th = onet._step(l, sat64[l], None, grd64[l], conf64[l], su, sv, th, None)
            loss = loss + (coef[:, i, l] * torch.cat([su, sv, th], 1)).sum()
    loss.backward()
    net = LM_S2GP(args).to(d)
    feats = ([_nh(s, d) for s in sat], [_nh(g, d) for g in grd], [c[:, 0].contiguous().to(d) for c in conf])
    dd = depth.to(d)
    torch.manual_seed(0)
    trace = net.lm_solve(*feats, GRD_HW, None, 0, init_pose=p0, keep_normal_eq=True, gt_depth=dd)
    neq = net.last_normal_eq
    d_sat, d_grd, d_conf, _ = net.lm_backward(*feats, GRD_HW, trace, neq, coef.float(), None, 0, init_pose=p0, gt_depth=dd)
    for l in range(L):
        for name, got, ref in (('sat', d_sat[l], sat64[l].grad), ('grd', d_grd[l], grd64[l].grad)):
            got = got.permute(0, 3, 1, 2).cpu().double().numpy()
            e = np.abs(got - ref.numpy()).max() / max(np.abs(ref.numpy()).max(), 1e-30)
            print(f'gt_depth lm bwd {kw} level {l} d_{name}: rel err {e:.2e} (max |ref| {np.abs(ref.numpy()).max():.2e})')
            assert e < 2e-4, (kw, l, name, e)
            assert not got[B - 1].any()                      # the all -1 sample: no pixel, no gradient
        if args.using_weight:
            got = d_conf[l].cpu().double().numpy()
            ref = conf64[l].grad[:, 0].numpy()
            e = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
            print(f'gt_depth lm bwd {kw} level {l} d_conf: rel err {e:.2e}')
            assert e < 2e-4
    # without the depth map the gradients are others: the backward reads it too
    plain = net.lm_backward(*feats, GRD_HW, trace, neq, coef.float(), None, 0, init_pose=p0)
    assert not torch.equal(plain[0][2], d_sat[2])
    net.args.deterministic_backward = 1
    a = net.lm_backward(*feats, GRD_HW, trace, neq, coef.float(), None, 0, init_pose=p0, gt_depth=dd)
    b = net.lm_backward(*feats, GRD_HW, trace, neq, coef.float(), None, 0, init_pose=p0, gt_depth=dd)
    for l in range(L):
        assert torch.equal(a[0][l], b[0][l]) and torch.equal(a[1][l], b[1][l]) and bool(a[0][l].any()), l
        rel = float((a[0][l].double() - d_sat[l].double()).norm() / d_sat[l].double().norm())
        assert rel < 1e-3, (l, rel)


def _train_step(net, sat, grd, gt, depth, seed):
    net.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    res = net(sat, grd, *gt, mode='train', gt_depth=depth)
    res[0].backward()
    torch.cuda.synchronize()
    return res, {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_e2e_kitti_gt_depth_vs_golden(precision):
    """LM_S2GP(use_gt_depth=1) with the fixture's 94 x 311 depth map, full KITTI shape, B = 1: the 15-step trace of both seeds in both
    loop orders under test_polar_gpu._pose_gate; the trace differs from the flat-ground run's by more than 1e-2 (a depth map that is
    silently ignored fails); use_gt_depth=1 without a map and use_gt_depth=0 with one are the plain run bit for bit; then, seed 1
    with train_damping = 1, the train tuple and gradient samples under test_polar_train_step_gradients_vs_golden's gates."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    g = load_golden('e2e_kitti_gt_depth.npz')
    B, d = int(g['B']), _dev()
    assert tuple(g['depth_hw']) == R.DEPTH_HW
    for seed in (int(s) for s in g['seeds']):
        sat, grd, *_ = (t.to(d) for t in O.synth_images(seed + 100, B))
        depth = R.depth_map(seed + int(g['depth_seed']), B).to(d)
        net = LM_S2GP(O.default_args(use_gt_depth=1, precision=precision))
        net.load_state_dict(O.synth_model_state(seed))
        net = net.to(d)

        def run(depth, lf=0):
            torch.manual_seed(seed)
            with torch.no_grad():
                res = net(sat, grd, mode='test', gt_depth=depth, level_first=lf)
            return net.last_trace.clone(), res
        plain, _ = run(None)
        for lf, tag in ((0, ''), (1, '_lf')):
            tr, res = run(depth, lf)
            trace = tr.reshape(B, -1, 3).cpu().numpy().astype(np.float64)
            _pose_gate(trace, g[f'otrace64{tag}_{seed}'], g[f'trace32{tag}_{seed}'], f'kitti gt_depth {precision} seed {seed} lf {lf}')
            final = torch.stack(res, -1).cpu().numpy()
            np.testing.assert_allclose(final, g[f'final32{tag}_{seed}'], atol=2e-3)          # ordering check (lat, lon, theta)
            if not lf:
                moved = float((tr - plain).abs().max())
                print(f'kitti gt_depth {precision} seed {seed}: |depth - flat ground| {moved:.2e} '
                      f'(reference {np.abs(g[f"trace32_{seed}"] - g[f"plain32_{seed}"]).max():.2e})')
                assert moved > 1e-2
        net.args.use_gt_depth = 0
        assert torch.equal(run(depth)[0], plain)
        net.args.use_gt_depth = 1
    seed = int(g['seeds'][0])
    net = LM_S2GP(O.default_args(use_gt_depth=1, train_damping=1, precision=precision))
    net.load_state_dict(O.synth_model_state(seed))
    net = net.to(d).train()
    sat, grd, gu, gv, gh = (t.to(d) for t in O.synth_images(seed + 100, B))
    depth = R.depth_map(seed + int(g['depth_seed']), B).to(d)
    res, grads = _train_step(net, sat, grd, [gu, gv, gh], depth, seed)
    ref_t = g['otuple64_td']
    assert abs(float(res[0].detach()) - ref_t[0][0]) < 1e-3 * abs(ref_t[0][0])
    for i in range(1, 9):
        np.testing.assert_allclose(res[i].detach().cpu().numpy(), ref_t[i], rtol=1e-3, atol=2e-3)
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
        print(f'gt_depth train grad [{precision}] {k:36s} max err {e:.2e} (ref fp32 gap {gap:.2e}, scale {scale:.2e}); l1 {got[0]:.4e} vs {ref[0]:.4e}')
        rel_tol = 2e-4 if 'conv_dec2' in k else 5e-3
        assert e <= max(rel_tol * scale, 3 * gap), (k, e, gap, scale)
        assert abs(got[0] - ref[0]) <= max(2e-3 * ref[0], 3 * abs(g['grad32_' + k][0] - ref[0]))


def test_gt_depth_argument_errors():
    from oracle import ref_cpu as O
    from highlyaccurate_amd import _lib
    from highlyaccurate_amd.models_kitti import LM_S2GP, LM_G2SP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    d = _dev()
    B = 2
    sat, grd = torch.rand(B, 3, 128, 128, device=d), torch.rand(B, 3, 64, 256, device=d)
    depth = R.depth_map(5, B, 20, 60).to(d)
    with pytest.raises(NotImplementedError, match='polar'):
        LM_S2GP(O.default_args(use_gt_depth=1, proj='polar')).to(d)(sat, grd, mode='test', gt_depth=depth)
    net = LM_S2GP(O.default_args(use_gt_depth=1)).to(d)
    for bad in (depth[:1], depth[0], torch.cat([depth, depth])):
        with pytest.raises(ValueError, match='gt_depth'):
            net(sat, grd, mode='test', gt_depth=bad)
    with torch.no_grad():
        net(sat, grd, mode='test', gt_depth=depth.cpu().double())        # any device / dtype: taken .to(device).float()
    # the C boundary: the Ford chain and the ground -> satellite loop refuse a depth map
    g = torch.Generator(device=d)
    g.manual_seed(1)
    sf = [torch.randn(B, 16 << l, 16 << l, c, device=d, generator=g) for l, c in enumerate((256, 128, 64))]
    gf = [torch.randn(B, 8 << l, 32 << l, c, device=d, generator=g) for l, c in enumerate((256, 128, 64))]
    ford = LM_S2GP_Ford(O.default_args()).to(d)
    extra = dict(R_FL=torch.eye(3).repeat(B, 1, 1), T_FL=torch.zeros(B, 3), side_m=112.64)
    with pytest.raises(_lib.HlaError, match='ford'):
        ford.lm_solve(sf, gf, [None] * 3, (64, 256), extra, 0, gt_depth=depth)
    g2s = LM_G2SP(O.default_args()).to(d)
    K = torch.tensor(O.KITTI_K).repeat(B, 1, 1)
    cfg, lv, Kd = g2s._structs(sf, gf, [None] * 3, K.to(d), None, None)
    lv[1].depth = depth.data_ptr()
    lib = _lib.load()
    trace = torch.empty(B, g2s.N_iters, 3, 3, device=d)
    nbytes = lib.hla_g2s_workspace_bytes(C.byref(cfg), lv, B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    rc = lib.hla_g2s_lm_solve(C.byref(cfg), lv, _lib.ptr(Kd), 64, 256, None, _lib.ptr(trace), None, _lib.ptr(ws), nbytes, B, _lib.stream_ptr())
    assert rc != 0 and 'depth' in lib.hla_last_error().decode()
    # half-given depth fields are refused, not guessed at
    cfg, lv, _, _ = net._lm_structs(sf, gf, [None] * 3, (64, 256), None, 0, None, None, depth)
    lv[0].depth_row = 0
    nbytes = lib.hla_s2g_workspace_bytes(C.byref(cfg), lv, B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    rand_uv = torch.zeros(15, 2, B, device=d)
    rc = lib.hla_s2g_lm_solve(C.byref(cfg), lv, None, None, None, _lib.ptr(rand_uv), _lib.ptr(trace.new_empty(B, 5, 3, 3)), None, _lib.ptr(ws), nbytes, B,
                              _lib.stream_ptr())
    assert rc != 0 and 'depth' in lib.hla_last_error().decode()
