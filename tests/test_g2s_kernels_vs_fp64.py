"""The ground -> satellite LM kernels (csrc/lm_g2s.hip: g2s_accum, g2s_ip_accum, g2s_solve, g2s_bwd_accum in its geo, weighted
and in-plane instantiations, g2s_bwd_solve) against the fp64 one-step reference of tests/g2s_geo_ref.py (tests/g2s_nn_ref.py for
the in-plane warp), through ``LM_G2SP.lm_solve`` / ``lm_backward`` with hand-made levels: fewer pixels than a tile, ragged last
tiles of 4 and 36 pixels, 67 tiles per sample (the strided closing loops), B = 8 / 9 (the XCD-affine block map with idle blocks),
intrinsics of every sample its own (skew entries, a perturbed third row, an image size the maps do not divide), pixels 2^-10 px
inside and outside each border of the ground map, an in-bounds pixel behind the camera, a sample with nothing in view, deferred
norms.  tests/test_g2s_geo_ref_cpu.py asserts those properties of the inputs on the reference alone.

Gates (those of test_lm_kernels_vs_fp64.py and of this direction's model-level tests; none measured on these kernels):
  sums       |hip - ref64| <= 2e-6 * T_k, T_k = the reference's fp64 sum of the absolute values of sum k's terms
  pose       |hip - ref64| <= max((5e-6, 5e-6, 5.7e-4), 2 |ref32 - ref64|) componentwise, one step from the kernel's own starting pose
  gradients  max|hip - ref64| / max|ref64| < 2e-4 per tensor (d_sat, d_grd, d_conf of every level)
  d_damping  |hip - ref64| <= max(1e-5 max|ref64|, 2 |ref32 - ref64|) componentwise (see TOL_LAM)
  exact      a sample with nothing in view, batch and slot independence, repeats, the pixel behind the camera
Measured errors: EXPERIMENTS.md, "G2S LM kernels against fp64 at tile and map borders"."""
import numpy as np
import pytest
import torch

import g2s_geo_ref as R
import g2s_nn_ref as NN
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
TOL_SUM, TOL_GRAD = 2e-6, 2e-4
# d_damping: 1e-5 of max|ref64|, the gate of test_g2s_lm_backward_small_vs_oracle_autograd, holds for B = 2 or 3 on small maps and
# cannot hold in general: d(loss)/d(lambda_p) = -sum over samples and steps of y_p d_p with d = (H + lambda)^-1 (U - V), where
# both the difference U - V of two sums of thousands of terms and the sum over samples and steps cancel (B = 9: per-sample
# heading terms of +-0.04 add up to -0.003; A = 130 in-plane: the reference run in fp32 is itself 1.3e-3 away from fp64).  Where
# the plain gate is missed the bound therefore comes from the reference side, in the form the pose gate has: twice the distance
# between the same reference run in fp32 and in fp64.  (max(a, b) evaluated lazily: the fp32 autograd pass runs only when a alone
# does not hold.  On the MI355X two cases need it: behind w1 1.9e-5 with ref32 at 5.3e-5, nn130 1.4e-5 with ref32 at 1.35e-3.)
TOL_LAM = 1e-5
TOL_POSE = np.array([5e-6, 5e-6, 5.7e-4])            # test_gpu_parity.py: shifts, heading
# d_grd and d_conf are sums of fp32 atomics whose order differs from launch to launch: n addends of one sign reorder to within
# n * 2^-24 of their sum; the busiest texel of these cases receives fewer than 2^9 pixels x 4 taps, and cancellation is bounded by
# the tensor's largest entry, so two launches of the same work differ by less than 2^11 * 2^-24 = 1.2e-4 of it.  (Used only
# where bitwise equality holds for everything else; the gradient gate above applies to each launch on its own.)
TOL_ATOMIC_ORDER = 2.0 ** -13


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


_NETS = {}


def _net(ranges, N, uw, proj):
    from highlyaccurate_amd.models_kitti import LM_G2SP
    key = (ranges, N, uw, proj)
    if key not in _NETS:
        net = LM_G2SP(R.make_args(ranges, N_iters=N, using_weight=uw, proj=proj)).to(_dev())
        with torch.no_grad():
            net.damping.copy_(R.lam_of(F32))
        _NETS[key] = net
    return _NETS[key]


class _Run:
    """One case on the GPU: lm_solve, then lm_backward on its trace."""

    def __init__(self, c, uw, proj='geo'):
        d = _dev()
        self.c, self.geo = c, proj == 'geo'
        self.net = _net(c.ranges, c.N, uw, proj)
        nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(d)
        sat, grd = R.raw_maps(c)
        conf = [x[:, 0].contiguous().to(d) for x in c.conf] if self.geo else [None] * len(sat)
        self.feats = ([nh(s) for s in sat], [nh(g) for g in grd], conf)
        self.K = c.K.to(d) if self.geo else None
        self.hw = c.ori_hw if self.geo else None
        self.inv = dict(sat_inv_norm=c.sat_inv.to(d), grd_inv_norm=c.grd_inv.to(d)) if hasattr(c, 'sat_inv') else {}

    def forward(self):
        """-> trace [B,N,L,3] fp32, normal_eq [steps,B,16] fp64 (CPU)."""
        self.trace = self.net.lm_solve(*self.feats, self.K, self.hw, init_pose=self.c.p0, keep_normal_eq=True, **self.inv)
        self.neq = self.net.last_normal_eq
        torch.cuda.synchronize()
        return self.trace.cpu(), self.neq.cpu()

    def backward(self, coef):
        """-> d_sat[l], d_grd[l] (NCHW), d_conf[l] ([B,h,w]) or None, d_damping [3]; CPU, fp32 values."""
        out = self.net.lm_backward(*self.feats, self.K, self.hw, self.trace, self.neq, coef.float().to(_dev()), init_pose=self.c.p0,
                                   **self.inv)
        torch.cuda.synchronize()
        nc = lambda t: t.permute(0, 3, 1, 2).cpu()
        return [nc(t) for t in out[0]], [nc(t) for t in out[1]], [None if t is None else t.cpu() for t in out[2]], out[3].cpu()


# ----------------------------------------------------------------------------------------------------------------------
# gates
# ----------------------------------------------------------------------------------------------------------------------
def _gate_sums(tag, got, sums, mags):
    got, sums, mags = np.asarray(got, np.float64), sums.numpy(), mags.numpy()
    assert np.isfinite(got).all(), (tag, got)
    err = np.abs(got - sums)
    ratio = (err / np.where(mags > 0, mags, 1.0)).max()
    print(f'G2SK sums {tag}: worst |hip - ref64| / T_k = {ratio:.2e} (limit {TOL_SUM:.0e})')
    assert (err <= TOL_SUM * mags).all(), (tag, (err / np.where(mags > 0, mags, 1.0)).max(0))


def _gate_pose(tag, got, p64, p32):
    got = np.asarray(got, np.float64)
    p64, p32 = (torch.cat(p, 1).double().numpy() for p in (p64, p32))
    allow = np.maximum(TOL_POSE, 2 * np.abs(p32 - p64))
    err = np.abs(got - p64)
    print(f'G2SK pose {tag}: max |hip - ref64| = {err.max():.2e}, ref32 gap {np.abs(p32 - p64).max():.2e}, worst ratio {(err / allow).max():.3f}')
    assert np.isfinite(got).all() and (err <= allow).all(), (tag, err, allow)


def _gate_damping(tag, got, ref64, ref32):
    """``ref32``: a function that returns d_damping of the reference run in fp32."""
    got, ref64 = got.double().reshape(3).numpy(), ref64.detach().double().reshape(3).numpy()
    scale = np.abs(ref64).max()
    assert scale > 0 and np.isfinite(got).all(), tag
    err = np.abs(got - ref64)
    print(f'G2SK grad {tag} d_damping: max|hip - ref64| / max|ref64| = {err.max() / scale:.2e} (limit {TOL_LAM:.0e})')
    if (err < TOL_LAM * scale).all():
        return
    gap = np.abs(ref32().detach().double().reshape(3).numpy() - ref64)
    allow = np.maximum(TOL_LAM * scale, 2 * gap)
    print(f'G2SK grad {tag} d_damping: ref32 gap / max|ref64| = {gap.max() / scale:.2e}, worst |hip - ref64| / allowed = {(err / allow).max():.3f}')
    assert (err <= allow).all(), (tag, err, allow)


def _gate_grad(tag, got, ref, limit=TOL_GRAD):
    got, ref = got.double().numpy(), ref.detach().double().numpy()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    scale = np.abs(ref).max()
    assert scale > 0 and np.isfinite(got).all(), tag
    e = np.abs(got - ref).max() / scale
    print(f'G2SK grad {tag}: max|hip - ref64| / max|ref64| = {e:.2e} (limit {limit:.0e})')
    assert e < limit, (tag, e)


# ----------------------------------------------------------------------------------------------------------------------
# the geo kernels
# ----------------------------------------------------------------------------------------------------------------------
def _check_forward(c, uw):
    """Every step of the first iteration, each from the pose the kernel itself left in the trace."""
    run = _Run(c, uw)
    trace, neq = run.forward()
    assert bool((neq[:, :, :2] == 1.0).all()) and bool(torch.isfinite(trace).all())
    args = R.make_args(c.ranges)
    maps = {dt: R.cast(c, dt) for dt in (F64, F32)}
    prev = R.start_pose(c)
    for l, (A, Cn, hw) in enumerate(c.levels):
        tag = f'{c.name} w{uw} step {l} (A{A} C{Cn} {hw})'
        p = R.pixel_classes(args, *R.cols(prev), c.K, A, hw, c.ori_hw)
        assert float(p.min_dist.min()) > R.GUARD, (tag, 'ill-conditioned at the pose the kernel left', p.min_dist)
        new = {}
        for dt in (F64, F32):
            sat, grd, conf = maps[dt]
            with torch.no_grad():
                new[dt] = R.step(args, R.lam_of(dt), R.cols(prev, dt), grd[l], conf[l], sat[l], c.K, c.ori_hw, uw)
        sat, grd, conf = maps[F64]
        sums, mags = R.normal_sums(args, *R.cols(prev), grd[l], conf[l], sat[l], c.K, c.ori_hw, uw)
        _gate_sums(tag, neq[l, :, 2:14], sums, mags)
        _gate_pose(tag, trace[:, 0, l], new[F64], new[F32])
        prev = trace[:, 0, l]
    return run, trace, neq


def _check_backward(c, uw):
    run = _Run(c, uw)
    trace, neq = run.forward()
    coef = R.coef_of(c)
    sat, grd, conf, lam, tr = R.reference_grads(c, uw, coef)
    print(f'G2SK trace {c.name} w{uw}: max |hip - ref64| over {c.N} x {len(c.levels)} steps {float((trace.double() - tr).abs().max()):.2e}')
    out = run.backward(coef)
    d_sat, d_grd, d_conf, d_lam = out
    for l in range(len(c.levels)):
        tag = f'{c.name} w{uw} L{l}'
        _gate_grad(tag + ' d_sat', d_sat[l], sat[l].grad)
        _gate_grad(tag + ' d_grd', d_grd[l], grd[l].grad)
        if uw:
            _gate_grad(tag + ' d_conf', d_conf[l], conf[l].grad[:, 0])
        else:
            assert d_conf[l] is None and conf[l].grad is None
    _gate_damping(f'{c.name} w{uw}', d_lam, lam.grad, lambda: R.reference_grads(c, uw, coef, F32)[3].grad)
    return run, coef, (trace, neq), out, (sat, grd, conf)


@pytest.mark.parametrize('uw', [0, 1])
@pytest.mark.parametrize('A,Cn', [s[:2] for s in R.SHAPES])
def test_forward_every_tile_shape_and_width(A, Cn, uw):
    """A = 7 (49 px, under one tile), 18 (last tile 4 px), 70 (128-px tiles, last 36), 130 (256-px tiles, 67 of them, last 4);
    C = 64 / 128 / 256; B = 2 with different intrinsics, from a random pose."""
    _check_forward(R.get('shape', A, Cn), uw)


@pytest.mark.parametrize('uw', [0, 1])
def test_forward_pixels_at_every_border(uw):
    """B = 8 at pose 0 (pose0 None): sample i has pixels 2^-10 px inside / outside border side i."""
    _check_forward(R.get('border'), uw)


@pytest.mark.parametrize('uw', [0, 1])
@pytest.mark.parametrize('name', ['octet8', 'octet9', 'deferred', 'deep', 'mid', 'out', 'behind'])
def test_forward_two_levels_teacher_forced(name, uw):
    _check_forward(R.get(name), uw)


@pytest.mark.parametrize('uw', [0, 1])
@pytest.mark.parametrize('name', ['octet8', 'octet9', 'deferred', 'deep', 'mid', 'border'])
def test_backward_two_iterations(name, uw):
    """2 iterations x 2 levels (border: one step at pose 0): ragged tiles, under one tile, 67 tiles closed by the strided loop of
    g2s_bwd_solve, B = 8 / 9, deferred norms (gradients w.r.t. the normalised maps), pose0 None and random."""
    _check_backward(R.get(name), uw)


@pytest.mark.parametrize('uw', [0, 1])
@pytest.mark.parametrize('A,Cn', [(7, 128), (18, 256), (70, 64), (70, 256), (130, 128)])
def test_backward_one_step_other_widths(A, Cn, uw):
    """The (tile shape, width) pairs the two-level cases do not hold."""
    _check_backward(R.get('shape', A, Cn), uw)


@pytest.mark.parametrize('uw', [0, 1])
def test_sample_with_nothing_in_view_is_exact(uw):
    """H = 0 exactly (what _g2sp.py relies on when it raises the reference's errors): sums 2..13 zero, pose bitwise unchanged over
    all steps, zero gradients, and its batch mates bitwise what they are without it."""
    c = R.get('out')
    run, coef, (trace, neq), (d_sat, d_grd, d_conf, d_lam), ref = _check_backward(c, uw)
    o = c.out
    assert not bool(neq[:, o, 2:14].any()) and bool((neq[:, o, :2] == 1.0).all())
    assert torch.equal(trace[o], torch.zeros_like(trace[o])) and not bool(torch.signbit(trace[o]).any())
    for l in range(len(c.levels)):
        assert not bool(d_sat[l][o].any()) and not bool(d_grd[l][o].any()) and not bool(ref[0][l].grad[o].any())
        assert not uw or not bool(d_conf[l][o].any())
    sel = [b for b in range(c.B) if b != o]
    c2 = R.take(c, sel)
    run2 = _Run(c2, uw)
    trace2, neq2 = run2.forward()
    assert torch.equal(trace2, trace[sel]) and torch.equal(neq2[:, :, :14], neq[:, sel, :14])
    coef2 = coef[sel]
    d_sat2, d_grd2, d_conf2, d_lam2 = run2.backward(coef2)
    for l in range(len(c.levels)):
        assert torch.equal(d_sat2[l], d_sat[l][sel]), l


@pytest.mark.parametrize('uw', [0, 1])
def test_slot_and_batch_independence_and_repeats(uw):
    """Sample 4 of the B = 9 batch: its trace, normal equations and d_sat are bitwise those of the same sample alone (B = 1) and in
    the last slot of a permuted B = 9 batch (another XCD, the second octet); a repeat of the whole call gives bitwise the same
    trace, normal equations and d_sat (d_grd / d_conf come from fp32 atomics)."""
    c = R.get('octet9')
    coef = R.coef_of(c)
    run = _Run(c, uw)
    trace, neq = run.forward()
    d_sat = run.backward(coef)[0]
    trace_b, neq_b = run.forward()
    d_sat_b = run.backward(coef)[0]
    assert torch.equal(trace, trace_b) and torch.equal(neq[:, :, :14], neq_b[:, :, :14])
    assert all(torch.equal(a, b) for a, b in zip(d_sat, d_sat_b)) and bool(d_sat[0].any())
    for idx in ([4], [8, 7, 6, 5, 0, 3, 2, 1, 4]):
        r2 = _Run(R.take(c, idx), uw)
        t2, n2 = r2.forward()
        s = idx.index(4)
        assert torch.equal(t2[s], trace[4]) and torch.equal(n2[:, s, :14], neq[:, 4, :14]), idx
        d2 = r2.backward(coef[idx])[0]
        for l in range(len(c.levels)):
            assert torch.equal(d2[l][s], d_sat[l][4]), (idx, l)


@pytest.mark.parametrize('uw', [0, 1])
def test_pixel_behind_the_camera_in_bounds_contributes_nothing(uw):
    """Sample 1's centre pixel is sampled (u = 0 exactly, v inside) with z <= 1e-6 at every step of both levels.  The gradient gates
    hold (the fp64 autograd reference gives it no Jacobian), and nothing depends on that satellite pixel's features: with them
    changed, trace, sums and d_sat are bitwise the same and d_grd / d_conf agree to the order of their atomics."""
    c = R.get('behind')
    run, coef, (trace, neq), (d_sat, d_grd, d_conf, d_lam), ref = _check_backward(c, uw)
    b = c.behind
    c2 = R.take(c, list(range(c.B)), 'behind, centre pixel changed')
    c2.sat = [t.clone() for t in c2.sat]
    for l, (A, _, _) in enumerate(c.levels):
        c2.sat[l][b, :, A // 2, A // 2] += 0.05
        assert not bool(d_sat[l][b, :, A // 2, A // 2].any())
    run2 = _Run(c2, uw)
    trace2, neq2 = run2.forward()
    assert torch.equal(trace2, trace) and torch.equal(neq2[:, :, :14], neq[:, :, :14])
    d_sat2, d_grd2, d_conf2, d_lam2 = run2.backward(coef)
    for l in range(len(c.levels)):
        assert torch.equal(d_sat2[l], d_sat[l]), l
        for a, a2 in ((d_grd[l], d_grd2[l]),) + (((d_conf[l], d_conf2[l]),) if uw else ()):
            assert float((a - a2).abs().max()) <= TOL_ATOMIC_ORDER * float(a.abs().max()), l
    assert float((d_lam - d_lam2).abs().max()) <= 1e-12 * float(d_lam.abs().max())


# ----------------------------------------------------------------------------------------------------------------------
# the in-plane kernels (proj = 'nn'): B = 9, and 67 tiles at C = 16
# ----------------------------------------------------------------------------------------------------------------------
NN_RANGES = (20.0, 20.0, 30.0)
NN_CASES = dict(nn9=dict(B=9, levels=[(18, 16, (18, 18)), (27, 64, (25, 30))]),
                nn130=dict(B=2, levels=[(130, 16, (130, 130)), (18, 64, (20, 17))]))
_NN = {}


def _nn_case(name):
    if name not in _NN:
        kw = NN_CASES[name]
        rs = np.random.RandomState(R._seed('nn', name))
        _NN[name] = R._case(name, kw['levels'], kw['B'], torch.zeros(kw['B'], 3, 3), 2, R._rand_pose(rs, kw['B'], 0.6), ranges=NN_RANGES)
    return _NN[name]


def _nn_args(c):
    return R.make_args(c.ranges, proj='nn', N_iters=c.N)


def _nn_sums(args, pose, grd, sat):
    uv, jac = NN.inplane_pose_to_uv(args, sat.shape[-1], *pose)
    f, J = O.grid_sample(grd, uv, torch.stack(jac, 0))
    return R.sums_of(f, None, J, sat)


@pytest.mark.parametrize('name', ['nn9', 'nn130'])
def test_inplane_forward_teacher_forced(name):
    c = _nn_case(name)
    args = _nn_args(c)
    run = _Run(c, 0, 'nn')
    trace, neq = run.forward()
    assert bool((neq[:, :, :2] == 1.0).all())
    prev = c.p0
    for l, (A, Cn, hw) in enumerate(c.levels):
        tag = f'{name} step {l} (A{A} C{Cn} {hw})'
        new = {}
        for dt in (F64, F32):
            with torch.no_grad():
                new[dt] = NN.lm_step(args, R.lam_of(dt), *R.cols(prev, dt), c.grd[l].to(dt), c.sat[l].to(dt))
        sums, mags = _nn_sums(args, R.cols(prev), c.grd[l].double(), c.sat[l].double())
        pinned = NN.normal_sums(args, *R.cols(prev), c.grd[l].double(), c.sat[l].double())         # the restatement's own sums
        assert float(((sums - pinned).abs() / mags).max()) < 1e-12
        _gate_sums(tag, neq[l, :, 2:14], sums, mags)
        _gate_pose(tag, trace[:, 0, l], new[F64], new[F32])
        prev = trace[:, 0, l]
    if name == 'nn9':       # sample 4 alone and in the last slot of the permuted batch: bitwise
        for idx in ([4], [8, 7, 6, 5, 0, 3, 2, 1, 4]):
            t2, n2 = _Run(R.take(c, idx), 0, 'nn').forward()
            assert torch.equal(t2[idx.index(4)], trace[4]) and torch.equal(n2[:, idx.index(4), :14], neq[:, 4, :14]), idx


@pytest.mark.parametrize('name', ['nn9', 'nn130'])
def test_inplane_backward_two_iterations(name):
    c = _nn_case(name)
    args = _nn_args(c)
    run = _Run(c, 0, 'nn')
    trace, _ = run.forward()
    coef = R.coef_of(c)

    def reference(dt):
        lam = R.lam_of(dt).requires_grad_(True)
        sat = [t.to(dt).requires_grad_(True) for t in c.sat]
        grd = [t.to(dt).requires_grad_(True) for t in c.grd]
        tr = NN.solve(args, lam, sat, grd, c.N, c.p0.to(dt))
        (coef.to(dt) * tr).sum().backward()
        return lam, sat, grd, tr

    lam, sat, grd, tr = reference(F64)
    print(f'G2SK trace {name}: max |hip - ref64| {float((trace.double() - tr.detach()).abs().max()):.2e}')
    d_sat, d_grd, d_conf, d_lam = run.backward(coef)
    for l in range(len(c.levels)):
        _gate_grad(f'{name} L{l} d_sat', d_sat[l], sat[l].grad)
        _gate_grad(f'{name} L{l} d_grd', d_grd[l], grd[l].grad)
    _gate_damping(name, d_lam, lam.grad, lambda: reference(F32)[0].grad)
