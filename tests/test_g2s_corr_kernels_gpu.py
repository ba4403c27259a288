"""``hla_g2s_corr`` / ``hla_g2s_corr_bwd`` / ``hla_g2s_corr_triplet_loss`` through ``_g2s_corr.corr_forward`` / ``corr_backward`` on
random arrays, against the CPU restatement (tests/g2s_corr_ref.py) in fp64.

Gate (tests/test_polar_gpu.py: _gate): max|hip - ref64| <= max(2 max|ref32 - ref64|, 8 * 2^-23 * max|ref64|), ref32 the fp32 run of
the same restatement; on corr, d_sat, d_g2s and the loss.  The small shapes run B = 3 on raw maps with inverse norms, sample 2 with
an all-zero satellite map (corr == 2 exactly, no gradient through E).  The KITTI level-2 shape (B = 1) is checked at sampled
entries by direct fp64 sums; the dense dot that beta and the projection need there comes from an fp64 FFT (checked against the
direct sums at the sampled shifts)."""
import numpy as np
import pytest
import torch

import g2s_corr_ref as GR

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
F64 = torch.float64
# (A, Hc, Wc, C)
SHAPES = [(40, 7, 9, 64), (36, 4, 5, 256), (48, 13, 16, 16), (24, 20, 17, 128), (33, 33, 33, 64)]
KITTI = (256, 153, 153, 64)
GT_U, GT_V = (0.3, -0.2, 0.1), (-0.4, 0.25, 0.0)


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _gate(got, r64, r32, what):
    got, r64, r32 = (np.asarray(a, dtype=np.float64) for a in (got, r64, r32))
    gap = np.abs(r32 - r64).max()
    err, allow = np.abs(got - r64).max(), max(2 * gap, 8 * EPS32 * np.abs(r64).max())
    print(f'{what}: max err {err:.2e}, allowed {allow:.2e}, ratio {err / allow if allow else float("inf"):.3f} '
          f'(ref fp32-fp64 gap {gap:.2e}, scale {np.abs(r64).max():.2e})')
    assert np.isfinite(got).all() and err <= allow, (what, err, allow)


def _case(shape, B, seed, zero_last=True):
    """raw NHWC fp32 maps and fp64 inverse norms."""
    A, Hc, Wc, C = shape
    g = torch.Generator().manual_seed(seed)
    sat = torch.randn(B, A, A, C, generator=g)
    g2s = torch.randn(B, Hc, Wc, C, generator=g) * 0.37
    if zero_last and B > 1:
        sat[B - 1] = 0
    sat_inv = 1.0 / sat.double().reshape(B, -1).norm(dim=1).clamp_min(1e-12)
    g2s_inv = torch.rand(B, generator=g, dtype=F64) * 0.05 + 0.01           # the ground map's inverse norm: any positive scale
    d_corr = torch.randn(B, A - Hc + 1, A - Wc + 1, generator=g)
    return sat, g2s, sat_inv, g2s_inv, d_corr


def _ranges(shape):
    """(lat, lon, mpp) that keep the ground-truth indices of GT_U / GT_V inside the plane."""
    A, Hc, Wc, _ = shape
    mpp = GR.level_mpp(2)
    return mpp * 0.9 * ((A - Hc) // 2), mpp * 0.9 * ((A - Wc) // 2), mpp


_REF = {}


def _reference(shape):
    """(dt -> dict(corr, loss, d_sat, d_g2s, d_sat_rand, d_g2s_rand)) for fp64 and fp32, made once per shape.  The gradients are
    w.r.t. the normalised satellite map s and the scaled crop f; NHWC."""
    if shape in _REF:
        return _REF[shape]
    sat, g2s, sat_inv, g2s_inv, d_corr = _case(shape, 3, 11)
    lat, lon, mpp = _ranges(shape)
    gu, gv = torch.tensor(GT_U), torch.tensor(GT_V)
    out = {}
    for dt in (F64, torch.float32):
        res = {}
        for which in ('loss', 'rand'):
            s = (sat.to(dt) * sat_inv.to(dt).view(-1, 1, 1, 1)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            f = (g2s.to(dt) * g2s_inv.to(dt).view(-1, 1, 1, 1)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            corr = GR.corr_from_crop(s, f, True)[0]
            res['corr'] = corr.detach()
            if which == 'loss':
                if corr.shape[1] * corr.shape[2] == 1:
                    continue                                  # one shift: the loss divides by zero, in the reference too
                loss = GR.triplet_level(corr, gu, gv, lat, lon, mpp)
                res['loss'] = float(loss.detach())
                loss.backward()
            else:
                (corr * d_corr.to(dt)).sum().backward()
            res['d_sat_' + which] = s.grad.permute(0, 2, 3, 1).contiguous()
            res['d_g2s_' + which] = f.grad.permute(0, 2, 3, 1).contiguous()
        out[dt] = res
    _REF[shape] = out
    return out


def _run(shape, B=3, seed=11, sel=None):
    from highlyaccurate_amd import _g2s_corr as G
    d = _dev()
    sat, g2s, sat_inv, g2s_inv, d_corr = (t.to(d) for t in _case(shape, 3, seed))
    if sel is not None:
        sat, g2s, sat_inv, g2s_inv, d_corr = (t[sel:sel + 1].contiguous() for t in (sat, g2s, sat_inv, g2s_inv, d_corr))
    corr, saved = G.corr_forward(sat, g2s, sat_inv, g2s_inv)
    d_sat, d_g2s = G.corr_backward(sat, g2s, sat_inv, g2s_inv, saved, d_corr)
    return (sat, g2s, sat_inv, g2s_inv, d_corr), corr, saved, d_sat, d_g2s


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_backward_and_loss_against_fp64(shape):
    from highlyaccurate_amd import _g2s_corr as G
    from types import SimpleNamespace
    ref = _reference(shape)
    r64, r32 = ref[F64], ref[torch.float32]
    (sat, g2s, sat_inv, g2s_inv, d_corr), corr, saved, d_sat, d_g2s = _run(shape)
    A, Hc, Wc, C = shape
    assert tuple(corr.shape) == (3, A - Hc + 1, A - Wc + 1) and corr.dtype == torch.float32
    per = lambda got, key, what: [_gate(got[b].cpu(), r64[key][b], r32[key][b], f'{what} {shape} sample {b}') for b in range(3)]
    per(corr, 'corr', 'corr')                                  # per sample: the zero map's gradient (D = 1e-6) dwarfs the others
    assert (corr[2] == 2).all()                                # the all-zero satellite map
    per(d_sat, 'd_sat_rand', 'd_sat')
    per(d_g2s, 'd_g2s_rand', 'd_g2s')
    assert (d_g2s[2] == 0).all()                               # s = 0: d_g and the projection vanish (d_sat does not: d dot / d s = g)
    if 'loss' not in r64:
        return
    lat, lon, mpp = _ranges(shape)
    args = SimpleNamespace(shift_range_lat=lat, shift_range_lon=lon)
    gu, gv = torch.tensor(GT_U, device=corr.device), torch.tensor(GT_V, device=corr.device)
    loss = torch.full((1,), float('nan'), device=corr.device)
    G.triplet_loss(corr, gu, gv, args, mpp, loss, False)
    _gate(loss.cpu(), [r64['loss']], [r32['loss']], f'loss {shape}')
    G.triplet_loss(corr, gu, gv, args, mpp, loss, True)
    assert abs(float(loss) - 2 * r64['loss']) < 1e-5 * abs(r64['loss'])        # accumulate adds
    dc = G.triplet_loss_bwd(corr, gu, gv, args, mpp, torch.ones(1, device=corr.device))
    ds, dg = G.corr_backward(sat, g2s, sat_inv, g2s_inv, saved, dc)
    per(ds, 'd_sat_loss', 'd_sat through the loss')
    per(dg, 'd_g2s_loss', 'd_g2s through the loss')


@pytest.mark.parametrize('shape', SHAPES[:3])
def test_bitwise_repeat_batch_independence_and_sentinels(shape):
    from highlyaccurate_amd import _g2s_corr as G
    (sat, g2s, sat_inv, g2s_inv, d_corr), corr, saved, d_sat, d_g2s = _run(shape)
    _, corr2, saved2, d_sat2, d_g2s2 = _run(shape)
    assert torch.equal(corr, corr2) and torch.equal(d_sat, d_sat2) and torch.equal(d_g2s, d_g2s2)
    assert all(torch.equal(a, b) for a, b in zip(saved, saved2))
    _, c1, s1, ds1, dg1 = _run(shape, sel=1)
    assert torch.equal(c1[0], corr[1]) and torch.equal(s1[0][0], saved[0][1]) and torch.equal(s1[1][0], saved[1][1])
    assert torch.equal(ds1[0], d_sat[1]) and torch.equal(dg1[0], d_g2s[1])
    # outputs handed over as NaN come back fully written and finite
    nan = lambda t: torch.full_like(t, float('nan'))
    out = (nan(saved[0]), nan(saved[1]), nan(saved[2]), nan(corr))
    c3, sv3 = G.corr_forward(sat, g2s, sat_inv, g2s_inv, out=out)
    assert all(torch.isfinite(t).all() for t in out) and torch.equal(c3, corr)
    ds3, dg3 = G.corr_backward(sat, g2s, sat_inv, g2s_inv, sv3, d_corr, out=(nan(d_sat), nan(d_g2s)))
    assert torch.equal(ds3, d_sat) and torch.equal(dg3, d_g2s)


def test_refusals_return_errors():
    from highlyaccurate_amd import _g2s_corr as G, _lib
    d = _dev()
    sat, g2s, sat_inv, g2s_inv, _ = (t.to(d) for t in _case((24, 20, 17, 128), 3, 5))
    need = _lib.load().hla_g2s_corr_workspace_bytes(3, 24, 20, 17, 128)
    assert need > 0
    with pytest.raises(_lib.HlaError, match='workspace'):
        G.corr_forward(sat, g2s, sat_inv, g2s_inv, workspace_bytes=need - 1)
    with pytest.raises(_lib.HlaError, match='channel'):
        G.corr_forward(sat[..., :32].contiguous(), g2s[..., :32].contiguous(), sat_inv, g2s_inv)
    with pytest.raises(_lib.HlaError, match='crop'):
        G.corr_forward(sat, torch.zeros(3, 25, 17, 128, device=d), sat_inv, g2s_inv)
    G.corr_forward(sat, g2s, sat_inv, g2s_inv)                 # and the library still works afterwards
    torch.cuda.synchronize()


def test_kitti_level2_shape_at_sampled_entries():
    """A = 256, crop 153 x 153, C = 64, B = 1: 104 x 104 shifts, 4 x 4 tiles of which the last row and column are partial, 14 K
    splits, 184 row steps (three flushes) per tile."""
    A, Hc, Wc, C = KITTI
    Ny, Nx = A - Hc + 1, A - Wc + 1
    g = torch.Generator().manual_seed(21)
    sat = torch.randn(1, A, A, C, generator=g)
    g2s = torch.randn(1, Hc, Wc, C, generator=g) * 0.37
    sat_inv = 1.0 / sat.double().reshape(1, -1).norm(dim=1)
    g2s_inv = torch.tensor([0.03], dtype=F64)
    d_corr = torch.randn(1, Ny, Nx, generator=g)
    from highlyaccurate_amd import _g2s_corr as G
    d = _dev()
    args_d = [t.to(d) for t in (sat, g2s, sat_inv, g2s_inv)]
    corr, saved = G.corr_forward(*args_d)
    d_sat, d_g2s = G.corr_backward(*args_d, saved, d_corr.to(d))
    corr2, saved2 = G.corr_forward(*args_d)
    d_sat2, d_g2s2 = G.corr_backward(*args_d, saved2, d_corr.to(d))
    assert torch.equal(corr, corr2) and torch.equal(d_sat, d_sat2) and torch.equal(d_g2s, d_g2s2)
    corr, d_sat, d_g2s = corr[0].cpu().numpy(), d_sat[0].cpu().numpy(), d_g2s[0].cpu().numpy()
    assert np.isfinite(corr).all() and np.isfinite(d_sat).all() and np.isfinite(d_g2s).all()

    rng = np.random.default_rng(4)
    am = int(corr.argmin())
    shifts = [(0, 0), (0, Nx - 1), (Ny - 1, 0), (Ny - 1, Nx - 1), (am // Nx, am % Nx)] + \
             [(int(a), int(b)) for a, b in zip(rng.integers(0, Ny, 11), rng.integers(0, Nx, 11))]

    def at_dtype(dt):
        s = (sat[0].numpy().astype(dt) * dt(float(sat_inv[0]))).astype(dt)
        f = (g2s[0].numpy().astype(dt) * dt(float(g2s_inv[0]))).astype(dt)
        n = dt(max(np.sqrt((f * f).sum(dtype=dt)), 1e-12))
        return s, f, (f / n).astype(dt), n

    s64, f64, g64, n64 = at_dtype(np.float64)
    s32, f32, g32, n32 = at_dtype(np.float32)
    # dense fp64 E (summed-area table) and dot (FFT); the dot is checked against the direct sums below
    e = (s64 * s64).sum(-1)
    sat_tab = np.zeros((A + 1, A + 1))
    sat_tab[1:, 1:] = e.cumsum(0).cumsum(1)
    E = sat_tab[Hc:, Wc:] - sat_tab[:Ny, Wc:] - sat_tab[Hc:, :Nx] + sat_tab[:Ny, :Nx]
    gp = np.zeros((A, A, C))
    gp[:Hc, :Wc] = g64
    dot = np.fft.irfft2(np.fft.rfft2(s64, axes=(0, 1)) * np.conj(np.fft.rfft2(gp, axes=(0, 1))), s=(A, A), axes=(0, 1)).sum(-1)[:Ny, :Nx]

    c64, c32 = [], []
    for dy, dx in shifts:
        d_, e_ = GR.dot_at(s64, g64, dy, dx)
        assert abs(d_ - dot[dy, dx]) < 1e-12 and abs(e_ - E[dy, dx]) < 1e-12
        c64.append(2 - 2 * d_ / max(np.sqrt(e_), 1e-6))
        win = s32[dy:dy + Hc, dx:dx + Wc]
        d3, e3 = (win * g32).sum(dtype=np.float32), (win * win).sum(dtype=np.float32)
        c32.append(np.float32(2) - np.float32(2) * d3 / max(np.sqrt(e3), np.float32(1e-6)))
    _gate([corr[dy, dx] for dy, dx in shifts], c64, c32, 'corr KITTI level 2 (16 shifts)')

    dc = d_corr[0].numpy().astype(np.float64)
    D = np.maximum(np.sqrt(E), 1e-6)
    ddot = -2 * dc / D
    beta = np.where(np.sqrt(E) > 1e-6, dc * dot / D ** 3, 0.0)
    kappa = (ddot * dot).sum()
    ddot32, beta32, kappa32 = ddot.astype(np.float32), beta.astype(np.float32), np.float32(kappa)
    want64, want32, got = [], [], []
    for r, x, c in zip(rng.integers(0, A, 32), rng.integers(0, A, 32), rng.integers(0, C, 32)):
        r, x, c = int(r), int(x), int(c)
        box = (slice(max(0, r - Hc + 1), min(Ny - 1, r) + 1), slice(max(0, x - Wc + 1), min(Nx - 1, x) + 1))
        want64.append(GR.d_sat_conv_at(g64, ddot, r, x, c) + 2 * s64[r, x, c] * beta[box].sum())
        want32.append(np.float32(GR.d_sat_conv_at(g32, ddot32, r, x, c)) + np.float32(2) * s32[r, x, c] * beta32[box].sum(dtype=np.float32))
        got.append(d_sat[r, x, c])
    _gate(got, want64, want32, 'd_sat KITTI level 2 (32 elements)')
    want64, want32, got = [], [], []
    for y, x, c in zip(rng.integers(0, Hc, 32), rng.integers(0, Wc, 32), rng.integers(0, C, 32)):
        y, x, c = int(y), int(x), int(c)
        want64.append((GR.d_g_at(s64, ddot, y, x, c) - g64[y, x, c] * kappa) / n64)
        want32.append((np.float32(GR.d_g_at(s32, ddot32, y, x, c)) - g32[y, x, c] * kappa32) / n32)
        got.append(d_g2s[y, x, c])
    _gate(got, want64, want32, 'd_g2s KITTI level 2 (32 elements)')


def test_triplet_index_rule_half_to_even_wrap_and_nan():
    """The index rule of hla_g2s_corr_triplet_loss against the restatement's (tests/test_g2s_corr_ref_cpu.py pins that one): ties
    round to even, a negative index counts from the end, an index outside the plane gives NaN; the backward's cotangent sums to
    zero over the shifts and matches autograd."""
    from highlyaccurate_amd import _g2s_corr as G
    from types import SimpleNamespace
    d = _dev()
    g = torch.Generator().manual_seed(2)
    corr = torch.rand(2, 9, 8, generator=g) * 0.2 + 1.9
    args, mpp = SimpleNamespace(shift_range_lat=1.0, shift_range_lon=1.0), 0.5
    loss = torch.empty(1, device=d)
    for gu, gv, ok in (((0.0, 0.25), (0.0, -0.5), True), ((0.75, -2.5), (0.0, 3.0), True), ((-6.0, 0.0), (0.0, 0.0), True),
                       ((0.0, -6.5), (0.0, 0.0), False), ((2.0, 0.0), (0.0, 0.0), False), ((0.0, 0.0), (0.0, -2.5), False)):
        tu, tv = torch.tensor(gu).view(2, 1), torch.tensor(gv).view(2, 1)
        c64 = corr.double().requires_grad_(True)
        want = GR.triplet_level(c64, tu, tv, 1.0, 1.0, mpp)
        G.triplet_loss(corr.to(d), tu.to(d)[:, 0], tv.to(d)[:, 0], args, mpp, loss, False)
        if not ok:
            assert torch.isnan(want) and torch.isnan(loss).all(), (gu, gv)
            continue
        assert abs(float(loss) - float(want)) < 8 * EPS32 * abs(float(want)), (gu, gv, float(loss), float(want))
        want.backward()
        dc = G.triplet_loss_bwd(corr.to(d), tu.to(d)[:, 0], tv.to(d)[:, 0], args, mpp, torch.ones(1, device=d)).cpu().double()
        assert (dc - c64.grad).abs().max() < 8 * EPS32 * c64.grad.abs().max(), (gu, gv)
        assert dc.sum(dim=(1, 2)).abs().max() < 1e-6
