"""The bf16 / fp16 VGG backward, launch by launch, against the fp64 restatement of ``vgg_bwd16_ref.py``.

One training forward, one backward into a workspace pre-filled with 0xFF bytes (NaN in bf16, fp16 and fp32: a read of a region
the pass never wrote shows up in a gradient), then every launch of ``vgg_backward_t<T>`` is restated on the CPU from the
operands THAT launch read on the GPU -- the saved forward workspace, the raw maps and the gradient maps in the backward
workspace -- and compared: stored 16-bit maps element by element (exact, except within the accumulation band of a rounding
midpoint: ``vgg_bwd16_ref.check_map``), fp32 weight / bias gradients by max |gpu - ref64| / S against 4 x the CPU's own
fp32-accumulating restatement (``check_sum``).  Shapes: those of ``test_vgg_kernels_vs_fp64.py``.
"""

import pytest
import torch

import vgg_round16 as R16
import vgg_bwd16_ref as BR

pytestmark = pytest.mark.gpu

_FWD = {}
_CASE_IDS = [(n, lv) for n, (_, _, _, lvs) in BR.CASES.items() for lv in lvs]


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _forward(shape, level, precision, window=False, sparse=False, names=None):
    """One training forward on the GPU and everything the restatement reads from it, on the CPU (once per key)."""
    key = (shape, level, precision, window, sparse)
    f = _FWD.get(key)
    if f is None:
        from highlyaccurate_amd.VGG import VGGUnet, vgg_forward_nhwc
        d, dt = _dev(), R16.DTYPES[precision]
        B, H, W = shape
        sd, x, ups, cups, pad = BR.case_inputs(shape, level)
        if sparse:      # the bottom-right quarter of every map (at least one pixel), nothing at the confidence maps
            for u in ups:
                h, w = u.shape[2], u.shape[3]
                m = torch.zeros_like(u, dtype=torch.bool)
                m[:, :, h - max(h // 4, 1):, w - max(w // 4, 1):] = True
                u[~m] = 0
        net = VGGUnet(level, precision=precision)
        net.load_state_dict(sd)
        net = net.to(d)
        if window:      # the same image as a row window of a taller one: the x_plane path of _image_window (not copied)
            big = torch.rand(B, 3, H + 24, W)
            big[:, :, 16:16 + H] = x
            xd = big.to(d)[:, :, 16:16 + H]
            assert not xd.is_contiguous()
        else:
            xd = x.to(d)
        feats, confs, inv, ctx = vgg_forward_nhwc(net, xd, want_conf=True, defer_norm=True, save_for_backward=True)
        if window:
            assert ctx['x_plane'] == (H + 24) * W, ctx['x_plane']
        d_feats, d_confs = BR.upstream(ups, cups, pad, dt)
        f = dict(sd=sd, x=x, net=net, ctx=ctx, confs_d=confs, dt=dt, level=level, shape=shape, d_feats=d_feats, d_confs=d_confs,
                 dfe=[t.permute(0, 2, 3, 1).contiguous().float().to(d) for t in d_feats],
                 dcs=[t.contiguous().float().to(d) for t in d_confs],
                 fw=BR.read_forward(ctx['ws'].cpu(), B, H, W, level, dt, names),
                 raws=[t.permute(0, 3, 1, 2).cpu() for t in feats], confs=[c.cpu() for c in confs], inv=inv.cpu())
        _FWD[key] = f
    return f


def _backward(f, tp, conf=True, names=None, **kw):
    """One backward into a 0xFF-filled workspace: (gradients on the CPU in fp64, maps, raw int16 maps)."""
    from highlyaccurate_amd import _lib
    from highlyaccurate_amd.VGG import vgg_backward_nhwc
    B, H, W = f['shape']
    nbytes = _lib.load().hla_vgg_bwd_workspace_bytes(B, H, W, f['level'], _lib.HLA_BF16 if f['dt'] == torch.bfloat16 else _lib.HLA_F16)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=_dev())
    grads = vgg_backward_nhwc(f['net'], f['ctx'], f['dfe'], f['confs_d'] if conf else None, f['dcs'] if conf else None,
                              wgrad_two_phase=tp, workspace=ws, **kw)
    grads = {k: g.detach().double().cpu() for k, g in grads.items()}
    maps, raws = BR.read_backward(ws.cpu(), B, H, W, f['level'], f['dt'], names)
    return grads, maps, raws


def _walks(f, maps, conf=True, **kw):
    """The fp64 restatement of every launch on the GPU's operands, and the fp32-accumulating one of the fp32 outputs."""
    a = (f['sd'], f['x'], f['fw'], f['raws'], f['inv'], f['d_feats'], f['confs'] if conf else None, f['d_confs'] if conf else None,
         f['level'], f['dt'])
    with torch.no_grad():
        rec64, wg64 = BR.walk(*a, torch.float64, forced=maps, **kw)
        _, wg32 = BR.walk(*a, torch.float32, forced=maps, want_S=False, dgrads=False, **kw)
    return rec64, wg64, wg32


def _report(tag, table):
    for name, mg, mc in table:
        print(f'TABLE {tag} | {name} | {mg:.3e} | {mc:.3e}')


def _same_maps(tag, raws_a, raws_b, skip=('g_a0',)):
    """Two backward calls that differ in their weight-gradient kernels leave bit-identical gradient maps."""
    for k in raws_a:
        if k not in skip:
            assert torch.equal(raws_a[k], raws_b[k]), (tag, k, 'the stored maps of the two calls differ')


def test_workspace_argument_is_checked():
    from highlyaccurate_amd.VGG import vgg_backward_nhwc
    f = _forward(BR.CASES['tiny'][:3], 3, 'bf16')
    with pytest.raises(ValueError):
        vgg_backward_nhwc(f['net'], f['ctx'], f['dfe'], workspace=torch.empty(1024, dtype=torch.uint8, device=_dev()))
    g_own, _, _ = _backward(f, 0)
    g_def = vgg_backward_nhwc(f['net'], f['ctx'], f['dfe'], f['confs_d'], f['dcs'])
    for k, g in g_def.items():
        assert torch.equal(g.double().cpu(), g_own[k]), k       # the caller's workspace changes no bit of the result


@pytest.mark.parametrize('case,level', _CASE_IDS, ids=[f'{n}-L{lv}' for n, lv in _CASE_IDS])
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_backward_per_launch(case, level, precision):
    """Every launch with confidence gradients, two-pass L2 backward: the stored maps (conv2's data gradient included: the
    two-phase call keeps it) and every gradient of both weight-gradient kernel sets -- the wave-specialised ones with the fused
    conv0 gradient (0) and the two-phase ones with the stored-map conv0 kernel (1) -- from the SAME stored maps."""
    shape = BR.CASES[case][:3]
    f = _forward(shape, level, precision)
    tag = f'per-launch {precision} {case} {shape} L{level}'
    g1, maps, raws = _backward(f, 1)
    g0, _, raws0 = _backward(f, 0)
    _same_maps(tag, raws, raws0, skip=('g_a0',) if level == 3 else ())
    rec64, wg64, wg32 = _walks(f, maps)
    fails, table = BR.check_run(tag + ' two-phase', maps, g1, rec64, wg64, wg32, f['sd'], level, f['dt'], raws)
    _report(tag + ' two-phase', table)
    fails0, table0 = BR.check_run(tag + ' ws', maps, g0, {}, wg64, wg32, f['sd'], level, f['dt'])
    _report(tag + ' ws', table0)
    assert not fails + fails0, fails + fails0


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_backward_without_confidence_gradients(precision):
    """odd_pooled, level 3, no head gradients: the L2-norm backward's outputs are checked on their own; wave-specialised
    weight gradients with the fused (0) and with the stored-map conv0 gradient (bit 1)."""
    shape = BR.CASES['odd_pooled'][:3]
    f = _forward(shape, 3, precision)
    tag = f'noconf {precision} {shape} L3'
    g2, maps, raws = _backward(f, 2, conf=False)
    g0, _, raws0 = _backward(f, 0, conf=False)
    _same_maps(tag, raws, raws0)
    rec64, wg64, wg32 = _walks(f, maps, conf=False)
    fails, table = BR.check_run(tag + ' conv0-unfused', maps, g2, rec64, wg64, wg32, f['sd'], 3, f['dt'], raws)
    _report(tag + ' conv0-unfused', table)
    fails0, table0 = BR.check_run(tag + ' fused', maps, g0, {}, wg64, wg32, f['sd'], 3, f['dt'])
    _report(tag + ' fused', table0)
    assert not fails + fails0, fails + fails0


# vgg_backward_t's first rows for first_row8 = 4 with confidence heads (vgg_backward.hip:644-663), restated by hand:
# n_x21 = 4 * 4 - 1, n_d2a = 14, rb_up18 = even(13) = 12 -> n_x18 = 6, n_x3p = 13, n_d1a = 5, rb_up15 = even(4) = 4 -> n_x15 = 2,
# n_x8p = 4, n_a12 = 2 * 2 - 1 = 3, n_a10 = 2, n_x8 = 1, n_a5 = 2 * 1 - 1 = 1, n_x3 = 0, n_a0 = 0.  First written row per map:
_TRIM_ROWS = {'g_x21': 15, 'l2_18': 6, 'l2_15': 2, 'g_d2a': 14, 'g_x18': 6, 'g_x3p': 13, 'g_d1a': 5, 'g_x15': 2, 'g_x8p': 4,
              'g_a12': 3, 'g_a10': 2, 'g_x8': 1, 'g_a5': 1, 'g_x3': 0, 'g_a0': 0}


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_backward_row_trimming(precision):
    """odd_pooled, level 3, ``scale_invariant=True, dense=True, first_row8=4`` with confidence heads: odd first rows through
    the upsample shift.  Every map starts at its restated first row and still holds the 0xFF fill above it."""
    shape = BR.CASES['odd_pooled'][:3]
    f = _forward(shape, 3, precision)
    tag = f'trimmed {precision} {shape} L3'
    kw = dict(scale_invariant=True, first_row8=4)
    g1, maps, raws = _backward(f, 1, dense=True, **kw)
    g0, _, raws0 = _backward(f, 0, dense=True, **kw)
    _same_maps(tag, raws, raws0)
    rec64, wg64, wg32 = _walks(f, maps, **kw)
    assert {k: r['row_begin'] for k, r in rec64.items()} == _TRIM_ROWS
    fails, table = BR.check_run(tag + ' two-phase', maps, g1, rec64, wg64, wg32, f['sd'], 3, f['dt'], raws)
    _report(tag + ' two-phase', table)
    fails0, table0 = BR.check_run(tag + ' ws', maps, g0, {}, wg64, wg32, f['sd'], 3, f['dt'])
    _report(tag + ' ws', table0)
    assert not fails + fails0, fails + fails0


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_backward_dynamic_trimming(precision):
    """odd_pooled, level 3, an upstream gradient on a corner block only with ``scale_invariant=True``: the launches visit their
    live tiles only.  A map may be left unwritten only where its restatement is exactly zero; the launches read those parts
    as zero (the restatement does), so no NaN of the fill reaches a gradient; and the short lists are really taken."""
    shape = BR.CASES['odd_pooled'][:3]
    f = _forward(shape, 3, precision, sparse=True)
    tag = f'dynamic {precision} {shape} L3'
    stats = {}
    g1, maps, raws = _backward(f, 1, conf=False, scale_invariant=True, stats=stats)
    assert 0 < stats['live_tiles'] < stats['total_tiles'], (tag, stats)
    g0, _, raws0 = _backward(f, 0, conf=False, scale_invariant=True)
    _same_maps(tag, raws, raws0)
    rec64, wg64, wg32 = _walks(f, maps, conf=False, scale_invariant=True, dynamic=True)
    fails, table = BR.check_run(tag + ' two-phase', maps, g1, rec64, wg64, wg32, f['sd'], 3, f['dt'], dynamic=True)
    _report(tag + ' two-phase', table)
    fails0, table0 = BR.check_run(tag + ' ws', maps, g0, {}, wg64, wg32, f['sd'], 3, f['dt'])
    _report(tag + ' ws', table0)
    print(f'{tag}: live tiles {stats["live_tiles"]} of {stats["total_tiles"]}')
    assert not fails + fails0, fails + fails0


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_backward_image_row_window(precision):
    """The input as a row window of a taller image (``x_plane``): conv0's weight and bias gradient, both routes."""
    shape = BR.CASES['odd_pooled'][:3]
    f = _forward(shape, 3, precision, window=True)
    tag = f'window {precision} {shape} L3'
    g1, maps, _ = _backward(f, 1)
    g0, _, _ = _backward(f, 0)
    _, wg64, wg32 = _walks(f, maps, only=(0,))
    fails = []
    for route, g in (('stored-map', g1), ('fused', g0)):
        fl, table = BR.check_run(f'{tag} {route}', maps, g, {}, wg64, wg32, f['sd'], 3, f['dt'])
        _report(f'{tag} {route}', table)
        fails += fl
    assert not fails, fails


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_backward_many_tiles(precision):
    """(4, 264, 296), level 3, both weight-gradient kernel sets: every k-split workgroup loops over several tiles.  Checked:
    the weight and bias gradients of conv2 (full resolution, g_unpool, KS 256 / 512), conv12 (256 x 256, KS 16 / 32) and
    conv_dec2.1 (two sources with the upsample, KS 85 / 170), from the stored maps they read."""
    shape = BR.MANY_TILES
    f = _forward(shape, 3, precision, names=('a0', 'idx3', 'a10', 'x18r', 'x3'))
    tag = f'many-tiles {precision} {shape} L3'
    names = ('g_x3', 'g_a12', 'g_d2a')
    fails = []
    wg64 = wg32 = None
    for tp in (1, 0):
        g, maps, _ = _backward(f, tp, names=names)
        if wg64 is None:
            _, wg64, wg32 = _walks(f, maps, only=(1, 5, 9))
        fl, table = BR.check_run(f'{tag} tp{tp}', maps, g, {}, wg64, wg32, f['sd'], 3, f['dt'])
        _report(f'{tag} tp{tp}', table)
        fails += fl
    assert not fails, fails


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_backward_free_running_attribution(precision):
    """odd_batch, level 3: the GPU's final gradients against the FREE-RUNNING fp64 emulation of the 16-bit backward started
    from the GPU's saved forward, under ``vgg_round16.gate``; and the deviation of the GPU from the exact (unrounded) backward
    on the same saved forward is at most twice the emulation's: the 16-bit backward's deviation is its own rounding.  (The
    heads' weight gradients have no 16-bit rounding in the backward -- fp32 dz, fp32 sums over the stored activation -- so their
    emulation IS the exact backward, 0 against 2e-6 .. 2e-7 of fp32 noise on the GPU: for them the ratio says nothing and the
    gate against the emulation stands alone.)"""
    shape = BR.CASES['odd_batch'][:3]
    f = _forward(shape, 3, precision)
    tag = f'free-running {precision} {shape} L3'
    g, _, _ = _backward(f, 0)
    saved = (f['fw'], f['raws'], f['confs'], f['inv'])
    with torch.no_grad():
        e64, e32, ex = (BR.backward(f['sd'], f['x'], f['d_feats'], f['d_confs'], 3, dt, acc, saved=saved)[0]
                        for dt, acc in ((f['dt'], torch.float64), (f['dt'], torch.float32), (None, torch.float64)))
    assert set(g) == set(e64), sorted(set(g) ^ set(e64))
    bad = []
    for k in sorted(g):
        gt = R16.gate(e64[k], e32[k], ex[k])
        l2, mx = R16.rel_l2(g[k], e64[k]), R16.max_rel(g[k], e64[k])
        emu, gpu = R16.rel_l2(e64[k], ex[k]), R16.rel_l2(g[k], ex[k])
        print(f"TABLE {tag} | {k} | emulation vs exact {emu:.3e} | gpu vs exact {gpu:.3e} | gpu vs emulation relL2 {l2:.3e} "
              f"(gate {gt['l2']:.3e}) max-rel {mx:.3e} (gate {gt['max']:.3e}) [{gt['regime']}]")
        if not (l2 <= gt['l2'] and mx <= gt['max'] and (gpu <= 2 * emu or (emu == 0 and k.startswith('conf')))):
            bad.append((k, l2, gt['l2'], mx, gt['max'], gpu, emu))
    assert not bad, (tag, bad)
