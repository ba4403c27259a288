"""The VGG kernels against fp64 references at the shapes where tiled kernels go wrong, in every arithmetic mode.

Shapes (B, H, W) -- H and W multiples of 8 -- and the edge each one hits:
  * (1, 8, 8): every resolution is below one 8 x 32 conv tile and one 4 x 32 weight-gradient tile
  * (3, 40, 72): odd pooled sizes (5 x 9 at H/8); W is not a multiple of 32 at any level
  * (2, 264, 40): tall and thin, many row tiles (33 conv row tiles at full resolution)
  * (1, 16, 296): wide, a 9.25-tile row at full resolution
  * (5, 88, 104): odd batch
  * (4, 264, 296), level 3, fp32 / fp16x3: every weight-gradient launch has more tiles than k-split workgroups (below)

fp32 / fp16x3 run forward and backward against fp64 (the oracle and its autograd); bf16 / fp16 run the forward against
``vgg_round16.forward`` -- the same fp64 arithmetic with the kernels' 16-bit rounding points -- see ``test_forward_16bit``;
here their backward is only checked for agreement between its two weight-gradient groupings
(``test_backward_16bit_wgrad_groupings_agree``): what it computes is checked launch by launch against fp64 in
``test_vgg_backward_16bit_vs_fp64.py`` (``vgg_bwd16_ref.py``).
The references of a case are computed once per session and shared by every precision (``_REFS``).
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
import vgg_decisions as D
import vgg_round16 as R16

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5          # fp32-class forward: max|hip - ref64| / max|ref64|, maps and confidence maps (test_vgg_small_vs_golden)
BWD_TOL = 2e-4          # fp32-class backward: max-rel of every parameter gradient against fp64 autograd
# Knife-edges.  A ReLU input |z|, or the gap between a 2x2 pool window's two largest values, below TAU x the sample's largest
# |value| of that map is within the forward error of the kernels (fp32-class modes: 1e-5 of a map's max at most, the forward
# gate), so they may decide it either way -- and a moved decision moves a gradient (one flipped ReLU at conv10's output in 'tall'
# costs conv10.weight 1.2e-2 max-rel).  The backward references take the kernels' side of exactly those decisions, read from
# the forward workspace the backward consumes (``_kernel_decisions``); every other decision must agree with fp64.
TAU = 1e-5
# The ref32 rule may excuse a tensor only while the fp32 reference (same decisions, fp32 arithmetic) is close to fp64.  Measured
# on the CPU: the largest relL2(ref32, ref64) of any tensor over all cases is 3.2e-6.  1e-4 is 30x above that and 1000x below
# the ~0.1 relative L2 that the cosine > 0.995 gate of fuzz_e2e.py admits.
REF32_L2_MAX = 1e-4

# (B, H, W, levels)
CASES = {
    'tiny': (1, 8, 8, (3, 4)),
    'odd_pooled': (3, 40, 72, (3, 4)),
    'tall': (2, 264, 40, (3,)),
    'wide': (1, 16, 296, (4,)),
    'odd_batch': (5, 88, 104, (3,)),
}
MANY_TILES = (4, 264, 296)
CASE_IDS = [(name, lv) for name, (_, _, _, lvs) in CASES.items() for lv in lvs]

_REFS = {}


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _rell2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _inputs(shape, level):
    B, H, W = shape
    rs = np.random.RandomState(7919 * H + 31 * W + 3 * B + level)
    sd = O.synth_vgg_state(rs, bias_scale=0.05)
    x = torch.from_numpy(rs.random_sample((B, 3, H, W)).astype(np.float32))
    return rs, sd, x


def _autograd(r, level, dtype, dec):
    """Parameter gradients of the case's upstream functional through ``vgg_decisions.forward`` with the decisions ``dec``."""
    onet = O.VGGUnet(level)
    onet.load_state_dict(r['sd'])
    onet = onet.to(dtype)
    feats, confs = D.forward(onet, r['x'].to(dtype), dec)
    loss = sum((u.to(dtype) * f).sum() for u, f in zip(r['ups'], feats))
    if r['cups'] is not None:
        loss = loss + sum((u.to(dtype) * c).sum() for u, c in zip(r['cups'], confs))
    loss.backward()
    return {k: p.grad.double().numpy() for k, p in onet.named_parameters() if p.grad is not None}


def _ref(shape, level, sixteen=False, sparse=False):
    """fp64 forward of one case, its ReLU / pool decisions and their knife-edges, the upstream gradient (a random linear
    functional of the normalised maps plus the confidence maps), and with ``sixteen`` the emulated bf16 / fp16 forwards in
    fp64 and fp32 accumulation.  ``sparse``: the upstream gradient is a corner block of the normalised maps only (no
    confidence term).  Gradients: ``_reference_grads``."""
    key = (shape, level, sparse)
    r = _REFS.get(key)
    if r is None:
        rs, sd, x = _inputs(shape, level)
        B, H, W = shape
        shapes = [(B, c, H >> (3 - l), W >> (3 - l)) for l, c in enumerate((256, 128, 64, 16)[:level])]
        ups = [torch.from_numpy(rs.standard_normal(s)) for s in shapes]
        cups = [torch.from_numpy(rs.standard_normal((s[0], 1, s[2], s[3]))) * 30.0 for s in shapes]
        if sparse:
            # the bottom-right quarter of every map (at least one pixel), nothing at the confidence maps; within the block
            # the fp64 map's own direction is projected out per sample -- HLA_VGG_BWD_SCALE_INVARIANT drops the L2 norm's
            # (x . dy) term, which is exact only for an upstream gradient orthogonal to the map (include/hla.h)
            onet = O.VGGUnet(level)
            onet.load_state_dict(sd)
            with torch.no_grad():
                feats = onet.double()(x.double())[0]
            for u, f in zip(ups, feats):
                h, w = u.shape[2], u.shape[3]
                m = torch.zeros_like(u, dtype=torch.bool)
                m[:, :, h - max(h // 4, 1):, w - max(w // 4, 1):] = True
                u[~m] = 0
                fb = torch.where(m, f, torch.zeros_like(f))
                a = (u * fb).sum((1, 2, 3), keepdim=True) / (fb * fb).sum((1, 2, 3), keepdim=True).clamp_min(1e-300)
                u -= a * fb
            cups = None
        onet = O.VGGUnet(level)
        onet.load_state_dict(sd)
        rec = {}
        with torch.no_grad():
            f64, c64 = D.forward(onet.double(), x.double(), record=rec)
        pad = rs.standard_normal((B, H, W, 48)).astype(np.float32) if level == 4 else None
        r = dict(sd=sd, x=x, ups=ups, cups=cups, pad=pad, f64=[f.numpy() for f in f64], c64=[c.numpy() for c in c64],
                 dec64={k: m for k, (m, _) in rec.items()}, edge={k: margin < TAU for k, (_, margin) in rec.items()}, grads={})
        _REFS[key] = r
    if sixteen and 'emu' not in r:
        r['emu'] = {}
        with torch.no_grad():
            for prec, dt in R16.DTYPES.items():
                r['emu'][prec] = {acc: [t.double().numpy() for t in sum(R16.forward(r['sd'], r['x'], level, dt, acc)[:2], [])]
                                  for acc in (torch.float64, torch.float32)}
    return r


def _net(sd, level, precision):
    from highlyaccurate_amd.VGG import VGGUnet
    net = VGGUnet(level, precision=precision)
    net.load_state_dict(sd)
    return net.to(_dev())


def _nhwc(u, d, pad=None):
    t = u.permute(0, 2, 3, 1).contiguous().float().to(d)
    if pad is not None:         # level 4: x24 is stored with 64 channels; the padded ones get (seeded) noise, to be ignored
        t = torch.cat([t, torch.from_numpy(pad).to(d)], -1).contiguous()
    return t


def _check_forward_fp32_class(tag, feats, confs, r):
    worst = (0.0, '')
    for l, (f, f64) in enumerate(zip(feats, r['f64'])):
        e = _maxrel(f, f64)
        ec = _maxrel(confs[l], r['c64'][l])
        worst = max(worst, (e, f'feat{l}'), (ec, f'conf{l}'))
        assert e <= FWD_TOL and ec <= FWD_TOL, (tag, l, e, ec)
    print(f'{tag}: forward worst max-rel {worst[0]:.2e} ({worst[1]}), gate {FWD_TOL:.0e}')


def _plan(B, H, W, level4):
    """Byte offsets of the training forward's workspace for the fp32-class modes (4-byte activations): ``vgg_plan`` of
    highlyaccurate_amd/csrc/vgg_layers.h, restated.  Its total is checked against hla_vgg_workspace_bytes."""
    p, o, es, P = {}, 0, 4, B * H * W

    def take(name, nbytes):
        nonlocal o
        p[name] = o
        o += -(-nbytes // 256) * 256
    for name, n in (('x3', P // 4 * 64), ('a5', P // 4 * 128), ('x8', P // 16 * 128), ('a10', P // 16 * 256),
                    ('a12', P // 16 * 256), ('x15r', P // 64 * 256), ('d1a', P // 16 * 128), ('x18r', P // 16 * 128),
                    ('d2a', P // 4 * 64), ('x21r', P // 4 * 64)):
        take(name, n * es)
    tiles = lambda h, w: ((h + 7) // 8) * ((w + 31) // 32)
    for i, n in enumerate((tiles(H // 4, W // 4) * 2, tiles(H // 4, W // 4), tiles(H // 2, W // 2), tiles(H, W))):
        take(f'ss{i}', B * n * 8)
    take('inv', 4 * B * 8)
    take('amax', 16 * B * 4)
    if level4:
        for name in ('x2r', 'd3a', 'x24r'):
            take(name, P * 64 * es)
    take('a0', P * 64 * es)
    take('idx3', P // 4 * 64)
    take('idx8', P // 16 * 128)
    take('idx15', P // 64 * 256)
    return p, o


# decision point -> (workspace map, resolution divisor, stored channels, real channels)
_RELU_MAPS = {'a0': ('a0', 1, 64, 64), 'x3': ('x3', 2, 64, 64), 'a5': ('a5', 2, 128, 128), 'x8': ('x8', 4, 128, 128),
              'a10': ('a10', 4, 256, 256), 'a12': ('a12', 4, 256, 256), 'x15r': ('x15r', 8, 256, 256),
              'd1a': ('d1a', 4, 128, 128), 'x18r': ('x18r', 4, 128, 128), 'd2a': ('d2a', 2, 64, 64),
              'x21r': ('x21r', 2, 64, 64), 'x2r': ('x2r', 1, 64, 64), 'd3a': ('d3a', 1, 64, 32), 'x24r': ('x24r', 1, 64, 16)}
_POOL_MAPS = {'x3': ('idx3', 2, 64), 'x8': ('idx8', 4, 128), 'x15': ('idx15', 8, 256)}


def _kernel_decisions(ctx, level):
    """The decisions the backward kernels act on, read from the training forward's workspace: a ReLU passes where the stored
    activation is > 0 (the data-gradient epilogues' mask), a pool routes to the stored argmax byte (2 * row + col)."""
    ws = ctx['ws']
    B, _, H, W = ctx['x'].shape
    p, total = _plan(B, H, W, level == 4)
    assert ws.numel() == total, ('workspace layout', ws.numel(), total)
    dec = {}
    for name, (m, div, C, creal) in _RELU_MAPS.items():
        if name in D.RELUS4 and level != 4:
            continue
        h, w = H // div, W // div
        t = ws[p[m]:p[m] + B * h * w * C * 4].view(torch.float32).view(B, h, w, C)[..., :creal]
        dec['relu', name] = (t > 0).permute(0, 3, 1, 2).cpu()
    for name, (m, div, C) in _POOL_MAPS.items():
        h, w = H // div, W // div
        dec['pool', name] = ws[p[m]:p[m] + B * h * w * C].view(B, h, w, C).permute(0, 3, 1, 2).long().cpu()
    return dec


def _reference_grads(tag, r, level, kdec):
    """fp64 and fp32 gradients with the kernels' decisions at the knife-edges and fp64's everywhere else.  A kernel decision
    that differs from fp64's where the margin is not a knife-edge fails the case (a forward mask / argmax bug)."""
    dec, moved = {}, []
    for k, m64 in r['dec64'].items():
        g, edge = kdec[k], r['edge'][k]
        assert g.shape == m64.shape, (tag, k, g.shape, m64.shape)
        bad = (g != m64) & ~edge
        assert not bad.any(), (tag, 'kernel decision off fp64 beyond a knife-edge', k, int(bad.sum()),
                               torch.nonzero(bad)[:4].tolist())
        flip = (g != m64) & edge
        if flip.any():
            moved.append((k, tuple(map(tuple, torch.nonzero(flip).tolist()))))
        dec[k] = torch.where(edge, g, m64)
    key = tuple(moved)
    if key not in r['grads']:
        r['grads'][key] = (_autograd(r, level, torch.float64, dec), _autograd(r, level, torch.float32, dec))
    n_edge = sum(int(e.sum()) for e in r['edge'].values())
    print(f'{tag}: {n_edge} knife-edge decision(s) below {TAU:.0e}, {sum(len(m[1]) for m in moved)} taken the other way '
          f'by the kernels: {[m[0] for m in moved]}')
    return r['grads'][key]


def _check_backward(tag, grads, r, g64, g32):
    assert set(grads) == set(g64), (tag, sorted(set(grads) ^ set(g64)))
    r32 = {k: _rell2(g32[k], g64[k]) for k in g64}
    k32 = max(r32, key=r32.get)
    assert r32[k32] <= REF32_L2_MAX, (tag, 'the fp32 reference is too far from fp64 for the ref32 rule to mean anything', k32, r32[k32])
    worst, excused, failed = (0.0, ''), [], []
    for k, g in grads.items():
        g = g.detach().cpu().double().numpy()
        assert g.shape == g64[k].shape, (tag, k)
        e = _maxrel(g, g64[k])
        worst = max(worst, (e, k))
        if e <= BWD_TOL:
            continue
        l2, l2_32, e32 = _rell2(g, g64[k]), r32[k], _maxrel(g32[k], g64[k])
        ok = l2 <= 3 * l2_32 and e <= 3 * e32
        print(f'{tag}: {k} max-rel {e:.2e} (ref32 {e32:.2e}), relL2 {l2:.2e} (ref32 {l2_32:.2e}) -> {"ref32 rule" if ok else "FAIL"}')
        (excused if ok else failed).append((k, e, l2))
    print(f'{tag}: backward worst max-rel {worst[0]:.2e} ({worst[1]}), gate {BWD_TOL:.0e}; ref32 relL2 max {r32[k32]:.2e} ({k32}); '
          f'{len(excused)} tensor(s) via the ref32 rule')
    assert not failed, (tag, failed)


def _run_backward(tag, r, level, precision, d, wgrad_two_phase=0, window=False, **kw):
    """Training forward + backward on the GPU; returns the forward's maps, the gradients and the fp64 / fp32 reference
    gradients for the decisions this forward took (``_reference_grads``)."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc, vgg_backward_nhwc
    net = _net(r['sd'], level, precision)
    x = r['x']
    if window:      # the same image as a row window of a taller one: the x_plane path of _image_window (not copied)
        B, _, H, W = x.shape
        big = torch.rand(B, 3, H + 24, W)
        big[:, :, 16:16 + H] = x
        xd = big.to(d)[:, :, 16:16 + H]
        assert not xd.is_contiguous()
    else:
        xd = x.to(d)
    feats, confs, inv, ctx = vgg_forward_nhwc(net, xd, want_conf=True, defer_norm=True, save_for_backward=True)
    if window:
        assert ctx['x_plane'] == (H + 24) * W, ctx['x_plane']
    B = x.shape[0]
    normed = [(f[..., :16] if l == 3 else f).double() * inv[l].view(B, 1, 1, 1) for l, f in enumerate(feats)]
    fwd = ([n.permute(0, 3, 1, 2).cpu().numpy() for n in normed], [c.unsqueeze(1).double().cpu().numpy() for c in confs])
    g64, g32 = _reference_grads(tag, r, level, _kernel_decisions(ctx, level))
    dfe = [_nhwc(u, d, r['pad'] if l == 3 else None) for l, u in enumerate(r['ups'])]
    if r['cups'] is None:
        grads = vgg_backward_nhwc(net, ctx, dfe, wgrad_two_phase=wgrad_two_phase, **kw)
    else:
        grads = vgg_backward_nhwc(net, ctx, dfe, confs, [u[:, 0].contiguous().float().to(d) for u in r['cups']],
                                  wgrad_two_phase=wgrad_two_phase, **kw)
    return fwd, grads, g64, g32


FP32_CLASS = [('fp32', 0), ('fp16x3', 0), ('fp16x3', 1), ('fp16x3', 2)]
_P32_IDS = ['fp32', 'fp16x3', 'fp16x3-twophase', 'fp16x3-conv0unfused']


@pytest.mark.parametrize('case,level', CASE_IDS, ids=[f'{n}-L{lv}' for n, lv in CASE_IDS])
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_forward_fp32_class(case, level, precision):
    """Inference forward (in-kernel normalisation) of the fp32-class modes: every map and confidence map to 1e-5 of the
    fp64 oracle's.  Max-pool / ReLU flips barely move forward values, so there is no excuse path."""
    B, H, W, _ = CASES[case]
    r = _ref((B, H, W), level)
    d = _dev()
    net = _net(r['sd'], level, precision)
    with torch.no_grad():
        feats, confs = net(r['x'].to(d))
    _check_forward_fp32_class(f'fwd {precision} {case} {(B, H, W)} L{level}', [f.double().cpu().numpy() for f in feats],
                              [c.double().cpu().numpy() for c in confs], r)


@pytest.mark.parametrize('case,level', CASE_IDS, ids=[f'{n}-L{lv}' for n, lv in CASE_IDS])
@pytest.mark.parametrize('precision,two_phase', FP32_CLASS, ids=_P32_IDS)
def test_backward_fp32_class(case, level, precision, two_phase):
    """Training forward + hla_vgg_backward with gradients at every normalised map and confidence map, against fp64
    autograd: the training forward's maps to 1e-5, every parameter gradient to max-rel 2e-4 (or the ref32 rule).
    fp16x3 also with the two-phase weight-gradient kernels (bit 0) and with conv0's weight gradient unfused (bit 1)."""
    B, H, W, _ = CASES[case]
    r = _ref((B, H, W), level)
    d = _dev()
    tag = f'bwd {_P32_IDS[FP32_CLASS.index((precision, two_phase))]} {case} {(B, H, W)} L{level}'
    fwd, grads, g64, g32 = _run_backward(tag, r, level, precision, d, wgrad_two_phase=two_phase)
    _check_forward_fp32_class(tag, *fwd, r)
    _check_backward(tag, grads, r, g64, g32)


@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_backward_image_row_window(precision):
    """The input as a row window big[:, :, 16:16 + H] of a taller image (passed with its plane stride, not copied): the
    forward maps and every gradient against the references of the same pixels."""
    level = 3
    B, H, W, _ = CASES['odd_pooled']
    r = _ref((B, H, W), level)
    tag = f'window {precision} {(B, H, W)} L{level}'
    fwd, grads, g64, g32 = _run_backward(tag, r, level, precision, _dev(), window=True)
    _check_forward_fp32_class(tag, *fwd, r)
    _check_backward(tag, grads, r, g64, g32)


_SPARSE = [('tall', 3), ('odd_pooled', 3)]      # (the tile lists are built at level 3 only)


@pytest.mark.parametrize('case,level', _SPARSE, ids=[f'{n}-L{lv}' for n, lv in _SPARSE])
@pytest.mark.parametrize('mode', ['scale_invariant', 'dense'])
@pytest.mark.parametrize('precision', ['fp32', 'fp16x3'])
def test_backward_sparse_upstream(case, level, mode, precision):
    """An upstream gradient on a corner block only (orthogonal to the maps, as the flag requires): with ``scale_invariant`` the
    backward builds short tile lists (only tiles the block reaches), with ``dense`` it walks every tile -- both against fp64
    autograd of the same sparse functional."""
    B, H, W, _ = CASES[case]
    r = _ref((B, H, W), level, sparse=True)
    tag = f'sparse {mode} {precision} {case} {(B, H, W)} L{level}'
    stats = {}
    fwd, grads, g64, g32 = _run_backward(tag, r, level, precision, _dev(), stats=stats, scale_invariant=True,
                                         dense=mode == 'dense')
    if mode == 'scale_invariant':
        assert 0 < stats['live_tiles'] < stats['total_tiles'], (tag, stats)      # the short lists are really taken
        print(f'{tag}: live tiles {stats["live_tiles"]} of {stats["total_tiles"]}')
    _check_backward(tag, grads, r, g64, g32)


@pytest.mark.parametrize('precision,two_phase', FP32_CLASS, ids=_P32_IDS)
def test_backward_many_tiles(precision, two_phase):
    """(4, 264, 296), level 3: every weight-gradient launch has ntile > KS, so each k-split workgroup loops over several
    4 x 32 tiles and the fixed-order partial reduction adds several partials per workgroup.  KS = min(ntile, R / pairs),
    pairs = (Cout / 64) * (Cin / 64), R = 512 resident workgroups (two-phase kernels) or 256 (wave-specialised, fp16x3's
    default); ntile = B * ceil(h / 4) * ceil(w / 32):
      full res 264 x 296:  ntile 4 * 66 * 10 = 2640;  conv2 (64, 64): KS 512 / 256
      H/2 132 x 148:       ntile 4 * 33 * 5 = 660;    conv5 (128, 64): 256 / 128, conv7 (128, 128): 128 / 64,
                                                      dec2.1 (64, 192): 170 / 85, dec2.3 (64, 64): 512 / 256
      H/4 66 x 74:         ntile 4 * 17 * 3 = 204;    conv10 (256, 128): 64 / 32, conv12 / conv14 (256, 256): 32 / 16,
                                                      dec1.1 (128, 384): 42 / 21, dec1.3 (128, 128): 128 / 64"""
    level = 3
    r = _ref(MANY_TILES, level)
    tag = f'many-tiles {_P32_IDS[FP32_CLASS.index((precision, two_phase))]} {MANY_TILES} L{level}'
    fwd, grads, g64, g32 = _run_backward(tag, r, level, precision, _dev(), wgrad_two_phase=two_phase)
    _check_forward_fp32_class(tag, *fwd, r)
    _check_backward(tag, grads, r, g64, g32)


GROUPING_TOL = 1e-5     # the same exact products in another split-K grouping: relative L2 of a tensor (fp32 summation order only)
CONV0_TOL = 2e-3        # conv0.*: bit 0 also moves conv0's gradient from the fused epilogue to the stored 16-bit map's kernel
_GROUPINGS = [(n, lv, {}) for n, lv in CASE_IDS] + [('odd_pooled', 3, dict(scale_invariant=True, dense=True, first_row8=4))]
_GROUPING_IDS = [f'{n}-L{lv}' for n, lv in CASE_IDS] + ['odd_pooled-L3-first_row8']


@pytest.mark.parametrize('case,level,kw', _GROUPINGS, ids=_GROUPING_IDS)
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_backward_16bit_wgrad_groupings_agree(case, level, kw, precision):
    """bf16 / fp16: one training forward, then the backward twice on the same saved context and upstream gradient -- with the
    wave-specialised weight-gradient kernel (256 k-split workgroups) and with the two-phase kernel (``wgrad_two_phase`` = 1,
    512).  A product of two 16-bit values is exact in fp32, so the two runs differ in the order of fp32 sums only: every
    gradient to 1e-5 of its norm (the split-mode bound of test_wave_specialised_wgrad_matches_the_two_phase_kernels; no LM
    backward here, so no atomics), conv0.* to 2e-3 (bit 0 also selects the stored-map conv0 kernel:
    test_fused_conv0_weight_gradient_matches_the_stored_map_kernel).  The extra case trims the launches to ODD first rows
    (first_row8 = 4 at H = 40 with confidence heads: row 15 at H/2) -- the tile origins the loaders must carry through the
    upsample shift; both runs get the same flags."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc, vgg_backward_nhwc
    B, H, W, _ = CASES[case]
    r = _ref((B, H, W), level)
    d = _dev()
    tag = f'groupings {precision} {case} {(B, H, W)} L{level} {kw}'
    net = _net(r['sd'], level, precision)
    feats, confs, inv, ctx = vgg_forward_nhwc(net, r['x'].to(d), want_conf=True, defer_norm=True, save_for_backward=True)
    dfe = [_nhwc(u, d, r['pad'] if l == 3 else None) for l, u in enumerate(r['ups'])]
    dcs = [u[:, 0].contiguous().float().to(d) for u in r['cups']]
    g_ws, g_tp = [{k: g.detach().double().cpu() for k, g in vgg_backward_nhwc(net, ctx, dfe, confs, dcs, wgrad_two_phase=tp, **kw).items()}
                  for tp in (0, 1)]
    assert set(g_ws) == set(g_tp), (tag, sorted(set(g_ws) ^ set(g_tp)))
    worst, worst0, bad = (0.0, ''), (0.0, ''), []
    for k in sorted(g_ws):
        n_ws, n_tp = float(g_ws[k].norm()), float(g_tp[k].norm())
        assert n_ws > 0 and n_tp > 0 and np.isfinite(n_ws) and np.isfinite(n_tp), (tag, k, n_ws, n_tp)
        e = float((g_ws[k] - g_tp[k]).norm()) / n_tp
        conv0 = k.startswith('conv0.')
        if conv0:
            worst0 = max(worst0, (e, k))
        else:
            worst = max(worst, (e, k))
        if e > (CONV0_TOL if conv0 else GROUPING_TOL):
            bad.append((k, e))
    print(f'{tag}: worst relative L2 {worst[0]:.2e} ({worst[1]}), gate {GROUPING_TOL:.0e}; conv0 {worst0[0]:.2e} ({worst0[1]}), '
          f'gate {CONV0_TOL:.0e}; {len(g_ws)} tensors')
    assert not bad, (tag, bad)


def _check_forward_16bit(tag, got, emu, exact):
    """Every map against the fp64 emulation within ``vgg_round16.gate`` (the CPU's flip noise, by regime); on flip-free maps
    the gate must also lie 10x below the rounding the emulation models."""
    names = [f'feat{l}' for l in range(len(got) // 2)] + [f'conf{l}' for l in range(len(got) // 2)]
    worst = (0.0, '', 0.0)
    for name, g, e64, e32, ex in zip(names, got, emu[torch.float64], emu[torch.float32], exact):
        assert g.shape == e64.shape and np.isfinite(g).all(), (tag, name)
        gt = R16.gate(e64, e32, ex)
        l2, mx = _rell2(g, e64), _maxrel(g, e64)
        worst = max(worst, (l2 / gt['l2'], name, l2), (mx / gt['max'], name, mx))
        print(f"{tag} {name} [{gt['regime']}]: relL2 {l2:.2e} (gate {gt['l2']:.2e}, noise {gt['noise_l2']:.2e}, rounding "
              f"{gt['rnd_l2']:.2e}), max-rel {mx:.2e} (gate {gt['max']:.2e}, rounding {gt['rnd_max']:.2e})")
        assert l2 <= gt['l2'] and mx <= gt['max'], (tag, name, gt['regime'], l2, gt['l2'], mx, gt['max'])
        if gt['regime'] == 'flip-free':
            assert gt['rnd_l2'] >= 10 * gt['l2'], (tag, name, gt)
    print(f'{tag}: worst error / gate {worst[0]:.2f} ({worst[1]}: {worst[2]:.2e})')


@pytest.mark.parametrize('case,level', CASE_IDS, ids=[f'{n}-L{lv}' for n, lv in CASE_IDS])
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_forward_16bit(case, level, precision):
    """bf16 / fp16 inference forward against the rounding-aware fp64 emulation of the kernels (``vgg_round16``): every
    normalised map and confidence map within k x the emulation's own fp32-vs-fp64 noise (``vgg_round16.gate``)."""
    B, H, W, _ = CASES[case]
    r = _ref((B, H, W), level, sixteen=True)
    net = _net(r['sd'], level, precision)
    with torch.no_grad():
        feats, confs = net(r['x'].to(_dev()))
    got = [t.double().cpu().numpy() for t in feats + confs]
    _check_forward_16bit(f'fwd {precision} {case} {(B, H, W)} L{level}', got, r['emu'][precision], r['f64'] + r['c64'])


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_forward_16bit_feat16(precision):
    """``feat16``: the raw maps returned as saturated fp16 (both modes), their sum of squares and the confidence heads' input
    taken from that value -- against the emulation with the same rounding, level 3."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc
    level = 3
    B, H, W, _ = CASES['odd_batch']
    r = _ref((B, H, W), level, sixteen=True)
    key = 'emu_feat16_' + precision
    if key not in r:
        with torch.no_grad():
            r[key] = {acc: [t.double().numpy() for t in sum(R16.forward(r['sd'], r['x'], level, R16.DTYPES[precision], acc,
                                                                        feat16=True)[:2], [])]
                      for acc in (torch.float64, torch.float32)}
    net = _net(r['sd'], level, precision)
    feats, confs, inv = vgg_forward_nhwc(net, r['x'].to(_dev()), want_conf=True, defer_norm=True, feat16=True)
    assert all(f.dtype == torch.float16 for f in feats)
    got = [(f.double() * inv[l].view(B, 1, 1, 1)).permute(0, 3, 1, 2).cpu().numpy() for l, f in enumerate(feats)] + \
          [c.unsqueeze(1).double().cpu().numpy() for c in confs]
    _check_forward_16bit(f'fwd feat16 {precision} {(B, H, W)} L{level}', got, r[key], r['f64'] + r['c64'])
