"""Placement checks of the 16-bit forward conv3x3 kernels: which lane, register, pixel, tap and channel every value goes through.

*Exact-integer networks.*  Every output channel of every convolution is ``x[c1, tap1] - x[c2, tap2]`` (weights +1 / -1, biases
zero; channels and taps drawn per (layer, cout) from a seeded RNG) and the image holds small integers.  Every activation and raw
map is then an integer of magnitude <= 127: exact in bf16 and fp16, in fp32 accumulation and in ANY summation order.  So the maps
of the kernels must EQUAL the fp64 oracle's (``oracle.ref_cpu.VGGUnet.raw_maps``) element for element, and a wrong lane, cout,
pixel, tap or channel anywhere shows as an integer mismatch.  Two draws:

  * ``uniform``: image 0..7, both channels and both taps uniform.  The hardest placement test (both operands of every cout are
    live everywhere), but its 2x2 pool windows tie often: after a ReLU half of a symmetric difference is zero, and only
    0.55-0.76 of the windows of the multi-tile cases have a unique maximum (0.11 at x15 of the one-tile case, where most taps
    of a 2x2 map read the zero padding).
  * ``spread``: arranged so that ties are rare.  Image channel 0 holds 64..127, channels 1-2 hold 0..15; in every layer the
    couts with ``k % 16 == 5`` are "low" (low - low), all others "high" (a high channel minus a low one: positive and spread
    over ~100 values); the high operand's tap is the centre in 0.6 of the draws and uniform otherwise (on the 2x2 and 4x4
    maps of the one-tile case a chain of off-centre taps ends in the padding), the low operand's tap is uniform.  The CPU
    test asserts that in EVERY case at least 90 % of all pool windows have a unique maximum in the oracle alone (0.93-0.95).

``test_integer_network_draws_cpu`` also checks that both draws reach all nine taps (layers of 64 couts or more), both 16-channel halves of a 32-channel
stage, every stage and both sources of the decoder's concatenations.

*Pool argmax bytes* (training forward, both draws).  Where a window's maximum is unique the byte must be the oracle's argmax
(2 * row + col); on ``spread`` the test asserts that this strict comparison covers >= 90 % of the windows.  On top of that,
since the arithmetic is exact, EVERY byte -- tied windows too -- must follow the kernels' own rule (``_kernel_argmax``): the
upper row wins a tie inside a column, then the left column wins a tie between the columns' maxima.  That is not
``F.max_pool2d``'s row-major first maximum: maxima at (0,1) and (1,0) give 2, not 1.

*4-row against 8-row tiles.*  A launch below CONV_SMALL_GRID workgroups takes 4-row tiles (conv_kernels.h, launch_conv); every
output element's sum is formed in the same order, so one sample alone (4-row tiles) and the same sample inside a batch (8-row
tiles) must give bitwise equal maps.  The test computes the grids and asserts that a layer of each kernel class crosses.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
import vgg_decisions as D

PRECISIONS = ['bf16', 'fp16']
# (B, H, W), levels, first_row8
CASES = {
    'tiny': ((1, 8, 8), (3, 4), 0),            # below one tile at every resolution
    'odd_pooled': ((3, 40, 72), (3,), 0),      # odd pooled sizes, W not a multiple of 32 at any level
    'trimmed': ((2, 72, 40), (3,), 5),         # row trimming: conv5 starts at row 4 * 5 - 15 = 5 (odd)
}
CASE_IDS = [(n, lv) for n, (_, lvs, _) in CASES.items() for lv in lvs]
CONV_LAYERS = [n for n, *_ in O.VGG_LAYOUT if not n.startswith('conf')]
# layer -> channels of its first source when it reads a concatenation (VGG.py:144-155)
CONCAT_SPLIT = {'conv_dec1.1': 256, 'conv_dec2.1': 128, 'conv_dec3.1': 64}
_REFS = {}


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


DRAWS = ['uniform', 'spread']
# layer -> the layers whose output channels it reads, in concatenation order (VGG.py:121-155); None: the image
SOURCES = {'conv0': None, 'conv2': ['conv0'], 'conv5': ['conv2'], 'conv7': ['conv5'], 'conv10': ['conv7'], 'conv12': ['conv10'],
           'conv14': ['conv12'], 'conv_dec1.1': ['conv14', 'conv7'], 'conv_dec1.3': ['conv_dec1.1'],
           'conv_dec2.1': ['conv_dec1.3', 'conv2'], 'conv_dec2.3': ['conv_dec2.1'], 'conv_dec3.1': ['conv_dec2.3', 'conv2'],
           'conv_dec3.3': ['conv_dec3.1']}
CENTRE_P = 0.6      # 'spread': share of the high operand's taps forced to the centre


def _integer_state(seed, draw):
    """state dict of an exact-integer network and, per layer, the drawn (c1, tap1, c2, tap2) rows"""
    rs = np.random.RandomState(seed)
    sd, draws, low = {}, {}, {}
    for name, co, ci, has_b in O.VGG_LAYOUT:
        w = np.zeros((co, ci, 9), np.float32)
        if name in CONV_LAYERS:
            low_in = np.array([False, True, True]) if SOURCES[name] is None else np.concatenate([low[s] for s in SOURCES[name]])
            assert len(low_in) == ci, name
            highs, lows = np.flatnonzero(~low_in), np.flatnonzero(low_in)
            low[name] = np.arange(co) % 16 == 5
            rows = []
            for k in range(co):
                while True:
                    if draw == 'uniform':
                        c1, t1, c2, t2 = rs.randint(ci), rs.randint(9), rs.randint(ci), rs.randint(9)
                    else:
                        t1, t2 = (4 if rs.rand() < CENTRE_P else rs.randint(9)), rs.randint(9)
                        c1, c2 = rs.choice(lows if low[name][k] else highs), rs.choice(lows)
                    if (c1, t1) != (c2, t2):
                        break
                w[k, c1, t1], w[k, c2, t2] = 1.0, -1.0
                rows.append((c1, t1, c2, t2))
            draws[name] = np.array(rows)
        sd[name + '.weight'] = torch.from_numpy(w.reshape(co, ci, 3, 3))
        if has_b:
            sd[name + '.bias'] = torch.zeros(co)
    return sd, draws


def _integer_image(seed, shape, draw):
    B, H, W = shape
    rs = np.random.RandomState(seed)
    if draw == 'uniform':
        return torch.from_numpy(rs.randint(0, 8, (B, 3, H, W)).astype(np.float32))
    x = rs.randint(0, 16, (B, 3, H, W))
    x[:, 0] = rs.randint(64, 128, (B, H, W))
    return torch.from_numpy(x.astype(np.float32))


def _kernel_argmax(w):
    """the byte the pooling epilogues store for windows ``w`` [..., 4] (index 2 * row + col): per column the upper row wins a
    tie, then the left column wins a tie (conv_epilogue, conv_kernels.h)"""
    r0, r1 = (w[..., 2] > w[..., 0]).long(), (w[..., 3] > w[..., 1]).long()
    m0, m1 = torch.maximum(w[..., 0], w[..., 2]), torch.maximum(w[..., 1], w[..., 3])
    return torch.where(m1 > m0, 2 * r1 + 1, 2 * r0)


def _prepool(net, x):
    """the three maps the 2x2 max-pools read (VGG.py:123-141): x2, x7, x14"""
    r = F.relu
    x2 = net.conv2(r(net.conv0(x)))
    x7 = net.conv7(r(net.conv5(r(F.max_pool2d(x2, 2)))))
    x14 = net.conv14(r(net.conv12(r(net.conv10(r(F.max_pool2d(x7, 2)))))))
    return x2, x7, x14


def _ref(case, level, draw='uniform'):
    """fp64 oracle of one case, computed once per session: raw maps [B,C,h,w], and per pool the windows' argmax (2 * row + col),
    whether the maximum is unique, and the byte the kernels' tie rule gives"""
    key = (case, level, draw)
    r = _REFS.get(key)
    if r is None:
        (B, H, W), _, f8 = CASES[case]
        sd, draws = _integer_state(1009 * H + 13 * W + level, draw)
        x = _integer_image(77 + H + W, (B, H, W), draw)
        net = O.VGGUnet(level)
        net.load_state_dict(sd)
        net = net.double()
        with torch.no_grad():
            raws = net.raw_maps(x.double())[:level]
            pools = {}
            for name, t in zip(D.POOLS, _prepool(net, x.double())):
                w = D.windows(t)
                top = w.topk(2, -1).values
                pools[name] = dict(argmax=w.argmax(-1), unique=top[..., 0] > top[..., 1], kernel=_kernel_argmax(w))
        r = dict(sd=sd, draws=draws, x=x, raws=[t.numpy() for t in raws], pools=pools, first_row8=f8)
        _REFS[key] = r
    return r


def _net(sd, level, precision):
    from highlyaccurate_amd.VGG import VGGUnet
    net = VGGUnet(level, precision=precision)
    net.load_state_dict(sd)
    return net.to(_dev())


def _assert_maps_equal(tag, feats, r, first_row8=0):
    for l, (f, ref) in enumerate(zip(feats, r['raws'])):
        got = f.float().cpu().permute(0, 3, 1, 2).numpy()
        if l == 3:      # x24: 16 real channels of 64 stored, the padded ones exactly zero
            assert not got[:, 16:].any(), (tag, 'x24 padding')
            got = got[:, :16]
        y0 = first_row8 << l     # rows above it are not written (include/hla.h, first_row8)
        bad = got[:, :, y0:] != ref[:, :, y0:]
        assert not bad.any(), (tag, f'map {l}', int(bad.sum()), 'of', bad.size, 'first at (b, c, y, x)',
                               np.argwhere(bad)[:4].tolist(), got[:, :, y0:][bad][:4].tolist(), ref[:, :, y0:][bad][:4].tolist())


def test_integer_network_draws_cpu():
    """The oracle side alone: the networks stay in the exact integers, the draws cover what they must, the kernels' tie rule
    agrees with the oracle's argmax wherever the maximum is unique, and on the 'spread' draw at least 90 % of the pool windows
    of every case have a unique maximum."""
    for draw in DRAWS:
        for case, level in CASE_IDS:
            r = _ref(case, level, draw)
            for t in r['raws']:
                assert np.array_equal(t, np.rint(t)) and np.abs(t).max() <= (7 if draw == 'uniform' else 127), (draw, case, level)
            for name, d in r['draws'].items():
                ci = r['sd'][name + '.weight'].shape[1]
                ch = np.concatenate([d[:, 0], d[:, 2]])
                if len(d) >= 64:      # (conv_dec3.1 / 3.3 have 32 / 16 output channels: too few draws to promise every tap)
                    assert set(np.concatenate([d[:, 1], d[:, 3]])) == set(range(9)), (draw, name, 'taps')
                if ci >= 32:
                    assert set(ch // 32) == set(range(ci // 32)), (draw, name, 'stages')
                    assert set((ch % 32) // 16) == {0, 1}, (draw, name, 'K-halves')
                if name in CONCAT_SPLIT:
                    assert (ch < CONCAT_SPLIT[name]).any() and (ch >= CONCAT_SPLIT[name]).any(), (draw, name, 'sources')
            for p in r['pools'].values():
                assert torch.equal(p['kernel'][p['unique']], p['argmax'][p['unique']])
            uniq = {k: round(float(p['unique'].double().mean()), 3) for k, p in r['pools'].items()}
            n_u = sum(int(p['unique'].sum()) for p in r['pools'].values())
            n = sum(p['unique'].numel() for p in r['pools'].values())
            print(f'{draw} {case} L{level}: unique-maximum windows {uniq}, all pools {n_u / n:.3f}')
            if draw == 'spread':
                assert n_u >= 0.9 * n, (case, level, uniq, n_u / n)


@pytest.mark.gpu
@pytest.mark.parametrize('case,level', CASE_IDS, ids=[f'{n}-L{lv}' for n, lv in CASE_IDS])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_integer_network_inference(case, level, precision):
    """Inference: the 16-bit raw maps (feat16, level 3) and the fp32 raw maps of the plain path equal the oracle's."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc
    r = _ref(case, level)
    net, xd, f8 = _net(r['sd'], level, precision), r['x'].to(_dev()), r['first_row8']
    with torch.no_grad():
        if level == 3:
            feats, _, _ = vgg_forward_nhwc(net, xd, want_conf=False, defer_norm=True, feat16=True, first_row8=f8)
            assert feats[0].dtype == torch.float16
            _assert_maps_equal(f'{case} {precision} feat16', feats, r, f8)
        feats, _, _ = vgg_forward_nhwc(net, xd, want_conf=True, defer_norm=True, first_row8=f8)
        assert feats[0].dtype == torch.float32
        _assert_maps_equal(f'{case} {precision} plain', feats, r, f8)


def _argmax_maps(ws, B, H, W):
    """the three pool argmax maps [B,h,w,C] (u8) of a training forward's workspace: its last three blocks, each padded to 256
    bytes, in the order idx3, idx8, idx15 (``vgg_plan``, highlyaccurate_amd/csrc/vgg_layers.h)"""
    out, end = {}, ws.numel()
    for name, div, C in (('x15', 8, 256), ('x8', 4, 128), ('x3', 2, 64)):
        h, w = H // div, W // div
        n = B * h * w * C
        end -= -(-n // 256) * 256
        out[name] = ws[end:end + n].view(B, h, w, C)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('case,level', CASE_IDS, ids=[f'{n}-L{lv}' for n, lv in CASE_IDS])
@pytest.mark.parametrize('draw', DRAWS)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_integer_network_training_forward(case, level, draw, precision):
    """Training forward (every row, generic epilogues): the maps equal the oracle's; the pool argmax bytes are the oracle's
    where the window maximum is unique -- at least 90 % of all windows on the 'spread' draw -- and follow the kernels' tie
    rule everywhere."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc
    r = _ref(case, level, draw)
    (B, H, W), _, _ = CASES[case]
    net, xd = _net(r['sd'], level, precision), r['x'].to(_dev())
    with torch.no_grad():
        feats, _, _, ctx = vgg_forward_nhwc(net, xd, want_conf=True, defer_norm=True, save_for_backward=True)
    _assert_maps_equal(f'{case} {draw} {precision} train', feats, r)
    n_all = n_strict = 0
    for name, m in _argmax_maps(ctx['ws'], B, H, W).items():
        idx = m.permute(0, 3, 1, 2).long().cpu()
        ref = r['pools'][name]
        u = ref['unique']
        bad = (idx != ref['argmax']) & u
        assert not bad.any(), (case, draw, precision, name, 'argmax byte', int(bad.sum()), torch.nonzero(bad)[:4].tolist())
        n_all += u.numel()
        n_strict += int(u.sum())
        bad = idx != ref['kernel']
        assert not bad.any(), (case, draw, precision, name, 'tie rule', int(bad.sum()), torch.nonzero(bad)[:4].tolist())
    print(f'{case} {draw} {precision}: {n_all} windows, {n_strict} compared with the oracle\'s argmax ({n_strict / n_all:.3f})')
    if draw == 'spread':
        assert n_strict >= 0.9 * n_all, (n_strict, n_all)


CONV_SMALL_GRID = 320      # conv_kernels.h
SMALL_GRID_SHAPE = (8, 120, 264)


def _grid(B, h, w, cout):
    return -(-w // 32) * -(-h // 8) * B * (cout // 128 if cout >= 128 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_small_grid_tiles_bitwise(precision):
    """One sample alone (4-row tiles in the layers below CONV_SMALL_GRID workgroups) against the same sample inside a batch
    (8-row tiles): every returned map and 1 / norm bitwise equal."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc
    B, H, W = SMALL_GRID_SHAPE
    # a layer of each kernel class without a sum-of-squares output: (name, class, resolution divisor, Cout)
    for name, cls, div, cout in (('conv5', 'plain NT2', 2, 128), ('conv7', 'pooled NT2', 2, 128), ('conv_dec2.1', 'NT1', 2, 64)):
        g1, gB = _grid(1, H // div, W // div, cout), _grid(B, H // div, W // div, cout)
        assert g1 < CONV_SMALL_GRID <= gB, (name, cls, g1, gB)
    rs = np.random.RandomState(4242)
    sd = O.synth_vgg_state(rs, bias_scale=0.05)
    x = torch.from_numpy(rs.random_sample((B, 3, H, W)).astype(np.float32)).to(_dev())
    net = _net(sd, 3, precision)
    s = 5
    for kw in (dict(want_conf=False, feat16=True), dict(want_conf=True)):
        with torch.no_grad():
            fb, cb, ib = vgg_forward_nhwc(net, x, defer_norm=True, **kw)
            f1, c1, i1 = vgg_forward_nhwc(net, x[s:s + 1].contiguous(), defer_norm=True, **kw)
        for l in range(3):
            assert torch.equal(fb[l][s].view(torch.int16 if kw.get('feat16') else torch.int32),
                               f1[l][0].view(torch.int16 if kw.get('feat16') else torch.int32)), (precision, kw, 'map', l)
            if cb[l] is not None:
                assert torch.equal(cb[l][s].view(torch.int32), c1[l][0].view(torch.int32)), (precision, kw, 'conf', l)
        assert torch.equal(ib[:, s].view(torch.int64), i1[:, 0].view(torch.int64)), (precision, kw, 'inv_norm')
