"""The weight ring of the 16-bit forward conv3x3 kernels, layer by layer (conv_kernels.h: WeightRing ASYNC, stage_mma).

These kernels request their weight fragments and count the waits for them by hand, next to the halo tile's DMA loads.  A wrong
count or a wrong ring slot makes an MFMA read a fragment that has not landed or that belongs to another tap, so the checks are
exact: single layers of every stage count and kernel class, run through ``hla_debug_conv_layer`` (vgg.hip: launch_conv outside
the network's layer graph) on exact-integer data and compared element for element with an fp64 oracle.

*Cases.*  Cin in {32, 64, 96, 128} = 1, 2, 3, 4 pipeline stages (no next stage, the first hand-over, the ring's slots coming
round again across stage boundaries); Cout in {64, 128, 256} = the 32-channel wave tile, the 64-channel one, two channel
blocks; plain and pooled; H x W in {9 x 33, 16 x 32, 17 x 65}, B = 2 (ragged last tiles, one and several tiles).  The 2x2
pool is only defined on even maps (the network pools multiples of 4), so the pooled form runs the odd sizes rounded up to
10 x 34 and 18 x 66: the tiles stay ragged in both directions.

*Both tiles of each class.*  A launch of fewer than CONV_SMALL_GRID workgroups takes 4-row tiles unless it writes sum-of-squares
partials (conv_plan).  Every case here is far below the threshold, so each layer runs twice: as a plain activation layer (4-row
tiles) and as a feature layer with the raw fp32 map and its partials (8-row tiles).

*Exact integers.*  As in tests/test_conv_mfma_shape.py: the input holds integers 0..7 and every output channel is a signed sum
of eight input taps (weights +1 / -1), so every map is an integer of magnitude <= 56 <= 127: exact in bf16 and fp16, in fp32
accumulation and in any summation order.  The eight (stage, tap) positions of output channel k are 8k .. 8k+7 modulo
9 * stages, so every tap of every stage is read by many channels of every 32-channel tile.

*Paired launch.*  Two such layers (different data, different sizes) as the two segments of one launch must give the bits of
the two plain launches.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

PRECISIONS = ['bf16', 'fp16']
CINS = (32, 64, 96, 128)
COUTS = (64, 128, 256)
SIZES = ((9, 33), (16, 32), (17, 65))
B = 2
CONV_SMALL_GRID = 320      # conv_kernels.h
_DT = {'bf16': (1, torch.bfloat16), 'fp16': (2, torch.float16)}      # HLA_BF16, HLA_F16 (include/hla.h)
_REFS = {}


class Seg(C.Structure):      # HlaConvLayerSeg (vgg.hip)
    _fields_ = [('src', C.c_void_p), ('w', C.c_void_p), ('wpk', C.c_void_p), ('out', C.c_void_p), ('raw', C.c_void_p),
                ('sumsq', C.c_void_p), ('H', C.c_int), ('W', C.c_int)]


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _size(hw, pool):
    h, w = hw
    return (h + (h & 1), w + (w & 1)) if pool else (h, w)


def _layer(cin, cout, hw, pool, seed=0):
    """one exact-integer layer and its fp64 oracle, computed once per session: x [B,Cin,H,W], w [Cout,Cin,3,3], the raw map
    (pooled where the layer pools, before the ReLU) and the activation, both NCHW"""
    key = (cin, cout, hw, pool, seed)
    r = _REFS.get(key)
    if r is None:
        h, w_ = hw
        rs = np.random.RandomState(1000 * cin + cout + 7 * h + w_ + 100003 * seed)
        x = rs.randint(0, 8, (B, cin, h, w_)).astype(np.float64)
        wt = np.zeros((cout, cin, 9))
        nst = cin // 32
        for k in range(cout):
            for i in range(8):
                p = (8 * k + i) % (9 * nst)
                sg, tap = divmod(p, 9)
                while True:      # a channel of that stage whose tap is still free
                    c = 32 * sg + rs.randint(32)
                    if wt[k, c, tap] == 0:
                        break
                wt[k, c, tap] = 1.0 if i % 2 == 0 else -1.0
        wt = wt.reshape(cout, cin, 3, 3)
        raw = F.conv2d(torch.from_numpy(x), torch.from_numpy(wt), padding=1)
        if pool:
            raw = F.max_pool2d(raw, 2)
        assert float(raw.abs().max()) <= 56 and torch.equal(raw, raw.round())
        r = dict(x=torch.from_numpy(x).float(), w=torch.from_numpy(wt).float(), raw=raw.numpy(), act=raw.clamp_min(0).numpy())
        _REFS[key] = r
    return r


def _lib():
    from highlyaccurate_amd import _lib as L
    lib = L.load()
    lib.hla_debug_conv_layer.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.hla_debug_conv_layer.restype = C.c_int
    lib.hla_last_error.restype = C.c_char_p
    return lib


def _run(precision, cin, cout, pool, layers, feature):
    """launch one layer (one entry) or a paired launch (two entries: same channels and pooling, own data and size); returns per
    entry (act [B,Ho,Wo,Cout] in the 16-bit type, raw fp32 or None).  feature: with the raw map and its partials (8-row tiles)"""
    code, tdt = _DT[precision]
    d = _dev()
    segs, keep, outs = (Seg * len(layers))(), [], []
    for k, r in enumerate(layers):
        h, w = r['x'].shape[2:]
        ho, wo = (h // 2, w // 2) if pool else (h, w)
        g = -(-w // 32) * -(-h // 8) * B * max(1, cout // 128)
        assert g < CONV_SMALL_GRID, 'the plain form of every case takes 4-row tiles'
        src = r['x'].to(d).permute(0, 2, 3, 1).contiguous().to(tdt)
        wsrc = r['w'].to(d).contiguous()
        wpk = torch.zeros(cout * (cin * 9 + 256) * 2, dtype=torch.uint8, device=d)
        out = torch.full((B, ho, wo, cout), -7.0, dtype=tdt, device=d)
        raw = torch.full((B, ho, wo, cout), -7.0, dtype=torch.float32, device=d) if feature else None
        ss = torch.zeros(B * -(-h // 8) * -(-w // 32) * max(1, cout // 128), dtype=torch.float64, device=d) if feature else None
        keep += [src, wsrc, wpk, ss]
        outs.append((out, raw))
        segs[k] = Seg(src.data_ptr(), wsrc.data_ptr(), wpk.data_ptr(), out.data_ptr(), raw.data_ptr() if feature else None,
                      ss.data_ptr() if feature else None, h, w)
    lib = _lib()
    rc = lib.hla_debug_conv_layer(code, B, cin, cout, int(pool), C.cast(segs, C.c_void_p), len(layers),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.hla_last_error()
    torch.cuda.synchronize()
    return outs


def _check(tag, got, r):
    out, raw = got
    for name, t, ref in (('act', out, r['act']), ('raw', raw, r['raw'])):
        if t is None:
            continue
        g = t.float().cpu().permute(0, 3, 1, 2).numpy()
        bad = g != ref
        assert not bad.any(), (tag, name, int(bad.sum()), 'of', bad.size, 'first at (b, c, y, x)', np.argwhere(bad)[:4].tolist(),
                               g[bad][:4].tolist(), ref[bad][:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('pool', [False, True], ids=['plain', 'pooled'])
@pytest.mark.parametrize('hw', SIZES, ids=[f'{h}x{w}' for h, w in SIZES])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_single_layers_equal_the_oracle(precision, hw, pool):
    """Every (Cin, Cout) as an activation layer (4-row tiles) and as a feature layer (8-row tiles): all maps equal the oracle's."""
    for cin in CINS:
        for cout in COUTS:
            r = _layer(cin, cout, _size(hw, pool), pool)
            for feature in (False, True):
                got = _run(precision, cin, cout, pool, [r], feature)[0]
                _check((precision, cin, cout, hw, pool, '8-row' if feature else '4-row'), got, r)


@pytest.mark.gpu
@pytest.mark.parametrize('pool', [False, True], ids=['plain', 'pooled'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_paired_launch_equals_the_plain_launches(precision, pool):
    """Two layers of different data and sizes as one two-segment launch: the bits of the two plain launches, and the oracle's."""
    for cin in CINS:
        for cout in COUTS:
            ra = _layer(cin, cout, _size(SIZES[2], pool), pool)
            rb = _layer(cin, cout, _size(SIZES[0], pool), pool, seed=1)
            for feature in (False, True):
                pair = _run(precision, cin, cout, pool, [ra, rb], feature)
                for k, r in enumerate((ra, rb)):
                    tag = (precision, cin, cout, pool, '8-row' if feature else '4-row', 'segment', k)
                    plain = _run(precision, cin, cout, pool, [r], feature)[0]
                    _check(tag, pair[k], r)
                    for p, q in zip(pair[k], plain):
                        if p is not None:
                            assert torch.equal(p.view(torch.int16 if p.dtype != torch.float32 else torch.int32),
                                               q.view(torch.int16 if q.dtype != torch.float32 else torch.int32)), tag
