"""What the extractor's host code launches, pinned launch by launch.  With the library's per-launch records on
(``_lib.prof_enable``), every forward / backward entry below is run once at B = 2, H = 64, W = 160 -- the smallest shape that admits
first_row8 = 5, first_col32 = 1 and the folded decoder, with partial 32-pixel tiles at W/2, W/4 and W/8 -- and the sequence of
(kernel_id, flops, bytes) must EQUAL the fixture ``tests/golden/vgg_launch_records.json``.  Both numbers are host arithmetic on the
launch geometry (rows and columns a launch computes, its channel counts), so equality is exact: a layer that starts at another
row, takes another kernel class or is launched in another order shows here.  The pointer wiring, which the records do not show,
is covered by the bit-exact trimmed-against-full comparisons of the other VGG tests.

The data-dependent backward walk scales its records by the live-tile share found on the device, so there only the kernel-id
sequence is compared, plus the live / total tile counts.

The fixture is written by this file run as a script (``python tests/test_vgg_launch_records_gpu.py [out.json]``); it was recorded
on a checkout of the commit before the layer graph moved into csrc/vgg_graph.h.
"""
import ctypes as C
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'vgg_launch_records.json')
B, H, W = 2, 64, 160
PAIR_HW = ((64, 160), (96, 144))


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


_NETS = {}


def _net(kind, precision, seed=0):
    """kind: 3 / 4 = VGGUnet(level), 'fold' = VGGUnet_G2S(3).  Seeded default initialisation: no record depends on a weight."""
    key = (kind, precision, seed)
    if key not in _NETS:
        from highlyaccurate_amd.VGG import VGGUnet, VGGUnet_G2S
        torch.manual_seed(100 + seed)
        net = VGGUnet_G2S(3, precision=precision) if kind == 'fold' else VGGUnet(kind, precision=precision)
        _NETS[key] = net.to(_dev())
    net = _NETS[key]
    # every case packs its weights again, so the pack launch is part of every forward's records whatever ran before
    net.__dict__.pop('_hla_packed', None)
    return net


def _image(hw=(H, W), seed=1):
    g = torch.Generator(device=_dev())
    g.manual_seed(seed)
    return torch.rand(B, 3, *hw, device=_dev(), generator=g)


def _fetch():
    """[[kernel_id, flops, bytes]] of every launch since the last fetch (synchronises)."""
    from highlyaccurate_amd import _lib
    lib = _lib.load()
    buf = (_lib.ProfRecord * 4096)()
    n = C.c_int(0)
    lib.hla_prof_fetch(buf, 4096, C.byref(n))
    assert n.value < 4096
    return [[buf[k].kernel_id, buf[k].flops, buf[k].bytes] for k in range(n.value)]


def _recorded(fn):
    from highlyaccurate_amd import _lib
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        _fetch()
        extra = fn() or {}
        recs = _fetch()
    finally:
        _lib.prof_enable(False)
    return dict(records=recs, **extra)


def _forward(kind, precision, **kw):
    from highlyaccurate_amd.VGG import vgg_forward_nhwc
    net, x = _net(kind, precision), _image()
    return _recorded(lambda: vgg_forward_nhwc(net, x, defer_norm=True, **kw) and None)


def _column_trim():
    from highlyaccurate_amd import VGG
    net, x = _net(3, 'bf16'), _image()
    gate = torch.tensor([0, 1], dtype=torch.int32, device=_dev())

    def run():
        state = {}
        VGG.vgg_forward_nhwc(net, x, want_conf=False, defer_norm=True, first_col32=1, col_state=state)
        assert state['first_col32'] == 1
        VGG.vgg_fixup_nhwc(state, gate, one_launch=False)
    return _recorded(run)


def _pair(precision, first_row8, first_col32):
    from highlyaccurate_amd.VGG import vgg_forward_pair_nhwc
    nets = (_net(3, precision, 0), _net(3, precision, 1))
    xs = tuple(_image(hw, 2 + k) for k, hw in enumerate(PAIR_HW))
    return _recorded(lambda: dict(paired=vgg_forward_pair_nhwc(nets, xs, first_row8=first_row8, first_col32=first_col32,
                                                               feat16=precision == 'bf16')[2]))


def _backward(kind, precision, conf=False, block=False, **kw):
    """Records of the backward call alone.  block: every input gradient is zero outside rows h/4..h/2, columns w/2..3w/4."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc, vgg_backward_nhwc
    net, x = _net(kind, precision), _image()
    feats, confs, _, ctx = vgg_forward_nhwc(net, x, want_conf=True, defer_norm=True, save_for_backward=True)
    g = torch.Generator(device=_dev())
    g.manual_seed(9)
    d_feats = [torch.rand(f.shape, device=_dev(), generator=g) - 0.5 for f in feats]
    if block:
        for d in d_feats:
            keep = torch.zeros_like(d)
            h, w = d.shape[1], d.shape[2]
            keep[:, h // 4:h // 2, w // 2:3 * w // 4] = 1
            d *= keep
    d_confs = [torch.rand(c.shape, device=_dev(), generator=g) - 0.5 for c in confs] if conf else None

    def run():
        stats = {} if block else None
        vgg_backward_nhwc(net, ctx, d_feats, confs if conf else None, d_confs, stats=stats, **kw)
        return stats
    return _recorded(run)


def _cases():
    c = {}
    for p in ('bf16', 'fp32'):
        for f in (0, 5):
            for conf in (False, True):
                c[f'fwd {p} f{f} conf{int(conf)}'] = lambda p=p, f=f, conf=conf: _forward(3, p, want_conf=conf, first_row8=f)
        c[f'fwd {p} level4'] = lambda p=p: _forward(4, p, want_conf=True)
        c[f'fwd {p} fold'] = lambda p=p: _forward('fold', p, want_conf=True)
        c[f'fwd {p} train'] = lambda p=p: _forward(3, p, want_conf=True, save_for_backward=True)
        for f in (0, 5):
            c[f'bwd {p} dense f{f}'] = lambda p=p, f=f: _backward(3, p, scale_invariant=True, dense=True, first_row8=f)
        c[f'bwd {p} conf'] = lambda p=p: _backward(3, p, conf=True)
        c[f'bwd {p} conf dense f5'] = lambda p=p: _backward(3, p, conf=True, scale_invariant=True, dense=True, first_row8=5)
        c[f'bwd {p} level4'] = lambda p=p: _backward(4, p, conf=True)
        c[f'bwd {p} fold'] = lambda p=p: _backward('fold', p, conf=True)
        c[f'bwd {p} wgrad0 unfused'] = lambda p=p: _backward(3, p, scale_invariant=True, dense=True, wgrad_two_phase=2)
        c[f'bwd {p} walk'] = lambda p=p: _backward(3, p, block=True, scale_invariant=True)
    c['fwd bf16 column trim'] = _column_trim
    c['pair bf16 trimmed'] = lambda: _pair('bf16', (0, 4), (1, 0))
    c['pair fp32'] = lambda: _pair('fp32', (0, 0), (0, 0))
    return c


CASES = _cases()


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_lists_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_launch_records(name, golden):
    got, want = CASES[name](), golden[name]
    assert len(got['records']) > 0
    if name.endswith('walk'):
        assert [r[0] for r in got['records']] == [r[0] for r in want['records']], name
        assert got['total_tiles'] > got['live_tiles'] > 0
        assert (got['live_tiles'], got['total_tiles']) == (want['live_tiles'], want['total_tiles']), name
        return
    assert len(got['records']) == len(want['records']), (name, [r[0] for r in got['records']], [r[0] for r in want['records']])
    for k, (g, w) in enumerate(zip(got['records'], want['records'])):
        assert g == w, (name, k, g, w)
    assert {k: v for k, v in got.items() if k != 'records'} == {k: v for k, v in want.items() if k != 'records'}, name


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    res = {}
    for name in sorted(CASES):
        res[name] = CASES[name]()
        print(name, len(res[name]['records']), {k: v for k, v in res[name].items() if k != 'records'}, flush=True)
    with open(out, 'w') as f:
        f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(res.items())) + '\n}\n')
    print('wrote', out)
