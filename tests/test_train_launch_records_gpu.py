"""What one training step of every model launches, pinned launch by launch: the host layer between the public methods and the C
ABI (the autograd Functions of both directions, their shared extractor-backward tail, the pose-score plumbing) decides which entry
points run, in which order and with which flags, and the library's per-launch records (``_lib.prof_enable``) show all three.

Each case builds a fresh model (so the weight packs are part of its records), runs one forward + backward -- or one no-grad
``forward_search`` -- at the shapes of tests/test_score_loss_gpu.py (grd 64 x 256, sat 128 x 128, B = 2, N_iters = 2, 'fp32', the
oracle's seeded weights and images: the smallest the extractors and the proj='nn' fold admit), and its sequence of kernel ids must
EQUAL the fixture ``tests/golden/train_launch_records.json``.  The cases whose extractor backward takes the dense walk
(``args.bwd_trim = 0``) must equal it in the full (kernel_id, flops, bytes) triples, which are host arithmetic on the launch
geometry; the data-dependent walk scales its own records by the live-tile share found on the device, so elsewhere only the ids
are compared (as in tests/test_vgg_launch_records_gpu.py).

The records are appended on the host as the launches are issued (csrc/prof.hip), whatever stream they go to, so the satellite
branch's backward on the side stream (``args.bwd_two_streams``, the default) appears in issue order and the ``_LocaliseFn`` cases
run with the default.

The fixture is written by this file run as a script (``python tests/test_train_launch_records_gpu.py [out.json]``); it was
recorded on a checkout of the commit before the five Functions' backward tails and the two directions' pose-score plumbing were
merged into shared helpers.
"""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'train_launch_records.json')
GRD_HW, SAT_A, B = (64, 256), 128, 2
FORD_SIDE_M = 112.64
G2S_RANGES, CORR_RANGES = (20.0, 20.0, 10.0), (4.0, 6.0, 10.0)     # of test_g2s_score_loss_gpu.py / test_g2s_corr_gpu.py


def _images():
    from oracle import ref_cpu as O
    from test_vgg_launch_records_gpu import _dev
    return [t.to(_dev()) for t in O.synth_images(9, B, grd_hw=GRD_HW, sat_a=SAT_A)]


def _candidates():
    from highlyaccurate_amd.models_kitti import pose_grid
    return pose_grid(3, 3, 3)[1:].contiguous()


def _load(net):
    from oracle import ref_cpu as O
    from test_vgg_launch_records_gpu import _dev
    net.load_state_dict(O.synth_model_state(4, bias_scale=0.02))
    return net.to(_dev()).train()


def _s2g(ford, **kw):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    from highlyaccurate_amd.models_kitti import LM_S2GP
    args = O.default_args(N_iters=2, precision='fp32', **kw)
    return _load((LM_S2GP_Ford if ford else LM_S2GP)(args))


def _ford_extra():
    from test_vgg_launch_records_gpu import _dev
    R_FL = torch.tensor([[[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]]).repeat(B, 1, 1).to(_dev())
    T_FL = torch.tensor([[1.7, 0.3, -1.2]]).repeat(B, 1).to(_dev())
    return FORD_SIDE_M, R_FL, T_FL


def _g2s(ranges=G2S_RANGES, **kw):
    import g2s_geo_ref as R
    from highlyaccurate_amd.models_kitti import LM_G2SP
    a = R.make_args(ranges, **{'N_iters': 2, 'damping': 1.0, 'using_weight': 0, 'proj': 'geo', **kw})
    a.precision = 'fp32'
    return _load(LM_G2SP(a))


def _camera():
    from test_g2s_pose_search_gpu import CAMERA_K
    from test_vgg_launch_records_gpu import _dev
    return torch.tensor(CAMERA_K, dtype=torch.float32).to(_dev())


def _run(step):
    """Records of ``step()`` -> a loss to back-propagate, or None (a no-grad call)."""
    from test_vgg_launch_records_gpu import _recorded
    torch.manual_seed(0)                    # (the S2G loop draws its re-initialisation values from the global generator)

    def fn():
        loss = step()
        if loss is not None:
            loss.backward()
    return _recorded(fn)


def _s2g_train(ford, **kw):
    net = _s2g(ford, **kw)
    sat, grd, gu, gv, gh = _images()
    if ford:
        return _run(lambda: net(sat, grd, *_ford_extra(), gu[:, 0], gv[:, 0], gh[:, 0], mode='train')[0])
    return _run(lambda: net(sat, grd, gu, gv, gh, mode='train')[0])


def _s2g_score_loss(**kw):
    net = _s2g(0, **kw)
    sat, grd, gu, gv, gh = _images()
    return _run(lambda: net.score_loss(sat, grd, _candidates(), gu, gv, gh))


def _s2g_search():
    net = _s2g(0)
    sat, grd, *_ = _images()
    with torch.no_grad():
        return _run(lambda: net.forward_search(sat, grd, _candidates(), top_m=2) and None)


def _g2s_train(**kw):
    net = _g2s(**kw)
    sat, grd, gu, gv, gh = _images()
    return _run(lambda: net(sat, grd, _camera(), gu, gv, gh, mode='train')[0])


def _g2s_score_loss(**kw):
    net = _g2s(**kw)
    sat, grd, gu, gv, gh = _images()
    return _run(lambda: net.score_loss(sat, grd, _camera(), _candidates(), gu, gv, gh))


def _g2s_corr():
    net = _g2s(CORR_RANGES)
    sat, grd, gu, gv, gh = _images()
    return _run(lambda: net.corr(sat, grd, _camera(), gu, gv, gh, mode='train'))


def _g2s_search():
    net = _g2s()
    sat, grd, *_ = _images()
    with torch.no_grad():
        return _run(lambda: net.forward_search(sat, grd, _camera(), _candidates(), top_m=2) and None)


# '... dense': args.bwd_trim = 0, compared in the full triples
CASES = {
    's2g kitti train': lambda: _s2g_train(0),
    's2g kitti train dense': lambda: _s2g_train(0, bwd_trim=0),
    's2g kitti train weighted dense': lambda: _s2g_train(0, using_weight=1, bwd_trim=0),
    's2g ford train': lambda: _s2g_train(1),
    's2g ford train dense': lambda: _s2g_train(1, bwd_trim=0),
    's2g score_loss': lambda: _s2g_score_loss(),
    's2g score_loss dense': lambda: _s2g_score_loss(bwd_trim=0),
    's2g score_loss weighted dense': lambda: _s2g_score_loss(using_weight=1, bwd_trim=0),
    's2g forward_search': _s2g_search,
    'g2s geo train': lambda: _g2s_train(),
    'g2s geo train weighted': lambda: _g2s_train(using_weight=1),
    'g2s nn train': lambda: _g2s_train(proj='nn'),
    'g2s score_loss': lambda: _g2s_score_loss(),
    'g2s score_loss weighted': lambda: _g2s_score_loss(using_weight=1),
    'g2s corr train': _g2s_corr,
    'g2s forward_search': _g2s_search,
}


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_lists_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_launch_records(name, golden):
    got, want = CASES[name]()['records'], golden[name]['records']
    assert len(got) > 0
    assert [r[0] for r in got] == [r[0] for r in want], name
    if name.endswith('dense'):
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, k, g, w)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    res = {}
    for name in sorted(CASES):
        res[name] = CASES[name]()
        print(name, len(res[name]['records']), flush=True)
    with open(out, 'w') as f:
        f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(res.items())) + '\n}\n')
    print('wrote', out)
