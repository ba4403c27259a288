"""The forward LM loop on stream groups (lm_solve.hip): a batch of HLA_LM_SPLIT_MIN = 16 samples or more runs as two sample
ranges, each a chain of launches on its own stream, forked from and joined on the caller's stream.  Nothing about a sample's
pose may depend on that: every comparison here is bitwise.

The serial loop (one group on the caller's stream) is what the library runs while its event profiler is on, so the same call
made under ``prof_enable(True)`` is the reference.  B = 24 splits into 16 + 8 samples, B = 19 (no multiple of 8) into 16 + 3:
the smallest batches above the threshold with unequal groups.  Shapes are the smallest with several tiles per sample on the finest
level (grd 64x256, sat 128: 4 / 2 / 1 tiles); N_iters = 2 gives six steps over three levels with three different tile counts.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRD_HW, SAT_A, CS = (64, 256), 128, (256, 128, 64)
BATCHES = (24, 19)
GROUP0 = 16          # samples [0, 16) are group 0 at both batch sizes


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


_PYRAMIDS = {}


def _pyramid(B):
    """Random NHWC fp32 feature pyramids + confidence maps on the device: made once per batch size and never written to."""
    if B not in _PYRAMIDS:
        d = _dev()
        g = torch.Generator(device=d)
        g.manual_seed(100 + B)
        sat, grd, conf = [], [], []
        for l in range(3):
            A = SAT_A >> (2 - l)
            h, w = GRD_HW[0] >> (3 - l), GRD_HW[1] >> (3 - l)
            sat.append(torch.randn(B, A, A, CS[l], device=d, generator=g))
            grd.append(torch.randn(B, h, w, CS[l], device=d, generator=g))
            conf.append(torch.rand(B, h, w, device=d, generator=g) * 0.23 + 0.27)
        _PYRAMIDS[B] = (sat, grd, conf)
    return _PYRAMIDS[B]


def _ford_extra(B):
    """Per-sample R_FL / T_FL: the usual axis permutation turned by a different small yaw for every sample."""
    rs = np.random.RandomState(9)
    P = np.array([[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]])
    R = []
    for a in rs.uniform(-0.2, 0.2, size=B):
        c, s = np.cos(a), np.sin(a)
        R.append(np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]]) @ P)
    T = np.array([1.7, 0.3, -1.2]) + rs.uniform(-0.3, 0.3, size=(B, 3))
    return dict(R_FL=torch.from_numpy(np.stack(R)).float(), T_FL=torch.from_numpy(T).float(), side_m=112.64)


def _net(ford=False, strict=False, **kw):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    args = O.default_args(**{'N_iters': 2, 'damping': 1.0, **kw})
    if strict:
        args.strict_errors = 1
    return (LM_S2GP_Ford if ford else LM_S2GP)(args).to(_dev())


def _solve(net, feats, serial, level_first=0, init_pose=None, extra=None, seed=0):
    """One lm_solve under fixed torch / numpy seeds -> (trace, normal_eq), both cloned.  serial: with the event profiler on."""
    from highlyaccurate_amd import _lib
    sat, grd, conf = feats
    torch.manual_seed(seed)
    np.random.seed(seed)
    if serial:
        _lib.prof_enable(True)
    try:
        trace = net.lm_solve(sat, grd, conf, GRD_HW, extra, level_first, init_pose=init_pose, keep_normal_eq=True)
    finally:
        if serial:
            recs = _lib.prof_fetch()
            _lib.prof_enable(False)
            assert len([r for r in recs if r[0].startswith('lm_accum')]) == 6, recs     # one launch per step: the serial loop
    return trace.clone(), net.last_normal_eq.clone()


def _same(a, b):
    """Bitwise (NaN-safe) equality of two tensors."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _start_poses(B, seed=4, lim=0.3):
    return torch.from_numpy(np.random.RandomState(seed).uniform(-lim, lim, size=(B, 3)).astype(np.float32))


CASES = {
    'default': dict(),
    'using_weight': dict(kw=dict(using_weight=1)),
    'dropout': dict(kw=dict(dropout=1)),
    'level_first': dict(level_first=1),
    'ford': dict(ford=True),
    'init_pose': dict(init=True),
    'feat16': dict(half=True),
}


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('case', list(CASES))
def test_split_equals_serial(case, B):
    """The pose trace and the normal equations of every step are the same bits from the split loop and from the serial one;
    with args.strict_errors the in-view counts (normal_eq[..., 14], one more launch per step and group) are too."""
    c = CASES[case]
    sat, grd, conf = _pyramid(B)
    if c.get('half'):
        sat, grd = [t.half() for t in sat], [t.half() for t in grd]
    extra = _ford_extra(B) if c.get('ford') else None
    init = _start_poses(B) if c.get('init') else None
    for strict in (False, True):
        net = _net(ford=bool(c.get('ford')), strict=strict, **c.get('kw', {}))
        run = lambda serial: _solve(net, (sat, grd, conf), serial, c.get('level_first', 0), init, extra)
        tr_split, ne_split = run(False)
        tr_serial, ne_serial = run(True)
        assert torch.isfinite(tr_serial).all()
        assert _same(tr_split, tr_serial), (case, B, strict, (tr_split != tr_serial).nonzero()[:4])
        assert _same(ne_split, ne_serial), (case, B, strict)
        if strict:
            assert (ne_serial[:, :, 14] > 0).all()          # the counts were made, for the samples of both groups


@pytest.mark.parametrize('B', BATCHES)
def test_reinit_indexing_across_groups(B):
    """rand_uv is [steps, 2, B]: its second row keeps the whole batch as stride whatever range a launch covers.  Samples of
    both groups start so far outside the map that no pixel is in view: the step leaves the pose where it is, the +-2.5 rule
    fires, and the trace must hold exactly the values draw_reinit draws under the same seed -- u for some samples, v for others."""
    from highlyaccurate_amd._s2gp import draw_reinit
    feats = _pyramid(B)
    far_u, far_v = [1, GROUP0 - 1, GROUP0, B - 1], [5, GROUP0 + 1]
    p0 = _start_poses(B)
    p0[far_u, 0] = 50.0
    p0[far_v, 1] = -50.0
    net = _net()
    tr_split, ne_split = _solve(net, feats, False, init_pose=p0)
    tr_serial, ne_serial = _solve(net, feats, True, init_pose=p0)
    torch.manual_seed(0)
    rand = draw_reinit(6, B, 'cpu')                          # [steps, 2, B]; step 0 is (iteration 0, level 0)
    t0 = tr_split[:, 0, 0].cpu()
    for b in far_u:
        assert t0[b, 0] == rand[0, 0, b], (b, t0[b], rand[0, :, b])
    for b in far_v:
        assert t0[b, 1] == rand[0, 1, b], (b, t0[b], rand[0, :, b])
    untouched = [b for b in range(B) if b not in far_u]
    assert not (t0[untouched, 0] == rand[0, 0, untouched]).any()
    assert _same(tr_split, tr_serial) and _same(ne_split, ne_serial)


@pytest.mark.parametrize('B', BATCHES)
def test_batch_independence_through_split(B):
    """Samples of both groups, run alone (B = 1: serial loop, no XCD-affine map), give bitwise the trace rows they have in the
    split batch.  Damping 10 keeps the steps small: no re-initialisation fires (a lone sample would draw other values)."""
    from highlyaccurate_amd._s2gp import draw_reinit
    sat, grd, conf = _pyramid(B)
    p0 = _start_poses(B, lim=0.1)
    net = _net(damping=10.0)
    trace, _ = _solve(net, (sat, grd, conf), False, init_pose=p0)
    torch.manual_seed(0)
    rand = draw_reinit(6, B, 'cpu').reshape(2, 3, 2, B).permute(3, 0, 1, 2)       # [B, iteration, level, (u, v)]
    assert not (trace[..., :2].cpu() == rand).any(), 're-initialisation fired: the lone runs are not comparable'
    for b in (0, GROUP0 - 1, GROUP0, B - 1):
        one = lambda ts: [t[b:b + 1].contiguous() for t in ts]
        alone, _ = _solve(net, (one(sat), one(grd), one(conf)), False, init_pose=p0[b:b + 1])
        assert _same(alone[0], trace[b]), (b, alone[0], trace[b])


@pytest.mark.parametrize('side', [False, True])
def test_caller_stream_orders_the_loop(side):
    """After the call the caller's stream alone orders everything the loop launched: a kernel enqueued on it right away that
    overwrites the feature maps changes nothing.  Also from a non-default torch stream."""
    B = BATCHES[0]
    sat, grd, conf = _pyramid(B)
    net = _net()
    ref, _ = _solve(net, (sat, grd, conf), True)
    torch.cuda.synchronize()
    sat2, grd2 = [t.clone() for t in sat], [t.clone() for t in grd]
    cur = torch.cuda.current_stream()
    st = torch.cuda.Stream() if side else cur
    st.wait_stream(cur)
    with torch.cuda.stream(st):
        torch.manual_seed(0)
        np.random.seed(0)
        trace = net.lm_solve(sat2, grd2, conf, GRD_HW, None, 0)
        for t in sat2 + grd2:
            t.fill_(float('nan'))
        out = trace.clone()
    cur.wait_stream(st)
    torch.cuda.synchronize()
    assert _same(out, ref)
