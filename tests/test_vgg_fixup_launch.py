"""The fix-up pass of the satellite column trim as ONE launch (vgg_fixup_loop, hla_vgg_fixup with one_launch = 1) against the ten
gated conv launches + gated inv_norm it replaces (one_launch = 0) and against the untrimmed forward.  Every comparison is bitwise.

Shapes
  Satellite 3 x 256 x 256, the smallest image that leaves a column with first_col32 = 1: two tile columns at H/4, the left one fixed
  up (three of four at H/2, four of eight for conv0 + conv2).  B = 3, gate (1, 0, 1); bf16 and fp16 activations, fp32 and fp16 raw
  maps.  At this size every gated launch but the feature layers' takes the 4-row kernels of the small-grid side, the loop always
  the 8-row ones: the comparison also holds the two tile heights to the same bits.
  The model: LM_S2GP, B = 6, satellite 256, ground 64 x 256, five samples started at shift_u = -2 (outside the reach, asserted on
  last_reach_flag), one at shift_u = +1 with damping 100 (inside): args.fixup_one_launch 1 against 0 and against sat_reach_crop 0.
Buffers come NaN-filled from VGG._alloc, so nothing unwritten can pass for a computed value.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, HW, GATE = 3, (256, 256), (1, 0, 1)
CASES = [('bf16', True), ('bf16', False), ('fp16', True), ('fp16', False)]


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    """Bitwise (NaN-safe) equality of two tensors."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


def _nan_alloc(*shape, dtype, device):
    t = torch.empty(*shape, dtype=dtype, device=device)
    t.view(torch.uint8).fill_(0xFF)          # all-ones bytes: a NaN in fp32, fp16 and bf16
    return t


_NETS = {}


def _net(precision):
    if precision not in _NETS:
        from oracle import ref_cpu as O
        from highlyaccurate_amd.VGG import VGGUnet
        net = VGGUnet(3, precision=precision)
        net.load_state_dict(O.synth_vgg_state(np.random.RandomState(5), bias_scale=0.05))
        _NETS[precision] = net.to(_dev())
    return _NETS[precision]


_FULL = {}


def _full(precision, feat16):
    """The image and the untrimmed forward's maps and inv_norm: computed once per case, never written to."""
    key = (precision, feat16)
    if key not in _FULL:
        from highlyaccurate_amd import VGG
        g = torch.Generator(device=_dev())
        g.manual_seed(91)
        x = torch.rand(B, 3, *HW, device=_dev(), generator=g)
        feats, _, inv = VGG.vgg_forward_nhwc(_net(precision), x, want_conf=False, defer_norm=True, feat16=feat16)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(f.float()).all()) for f in feats) and bool(torch.isfinite(inv).all())
        _FULL[key] = (x, feats, inv)
    return _FULL[key]


def _fixed_up(precision, feat16, gate, one_launch, monkeypatch):
    """A trimmed forward into NaN-filled buffers, then the fix-up pass: (maps, inv_norm, workspace) before and after."""
    from highlyaccurate_amd import VGG
    x = _full(precision, feat16)[0]
    monkeypatch.setattr(VGG, '_alloc', _nan_alloc)
    state = {}
    feats, _, inv = VGG.vgg_forward_nhwc(_net(precision), x, want_conf=False, defer_norm=True, feat16=feat16, first_col32=1,
                                         col_state=state)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert state['first_col32'] == 1
    before = [f.clone() for f in feats], inv.clone(), state['ws'].clone()
    VGG.vgg_fixup_nhwc(state, torch.tensor(gate, dtype=torch.int32, device=_dev()), one_launch=one_launch)
    torch.cuda.synchronize()
    return before, (feats, inv, state['ws'])


@pytest.mark.parametrize('precision,feat16', CASES)
def test_one_launch_against_ten_launches_and_the_full_forward(precision, feat16, monkeypatch):
    _, full, full_inv = _full(precision, feat16)
    before, (maps, inv, ws) = _fixed_up(precision, feat16, GATE, True, monkeypatch)
    before10, (maps10, inv10, ws10) = _fixed_up(precision, feat16, GATE, False, monkeypatch)
    assert all(_same(a, b) for a, b in zip(before[0], before10[0])) and _same(before[1], before10[1]) and _same(before[2], before10[2])
    for l in range(3):
        assert bool(torch.isnan(before[0][l][:, :, :16 << l].float()).all()), (precision, l)      # the strip the fix-up has to fill
        for b in range(B):
            if GATE[b]:      # the gated samples: every column is the untrimmed forward's and the ten-launch pass's
                assert _same(maps[l][b], full[l][b]), (precision, feat16, l, b)
                assert _same(maps[l][b], maps10[l][b]), (precision, feat16, l, b)
            else:            # the other: what it was
                assert _same(maps[l][b], before[0][l][b]), (precision, feat16, l, b)
    for b in range(B):
        want = full_inv if GATE[b] else before[1]
        assert _same(inv[:, b], want[:, b]) and _same(inv[:, b], inv10[:, b]), (precision, feat16, b)
    assert not _same(before[1][:, 0], full_inv[:, 0])      # (the first pass's norm covered fewer columns)
    # the workspace (every layer's activations, the sum-of-squares slots): byte for byte what the ten launches leave
    assert _same(ws, ws10), (precision, feat16)


@pytest.mark.parametrize('precision,feat16', [('bf16', True), ('fp16', False)])
def test_ungated_sample_rows_are_not_written(precision, feat16, monkeypatch):
    """The workspace bytes the pass changes under gate (1, 0, 1) and under (0, 1, 0) are disjoint, and together they are the bytes
    it changes under (1, 1, 1): a workgroup writes its own sample's rows only (the NaN fill makes every strip byte count)."""
    def changed(gate):
        before, (maps, inv, ws) = _fixed_up(precision, feat16, gate, True, monkeypatch)
        return _bytes(ws) != _bytes(before[2]), maps, inv, before
    c101, *_ = changed((1, 0, 1))
    c010, maps, inv, before = changed((0, 1, 0))
    c111, *_ = changed((1, 1, 1))
    assert bool(c101.any()) and bool(c010.any())
    assert not bool((c101 & c010).any())
    assert torch.equal(c101 | c010, c111)
    _, full, full_inv = _full(precision, feat16)
    for l in range(3):
        assert _same(maps[l][1], full[l][1]) and _same(maps[l][0::2], before[0][l][0::2]), l
    assert _same(inv[:, 1], full_inv[:, 1]) and _same(inv[:, 0::2], before[1][:, 0::2])


@pytest.mark.parametrize('precision,feat16', CASES)
def test_gate_extremes(precision, feat16, monkeypatch):
    _, full, full_inv = _full(precision, feat16)
    _, (maps, inv, _) = _fixed_up(precision, feat16, (1, 1, 1), True, monkeypatch)
    assert all(_same(a, b) for a, b in zip(maps, full)) and _same(inv, full_inv), (precision, feat16)
    before, (maps, inv, ws) = _fixed_up(precision, feat16, (0, 0, 0), True, monkeypatch)      # none gated: nothing is written
    assert all(_same(a, b) for a, b in zip(maps, before[0])) and _same(inv, before[1]) and _same(ws, before[2]), (precision, feat16)


def _localise(precision, sat, grd, pose, crop, one_launch):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    args = O.default_args(precision=precision, sat_reach_crop=crop, fixup_one_launch=one_launch, damping=100.0, N_iters=2)
    net = LM_S2GP(args)
    net.load_state_dict(O.synth_model_state(7, rotation_range=args.rotation_range))
    net.keep_normal_eq = True
    net = net.to(_dev())
    if crop:      # (at satellite 256 the model's own trim is 0 -- the camera sits left of the first promised column: tests/test_sat_reach_gpu.py)
        net.sat_first_col32 = lambda A, H, W: 1
    torch.manual_seed(3)
    np.random.seed(3)
    with torch.no_grad():
        res = net(sat, grd, mode='test', init_pose=pose)
    torch.cuda.synchronize()
    flag = None if net.last_reach_flag is None else net.last_reach_flag.cpu().tolist()
    return dict(trace=net.last_trace.clone(), neq=net.last_normal_eq.clone(), res=[r.clone() for r in res if torch.is_tensor(r)], flag=flag)


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_through_the_model(precision):
    from oracle import ref_cpu as O
    n = 6
    sat, grd, _, _, _ = O.synth_images(431, n, grd_hw=(64, 256), sat_a=256)
    sat, grd = sat.to(_dev()), grd.to(_dev())
    pose = torch.tensor([[-2.0, 0.0, 0.0]] * n, dtype=torch.float32)
    pose[3] = torch.tensor([1.0, 0.0, 0.0])
    want_flag = [0 if b == 3 else 1 for b in range(n)]
    one = _localise(precision, sat, grd, pose, 1, 1)
    ten = _localise(precision, sat, grd, pose, 1, 0)
    ref = _localise(precision, sat, grd, pose, 0, 1)
    assert one['flag'] == want_flag and ten['flag'] == want_flag and ref['flag'] is None, (one['flag'], ten['flag'])
    for k in ('trace', 'neq'):
        assert bool(torch.isfinite(one[k]).all()), k
    assert _same(one['trace'], ten['trace']) and _same(one['neq'], ten['neq'])
    assert len(one['res']) == len(ten['res']) and all(_same(a, b) for a, b in zip(one['res'], ten['res']))
    for b in range(n):
        if want_flag[b]:      # a flagged sample ends with the whole-map run's trace, normal equations and poses
            assert _same(one['trace'][b], ref['trace'][b]), b
            assert _same(one['neq'][:, b], ref['neq'][:, b]), b
            assert all(_same(a[b], r[b]) for a, r in zip(one['res'], ref['res']) if a.dim() and a.shape[0] == n), b
