"""args.sat_reach_crop on the GPU: the satellite extractor started at a tile column (hla_vgg_forward_cols, first_col32), the LM
loop's detection of a pose that leaves the reach, and the exact per-sample fallback.  Every map comparison is bitwise.

Maps
  B = 2, 3 x 64 x 256 (maps 8 x 32, 16 x 64, 32 x 128: two tile columns at H/4; every layer but the feature layers takes the 4-row
  kernels of the small-grid side) in bf16 / fp32 / fp16x3, and B = 8, 3 x 128 x 512 in bf16 (conv0 + conv2, conv5, conv7 and the
  dec2 layers stay above CONV_SMALL_GRID also when trimmed: the 8-row kernels).  first_col32 = 1 against the full forward: the
  promised columns; the fix-up pass for one sample of the batch: that sample's whole maps and inv_norm, the other untouched; NaN
  pre-filled buffers; the pair entry with first_row8 on the ground segment against the two plain forwards.
  Beyond c = 1 (tests/sat_reach_cases.py, TRIM_CASES): c = 1 / 2 / 3 at widths 512, 264, 296 and 392 (ragged last tiles at all three
  resolutions), B = 2 / 9 / 8, bf16 and fp16 with fp16 feature maps, fp32, bf16 with fp32 raw maps: the promised columns, the
  untouched strip, inv_norm of the trimmed and of the full forward against an fp64 sum over the stored maps (gates 1e-4 for fp32
  maps, 2^-9 for fp16 maps: tests/sat_reach_cases.py), the fix-up pass under the gate patterns none / all / alternating / one
  of two, twice; the calls outside the trim's scope (level 4, confidence heads, save_for_backward, fp16x3) and its argument
  errors; the pair entry at c = 2.
Loop
  LM_S2GP.forward(mode='test') with sat_reach_crop 1 against 0.  At sat 512 / grd 256 x 1024 the trim is the one the model derives
  (c = 1).  At sat 256 / grd 128 x 512 (B = 2 and B = 16, both stream groups) no pose range gives c >= 1 -- the camera sits at
  column 16 of the 32-wide x15, left of the first promised column 18 -- so there the model's own c is replaced by 1 and the start
  poses decide: shift_u = +1 with damping 100 keeps a sample inside the reach (its smallest tap columns are 24 / 48 / 97 against
  the promised 18 / 38 / 78), shift_u = -2 puts it outside (5 / 10 / 20).
  Trace tolerance of an unflagged sample against sat_reach_crop = 0: 2e-6, the gate of test_dead_ground_rows_elimination_is_exact
  for the same cancelling L2_norm scale (inv_norm covers fewer columns).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sat_reach_cases as SC

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _same(a, b):
    """Bitwise (NaN-safe) equality of two tensors."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


_NETS = {}


def _nets(precision):
    if precision not in _NETS:
        from oracle import ref_cpu as O
        from highlyaccurate_amd.VGG import VGGUnet
        nets = []
        for seed in (5, 6):
            net = VGGUnet(3, precision=precision)
            net.load_state_dict(O.synth_vgg_state(np.random.RandomState(seed), bias_scale=0.05))
            nets.append(net.to(_dev()))
        _NETS[precision] = tuple(nets)
    return _NETS[precision]


def _image(B, hw, seed):
    g = torch.Generator(device=_dev())
    g.manual_seed(seed)
    return torch.rand(B, 3, *hw, device=_dev(), generator=g)


def _nan_alloc(*shape, dtype, device):
    t = torch.empty(*shape, dtype=dtype, device=device)
    t.view(torch.uint8).fill_(0xFF)          # all-ones bytes: a NaN in fp32, fp16 and bf16
    return t


MAP_CASES = [('bf16', 2, (64, 256)), ('fp32', 2, (64, 256)), ('fp16x3', 2, (64, 256)), ('bf16', 8, (128, 512))]


@pytest.mark.parametrize('precision,B,hw', MAP_CASES)
def test_trimmed_maps_and_fixup(precision, B, hw, monkeypatch):
    from highlyaccurate_amd import VGG
    net = _nets(precision)[0]
    x = _image(B, hw, 77)
    f16 = precision == 'bf16'
    kw = dict(want_conf=False, defer_norm=True, feat16=f16)
    full, _, full_inv = VGG.vgg_forward_nhwc(net, x, **kw)
    cols = VGG.promised_cols(1)
    monkeypatch.setattr(VGG, '_alloc', _nan_alloc)
    state = {}
    trim, _, trim_inv = VGG.vgg_forward_nhwc(net, x, first_col32=1, col_state=state, **kw)
    monkeypatch.undo()
    torch.cuda.synchronize()
    for l in range(3):
        assert torch.isfinite(full[l].float()).all()
        assert _same(trim[l][:, :, cols[l]:], full[l][:, :, cols[l]:]), (precision, l)
        if precision != 'fp16x3':      # (split mode computes every column: include/hla.h)
            assert torch.isnan(trim[l][:, :, :16 << l].float()).all(), (precision, l)          # the skipped strip was never written
            assert torch.isfinite(trim[l][:, :, 16 << l:].float()).all(), (precision, l)       # and no NaN came in from it
    assert torch.isfinite(trim_inv).all()
    before = [t.clone() for t in trim], trim_inv.clone()
    gate = torch.zeros(B, dtype=torch.int32, device=_dev())
    gate[0] = 1
    VGG.vgg_fixup_nhwc(state, gate)
    torch.cuda.synchronize()
    for l in range(3):
        assert _same(trim[l][0], full[l][0]), (precision, l)                 # the gated sample: the full forward's maps
        assert _same(trim[l][1:], before[0][l][1:]), (precision, l)          # the others: not touched
    assert _same(trim_inv[:, 0], full_inv[:, 0]) and _same(trim_inv[:, 1:], before[1][:, 1:])
    if precision != 'fp16x3':
        assert not _same(before[1][:, 0], full_inv[:, 0])                    # (the first pass's norm covered fewer columns)


@pytest.mark.parametrize('precision,B,hw', [('bf16', 2, (64, 256)), ('fp32', 2, (64, 256)), ('fp16x3', 2, (64, 256)),
                                            ('bf16', 8, (128, 512))])
def test_pair_entry_with_both_trims(precision, B, hw):
    """The satellite segment starts at tile column 1 while the ground segment starts at row first_row8 = 4."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc, vgg_forward_pair_nhwc, promised_cols
    nets = _nets(precision)
    xs = (_image(B, hw, 78), _image(B, (64, 128), 79))
    f16 = precision == 'bf16'
    kw = dict(want_conf=False, defer_norm=True, feat16=f16)
    full = vgg_forward_nhwc(nets[0], xs[0], **kw)
    plain = [vgg_forward_nhwc(nets[0], xs[0], first_col32=1, **kw), vgg_forward_nhwc(nets[1], xs[1], first_row8=4, **kw)]
    p0, p1, _ = vgg_forward_pair_nhwc(nets, xs, first_row8=(0, 4), feat16=f16, first_col32=(1, 0))
    torch.cuda.synchronize()
    cols = promised_cols(1)
    skip = 0 if precision == 'fp16x3' else 1
    for l in range(3):
        assert _same(p0[0][l][:, :, cols[l]:], full[0][l][:, :, cols[l]:]), (precision, l)
        assert _same(p0[0][l][:, :, (16 << l) * skip:], plain[0][0][l][:, :, (16 << l) * skip:]), (precision, l)
        assert _same(p1[0][l][:, 4 << l:], plain[1][0][l][:, 4 << l:]), (precision, l)
    assert _same(p0[1], plain[0][2]) and _same(p1[1], plain[1][2])


# ----------------------------------------------------------------------------------------------------------------------
# beyond c = 1
# ----------------------------------------------------------------------------------------------------------------------
def _is_fill(t):
    """Every byte still the 0xFF of _nan_alloc."""
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _inv_against_fp64(tag, maps, inv, first, tol):
    """inv[l, b] * sqrt(sum over columns >= first[l] of map^2) = 1 within tol, the sum in fp64 over the maps as stored."""
    worst = 0.0
    for l in range(3):
        m = maps[l][:, :, first[l]:].double()
        assert bool(torch.isfinite(m).all()), (tag, l)
        sq = m * m
        ss = sq.sum((1, 2, 3))
        if maps[l].dtype == torch.float16:      # the gate's premise: no saturated element, and the subnormal ones carry no weight
            assert float(m.abs().max()) < 65504.0, (tag, l)
            assert bool(((sq * (m.abs() < 2.0 ** -14)).sum((1, 2, 3)) <= 2.0 ** -11 * ss).all()), (tag, l)
        worst = max(worst, float((inv[l] * ss.sqrt() - 1.0).abs().max()))
    print(f'SATREACH inv_norm {tag}: worst |inv * sqrt(sum map^2) - 1| = {worst:.2e} (limit {tol:.2e})')
    assert worst <= tol, (tag, worst, tol)
    return worst


def _gate_patterns(B):
    alt = [b % 2 for b in range(B)]
    return {2: [[1, 0]], 8: [alt], 9: [[0] * B, [1] * B, alt]}[B]


def _trimmed(VGG, net, x, c, kw, monkeypatch):
    monkeypatch.setattr(VGG, '_alloc', _nan_alloc)
    state = {}
    out = VGG.vgg_forward_nhwc(net, x, first_col32=c, col_state=state, **kw)
    monkeypatch.undo()
    torch.cuda.synchronize()
    return out, state


@pytest.mark.parametrize('precision,feat16,B,H,W,c', SC.TRIM_CASES)
def test_trim_and_fixup_beyond_the_first_tile_column(precision, feat16, B, H, W, c, monkeypatch):
    from highlyaccurate_amd import VGG
    net = _nets(precision)[0]
    x = _image(B, (H, W), 80 + c)
    kw = dict(want_conf=False, defer_norm=True, feat16=feat16)
    tol = SC.tol_inv(feat16)
    tag = f'{precision} feat16 {int(feat16)} B{B} {H}x{W} c{c}'
    assert max(SC.slot_counts(H, W)) <= SC.MAX_SLOTS      # a lost or stale slot is 1 / slots of the sum or more: above the gate
    full, _, full_inv = VGG.vgg_forward_nhwc(net, x, **kw)
    cols, strip = VGG.promised_cols(c), SC.strip_cols(c)
    _inv_against_fp64(tag + ' full', full, full_inv, (0, 0, 0), tol)
    for n, pattern in enumerate(_gate_patterns(B)):
        (trim, _, trim_inv), state = _trimmed(VGG, net, x, c, kw, monkeypatch)
        if n == 0:
            for l in range(3):
                # (W = 264, c = 2 and W = 392, c = 3: the promised columns lie beyond the map and this comparison is empty; there the
                # strip, inv_norm and fix-up checks are what bite)
                assert _same(trim[l][:, :, cols[l]:], full[l][:, :, cols[l]:]), (tag, l)
                assert strip[l] < trim[l].shape[2]
                assert _is_fill(trim[l][:, :, :strip[l]]), (tag, l)                               # the strip: never written
                assert bool(torch.isfinite(trim[l][:, :, strip[l]:].float()).all()), (tag, l)    # and nothing came in from it
            _inv_against_fp64(tag + ' trimmed', trim, trim_inv, strip, tol)
        before = [t.clone() for t in trim], trim_inv.clone(), state['ws'].clone()
        gate = torch.tensor(pattern, dtype=torch.int32, device=_dev())
        VGG.vgg_fixup_nhwc(state, gate)
        torch.cuda.synchronize()
        for b in range(B):
            want = (full, full_inv) if pattern[b] else (before[0], before[1])        # gated: the full forward's; else untouched
            for l in range(3):
                assert _same(trim[l][b], want[0][l][b]), (tag, pattern, b, l)
            assert _same(trim_inv[:, b], want[1][:, b]), (tag, pattern, b)
        if not any(pattern):
            assert _same(state['ws'], before[2]), (tag, 'an all-zero gate wrote to the workspace')
        again = [t.clone() for t in trim], trim_inv.clone()
        VGG.vgg_fixup_nhwc(state, gate)
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(trim, again[0])) and _same(trim_inv, again[1]), (tag, pattern, 'second fix-up')


@pytest.mark.parametrize('what', ['level4', 'want_conf', 'save_for_backward', 'fp16x3'])
def test_trim_outside_its_scope_computes_every_column(what, monkeypatch):
    """vgg_first_col32 (csrc/vgg.hip): with level 4, the confidence heads, save_for_backward or fp16x3 a first_col32 > 0 call is the
    plain forward, bit for bit, no byte of the NaN fill is left in a map, and its fix-up pass has nothing to do."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd import VGG
    if what == 'level4':
        net = VGG.VGGUnet(4, precision='fp32')
        net.load_state_dict(O.synth_vgg_state(np.random.RandomState(5), bias_scale=0.05))
        net = net.to(_dev())
    else:
        net = _nets('fp16x3' if what == 'fp16x3' else 'fp32')[0]
    x = _image(2, (64, 256), 81)
    kw = dict(want_conf=what == 'want_conf', defer_norm=True, save_for_backward=what == 'save_for_backward')
    plain = VGG.vgg_forward_nhwc(net, x, **kw)
    got, state = _trimmed(VGG, net, x, 1, kw, monkeypatch)
    assert len(got[0]) == len(plain[0]) == (4 if what == 'level4' else 3)

    def check():
        for l, (a, b) in enumerate(zip(got[0], plain[0])):
            if l == 3:      # x24: the 16 real channels of the 64 stored
                a, b = a[..., :16], b[..., :16]
            assert bool(torch.isfinite(a).all()) and _same(a, b), (what, l)
        assert _same(got[2], plain[2])
        if what == 'want_conf':
            assert all(_same(a, b) for a, b in zip(got[1], plain[1]))
    check()
    VGG.vgg_fixup_nhwc(state, torch.ones(2, dtype=torch.int32, device=_dev()))
    torch.cuda.synchronize()
    check()


def _raw_cols_call(state, c, gate):
    """hla_vgg_forward_cols on the buffers of an earlier forward, as vgg_fixup_nhwc calls it, with any first_col32 / col_gate."""
    from highlyaccurate_amd import _lib
    s = state
    fp = (C.c_void_p * 4)(*([f.data_ptr() for f in s['feats']] + [0]))
    cp = (C.c_void_p * 4)(0, 0, 0, 0)
    return _lib.load().hla_vgg_forward_cols(_lib.ptr(s['x']), s['x_plane'], C.byref(s['prm']), _lib.ptr(s['packed']), fp, cp,
                                            _lib.ptr(s['inv_norm']), _lib.ptr(s['ws']), s['ws'].numel(), s['B'], s['H'], s['W'], 3, s['dt'],
                                            s['flags'], 0, c, _lib.ptr(gate), _lib.stream_ptr())


def test_trim_argument_errors():
    from highlyaccurate_amd import VGG, _lib
    net = _nets('fp32')[0]
    x = _image(2, (64, 256), 82)
    kw = dict(want_conf=False, defer_norm=True)
    for c in (2, 3, -1):                                   # 128 c >= W = 256
        with pytest.raises(ValueError, match='first_col32'):
            VGG.vgg_forward_nhwc(net, x, first_col32=c, **kw)
        with pytest.raises(ValueError, match='first_col32'):
            VGG.vgg_forward_pair_nhwc(_nets('fp32'), (x, _image(2, (64, 128), 83)), first_col32=(c, 0))
    state = {}
    feats, _, inv = VGG.vgg_forward_nhwc(net, x, first_col32=1, col_state=state, **kw)
    torch.cuda.synchronize()
    before = [t.clone() for t in feats], inv.clone()
    gate = torch.ones(2, dtype=torch.int32, device=_dev())
    # the C entry refuses the same, and a col_gate without a trim; nothing is launched
    for c, g, word in ((2, None, 'first_col32'), (-1, None, 'first_col32'), (0, gate, 'col_gate')):
        assert _raw_cols_call(state, c, g) != 0
        assert word in _lib.load().hla_last_error().decode()
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(feats, before[0])) and _same(inv, before[1])
    with pytest.raises(ValueError, match='gate'):
        VGG.vgg_fixup_nhwc(state, torch.ones(3, dtype=torch.int32, device=_dev()))


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_pair_entry_second_tile_column(precision):
    """first_col32 = (2, 0) with first_row8 = (0, 4) at W = 512: the checks of test_pair_entry_with_both_trims."""
    from highlyaccurate_amd.VGG import vgg_forward_nhwc, vgg_forward_pair_nhwc, promised_cols
    nets = _nets(precision)
    B, c = 2, 2
    xs = (_image(B, (64, 512), 84), _image(B, (64, 128), 85))
    f16 = precision == 'bf16'
    kw = dict(want_conf=False, defer_norm=True, feat16=f16)
    full = vgg_forward_nhwc(nets[0], xs[0], **kw)
    plain = [vgg_forward_nhwc(nets[0], xs[0], first_col32=c, **kw), vgg_forward_nhwc(nets[1], xs[1], first_row8=4, **kw)]
    p0, p1, _ = vgg_forward_pair_nhwc(nets, xs, first_row8=(0, 4), feat16=f16, first_col32=(c, 0))
    torch.cuda.synchronize()
    cols, strip = promised_cols(c), SC.strip_cols(c)
    for l in range(3):
        assert cols[l] < p0[0][l].shape[2]
        assert _same(p0[0][l][:, :, cols[l]:], full[0][l][:, :, cols[l]:]), (precision, l)
        assert _same(p0[0][l][:, :, strip[l]:], plain[0][0][l][:, :, strip[l]:]), (precision, l)
        assert _same(p1[0][l][:, 4 << l:], plain[1][0][l][:, 4 << l:]), (precision, l)
    assert _same(p0[1], plain[0][2]) and _same(p1[1], plain[1][2])
    _inv_against_fp64(f'pair {precision} c{c}', p0[0], p0[1], strip, SC.tol_inv(f16))


def _model(crop, damping, precision='bf16'):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    args = O.default_args(precision=precision, sat_reach_crop=crop, damping=damping, N_iters=2)
    net = LM_S2GP(args)
    net.load_state_dict(O.synth_model_state(7, rotation_range=args.rotation_range))
    net.keep_features = net.keep_normal_eq = True
    return net.to(_dev())


def _run(net, sat, grd, init_pose, force_c=None, nan=False, monkeypatch=None, level_first=0):
    from highlyaccurate_amd import VGG
    if force_c is not None and net.args.sat_reach_crop:
        net.sat_first_col32 = lambda A, H, W: force_c
    if nan:
        monkeypatch.setattr(VGG, '_alloc', _nan_alloc)
    torch.manual_seed(3)
    np.random.seed(3)
    with torch.no_grad():
        res = net(sat, grd, mode='test', init_pose=init_pose, level_first=level_first)
    if nan:
        monkeypatch.undo()
    torch.cuda.synchronize()
    flag = None if net.last_reach_flag is None else net.last_reach_flag.cpu().tolist()
    return dict(trace=net.last_trace.clone(), neq=net.last_normal_eq.clone(), res=[r.clone() for r in res], flag=flag,
                sat=[t.clone() for t in net.last_features[0]], inv=net.last_features[1].clone())


def _check_reach(B, sat_a, grd_hw, inside, outside, damping, force_c, monkeypatch, level_first=0):
    from oracle import ref_cpu as O
    from highlyaccurate_amd.VGG import promised_cols
    sat, grd, _, _, _ = O.synth_images(400 + B, B, grd_hw=grd_hw, sat_a=sat_a)
    sat, grd = sat.to(_dev()), grd.to(_dev())
    pose_in = torch.tensor([inside] * B, dtype=torch.float32)
    pose_mix = pose_in.clone()
    out_b = [0] if B == 2 else [1, B - 2]              # (B = 16: one sample of either stream group)
    for b in out_b:
        pose_mix[b] = torch.tensor(outside)
    cols = promised_cols(1)
    lf = dict(level_first=level_first)
    ref_in = _run(_model(0, damping), sat, grd, pose_in, **lf)
    ref_mix = _run(_model(0, damping), sat, grd, pose_mix, **lf)
    assert ref_in['flag'] is None
    got_in = _run(_model(1, damping), sat, grd, pose_in, force_c, nan=True, monkeypatch=monkeypatch, **lf)
    got_mix = _run(_model(1, damping), sat, grd, pose_mix, force_c, **lf)
    # all inside: nothing is flagged, the promised columns are the full maps', the trace is the full run's up to the norm's rounding
    assert got_in['flag'] == [0] * B, got_in['flag']
    for l in range(3):
        assert _same(got_in['sat'][l][:, :, cols[l]:], ref_in['sat'][l][:, :, cols[l]:]), l
    for k in ('trace', 'neq', 'inv'):
        assert torch.isfinite(got_in[k]).all(), k                  # (on NaN pre-filled buffers)
    assert all(torch.isfinite(r).all() for r in got_in['res'])
    err = (got_in['trace'] - ref_in['trace']).abs().max().item()
    print(f'B = {B}, sat {sat_a}: max |trace(crop) - trace(full)| of the unflagged samples = {err:.3e}')
    assert err <= 2e-6, err
    # mixed: exactly the samples started outside are flagged ...
    assert got_mix['flag'] == [1 if b in out_b else 0 for b in range(B)], got_mix['flag']
    for b in range(B):
        if b in out_b:      # ... they end with the full run's maps, norms, trace and normal equations, bit for bit
            for l in range(3):
                assert _same(got_mix['sat'][l][b], ref_mix['sat'][l][b]), (b, l)
            assert _same(got_mix['inv'][:, b], ref_mix['inv'][:, b]), b
            assert _same(got_mix['trace'][b], ref_mix['trace'][b]), (b, got_mix['trace'][b], ref_mix['trace'][b])
            assert _same(got_mix['neq'][:, b], ref_mix['neq'][:, b]), b
        else:               # ... and their batch mates with what they have in the all-inside run, bit for bit
            assert _same(got_mix['trace'][b], got_in['trace'][b]), b
            assert _same(got_mix['neq'][:, b], got_in['neq'][:, b]), b
            for l in range(3):
                assert _same(got_mix['sat'][l][b][:, cols[l]:], got_in['sat'][l][b][:, cols[l]:]), (b, l)


@pytest.mark.parametrize('B', [2, 16])
def test_detection_and_fallback_sat256(B, monkeypatch):
    _check_reach(B, 256, (128, 512), inside=[1.0, 0.0, 0.0], outside=[-2.0, 0.0, 0.0], damping=100.0, force_c=1, monkeypatch=monkeypatch)


def test_detection_and_fallback_sat256_level_first(monkeypatch):
    """The level-first loop order (all iterations of a level before the next level)."""
    _check_reach(2, 256, (128, 512), inside=[1.0, 0.0, 0.0], outside=[-2.0, 0.0, 0.0], damping=100.0, force_c=1, monkeypatch=monkeypatch,
                 level_first=1)


def test_detection_and_fallback_kitti_shape(monkeypatch):
    """The model's own c (= 1) at the KITTI shape: pose 0 is inside the reach, shift_u = -2 is not."""
    from oracle import ref_cpu as O
    from highlyaccurate_amd.models_kitti import LM_S2GP
    assert LM_S2GP(O.default_args()).sat_first_col32(512, 256, 1024) == 1
    _check_reach(2, 512, (256, 1024), inside=[0.0, 0.0, 0.0], outside=[-2.0, 0.0, 0.0], damping=100.0, force_c=None, monkeypatch=monkeypatch)
