"""Paired extractor launches (hla_vgg_forward_pair): in inference every convolution layer of the satellite and the ground
extractor runs as ONE launch of two segments.  A workgroup of such a launch finds its tile, its XCD-contiguous position and its
sum-of-squares slot from its segment-local id, so nothing a sample's maps hold may depend on it: every comparison here is bitwise,
against the two plain forwards (vgg_forward_nhwc) on the same seeded images and weights.

A  B = 2, sat 64x64, grd 64x128 with first_row8 = 4: the ground segment starts at odd rows inside (conv5 at row 1, conv12 at 3)
   while the satellite one starts at 0; all four precisions.  Every layer but the three feature layers takes the 4-row kernels.
B  B = 9 (the XCD-affine map with a batch that is no multiple of 8), sat 72x72, grd 80x136: partial tiles in x and in y, and the
   two segments' grids differ in every layer; bf16 and fp16x3.
C  B = 4, sat 64x64, grd 256x512: conv5 / conv7 of the ground image are 512 workgroups (8-row kernels), the satellite's 16
   (4-row kernels): different instantiations, so the entry must run the two plain forwards -- and still return the same bits.
E  B = 16, sat 256x256, grd 128x512 with first_row8 = 5: both segments of conv5, conv7, conv10, conv12, dec2.1 are 512-1024
   workgroups, so the 8-row pair kernels of every class are compared map by map (dec1.1 takes the 4-row ones); bf16 and fp16x3.
D  LM_S2GP.forward(mode='test') with args.pair_extractor_launches = 0 against 1: the same poses, B = 4 (the two-stream path, where
   the option is inert) and B = 16 (paired, 8-row kernels, first_row8 from dead_ground_rows).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _same(a, b):
    """Bitwise (NaN-safe) equality of two tensors."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


_NETS = {}


def _nets(precision):
    """The two extractors with seeded weights (different ones), made once per precision."""
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


def _images(B, sat_a, grd_hw, seed):
    g = torch.Generator(device=_dev())
    g.manual_seed(seed)
    return (torch.rand(B, 3, sat_a, sat_a, device=_dev(), generator=g), torch.rand(B, 3, *grd_hw, device=_dev(), generator=g))


def _pair_vs_plain(precision, B, sat_a, grd_hw, f8, expect_paired, lm=True, count_launches=False):
    from highlyaccurate_amd import _lib
    from highlyaccurate_amd.VGG import vgg_forward_nhwc, vgg_forward_pair_nhwc
    nets = _nets(precision)
    xs = _images(B, sat_a, grd_hw, 1000 + B)
    feat16 = precision in ('bf16', 'fp16')
    plain = [vgg_forward_nhwc(net, x, want_conf=False, defer_norm=True, first_row8=f, feat16=feat16)
             for net, x, f in zip(nets, xs, (0, f8))]
    if count_launches:
        _lib.prof_enable(True)
    try:
        p0, p1, paired = vgg_forward_pair_nhwc(nets, xs, first_row8=(0, f8), feat16=feat16)
    finally:
        if count_launches:
            recs = _lib.prof_fetch()
            _lib.prof_enable(False)
    torch.cuda.synchronize()
    assert paired == expect_paired, (precision, B, paired)
    if count_launches:      # conv0 + conv2 fused and the nine conv3x3 layers: 10 launches for both networks (20 from the two plain
        assert len([r for r in recs if r[0].startswith('conv')]) == 10, recs      # forwards), and one inv_norm launch
        assert len([r for r in recs if r[0].startswith('inv_norm')]) == 1, recs
    for k, ((feats, inv), (rf, _, rinv), f) in enumerate(zip((p0, p1), plain, (0, f8))):
        assert _same(inv, rinv), (precision, B, k, inv, rinv)
        for l in range(3):
            r = f << l           # rows above first_row8 * 2^l are never written: not compared
            assert torch.isfinite(rf[l][:, r:].float()).all()
            assert _same(feats[l][:, r:], rf[l][:, r:]), (precision, B, k, l)
    if lm:      # the pose trace of the LM loop on the paired maps and on the plain ones
        from oracle import ref_cpu as O
        from highlyaccurate_amd.models_kitti import LM_S2GP
        net = LM_S2GP(O.default_args(N_iters=2, damping=1.0, precision=precision)).to(_dev())
        traces = []
        for sat, grd in ((p0, p1), ((plain[0][0], plain[0][2]), (plain[1][0], plain[1][2]))):
            torch.manual_seed(0)
            np.random.seed(0)
            traces.append(net.lm_solve(sat[0], grd[0], [None] * 3, grd_hw, None, 0, None, sat[1], grd[1]).clone())
        assert torch.isfinite(traces[1]).all()
        assert _same(traces[0], traces[1]), (precision, B)


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp32', 'fp16x3'])
def test_case_a_row_trimmed_ground_segment(precision):
    _pair_vs_plain(precision, 2, 64, (64, 128), 4, True, count_launches=precision == 'bf16')


@pytest.mark.parametrize('precision', ['bf16', 'fp16x3'])
def test_case_b_partial_tiles_and_odd_batch(precision):
    _pair_vs_plain(precision, 9, 72, (80, 136), 0, True)


def test_case_c_falls_back_across_the_small_grid_threshold():
    _pair_vs_plain('bf16', 4, 64, (256, 512), 0, False, lm=False)


@pytest.mark.parametrize('precision', ['bf16', 'fp16x3'])
def test_case_e_eight_row_pair_kernels(precision):
    _pair_vs_plain(precision, 16, 256, (128, 512), 5, True)


@pytest.mark.parametrize('B', [4, 16])
def test_case_d_model_option_gives_the_same_poses(B, monkeypatch):
    from oracle import ref_cpu as O
    from highlyaccurate_amd import _s2gp
    from highlyaccurate_amd.models_kitti import LM_S2GP
    d = _dev()
    seen = []
    real = _s2gp.vgg_forward_pair_nhwc

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append(r[2])
        return r
    monkeypatch.setattr(_s2gp, 'vgg_forward_pair_nhwc', spy)
    sat, grd, _, _, _ = O.synth_images(300 + B, B, grd_hw=(128, 512), sat_a=256)
    sat, grd = sat.to(d), grd.to(d)
    out = []
    for on in (0, 1):
        args = O.default_args(precision='bf16', pair_extractor_launches=on)
        net = LM_S2GP(args)
        net.load_state_dict(O.synth_model_state(7, rotation_range=args.rotation_range))
        net = net.to(d)
        torch.manual_seed(3)
        np.random.seed(3)
        with torch.no_grad():
            res = net(sat, grd, mode='test')
        out.append((net.last_trace.clone(), [r.clone() for r in res]))
        # the pair entry is reached only with the option on and above small_batch_two_streams, and there it pairs
        assert seen == ([True] if on and B == 16 else []), (B, on, seen)
        seen.clear()
    assert torch.isfinite(out[0][0]).all()
    assert _same(out[0][0], out[1][0]), (B, (out[0][0] != out[1][0]).nonzero()[:4])
    assert len(out[0][1]) == len(out[1][1]) and all(_same(a, b) for a, b in zip(*[o[1] for o in out]))
