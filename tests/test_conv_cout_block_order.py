"""The conv3x3 launches with more than one block of output channels (conv10, conv12, conv14: 256 = 2 x 128; the training backward's
data gradients: up to 384 = 3 x 128) run as 1-D grids whose XCD-contiguous order has the channel block innermost
(csrc/conv_block_map.h): a tile's blocks follow one another on one XCD.  A workgroup finds its tile, its channel block and its
sum-of-squares slot from its id alone, so a mistake there computes a tile twice, never, or with another block's weights.

Exact-integer networks (``test_conv_mfma_shape._integer_state``, the 'uniform' draw: weights +1 / -1, image 0..7, every map an
integer of magnitude <= 7): the kernels' maps must EQUAL the fp64 maps of ``oracle.ref_cpu`` element for element, in every
precision.  The squares of such a map sum to an exact integer in fp32 (per wave < 2^24) and in fp64, so the sum the kernels'
inv_norm was formed from -- recovered as 1 / inv_norm^2, good to a few parts in 2^52 against integers that differ by >= 1 -- must
be the oracle's: that pins conv14's slots, tile * 2 + channel block.

Shapes, by the grid conv10 / conv12 / conv14 run (restated from conv_plan, conv_kernels.h, and asserted, so that a change of
CONV_SMALL_GRID cannot silently empty a case):
  a  B = 3, 40 x 72: conv10 / conv12 take 4-row tiles, 9 tiles x 2 = 18 workgroups; conv14 (8-row: it has a sum of squares) 12.
  b  B = 19, 88 x 288: 8-row tiles, 9 tiles per sample (odd) x 19 x 2 = 342 workgroups, no multiple of 8.
  c  the paired entry, B = 19, satellite 136 x 136 and ground 48 x 520 with first_row8 = 4: the ground segment's conv12 starts at
     row 3; both segments of conv10 / conv12 are 380 workgroups (8-row side), so segment 1 starts at workgroup 380 = 4 mod 8.
     Also compared bitwise with the two plain forwards.
Training: (2, 72, 136), level 3 -- dec1.1's data gradient (128 -> 384 channels) is 12 tiles x 3 blocks = 36 workgroups -- under the
gates of ``test_vgg_backward_16bit_vs_fp64`` (``vgg_bwd16_ref.check_run``), unchanged.
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
import test_conv_mfma_shape as S

pytestmark = pytest.mark.gpu

CONV_SMALL_GRID = 320      # conv_kernels.h
_REFS = {}


def _plan(B, h, w, cout, row_begin=0, sumsq=False):
    """conv_plan (conv_kernels.h) for an inference launch: (4-row tiles?, tiles in the grid, channel blocks)"""
    tx, gy = -(-w // 32), (cout // 128 if cout >= 128 else 1)
    small = not sumsq and tx * ((h - row_begin + 7) // 8) * B * gy < CONV_SMALL_GRID
    return small, tx * ((h - row_begin + (3 if small else 7)) // (4 if small else 8)) * B, gy


def _first_rows(f):
    """first rows of conv10, conv12, conv14 for first_row8 = f without confidence heads (vgg_build_convs, vgg.hip)"""
    return (2 * f - 6, 2 * f - 5, 2 * f - 4) if f else (0, 0, 0)


def _ref(shape, f8=0):
    """fp64 oracle of one image batch, once per session: raw maps and, per map, the per-sample sums of squares of the rows the
    kernels compute with first_row8 = f8 (x15 from row f8 - 2, x18 from 2 f8 - 1, x21 from 4 f8: vgg.hip)"""
    key = (shape, f8)
    r = _REFS.get(key)
    if r is None:
        B, H, W = shape
        sd, _ = S._integer_state(1009 * H + 13 * W + 3, 'uniform')
        x = S._integer_image(77 + H + W, shape, 'uniform')
        net = O.VGGUnet(3)
        net.load_state_dict(sd)
        with torch.no_grad():
            raws = [t.numpy() for t in net.double().raw_maps(x.double())[:3]]
        for t in raws:
            assert np.array_equal(t, np.rint(t)) and np.abs(t).max() <= 7
        rows = (f8 - 2, 2 * f8 - 1, 4 * f8) if f8 else (0, 0, 0)
        ss = [np.square(t[:, :, r0:]).sum(axis=(1, 2, 3)) for t, r0 in zip(raws, rows)]
        r = dict(sd=sd, x=x, raws=raws, ss=ss, first_row8=f8)
        _REFS[key] = r
    return r


def _assert_sums(tag, inv, r):
    """inv_norm [3, B] fp64 = 1 / sqrt(sum of squares): the sums, exact integers, must be the oracle's"""
    inv = inv.double().cpu().numpy()
    for l in range(3):
        got = np.rint(1.0 / np.square(inv[l]))
        assert np.all(np.abs(1.0 / np.square(inv[l]) - got) <= 1e-6 * np.maximum(got, 1.0)), (tag, l, 'not an integer sum')
        print(f'{tag} map {l}: sums of squares {got[:4].tolist()} oracle {r["ss"][l][:4].tolist()}')
        assert np.array_equal(got, r['ss'][l]), (tag, f'inv_norm {l}', got.tolist(), r['ss'][l].tolist())


def _forward_checks(shape, precision):
    from highlyaccurate_amd.VGG import vgg_forward_nhwc
    r = _ref(shape)
    net, xd = S._net(r['sd'], 3, precision), r['x'].to(S._dev())
    with torch.no_grad():
        if precision in ('bf16', 'fp16'):
            feats, _, inv = vgg_forward_nhwc(net, xd, want_conf=False, defer_norm=True, feat16=True)
            S._assert_maps_equal(f'{shape} {precision} feat16', feats, r)
            _assert_sums(f'{shape} {precision} feat16', inv, r)
        feats, _, inv = vgg_forward_nhwc(net, xd, want_conf=False, defer_norm=True)
    S._assert_maps_equal(f'{shape} {precision}', feats, r)
    _assert_sums(f'{shape} {precision}', inv, r)


SHAPE_A, SHAPE_B = (3, 40, 72), (19, 88, 288)


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp16x3', 'fp32'])
def test_four_row_path_small_grid(precision):
    B, H, W = SHAPE_A
    for cout_layer in ('conv10', 'conv12'):
        small, tiles, gy = _plan(B, H // 4, W // 4, 256)
        assert small and gy == 2 and tiles == 9 and (tiles * gy) % 8, (cout_layer, small, tiles, gy)
    small, tiles, gy = _plan(B, H // 4, W // 4, 256, sumsq=True)      # conv14
    assert not small and gy == 2 and tiles == 6 and (tiles * gy) % 8, (small, tiles, gy)
    _forward_checks(SHAPE_A, precision)


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp16x3'])
def test_eight_row_path_odd_tile_counts(precision):
    B, H, W = SHAPE_B
    for sumsq in (False, True):      # conv10 / conv12, conv14
        small, tiles, gy = _plan(B, H // 4, W // 4, 256, sumsq=sumsq)
        assert not small and gy == 2 and tiles == 9 * B and (tiles // B) % 2 == 1 and (tiles * gy) % 8, (small, tiles, gy)
    _forward_checks(SHAPE_B, precision)


PAIR_B, PAIR_SAT, PAIR_GRD, PAIR_F8 = 19, 136, (48, 520), 4


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp16x3'])
def test_paired_entry_unequal_segments(precision):
    from highlyaccurate_amd.VGG import vgg_forward_nhwc, vgg_forward_pair_nhwc
    B = PAIR_B
    shapes = ((B, PAIR_SAT, PAIR_SAT), (B, *PAIR_GRD))
    f8s = (0, PAIR_F8)
    for k, (name, sumsq) in enumerate((('conv10', False), ('conv12', False), ('conv14', True))):
        plans = [_plan(B, h // 4, w // 4, 256, _first_rows(f)[k], sumsq) for (_, h, w), f in zip(shapes, f8s)]
        assert not plans[0][0] and not plans[1][0], (name, plans)                         # both on the 8-row side
        assert plans[0][2] == plans[1][2] == 2 and (plans[0][1] * 2) % 8 == 4, (name, plans)  # segment 1 starts out of phase with the XCDs
        assert sumsq or plans[0][1] * 2 >= CONV_SMALL_GRID <= plans[1][1] * 2, (name, plans)
    assert _first_rows(PAIR_F8)[1] % 2 == 1                                               # the ground segment's conv12: an odd first row
    refs = [_ref(s, f) for s, f in zip(shapes, f8s)]
    nets = [S._net(r['sd'], 3, precision) for r in refs]
    xs = [r['x'].to(S._dev()) for r in refs]
    feat16 = precision in ('bf16', 'fp16')
    with torch.no_grad():
        p0, p1, paired = vgg_forward_pair_nhwc(nets, xs, first_row8=f8s, feat16=feat16)
        plain = [vgg_forward_nhwc(net, x, want_conf=False, defer_norm=True, first_row8=f, feat16=feat16)
                 for net, x, f in zip(nets, xs, f8s)]
    assert paired
    for k, ((feats, inv), (pf, _, pinv), r, f) in enumerate(zip((p0, p1), plain, refs, f8s)):
        tag = f'pair segment {k} {precision}'
        S._assert_maps_equal(tag, feats, r, f)
        _assert_sums(tag, inv, r)
        assert torch.equal(inv.view(torch.int64), pinv.view(torch.int64)), (tag, 'inv_norm against the plain forward')
        for l in range(3):
            r0 = f << l      # rows above it are never written
            a, b = feats[l][:, r0:].contiguous().view(torch.uint8), pf[l][:, r0:].contiguous().view(torch.uint8)
            assert torch.equal(a, b), (tag, 'map', l, 'against the plain forward')


TRAIN_SHAPE = (2, 72, 136)


def test_training_backward_three_channel_blocks():
    """dec1.1's data gradient, 128 -> 384 channels: three channel blocks per tile, 36 workgroups.  Every stored gradient map and
    every parameter gradient under the gates of the 16-bit backward test, from the same restatement."""
    import vgg_bwd16_ref as BR
    import test_vgg_backward_16bit_vs_fp64 as T
    B, H, W = TRAIN_SHAPE
    tiles = -(-(W // 4) // 32) * -(-(H // 4) // 8) * B
    assert tiles * 3 == 36 and (tiles * 3) % 8
    f = T._forward(TRAIN_SHAPE, 3, 'bf16')
    tag = f'cout-blocks bf16 {TRAIN_SHAPE} L3'
    g1, maps, raws = T._backward(f, 1)      # (the two-phase call keeps conv2's data gradient map: every map is compared)
    rec64, wg64, wg32 = T._walks(f, maps)
    fails, table = BR.check_run(tag, maps, g1, rec64, wg64, wg32, f['sd'], 3, f['dt'], raws)
    T._report(tag, table)
    assert not fails, fails
