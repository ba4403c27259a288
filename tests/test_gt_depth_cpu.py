"""CPU checks of ``args.use_gt_depth`` for ``LM_S2GP``: the fp64-capable restatement (tests/gt_depth_ref.py) is pinned to what the
REAL reference recorded (tools/make_golden_gt_depth.py), the product's ray tables to the reference's ``xyz_grds[l][2]`` bit for
bit, its nearest-neighbour source indices to ``F.interpolate`` itself, and the argument rules of the module surface.  Tolerances
of the pins are those tests/test_polar_cpu.py uses for the same purpose."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from make_idx import sample_idx
from oracle import ref_cpu as O
import gt_depth_ref as R

TABLE_SALT = 51          # tools/make_golden_gt_depth.py


def _tuple9(res):
    return np.stack([np.atleast_1d(r.detach().double().numpy()) if r.dim() else np.full(3, float(r.detach())) for r in res[:9]])


def test_ray_table_is_bit_identical_to_the_reference():
    """``ray_table`` and the model's per-level tables against sampled entries and the sum of the reference's xyz_grds[l][2]; the
    ground-plane tables, now built from the same rays, are still the oracle's bit for bit."""
    from highlyaccurate_amd._s2gp import KITTI_K, ground_plane_table, ray_table
    from highlyaccurate_amd.models_kitti import LM_S2GP
    g = load_golden('e2e_kitti_gt_depth.npz')
    net = LM_S2GP(O.default_args(use_gt_depth=1, level=4))
    tabs = net.ray_tables(256, 1024, 'cpu')
    assert len(tabs) == 4 and net.ray_tables(256, 1024, 'cpu') is tabs
    for l in range(4):
        h, w = 256 / 2 ** (3 - l), 1024 / 2 ** (3 - l)
        t = ray_table(KITTI_K, h, w, 256, 1024)
        assert tuple(t.shape) == tuple(g[f'ray_shape_l{l}']) == (int(h), int(w), 3) and t.dtype == torch.float32 and t.is_contiguous()
        assert torch.equal(tabs[l], t)
        flat = t.reshape(-1)
        np.testing.assert_array_equal(flat[sample_idx(flat.numel(), TABLE_SALT + l)].numpy(), g[f'ray_samples_l{l}'])
        assert flat.double().sum().item() == float(g[f'ray_sum_l{l}'])
        assert torch.equal(R.camera_rays(O.KITTI_K, h, w, 256, 1024)[0], t)
        assert bool((t[..., 2] == 1).all())                                      # K^-1 [u,v,1]: z = 1, the depth is along z
        assert torch.equal(ground_plane_table(KITTI_K, h, w, 256, 1024), O.ground_points(O.KITTI_K, h, w, 256, 1024)[0][0])
    # any ground-image size, like the ground-plane tables
    small = LM_S2GP(O.default_args(use_gt_depth=1)).ray_tables(72, 264, 'cpu')
    assert [tuple(t.shape) for t in small[:3]] == [(9, 33, 3), (18, 66, 3), (36, 132, 3)]
    assert torch.equal(small[0], R.camera_rays(O.KITTI_K, 9.0, 33.0, 256, 1024)[0])


@pytest.mark.parametrize('pair', [((32, 128), (32, 128)), ((375, 1242), (32, 128)), ((375, 1242), (64, 256)), ((375, 1242), (128, 512)),
                                  ((23, 77), (9, 33)), ((23, 77), (18, 66)), ((23, 77), (36, 132)), ((94, 311), (128, 512)),
                                  ((37, 100), (16, 64)), ((5, 7), (64, 256)), ((1, 1), (9, 33))])
def test_nearest_indices_reproduce_interpolate(pair):
    """The host-side source indices against ``F.interpolate(..., mode='nearest')`` of an index-coded image: equal sizes, the real
    KITTI depth size, sizes that are no multiple of each other, up-sampling."""
    from highlyaccurate_amd._s2gp import nearest_indices
    from highlyaccurate_amd.models_kitti import LM_S2GP
    (dH, dW), (h, w) = pair
    img = (torch.arange(dH)[:, None] * dW + torch.arange(dW)[None]).float()[None, None]        # exact in fp32 (< 2^24)
    ref = F.interpolate(img, (h, w), mode='nearest')[0, 0].long()
    assert torch.equal(F.interpolate(img, (h, w))[0, 0].long(), ref)                            # the default mode is 'nearest'
    ri, ci = nearest_indices(dH, h), nearest_indices(dW, w)
    assert ri.dtype == ci.dtype == torch.int32 and tuple(ri.shape) == (h,) and tuple(ci.shape) == (w,)
    assert 0 <= int(ri.min()) and int(ri.max()) < dH and 0 <= int(ci.min()) and int(ci.max()) < dW
    assert torch.equal(ri.long()[:, None] * dW + ci.long()[None], ref)
    net = LM_S2GP(O.default_args())
    a = net.depth_indices(h, w, dH, dW, 'cpu')
    assert torch.equal(a[0], ri) and torch.equal(a[1], ci) and net.depth_indices(h, w, dH, dW, 'cpu') is a
    # mask before or after the resampling: the same
    d = R.depth_map(3, 1, dH, dW)
    m1 = F.interpolate((d != -1).float()[:, None], (h, w), mode='nearest')[:, 0]
    assert torch.equal(m1, (d[:, ri.long()][:, :, ci.long()] != -1).float())


def test_synthetic_depth_map():
    from highlyaccurate_amd import synthetic
    d = synthetic.gt_depth(3, 94, 311, 7)
    assert tuple(d.shape) == (3, 94, 311) and d.dtype == torch.float32
    assert torch.equal(d, R.depth_map(7, 3)) and torch.equal(d, synthetic.gt_depth(3, 94, 311, 7))
    holes = (d == -1).float().mean(dim=(1, 2))
    assert bool(((holes > 0.12) & (holes < 0.18)).all())
    assert not torch.equal(d[0], d[1]) and bool((d[d != -1] > 0).all()) and float(d.max()) <= 240.0
    # below the horizon: the flat ground's depth, up to the 20 % noise
    fy, cy = 482.7076 * 94 / 256.0, 125.0034 * 94 / 256.0
    row = 80
    plane = 1.65 * fy / (row - cy)
    v = d[:, row][d[:, row] != -1]
    assert float(v.min()) >= plane * 0.999 and float(v.max()) <= plane * 1.2001


def test_depth_argument_rules():
    """What ``forward`` checks before anything runs on the GPU, and the binding's view of the extended C struct."""
    from highlyaccurate_amd import _lib
    from highlyaccurate_amd.models_kitti import LM_S2GP
    net = LM_S2GP(O.default_args(use_gt_depth=1))
    d = R.depth_map(1, 2, 20, 60)
    assert net._depth_arg(None, 2, 'cpu') is None
    got = net._depth_arg(d.double()[:, ::1], 2, 'cpu')
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, d)
    assert net._depth_arg(d.transpose(1, 2), 2, 'cpu').is_contiguous()
    for bad in (d[:1], d[0], d[:, None], torch.cat([d, d])):
        with pytest.raises(ValueError, match='gt_depth'):
            net._depth_arg(bad, 2, 'cpu')
    with pytest.raises(NotImplementedError, match='polar'):
        LM_S2GP(O.default_args(use_gt_depth=1, proj='polar'))._depth_arg(d, 2, 'cpu')
    assert LM_S2GP(O.default_args(use_gt_depth=1, proj='polar'))._depth_arg(None, 2, 'cpu') is None
    names = [f[0] for f in _lib.S2GLevel._fields_]
    assert names[-6:] == ['ray', 'depth', 'depth_row', 'depth_col', 'depth_h', 'depth_w']
    lv = _lib.S2GLevel()
    assert not lv.ray and not lv.depth and not lv.depth_row and not lv.depth_col and lv.depth_h == 0 and lv.depth_w == 0
    assert C.sizeof(_lib.S2GLevel) % 8 == 0
    hdr = open(__import__('os').path.join(__import__('os').path.dirname(__file__), '..', 'include', 'hla.h')).read()
    assert f'#define HLA_ABI_VERSION {_lib.ABI_VERSION}\n' in hdr and 'models_kitti.py:741-748' in hdr


def test_restatement_matches_reference_golden():
    """Full KITTI shape, fp32: the 15-step trace of every recorded seed (seed 1 in both loop orders), the final pose and the
    train-mode tuple, against what the REAL reference recorded with the same depth map."""
    g = load_golden('e2e_kitti_gt_depth.npz')
    B = int(g['B'])
    assert tuple(g['depth_hw']) == R.DEPTH_HW
    for seed in (int(s) for s in g['seeds']):
        net = R.build(O.default_args(use_gt_depth=1), seed)
        sat, grd, gu, gv, gh = O.synth_images(seed + 100, B)
        depth = R.depth_map(seed + int(g['depth_seed']), B)
        for lf, tag in ((0, ''), (1, '_lf'))[:2 if seed == int(g['seeds'][0]) else 1]:
            torch.manual_seed(seed)
            with torch.no_grad():
                res = net(sat, grd, mode='test', gt_depth=depth, level_first=lf)
            got = R.stacked_trace(net, B)
            err = np.abs(got - g[f'trace32{tag}_{seed}']).max()
            print(f'restatement vs reference, kitti gt_depth seed {seed} lf {lf} fp32: max pose err {err:.2e}')
            assert err < 2e-5
            np.testing.assert_allclose(torch.stack(res, -1).double().numpy(), g[f'final32{tag}_{seed}'], rtol=0, atol=2e-5)
            assert np.abs(g[f'otrace64{tag}_{seed}'] - g[f'trace32{tag}_{seed}']).max() < 1e-3     # well conditioned in the reference
        torch.manual_seed(seed)
        with torch.no_grad():
            res = net(sat, grd, gu, gv, gh, mode='train', gt_depth=depth)
        assert len(res) == 14
        np.testing.assert_allclose(_tuple9(res), g[f'tuple32_{seed}'], rtol=2e-3, atol=2e-4)
        # the depth map matters in the reference: a run that ignores it is > 1e-2 away
        assert np.abs(g[f'trace32_{seed}'] - g[f'plain32_{seed}']).max() > 1e-2


def test_inactive_depth_is_the_plain_restatement():
    """use_gt_depth=1 without a map, and use_gt_depth=0 with one, equal the oracle's plain model exactly (small shape)."""
    B, grd_hw, sat_a = 2, (64, 256), 128
    sat, grd, *_ = O.synth_images(9, B, grd_hw=grd_hw, sat_a=sat_a)
    depth = R.depth_map(4, B, 20, 60)
    runs = []
    for build, kw, dep in ((lambda a: O.build('kitti', a, 3, grd_hw=grd_hw), dict(), None),
                           (lambda a: R.build(a, 3, grd_hw=grd_hw), dict(use_gt_depth=1), None),
                           (lambda a: R.build(a, 3, grd_hw=grd_hw), dict(use_gt_depth=0), depth),
                           (lambda a: R.build(a, 3, grd_hw=grd_hw), dict(use_gt_depth=1), depth)):
        net = build(O.default_args(N_iters=2, **kw))
        torch.manual_seed(0)
        with torch.no_grad():
            net(sat, grd, mode='test', gt_depth=dep)
        runs.append(torch.stack(net.trace, -1))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert float((runs[3] - runs[0]).abs().max()) > 1e-3
    with pytest.raises(IndexError):
        net = R.build(O.default_args(N_iters=2, use_gt_depth=1, proj='polar'), 3, grd_hw=grd_hw)
        with torch.no_grad():
            net(sat, grd, mode='test', gt_depth=depth)
