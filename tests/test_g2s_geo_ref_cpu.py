"""tests/g2s_geo_ref.py without a GPU: the reference's 12 sums reproduce ``oracle.ref_cpu.lm_update_g2s``'s update, and every case
of tests/test_g2s_kernels_vs_fp64.py has the property it exists for and is well conditioned -- asserted on the reference alone."""
import numpy as np
import pytest
import torch

import g2s_geo_ref as R
from oracle import ref_cpu as O

F64 = torch.float64
ALL = [('border',), ('out',), ('behind',), ('deep',), ('mid',), ('deferred',), ('octet9',)] + [('shape', A, C) for A, C, _ in R.SHAPES]
_ids = lambda k: '-'.join(str(x) for x in k)


def _walk(c, using_weight):
    """(step, level, pose the reference's own fp64 trajectory starts the step from) for every step of the case."""
    tr = R.reference_trace(c, using_weight)
    prev = R.start_pose(c).double()
    for it in range(c.N):
        for l in range(len(c.levels)):
            yield it * len(c.levels) + l, l, prev
            prev = tr[:, it, l]


def _classes(c, l, pose):
    A, _, hw = c.levels[l]
    return R.pixel_classes(R.make_args(c.ranges), *R.cols(pose), c.K, A, hw, c.ori_hw)


def _pin(args, lam, pose, grd, conf, sat, K, ori_hw, uw):
    sums, mags = R.normal_sums(args, *pose, grd, conf, sat, K, ori_hw, uw)
    new = torch.cat(R.step(args, lam, pose, grd, conf, sat, K, ori_hw, uw), 1)
    err = (torch.cat(pose, 1) + R.delta_from_sums(sums, lam) - new).abs().max()
    assert float(err) < 1e-12, err
    assert bool((mags >= sums.abs() * (1 - 1e-12)).all()) and sums.shape == mags.shape == (sat.shape[0], 12)


@pytest.mark.parametrize('uw', [0, 1])
def test_sums_reproduce_lm_update_at_the_oracles_geometry(uw):
    """KITTI_K for every sample, a 256 x 1024 image, the level-0 map: the geometry LM_G2SP itself runs at."""
    rs = np.random.RandomState(3)
    B, A, Cn, hw = 2, 32, 64, (8, 32)
    sat, grd, conf = (t[0].double() for t in R._maps(rs, B, [(A, Cn, hw)]))
    K = torch.tensor([O.KITTI_K], dtype=torch.float32).repeat(B, 1, 1)
    args = O.default_args(using_weight=uw, train_damping=1)
    pose = R.cols(R._rand_pose(rs, B))
    _pin(args, R.lam_of(), pose, grd, conf, sat, K, (256, 1024), uw)


@pytest.mark.parametrize('uw', [0, 1])
@pytest.mark.parametrize('key', [('shape', 18, 128), ('border',), ('behind',), ('deferred',), ('out',)], ids=_ids)
def test_sums_reproduce_lm_update_at_free_geometries(key, uw):
    c = R.get(*key)
    sat, grd, conf = R.cast(c, F64)
    _pin(R.make_args(c.ranges), R.lam_of(), R.cols(R.start_pose(c)), grd[0], conf[0], sat[0], c.K, c.ori_hw, uw)


def test_tile_rule_and_ragged_tiles():
    assert [R.tiles(A) for A in (7, 18, 70, 130)] == [(64, 1, 49), (64, 6, 4), (128, 39, 36), (256, 67, 4)]
    for key in ALL:
        c = R.get(*key)
        assert any(R.tiles(A)[2] < R.tiles(A)[0] for A, _, _ in c.levels), key
        for A, Cn, (h, w) in c.levels:
            assert Cn in (64, 128, 256) and R.ORI_HW[0] % h and R.ORI_HW[1] % w
    assert R.tiles(130)[1] > 64 and R.get('deep').levels[1][0] == 130


def test_every_sample_has_its_own_intrinsics():
    for key in ALL:
        K = R.get(*key).K
        for a in range(K.shape[0]):
            for b in range(a):
                assert not torch.equal(K[a], K[b]), (key, a, b)
    K = R.get('octet9').K
    assert bool((K[:, 0, 1] != 0).all() and (K[:, 1, 0] != 0).all() and (K[:, 2, :2] != 0).all())


@pytest.mark.parametrize('uw', [0, 1])
@pytest.mark.parametrize('key', ALL, ids=_ids)
def test_cases_are_well_conditioned_and_not_trivial(key, uw):
    """No pixel within GUARD of a texel line or a border at any step (the kernel forms u = q0 * (1/z), the reference q0 / z: a
    pixel on a line is decided by one ulp, and the Jacobian -- at the far border the value -- jumps there); at least 10 % of every
    ordinary sample's pixels in view; some pixels in the first / last cells; pixels in view in the ragged last tile of every
    level (or that tile would add zeros however it were handled)."""
    c = R.get(*key)
    edge = 0
    for k, l, pose in _walk(c, uw):
        p = _classes(c, l, pose)
        assert int(p.last.sum()) > 0, (key, k, p.last)
        assert float(p.min_dist.min()) > R.GUARD, (key, k, p.min_dist)
        for b in c.ordinary:
            assert int(p.inb[b]) >= 0.1 * p.npix, (key, k, b, int(p.inb[b]), p.npix)
        edge += int(p.edge.sum())
    assert edge > 0 or max(A for A, _, _ in c.levels) == 7, key         # (49 pixels need not reach a map's rim)


def test_border_case_sits_at_every_border_on_both_sides():
    c = R.get('border')
    p = _classes(c, 0, R.start_pose(c).double())
    print('border case: pixels within 2^-9 of (u0 in, u0 out, uw in, uw out, v0 in, v0 out, vh in, vh out):', p.near.tolist())
    for side in range(8):
        assert int(p.near[side, side]) >= 1, (side, p.near[side])
    # the u sides hold the whole centre row in front of the camera
    assert all(int(p.near[s, s]) >= 3 for s in range(4)), p.near
    # every border sample still has pixels in view
    assert bool((p.inb > 0).all())


@pytest.mark.parametrize('uw', [0, 1])
def test_behind_case_has_an_in_bounds_pixel_behind_the_camera_at_every_step(uw):
    c = R.get('behind')
    assert c.ranges[0] == 0.0 and c.ranges[1] > 0 and float(c.K[c.behind, 0, 2]) == 0.0 == float(c.K[c.behind, 1, 2])
    assert int(_classes(c, 0, R.start_pose(c).double()).inb[c.behind]) >= 0.1 * 18 * 18          # the sample is not trivial
    for k, l, pose in _walk(c, uw):
        p = _classes(c, l, pose)
        assert int(p.behind[c.behind]) >= 1 and int(p.behind[0]) == 0, (k, p.behind)
        # ... it is the centre pixel, at u = 0 exactly
        A, _, hw = c.levels[l]
        uv, _, mask = O.g2s_pose_to_uv(R.make_args(c.ranges), A, *R.cols(pose), c.K, *hw, *c.ori_hw, require_jac=False)
        ctr = A // 2
        assert float(uv[c.behind, ctr, ctr, 0]) == 0.0 and 0 < float(uv[c.behind, ctr, ctr, 1]) < hw[0] - 1 and not bool(mask[c.behind, ctr, ctr])


@pytest.mark.parametrize('uw', [0, 1])
def test_out_case_has_nothing_in_view_and_its_pose_stays(uw):
    c = R.get('out')
    tr = R.reference_trace(c, uw)
    assert not bool(tr[c.out].any())
    for k, l, pose in _walk(c, uw):
        p = _classes(c, l, pose)
        assert int(p.inb[c.out]) == 0
        sat, grd, conf = R.cast(c, F64)
        sums, mags = R.normal_sums(R.make_args(c.ranges), *R.cols(pose), grd[l], conf[l], sat[l], c.K, c.ori_hw, uw)
        assert not bool(sums[c.out].any()) and not bool(mags[c.out].any())


def test_deferred_case_scales_and_take():
    c = R.get('deferred')
    for inv in (c.sat_inv, c.grd_inv):
        assert tuple(inv.shape) == (2, 3) and float(inv.min()) >= 0.5 and float(inv.max()) <= 3.0
        assert torch.equal(inv.float().double(), inv)
    sat, grd = R.raw_maps(c)
    ref = R.cast(c, F64)
    for l in range(2):
        assert torch.equal(ref[0][l], sat[l].double() * c.sat_inv[l].view(-1, 1, 1, 1))
        assert float((ref[1][l] - c.grd[l].double()).abs().max()) < 1e-7 * 0.1
    o = R.get('octet9')
    t = R.take(o, [4, 0])
    assert torch.equal(t.K[0], o.K[4]) and torch.equal(t.sat[1][1], o.sat[1][0]) and torch.equal(t.p0[0], o.p0[4]) and t.B == 2
    assert torch.equal(R.get('octet8').grd[0], o.grd[0][:8])
