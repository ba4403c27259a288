"""CPU checks of tests/lm_kernel_ref.py, the free-geometry fp64 reference of the LM pose-loop kernels: at the oracle's own
metres-per-pixel and centre it IS the oracle (projections and one step, KITTI and Ford), the border table puts every listed
target where it says bit for bit, and the inputs of tests/test_lm_kernels_vs_fp64.py meet the conditions those tests rely on --
checked on the reference alone, so none of them depends on what a kernel computes."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
import lm_kernel_ref as R

F64 = torch.float64


def _rel(a, b):
    a, b = a.detach().double().numpy(), b.detach().double().numpy()
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _poses(B, seed):
    return torch.from_numpy(np.random.RandomState(seed).uniform(-0.3, 0.3, size=(B, 3)))


@pytest.mark.parametrize('ford', [0, 1])
def test_projections_are_the_oracles_at_its_own_geometry(ford):
    B, A = 3, 128
    args = O.default_args()
    ranges = (args.shift_range_lat, args.shift_range_lon, args.rotation_range)
    K = O.ford_K_256x1024() if ford else O.KITTI_K
    xyz, mask = O.ground_points(K, 16.0, 64.0, 256, 1024)
    su, sv, th = R.pose_cols(_poses(B, 1), F64)
    if ford:
        g = R.cast_geom(R.make_geom(1, B), F64)
        g.T_FL = g.T_FL + torch.tensor([[0.3, -0.1, 0.7]], dtype=F64)
        side = 112.64
        ref_uv, ref_jac = O.ford_pose_to_uv(args, xyz, g.R_FL, g.T_FL, su, sv, th, side, A)
        uv, jac, m = R.pose_to_uv_ford(xyz[0], g.R_FL, g.T_FL, su, sv, th, A, side / A, float(A // 2), ranges)
    else:
        ref_uv, ref_jac = O.kitti_pose_to_uv(args, xyz, su, sv, th, A)
        uv, jac, m = R.pose_to_uv_kitti(xyz[0], su, sv, th, A, O.meter_per_pixel() * O.SATMAP_PROCESS_SIDELENGTH / A, A / 2, ranges)
    assert _rel(uv, ref_uv) <= 1e-12
    for a, b in zip(jac, ref_jac):
        assert _rel(a, b) <= 1e-12
    assert torch.equal(m, mask.double())


@pytest.mark.parametrize('ford', [0, 1])
@pytest.mark.parametrize('using_weight', [0, 1])
def test_step_is_the_oracles_step(ford, using_weight):
    """``R.level_step`` against ``LM_S2GP._step`` / ``LM_S2GP_Ford._step`` fed the same table (``onet.xyz_grds[pos]`` overwritten)."""
    B, A, C, pos = 2, 16, 16, 0
    grd_hw = (64, 296)                       # level 0: 8 x 37, rows 4.. take part
    args = O.default_args(damping=1.0, using_weight=using_weight)
    onet = (O.LM_S2GP_Ford if ford else O.LM_S2GP)(args, grd_hw=grd_hw).double()
    side = 16.0
    mpp = side / A if ford else O.meter_per_pixel() * O.SATMAP_PROCESS_SIDELENGTH / A
    lv = R.cast_level(R.make_level(ford, (8, 37, 4, 0), C, A, B, 11, mpp), F64)
    geom = R.cast_geom(R.make_geom(ford, B), F64)
    geom.ranges = (args.shift_range_lat, args.shift_range_lon, args.rotation_range)
    onet.xyz_grds[pos] = (lv.table[None], (lv.table[None][..., 2] > 0).float())
    pose = R.pose_cols(_poses(B, 2) * 0.1, F64)
    extra = (geom.R_FL, geom.T_FL, side) if ford else None
    torch.manual_seed(0)
    ref = onet._step(pos, lv.sat, None, lv.grd, lv.conf, *pose, extra)
    ru = torch.full((B, 1), 9.0, dtype=F64)
    got = R.level_step(R.update_args(geom.ranges, damping=1.0), geom, lv, pose, using_weight, (ru, ru))
    for a, b, p in zip(got, ref, pose):
        assert float((a - p).abs().max()) > 1e-9             # the step moves the pose
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    # and the 14 sums are those of the same operands: ||s||^2 and H00 from the oracle's own projection
    f, _, jac, _, mask = onet.project_map_to_grd(lv.sat, None, *pose, pos, extra)
    sums, mags, count = R.level_sums(geom, lv, pose, using_weight)
    s0 = (f[:, :, 4:] ** 2).reshape(B, -1).sum(1)
    assert _rel(sums[:, 0], s0) <= 1e-12 and bool((mags >= sums.abs() * (1 - 1e-12)).all())
    w = (lv.conf * mask[:, None])[:, :, 4:] if using_weight else 1.0
    h00 = (w * jac[0][:, :, 4:] ** 2).reshape(B, -1).sum(1)
    assert _rel(sums[:, 2], h00) <= 1e-12
    assert int(count.min()) > 0


@pytest.mark.parametrize('ford,shape,C,A,B', sorted(set((f, s, 16, A, 1) for f, s, _, A, _ in R.BORDER_CASES)))
def test_border_table_is_exact(ford, shape, C, A, B):
    """Every target -- the 100 listed pairs and the random fill -- is what the fp32 table entry gives in fp64 at pose 0, bit for
    bit, by the plain formula and through the reference's whole projection chain (cos = 1, sin = 0)."""
    h, w, row0, _ = R.SHAPES[shape]
    table, tu, tv, ku, kv = R.border_table(ford, A, h, w, row0, 5)
    centre = R.centre_of(ford, A)
    u, v = R.targets_from_table(ford, table.numpy(), 0.5, centre)
    assert np.array_equal(u, tu) and np.array_equal(v, tv)
    vals = np.array(R.border_values(A))
    assert np.array_equal(tu[ku >= 0], vals[ku[ku >= 0]]) and np.array_equal(tv[kv >= 0], vals[kv[kv >= 0]])
    assert (ku >= 0).sum() == 100 and len(set(zip(ku[ku >= 0], kv[kv >= 0]))) == 100
    lv = R.make_level(ford, shape, C, A, B, 5)
    uv, _, _ = R.level_uv(R.cast_geom(R.make_geom(ford, B), F64), lv, R.pose_cols(torch.zeros(B, 3), F64))
    assert np.array_equal(uv[0, ..., 0].numpy(), lv.tu) and np.array_equal(uv[0, ..., 1].numpy(), lv.tv)


KITTI_U = {'onlim', 'abovelim', 'belowlim', 'texel', 'half', 'farcell'}      # z > 0 is u > centre
FORD_V = {'on0', 'below0', 'above0', 'texel', 'half', 'mid'}                 # z > 0 is v < centre + 4


@pytest.mark.parametrize('ford,shape,C,A,B', R.BORDER_CASES)
def test_border_case_inputs_meet_their_conditions(ford, shape, C, A, B):
    lv = R.cast_level(R.make_level(ford, shape, 16, A, 1, R.case_seed(ford, shape, C, A, B)), F64)     # (geometry does not depend on C, B)
    geom = R.cast_geom(R.make_geom(ford, 1), F64)
    _, _, count = R.level_sums(geom, lv, R.pose_cols(torch.zeros(1, 3), F64), 0)
    assert int(count[0]) >= 0.25 * lv.h * lv.w
    used = (lv.table[..., 2] > 0).numpy() & (np.arange(lv.h)[:, None] >= lv.row0)      # pixels the loop reads with gm = 1
    lim = A - 1
    inb_u, inb_v = (lv.tu >= 0) & (lv.tu <= lim), (lv.tv >= 0) & (lv.tv <= lim)
    cu = {R.BORDER_CLASSES[k] for k in lv.ku[used & inb_v & (lv.ku >= 0)]}
    cv = {R.BORDER_CLASSES[k] for k in lv.kv[used & inb_u & (lv.kv >= 0)]}
    # every class of one coordinate with the other one inside the map; together the two chains reach all four borders
    assert cu == (set(R.BORDER_CLASSES) if ford else KITTI_U), cu
    assert cv == (FORD_V if ford else set(R.BORDER_CLASSES)), cv
    # and every pair of classes: both coordinates on a border at once (map corners), border x clamped cell, ...
    pairs = set(zip(lv.ku[used & (lv.ku >= 0)], lv.kv[used & (lv.kv >= 0)]))
    assert len(pairs) == 60
    # masked pixels with a non-zero ground map exist among the rows read (gm = 0)
    dead = ~(lv.table[..., 2] > 0).numpy() & (np.arange(lv.h)[:, None] >= lv.row0)
    assert dead.sum() >= 0.15 * (lv.h - lv.row0) * lv.w and bool((lv.grd[0, :, torch.from_numpy(dead)] != 0).any())


@pytest.mark.parametrize('ford,level_first,use_keep,using_weight', R.RANDOM_CASES)
def test_random_pose_case_inputs_meet_their_conditions(ford, level_first, use_keep, using_weight):
    """The reference's own fp64 trajectory of every two-level case: enough pixels in view in every step, no pixel within 1e-6 of
    a border (so an in-view count is not a matter of rounding), no re-initialisation, and the out-of-view sample stays out."""
    seed = R.case_seed('random', ford, level_first)
    geom, levels, p0, rand_uv, keep = R.make_two_level_case(ford, seed)
    g64, l64 = R.cast_geom(geom, F64), [R.cast_level(lv, F64) for lv in levels]
    args = R.update_args()
    pose = R.pose_cols(p0, F64)
    out = 1
    assert levels[0].C != levels[1].C and levels[0].A != levels[1].A and levels[0].mpp != levels[1].mpp
    for k, (i, l) in enumerate(R.step_order(2, 2, level_first)):
        lv = l64[l]
        uv, _, _ = R.level_uv(g64, lv, pose)
        kp = keep[k, :(lv.h - lv.row0) * lv.w].bool() if use_keep else None
        _, _, count = R.level_sums(g64, lv, pose, using_weight, kp)
        for b in range(3):
            if b == out:
                assert int(count[b]) == 0
                continue
            assert int(count[b]) >= 0.25 * lv.h * lv.w, (k, b, int(count[b]))
            for c in (uv[b, ..., 0], uv[b, ..., 1]):
                assert float(torch.minimum(c.abs(), (c - (lv.A - 1)).abs()).min()) > 1e-6
        sentinel = torch.full((3, 1), 77.0, dtype=F64)
        new = R.level_step(args, g64, lv, pose, using_weight, (sentinel, sentinel), keep=kp)
        assert all(float(c.abs().max()) < 2.5 for c in new)            # nothing re-initialised
        assert all(float(a[out, 0]) == float(b[out, 0]) for a, b in zip(new, pose))
        pose = new
