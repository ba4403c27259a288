"""CPU checks of the reach-flag reference and inputs of tests/test_lm_reach_vs_fp64.py (tests/lm_kernel_ref.py: reach_flags,
reach_table, the one-level REACH_CASES and the moving-pose REACH2_CASES), on the references alone -- nothing here depends on what a
kernel computes.

* ``reach_flags`` is the rule its docstring states, pinned to a plain loop over pixels.
* The dyadic poses are exact: shift_u = -+2^-14 moves every u by -+3 * 2^-12 px and no v, shift_v = 0.25 every v by -3 px and no
  u, bit for bit, in the fp32 and in the fp64 reference.  So at pose 0 the smallest u of a clean table's pixels that take part is
  col0 itself, no such pixel of any one-level case lies within 2^-13 of the column without lying on it, and the two precisions
  give the same flags.
* Every pixel class the GPU tests rely on is there: left of the column but z <= 0 / outside in v / u < 0 / dropped / not read;
  the crossing pixel where the case says.
* Moving poses: the flag pattern per step, and |u - col0| >= m over all steps and pixels, m = 50 x the pixel displacement the
  pose gate max(1e-6, 2 |ref32 - ref64|) of tests/test_lm_kernels_vs_fp64.py allows."""
import numpy as np
import pytest
import torch

import lm_kernel_ref as R

F64, F32 = torch.float64, torch.float32
COL0, A = R.REACH_COL0, R.REACH_A


def _brute_force_flags(geom, levels, poses_per_step, col0, keep):
    B = poses_per_step[0][1][0].shape[0]
    flag = [0] * B
    for k, (l, pose) in enumerate(poses_per_step):
        lv = levels[l]
        uv, _, mask = R.level_uv(R.cast_geom(geom, pose[0].dtype), lv, pose)
        uv, z = uv.numpy(), lv.table[..., 2].numpy()
        for b in range(B):
            for r in range(lv.row0, lv.h):
                for c in range(lv.w):
                    if keep is not None and not int(keep[k, (r - lv.row0) * lv.w + c]):
                        continue
                    u, v = uv[b, r, c]
                    if z[r, c] > 0 and 0 <= u <= lv.A - 1 and 0 <= v <= lv.A - 1 and u < col0[l]:
                        flag[b] = 1
    return flag


@pytest.mark.parametrize('name', ['clean', 'first', 'last', 'not_read', 'dropped', 'conf0'])
def test_reach_flags_is_the_rule_pixel_by_pixel(name):
    geom, lv, p0, keep, _ = R.reach_case(name, 16)
    for dt in (F64, F32):
        steps = [(0, R.pose_cols(p0, dt))]
        assert R.reach_flags(geom, [lv], steps, [COL0], keep).tolist() == _brute_force_flags(geom, [lv], steps, [COL0], keep)


def test_reach_flags_is_the_rule_two_levels_with_dropout():
    geom, levels, p0, rand_uv, keep = R.reach2_case(1)
    steps, _ = R.trajectory(geom, levels, p0, rand_uv, 2, 1, 1, keep, F64)
    small = [R.SimpleNamespace(**vars(lv)) for lv in levels]
    got = R.reach_flags(geom, small, steps, R.REACH2_COL0, keep).tolist()
    assert got == _brute_force_flags(geom, small, steps, R.REACH2_COL0, keep) == [0, 1, 1, 1]


def test_dyadic_shifts_are_exact_in_both_precisions():
    geom, lv, _, _, _ = R.reach_case('clean', 16)
    p = R.reach_poses((0, 1, 2, 3))
    for dt in (F64, F32):
        uv, _, _ = R.level_uv(geom, lv, R.pose_cols(p, dt))
        u, v = uv[..., 0].double().numpy(), uv[..., 1].double().numpy()
        assert np.array_equal(u[0], lv.tu) and np.array_equal(v[0], lv.tv)                     # pose 0: the targets themselves
        assert np.array_equal(u[1], lv.tu - 3 * R.EPS) and np.array_equal(v[1], lv.tv)         # shift_u = -2^-14
        assert np.array_equal(u[2], lv.tu + 3 * R.EPS) and np.array_equal(v[2], lv.tv)         # shift_u = +2^-14
        assert np.array_equal(u[3], lv.tu) and np.array_equal(v[3], lv.tv - 3.0)               # shift_v = 0.25


EXPECTED = {'clean': [0, 1, 0, 1], 'first': [1, 0, 1], 'last': [1, 1, 1], 'many_last': [1, 1], 'not_read': [0, 0], 'dropped': [0, 0, 1],
            'conf0': [1, 0, 1], 'idle_blocks': [0] * 8 + [1], 'two_groups': [1] + [0] * 14 + [1, 1]}


@pytest.mark.parametrize('name', sorted(R.REACH_CASES))
def test_one_level_cases_meet_their_conditions(name):
    geom, lv, p0, keep, rc = R.reach_case(name, 16)
    shape, cross, idx, special = R.REACH_CASES[name]
    flags = {}
    for dt in (F64, F32):
        steps = [(0, R.pose_cols(p0, dt))]
        flags[dt] = R.reach_flags(geom, [lv], steps, [COL0], keep).tolist()
        # on the column or at least EPS away from it: never a matter of rounding
        part, u = R.reach_pixels(geom, lv, steps[0][1], None if keep is None else keep[0])
        d = (u.double() - COL0).abs()[part]
        assert not bool(((d > 0) & (d < 2.0 ** -13)).any())
        # what decides between "on" and "left of" is there: a sample at pose 0 has a pixel that takes part exactly on the column
        b0 = idx.index(0)
        assert bool((part & (u == COL0))[b0].any())
        if cross is None:
            assert float(u[b0][part[b0]].min()) == COL0
    assert flags[F64] == flags[F32] == EXPECTED[name], flags
    # enough pixels in view for the sum and pose gates to mean something
    _, _, count = R.level_sums(geom, R.cast_level(lv, F64), R.pose_cols(p0, F64), 0)
    assert int(count.min()) >= 0.25 * lv.h * lv.w
    read = np.arange(lv.h)[:, None] >= lv.row0
    z = lv.table[..., 2].numpy()
    inside = lambda t: (t >= 0) & (t <= A - 1)
    # pixels left of the column that must not set the flag, among the rows read: z <= 0 (z = 0 and z < 0), outside in v, u < 0
    left = read & (lv.tu < COL0)
    assert (left & inside(lv.tu) & inside(lv.tv) & (z == 0)).any() and (left & inside(lv.tu) & inside(lv.tv) & (z < 0)).any()
    assert (left & (z > 0) & (lv.tv < 0)).any() and (left & (z > 0) & (lv.tv > A - 1)).any()
    assert (left & (lv.tu < 0) & inside(lv.tv)).any()
    if cross is not None:
        r, c = rc
        assert lv.tu[r, c] == COL0 + cross[1] and lv.tv[r, c] == cross[2] and z[r, c] > 0 and inside(lv.tv[r, c])
        npix, tp = (lv.h - lv.row0) * lv.w, 128 if (lv.h - lv.row0) * lv.w < 4096 else (256 if (lv.h - lv.row0) * lv.w < 16384 else 512)
        p = (r - lv.row0) * lv.w + c
        if name == 'first':
            assert p == 0
        if name == 'last':
            assert p == npix - 1 and npix % tp == 3                   # the last pixel of a 3-pixel last tile
        if name == 'many_last':
            assert (npix + tp - 1) // tp == 65 and p // tp == 64      # more than 64 tiles: the two-pass closing
        if name == 'not_read':
            assert lv.skip <= r < lv.row0                             # stored, but above the rows the loop reads
        if special == 'drop':
            assert int(keep[0, p]) == 0 and 0.3 < float(keep.float().mean()) < 0.7
        if special == 'conf0':
            assert float(lv.conf[:, 0, r, c].abs().max()) == 0.0 and float(lv.conf[:, 0, lv.row0:].min()) == 0.0


def test_column_edges_of_validation():
    """col0 = A - 1 (legal): every pixel that takes part with u < A - 1 flags; col0 = 0: nothing can."""
    geom, lv, _, _, _ = R.reach_case('clean', 16)
    p0 = torch.tensor([R.REACH_POSES[0], R.REACH_POSES[1], R.OUT_OF_VIEW_POSE, R.REACH_POSES[2]], dtype=F32)
    for dt in (F64, F32):
        steps = [(0, R.pose_cols(p0, dt))]
        assert R.reach_flags(geom, [lv], steps, [A - 1]).tolist() == [1, 1, 0, 1]
        assert R.reach_flags(geom, [lv], steps, [0]).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize('level_first', [0, 1])
def test_moving_pose_cases_keep_their_distance(level_first):
    geom, levels, p0, rand_uv, keep = R.reach2_case(level_first)
    assert levels[0].A != levels[1].A and levels[0].C != levels[1].C and R.REACH2_COL0[0] != R.REACH2_COL0[1]
    t64, last64 = R.trajectory(geom, levels, p0, rand_uv, 2, level_first, 1, keep, F64)
    t32, last32 = R.trajectory(geom, levels, p0, rand_uv, 2, level_first, 1, keep, F32)
    order = R.step_order(2, 2, level_first)
    assert [l for l, _ in t64] == [l for _, l in order]
    # the flag of every single step, in both precisions
    for t in (t64, t32):
        per_step = [R.reach_flags(geom, levels, [t[k]], {t[k][0]: R.REACH2_COL0[t[k][0]]}, None if keep is None else keep[k:k + 1]).tolist()
                    for k in range(4)]
        assert [list(x) for x in zip(*per_step)] == R.REACH2_STEP_FLAGS[level_first]
    pat = R.REACH2_STEP_FLAGS[level_first]
    assert [k for k in range(4) if pat[3][k]] == [order.index((1, 1))]                          # only level 1, only iteration 2
    assert all(order[k][1] == 0 for k in range(4) if pat[1][k]) and any(pat[1])                 # only under col0[0]
    assert R.reach_flags(geom, levels, t64, R.REACH2_COL0, keep).tolist() == [0, 1, 1, 1]
    # ... and the wrong level's column would give other flags: sample 0 reads left of col0[0] at level 1
    assert R.reach_flags(geom, levels, t64, (R.REACH2_COL0[0],) * 2, keep).tolist() == [1, 1, 1, 1]
    # the margin: 50 x what the pose gate lets any step's pose error move a pixel
    after64 = [p for _, p in t64[1:]] + [last64]
    after32 = [p for _, p in t32[1:]] + [last32]
    m = 50 * max(R.pose_allowance_px(levels, a, b) for a, b in zip(after64, after32))
    margin = R.reach_margin(geom, levels, t64, R.REACH2_COL0, keep)
    print(f'level_first {level_first}: m = {m:.3e} px, margins {margin.tolist()}')
    assert m >= 50 * (6.0 / 0.5) * 1e-6 and float(margin.min()) >= m, (m, margin)
    # no re-initialisation on the way (rand_uv never enters)
    assert all(float(c.abs().max()) < 2.5 for _, p in t64 for c in p)
