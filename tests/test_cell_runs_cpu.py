"""CPU checks of the coherent ground tables of tests/lm_kernel_ref.py (``coherent_table``) and of every case
tests/test_cell_runs_vs_fp64.py runs on them.  All of it is about the INPUTS and the references; no kernel takes part.

1. ``run_stats`` -- the CPU mirror of how lm_bwd_accum and psb_accum deal pixels to lane groups and merge texel-cell runs -- on
   every coherent case at the poses it is run at: at least half of the live pixels are merged, the longest run is at least
   min(RUN, 8), holes sit inside open cells, runs sit in clamped cells, texels are fed by several lane groups and tiles.
   Two conditions cannot hold everywhere, by construction rather than by choice of inputs:
     * a run that goes on after a hole takes three pixels, so where a lane group has RUN = 2 (lm_bwd_accum at C = 16) the
       condition is a hole met with a cell open;
     * a clamped cell needs u == A - 1 or v == A - 1 EXACTLY, which no table can keep through a rotation: clamped runs are
       required at pose 0 (and under the zero hypothesis of the pose-score cases) only.
2. The references' own fp32 runs stay inside the project's gates on the new cases (LM gradients at half of TOL_GRAD, LM and
   pose-score sums at TOL_SUM, the pose-score backward at PB.REF32_WORST), so no gate has to move for them.
3. The gradient gate can see ONE lost pixel of a merged run.
4. Every out-of-view pose used with a coherent level leaves no pixel in view."""
import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import pose_score_bwd_ref as PB
import pose_score_ref as PS
from test_lm_kernels_vs_fp64 import TOL_GRAD, TOL_SUM, _reference_grads

F64, F32 = torch.float64, torch.float32
POSES = ((0.0, 0.0, 0.0), R.COHERENT_POSE)


def _check_stats(tag, s, exact_pose):
    print(f"CELLRUNS {tag}: live {s['live']} merged {s['merged']} longest {s['longest']} (RUN {s['run']}) across_hole {s['across_hole']} "
          f"open_hole {s['open_hole']} clamped {s['clamped']} multi_group {s['multi_group']} multi_tile {s['multi_tile']} tiles {s['tiles']}")
    assert s['merged'] >= 0.5 * s['live'] > 0, tag
    assert s['longest'] >= min(s['run'], 8), tag
    assert (s['across_hole'] if s['run'] >= 3 else s['open_hole']) >= 1, tag
    assert s['open_hole'] >= 1 and s['multi_group'] >= 1, tag
    if exact_pose:
        assert s['clamped'] >= 1, tag
    if s['tiles'] > 1:
        assert s['multi_tile'] >= 1, tag


@pytest.mark.parametrize('case', R.COHERENT_CASES, ids=str)
def test_lm_backward_cases_reach_the_merge_path(case):
    ford, shape, C, A, B = case
    _, lv = R.coherent_level(*case)
    for pose in POSES:
        _check_stats(f'lm_bwd {case} pose {pose}', R.run_stats(lv, pose, C, 'lm_bwd'), pose == POSES[0])
    # (b): a masked pixel (z <= 0, inside the map) between two pixels of one cell
    live, cell = R.pixel_cells(lv, POSES[0])
    z = lv.table[lv.row0:, :, 2].reshape(-1).numpy()
    tu, tv = lv.tu[lv.row0:].reshape(-1), lv.tv[lv.row0:].reshape(-1)
    inside = (tu >= 0) & (tu <= A - 1) & (tv >= 0) & (tv <= A - 1)
    mid = 0
    for p in np.flatnonzero((z <= 0) & inside):
        row = np.arange(p - p % lv.w, p - p % lv.w + lv.w)
        before, after = [q for q in row[max(p % lv.w - 2, 0):p % lv.w] if live[q]], [q for q in row[p % lv.w + 1:p % lv.w + 3] if live[q]]
        mid += int(bool(before) and bool(after) and tuple(cell[before[-1]]) == tuple(cell[after[0]]))
    assert mid >= 1, case


def test_border_cases_do_not_reach_it():
    """Why the coherent tables exist: on the border tables a lane group never holds a run of more than 2 (3 in one psb tiling of
    'many'); most of what is merged at all are the adjacent duplicates among the 100 border pairs."""
    for case in R.BORDER_CASES:
        ford, shape, C, A, B = case
        lv = R.make_level(ford, shape, 16, A, 1, R.case_seed(*case))
        for kind in ('lm_bwd', 'psb'):
            s = R.run_stats(lv, POSES[0], C, kind)
            print(f"CELLRUNS border {kind} {case}: live {s['live']} merged {s['merged']} longest {s['longest']} (RUN {s['run']})")
            assert s['longest'] <= 3, (case, kind, s['longest'])


@pytest.mark.parametrize('ford,level_first,use_keep,using_weight', R.COHERENT_TWO_LEVEL_CASES)
def test_two_level_cases_reach_the_merge_path(ford, level_first, use_keep, using_weight):
    """Along the fp64 reference's own trajectory: every step of every in-view sample, with the step's dropout mask (a dropped
    pixel is a hole); the out-of-view sample sees nothing in any step."""
    geom, levels, p0, rand_uv, keep = R.coherent_two_level_case(ford, level_first)
    keep = keep if use_keep else None
    traj, _ = R.trajectory(geom, levels, p0, rand_uv, 2, level_first, using_weight, keep, F64)
    assert bool((p0[[0, 2], 2] != 0).all())           # rotated start poses
    for k, (l, pose) in enumerate(traj):
        lv = levels[l]
        kp = None if keep is None else keep[k, :(lv.h - lv.row0) * lv.w].numpy()
        for b in range(3):
            pb = tuple(float(c[b, 0]) for c in pose)
            s = R.run_stats(lv, pb, lv.C, 'lm_bwd', kp)
            if b == 1:
                assert s['live'] == 0, (k, s['live'])
                continue
            _check_stats(f'two-level ford{ford} lf{level_first} keep{use_keep} step {k} sample {b}', s, False)


@pytest.mark.parametrize('case', PB.RUN_CASES, ids=str)
def test_pose_score_cases_reach_the_merge_path(case):
    ford, shape, C, A, B, w, K, out_k = case[:8]
    c = PB.reference(case)
    lv = c['run_lv']
    for b in range(B):
        for k in range(K):
            pose = tuple(float(x) for x in c['poses'][b, k])
            s = R.run_stats(lv, pose, C, 'psb')
            if k == out_k:
                assert s['live'] == 0 and int(c['counts'][b, k, 0]) == 0, (case, b, k, s['live'])
                continue
            assert s['live'] == int(c['counts'][b, k, 0])
            _check_stats(f'psb {case} sample {b} hypothesis {k}', s, k == 0)


def test_a_whole_row_in_one_cell():
    """The hypothesis of the one-cotangent case of tests/test_cell_runs_vs_fp64.py: under the zero pose the step-0 row of 'ragged'
    (w = 37) lies in ONE cell but for its holes, so every lane group of psb_accum that walks it holds one run."""
    _, lv = R.coherent_level(0, 'ragged', 64, 16, 3)
    live, cell = R.pixel_cells(lv, POSES[0])
    k = R.COHERENT_STEPS.index(0.0) + 1            # the row with step 0 (one row further down: row 3 is a copy)
    row = slice(k * lv.w, (k + 1) * lv.w)
    assert live[row].sum() >= lv.w - 4 and len({tuple(c) for c in cell[row][live[row]]}) == 1


# ----------------------------------------------------------------------------------------------------------------------
# the references' own fp32 runs
# ----------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.detach().double().numpy(), b.detach().double().numpy()
    return np.abs(a - b).max() / np.abs(b).max()


def _lm_ref32(tag, geom, levels, p0, rand_uv, N, level_first, w, coef, keep=None):
    r = {dt: _reference_grads(geom, levels, p0, rand_uv, N, level_first, w, coef, keep, keep is not None, dt=dt) for dt in (F64, F32)}
    worst = 0.0
    for l in range(len(levels)):
        for name in ('sat', 'grd') + (('conf',) if w else ()):
            a, b = getattr(r[F32][0][l], name).grad, getattr(r[F64][0][l], name).grad
            worst = max(worst, _rel(a, b))
    worst = max(worst, _rel(r[F32][1].grad, r[F64][1].grad))
    print(f'CELLRUNS ref32 {tag}: LM gradients max-rel |ref32 - ref64| = {worst:.2e} (limit {TOL_GRAD / 2:.0e})')
    assert worst <= TOL_GRAD / 2, (tag, worst)


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('case', R.COHERENT_CASES, ids=str)
def test_fp32_reference_of_the_lm_step_is_inside_the_gates(case, using_weight):
    ford, shape, C, A, B = case
    geom, lv = R.coherent_level(*case)
    coef = torch.from_numpy(np.random.RandomState(R.case_seed('coef', shape, C, B)).standard_normal((B, 1, 1, 3)))
    for pose in POSES:
        p0 = torch.tensor([pose], dtype=F32).repeat(B, 1)
        _lm_ref32(f'{case} w{using_weight} pose {pose}', geom, [lv], p0, torch.zeros(1, 2, B), 1, 0, using_weight, coef)
        s64, mags, n64 = R.level_sums(R.cast_geom(geom, F64), R.cast_level(lv, F64), R.pose_cols(p0, F64), using_weight)
        s32, _, n32 = R.level_sums(R.cast_geom(geom, F32), R.cast_level(lv, F32), R.pose_cols(p0, F32), using_weight)
        err = (s32.double() - s64).abs()
        print(f'CELLRUNS ref32 {case} w{using_weight} pose {pose}: LM sums |ref32 - ref64| / T_k = '
              f'{(err / torch.where(mags > 0, mags, torch.ones_like(mags))).max():.2e} (limit {TOL_SUM:.0e})')
        assert bool((err <= TOL_SUM * mags).all()) and torch.equal(n32, n64)


@pytest.mark.parametrize('ford,level_first,use_keep,using_weight', R.COHERENT_TWO_LEVEL_CASES)
def test_fp32_reference_of_the_two_level_cases_is_inside_the_gate(ford, level_first, use_keep, using_weight):
    geom, levels, p0, rand_uv, keep = R.coherent_two_level_case(ford, level_first)
    coef = torch.from_numpy(np.random.RandomState(R.case_seed('coherent2', ford, level_first) + 3).standard_normal((3, 2, 2, 3)))
    _lm_ref32(f'two-level ford{ford} lf{level_first} keep{use_keep} w{using_weight}', geom, levels, p0, rand_uv, 2, level_first,
              using_weight, coef, keep if use_keep else None)


@pytest.mark.parametrize('case', PB.RUN_CASES, ids=str)
def test_fp32_reference_of_the_pose_score_is_inside_the_gates(case):
    c = PB.reference(case)
    w = case[5]
    lv32, g32 = R.cast_level(c['ref_lv'], F32), R.cast_geom(c['geom'], F32)
    r32 = PS.score(g32, lv32, c['poses'], w)
    _, mags, counts, _, _ = PS.score(R.cast_geom(c['geom'], F64), c['ref_lv'], c['poses'], w)
    err = (r32[0].double() - c['sums']).abs()
    print(f'CELLRUNS ref32 {case}: pose-score sums |ref32 - ref64| / T_k = '
          f'{(err / torch.where(mags > 0, mags, torch.ones_like(mags))).max():.2e} (limit {TOL_SUM:.0e})')
    assert bool((err <= TOL_SUM * mags).all()) and torch.equal(r32[2], counts)
    got, _ = PB.grads(g32, lv32, c['poses'], w, r32[0], c['d_cost'])
    for name, a, b, t in zip(('d_sat', 'd_grd', 'd_conf'), got, c['grads'], c['T']):
        ratio, zeros = PB.worst_ratio(a, b, t)
        print(f'CELLRUNS ref32 {case} {name}: worst |ref32 - ref64| / T = {ratio:.2e} (limit {PB.REF32_WORST:.2e})')
        assert zeros and ratio <= PB.REF32_WORST, (case, name, ratio)


# ----------------------------------------------------------------------------------------------------------------------
# the gate sees one lost pixel
# ----------------------------------------------------------------------------------------------------------------------
def test_one_lost_pixel_of_a_merged_run_moves_d_sat_past_the_gate():
    """16 in-view pixels inside merged runs of coherent 'ragged' C = 64: the fp64 reference without that ONE pixel (``keep``) differs
    from the full one by at least 10 x TOL_GRAD x max|d_sat| somewhere in d_sat.  A kernel that loses such a pixel at a flush
    cannot pass ``_gate_grad``."""
    case = (0, 'ragged', 64, 16, 3)
    ford, shape, C, A, B = case
    geom, lv = R.coherent_level(*case)
    npix = (lv.h - lv.row0) * lv.w
    p0, ruv = torch.zeros(B, 3), torch.zeros(1, 2, B)
    coef = torch.from_numpy(np.random.RandomState(R.case_seed('coef', shape, C, B)).standard_normal((B, 1, 1, 3)))
    # (not in a clamped cell: there both weights of the clamped axis are 0 and the pixel's tap gradients cancel in exact arithmetic)
    _, cell = R.pixel_cells(lv, POSES[0])
    merged = [p for p in R.run_stats(lv, POSES[0], C, 'lm_bwd')['merged_pixels'] if cell[p][2] == 1 and cell[p][3] == 1]
    picks = [merged[i] for i in np.linspace(0, len(merged) - 1, 16).astype(int)]
    assert len(set(picks)) == 16
    full = _reference_grads(geom, [lv], p0, ruv, 1, 0, 1, coef)[0][0].sat.grad
    scale = float(full.abs().max())
    factors = []
    for p in picks:
        keep = torch.ones(1, npix, dtype=torch.uint8)
        keep[0, p] = 0
        lost = _reference_grads(geom, [lv], p0, ruv, 1, 0, 1, coef, keep, True)[0][0].sat.grad
        factors.append(float((lost - full).abs().max()) / (TOL_GRAD * scale))
    print('CELLRUNS sensitivity: |d_sat(full) - d_sat(one pixel lost)| / (TOL_GRAD max|d_sat|) per pixel: ' +
          ' '.join(f'{f:.0f}' for f in factors) + f'; smallest {min(factors):.1f}')
    assert min(factors) >= 10, factors


# ----------------------------------------------------------------------------------------------------------------------
# out-of-view poses
# ----------------------------------------------------------------------------------------------------------------------
def test_out_of_view_pose_clears_every_coherent_level_it_is_used_with():
    lvs = [PB.reference(case)['run_lv'] for case in PB.RUN_CASES if case[7] is not None]
    for ford, level_first, _, _ in R.COHERENT_TWO_LEVEL_CASES:
        lvs += R.coherent_two_level_case(ford, level_first)[1]
    for lv in lvs:
        live, _ = R.pixel_cells(lv, R.OUT_OF_VIEW_POSE)
        g = R.cast_geom(R.make_geom(lv.ford, 1), F64)
        uv, _, _ = R.level_uv(g, lv, R.pose_cols(torch.tensor([R.OUT_OF_VIEW_POSE]), F64))
        inb = (uv[..., 0] >= 0) & (uv[..., 0] <= lv.A - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= lv.A - 1)
        assert int(live.sum()) == 0 and int(inb.sum()) == 0, (lv.ford, lv.shape, lv.A, int(inb.sum()))
