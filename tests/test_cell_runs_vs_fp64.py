"""lm_bwd_accum (csrc/lm_backward.hip) and psb_accum (csrc/pose_score.hip) where pixel runs share a texel cell, against the fp64
references of tests/lm_kernel_ref.py and tests/pose_score_bwd_ref.py, through the C ABI, on the COHERENT tables of
tests/lm_kernel_ref.py.  Both kernels let a lane group walk a run of consecutive ground pixels, sum the four tap gradients of the
pixels of one texel cell in registers and flush them with one set of atomics when the cell changes and at the end of the run.  On
the border tables of the other kernel tests next to every pixel has a cell of its own (tests/test_cell_runs_cpu.py::
test_border_cases_do_not_reach_it); here 67 to 98 % of the live pixels are merged, runs fill whole lane groups, cells change in
mid-run, masked, out-of-view and dropped pixels sit inside open cells, runs sit in clamped cells (u == A - 1: two of the four
flushed taps are one address), and a texel is fed by several lane groups and tiles.  tests/test_cell_runs_cpu.py checks all of
that on the inputs, holds the references' own fp32 runs inside the gates, and shows that the gradient gate sees one lost pixel.

Gates: those of tests/test_lm_kernels_vs_fp64.py, tests/test_pose_score_gpu.py and tests/test_pose_score_bwd_gpu.py, unchanged and
imported from there.  Measured ratios (printed by the gates): EXPERIMENTS.md, "Cell runs: coherent ground tables"."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import pose_score_bwd_ref as PB
import pose_score_ref as PS
from test_lm_kernels_vs_fp64 import _Call, _backward_pose0, _forward_pose0, _gate_all_grads, _lambda, _reference_grads
from test_pose_score_gpu import _call, _gate as _gate_score, _gate_out_of_view, _score
from test_pose_score_bwd_gpu import _bwd, _gate as _gate_psb
from test_pose_score_bwd_gpu import test_ground_gradients_are_bitwise_reproducible_and_independent_of_the_batch as _reproducible

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
POSES = (None, R.COHERENT_POSE)


# ----------------------------------------------------------------------------------------------------------------------
# lm_bwd_accum
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('case', R.COHERENT_CASES, ids=str)
def test_lm_backward_on_cell_runs(case, using_weight):
    """One level, one step, from pose 0 (runs in clamped cells) and from a rotated pose: every channel count (RUN = 2, 8, 16 and
    32 pixels per lane group at 128-pixel tiles), both chains, A = 13, 256-pixel tiles with RUN = 16 ('mid'), stored rows offset
    by grd_row_skip, B = 9."""
    for pose in POSES:
        call, coef, out = _backward_pose0(*case, using_weight, pose=pose, level=R.coherent_level(*case))
        assert bool(out[0][0].any())
        # zero-filled ground-gradient rows that every visit adds to: the same bits as the overwriting first visit
        acc = call.backward(coef, overwrite=0)
        assert torch.equal(acc[1][0], out[1][0]) and torch.equal(acc[2][0], out[2][0])


@pytest.mark.parametrize('ford,level_first,use_keep,using_weight', R.COHERENT_TWO_LEVEL_CASES)
def test_lm_backward_two_levels_on_cell_runs(ford, level_first, use_keep, using_weight):
    """Two levels x two iterations from rotated start poses: the cells move from step to step while each launch closes the step
    before; with dropout masks a dropped pixel sits inside an open cell.  One sample never has a pixel in view."""
    geom, levels, p0, rand_uv, keep = R.coherent_two_level_case(ford, level_first)
    B, out_b = 3, 1
    call = _Call(geom, levels, N=2, level_first=level_first, using_weight=using_weight, keep=keep if use_keep else None, damping=_lambda())
    call.forward(p0, rand_uv)
    coef = torch.from_numpy(np.random.RandomState(R.case_seed('coherent2', ford, level_first) + 3).standard_normal((B, 2, 2, 3)))
    lvs, dparam = _reference_grads(geom, levels, p0, rand_uv, 2, level_first, using_weight, coef, keep, bool(use_keep))
    tag = f"bwd cell runs two levels {'ford' if ford else 'kitti'} lf{level_first} keep{use_keep} w{using_weight}"
    out = call.backward(coef, overwrite=1)
    _gate_all_grads(tag, levels, lvs, dparam, using_weight, *out)
    acc = call.backward(coef, overwrite=0)
    for l in range(2):
        assert torch.equal(acc[1][l], out[1][l]), l
        assert not bool(out[0][l][out_b].any()) and not bool(lvs[l].sat.grad[out_b].any())


def _one_sample(geom, lv, b):
    one = SimpleNamespace(**vars(lv))
    one.sat, one.grd, one.conf = lv.sat[b:b + 1].contiguous(), lv.grd[b:b + 1].contiguous(), lv.conf[b:b + 1].contiguous()
    return R.make_geom(geom.ford, 1), one


@pytest.mark.parametrize('shape,B', [('ragged', 3), ('mid', 2)])
def test_lm_backward_deterministic_mode_on_cell_runs(shape, B):
    """cfg.deterministic rounds a MERGED sum once to the sample's quantum: inside the gradient gate, no range overflow reported,
    two calls bitwise equal, and sample 1 alone (B = 1) gives the d_sat bits it has in the batch -- the quantum and the lane-group
    map depend on the sample and the level only."""
    case = (0, shape, 64, 16, B)
    geom, lv = R.coherent_level(*case)
    for pose in POSES:
        call, coef, out = _backward_pose0(*case, 1, deterministic=1, pose=pose, level=(geom, lv))
        assert float(out[3][3]) == 0.0
        again = call.backward(coef, overwrite=1, deterministic=1)
        for a, b in zip(out[:3], again[:3]):
            assert torch.equal(a[0], b[0])
        assert torch.equal(out[3], again[3]) and bool(out[0][0].any())
        b = 1
        geom1, lv1 = _one_sample(geom, lv, b)
        alone = _Call(geom1, [lv1], using_weight=1, damping=_lambda())
        alone.forward(call.p0[b:b + 1].cpu(), torch.zeros(1, 2, 1))
        one = alone.backward(coef[b:b + 1], overwrite=1, deterministic=1)
        assert float(one[3][3]) == 0.0 and torch.equal(one[0][0][0], out[0][0][b])


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['fp32', 'fp16', 'bf16'])
def test_lm_forward_sums_on_cell_runs(dtype, using_weight):
    case = (0, 'ragged', 64, 16, 3)
    _forward_pose0(*case, dtype, using_weight, level=R.coherent_level(*case, dtype))


# ----------------------------------------------------------------------------------------------------------------------
# ps_accum / psb_accum
# ----------------------------------------------------------------------------------------------------------------------
def _run(case):
    c = PB.reference(case)
    w, out_k = case[5], case[7]
    call = _call(c['geom'], c['run_lv'], w)
    cost, sums = _score(call, c['poses'])
    _gate_score(f'cell runs {case}', cost, sums, PS.score(R.cast_geom(c['geom'], F64), c['ref_lv'], c['poses'], w), w)
    if out_k is not None:
        _gate_out_of_view(str(case), cost, sums, out_k, w)
    got = _bwd(call, c['poses'], sums, c['d_cost'])
    _gate_psb(f'cell runs {case}', got, c, c['run_lv'])
    return c, call, sums, got


@pytest.mark.parametrize('case', PB.RUN_CASES, ids=str)
def test_pose_score_forward_and_backward_on_cell_runs(case):
    """Every channel count with and without weights (1 to 9 tiles of 'ragged'), 33 tiles x 33 hypotheses on 'mid', and the Ford
    chain with A = 13; hypotheses within 1.2 px and 1 degree of the zero pose, so that each keeps the table's cell runs."""
    _run(case)


@pytest.mark.parametrize('case', [PB.RUN_CASES[3], PB.RUN_CASES[-1]], ids=str)
def test_pose_score_backward_on_cell_runs_is_reproducible_and_independent_of_the_batch(case):
    """d_grd and d_conf bitwise equal across two runs and against sample 1 alone; d_sat inside the gate each time."""
    _reproducible(case)


def test_pose_score_backward_of_a_row_in_one_cell():
    """The only cotangent belongs to the zero pose, under which the step-0 row of 'ragged' lies in one cell: the lane groups that
    walk it flush once each, all to the same four texels."""
    case = PB.RUN_CASES[3]                               # C = 64 with weights
    c = PB.reference(case)
    call = _call(c['geom'], c['run_lv'], case[5])
    _, sums = _score(call, c['poses'])
    only = torch.zeros_like(c['d_cost'])
    only[:, 0] = 1.5
    assert bool((c['poses'][:, 0] == 0).all())
    got = _bwd(call, c['poses'], sums, only)
    ref, T = PB.grads(R.cast_geom(c['geom'], F64), c['ref_lv'], c['poses'], case[5], c['sums'], only)
    assert bool((got[0] != 0).any())
    for name, a, b, t in zip(('d_sat', 'd_grd', 'd_conf'), got, ref, T):
        ratio, zeros = PB.worst_ratio(a, b, t)
        print(f'PSB one cell {name}: worst |hip - ref64| / T = {ratio:.2e} (limit {PB.TOL:.2e})')
        assert zeros and ratio <= PB.TOL, (name, ratio)
