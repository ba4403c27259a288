"""``hla_s2g_pose_score_bwd`` (csrc/pose_score.hip: psb_coef, psb_accum) against the closed-form fp64 reference of
tests/pose_score_bwd_ref.py, through the C ABI with the hand-made border levels of tests/lm_kernel_ref.py, like
tests/test_pose_score_gpu.py.  The kernel gets the FORWARD kernel's sums, as a caller would hand them over.

Gate (not measured on the kernel): elementwise |hip - ref64| <= TOL * T, T = the reference's sum of the absolute values of the
element's terms.  TOL = 6.12e-4 = twice the worst ratio of the reference's own fp32 run (3.06e-4, d_sat at K = 33;
tests/test_pose_score_bwd_ref_cpu.py), because that run does not stay inside the project's TOL_SUM = 2e-6 on this scale; an
element with T = 0 must be exactly zero.  The measured ratios are printed.
Also: all outputs finite; stored ground rows above row0 exactly zero; d_grd and d_conf bitwise equal across two runs and across B
(a sample alone against the same sample in a batch), d_sat inside the gate both times; the out-of-view hypothesis leaves d_sat
untouched; refusals."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import lm_kernel_ref as R
import pose_score_bwd_ref as PB
import pose_score_ref as PS
from test_lm_kernels_vs_fp64 import _Call
from test_pose_score_gpu import _call, _same, _score

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
SENTINEL = 7.25


def _bwd(call, poses, sums, d_cost, ws_short=0):
    """-> (d_sat [B,C,A,A], d_grd [B,C,hs,w] (stored rows), d_conf [B,1,hs,w]) fp32 on the CPU, of level 0 of ``call``.  Every
    output buffer is handed over holding SENTINEL."""
    lib, _lib, d = call.lib, call._lib, call.dev
    p = poses.float().contiguous().to(d)
    B, K = p.shape[:2]
    sat, grd, conf, _ = call.t[0]
    d_sat, d_grd, d_conf = [torch.full_like(t, SENTINEL, dtype=F32) for t in (sat, grd, conf)]
    gr = _lib.S2GLevelGrad()
    gr.d_sat_feat, gr.d_grd_feat = d_sat.data_ptr(), d_grd.data_ptr()
    gr.d_grd_conf = d_conf.data_ptr() if call.cfg.using_weight else 0
    s, dc = sums.double().contiguous().to(d), d_cost.float().contiguous().to(d)
    assert tuple(s.shape) == (B, K, 8) and tuple(dc.shape) == (B, K)
    lvl = C.byref(call.lv[0])
    nbytes = lib.hla_s2g_pose_score_bwd_workspace_bytes(C.byref(call.cfg), lvl, B, K)
    assert nbytes > 0, lib.hla_last_error()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    rc = lib.hla_s2g_pose_score_bwd(C.byref(call.cfg), lvl, C.byref(gr), _lib.ptr(call.R_FL), _lib.ptr(call.T_FL), _lib.ptr(p), K,
                                    _lib.ptr(s), _lib.ptr(dc), _lib.ptr(ws), nbytes - ws_short, B, _lib.stream_ptr())
    _lib.check(rc, 'hla_s2g_pose_score_bwd')
    torch.cuda.synchronize()
    if not call.cfg.using_weight:
        assert (d_conf == SENTINEL).all()
        d_conf = torch.zeros_like(d_conf)
    return d_sat.permute(0, 3, 1, 2).cpu(), d_grd.permute(0, 3, 1, 2).cpu(), d_conf[:, None].cpu()


def _gate(tag, got, c, lv):
    """Kernel outputs against the reference dict of PB.reference (stored ground rows: skip..)."""
    ref = [c['grads'][0]] + [t[:, :, lv.skip:] for t in c['grads'][1:]]
    T = [c['T'][0]] + [t[:, :, lv.skip:] for t in c['T'][1:]]
    worst = []
    for name, a, b, t in zip(('d_sat', 'd_grd', 'd_conf'), got, ref, T):
        assert torch.isfinite(a).all(), (tag, name)
        ratio, zeros = PB.worst_ratio(a, b, t)
        print(f'PSB {tag} {name}: worst |hip - ref64| / T = {ratio:.2e} (limit {PB.TOL:.2e})')
        worst.append((name, ratio, zeros))
    for name, ratio, zeros in worst:
        assert zeros and ratio <= PB.TOL, (tag, name, ratio, zeros)
    top = lv.row0 - lv.skip
    assert (got[1][:, :, :top] == 0).all() and (got[2][:, :, :top] == 0).all(), tag


def _run(case):
    c = PB.reference(case)
    w = case[5]
    call = _call(c['geom'], c['run_lv'], w, c['inv'])
    _, sums = _score(call, c['poses'])
    got = _bwd(call, c['poses'], sums, c['d_cost'])
    _gate(str(case), got, c, c['run_lv'])
    return c, call, sums, got


@pytest.mark.parametrize('case', PB.CASES, ids=str)
def test_gradients_against_the_closed_form(case):
    """The C x weights grid on 'ragged'; both chains with A = 13 and 16, fewer pixels than a tile, rows offset by grd_row_skip, many
    tiles, B = 9; K = 1, 33 and 70 (across PS_KC = 32); deferred norms.  d_cost has exact zeros; one hypothesis is out of view."""
    _run(case)


def test_out_of_view_hypothesis_leaves_d_sat_untouched():
    """Only the out-of-view hypothesis carries a cotangent: d_sat is exactly zero, d_grd is the ground map's own norm term."""
    case = PB.CASES[3]                                   # C = 64 with weights
    c = PB.reference(case)
    call = _call(c['geom'], c['run_lv'], case[5])
    _, sums = _score(call, c['poses'])
    only = torch.zeros_like(c['d_cost'])
    only[:, PS.OUT_K] = 1.5
    assert (sums[:, PS.OUT_K, 6] == 0).all()
    d_sat, d_grd, d_conf = _bwd(call, c['poses'], sums, only)
    assert (d_sat == 0).all() and (d_grd != 0).any() and (d_conf != 0).any()
    ref, T = PB.grads(R.cast_geom(c['geom'], F64), c['ref_lv'], c['poses'], case[5], c['sums'], only)
    for a, b, t in zip((d_grd, d_conf), ref[1:], T[1:]):
        ratio, zeros = PB.worst_ratio(a, b, t)
        assert zeros and ratio <= PB.TOL, ratio
    none = _bwd(call, c['poses'], sums, torch.zeros_like(only))          # and no cotangent at all: everything is cleared
    assert all((t == 0).all() for t in none)


@pytest.mark.parametrize('case', [PB.CASES[3], PB.CASES[-4]], ids=str)
def test_ground_gradients_are_bitwise_reproducible_and_independent_of_the_batch(case):
    """Twice in a row; then sample 1 alone (B = 1) against itself in the batch.  d_sat (fp32 atomics) is inside the gate both times."""
    c, call, sums, first = _run(case)
    again = _bwd(call, c['poses'], sums, c['d_cost'])
    _gate(f'{case} again', again, c, c['run_lv'])
    assert _same(first[1], again[1]) and _same(first[2], again[2])
    b = 1
    lv = c['run_lv']
    one = SimpleNamespace(**vars(lv))
    one.sat, one.grd, one.conf = lv.sat[b:b + 1].contiguous(), lv.grd[b:b + 1].contiguous(), lv.conf[b:b + 1].contiguous()
    call1 = _call(R.make_geom(case[0], 1), one, case[5])
    cost1, sums1 = _score(call1, c['poses'][b:b + 1])
    assert _same(sums1[0], sums[b])
    alone = _bwd(call1, c['poses'][b:b + 1], sums1, c['d_cost'][b:b + 1])
    assert _same(alone[1][0], first[1][b]) and _same(alone[2][0], first[2][b])
    ratio, zeros = PB.worst_ratio(alone[0][0], c['grads'][0][b], c['T'][0][b])
    assert zeros and ratio <= PB.TOL


def test_refusals():
    """16-bit maps, a dropout mask, a depth map, cfg->deterministic and a short workspace: an error, not a crash."""
    from highlyaccurate_amd._lib import HlaError
    case = PB.CASES[2]
    c = PB.reference(case)
    poses, dc = c['poses'], c['d_cost']
    good = _call(c['geom'], c['run_lv'], 0)
    _, sums = _score(good, poses)
    dummy = torch.zeros(16, device=good.dev)
    lv16 = R.make_level(0, 'ragged', 64, 16, 3, 5, dtype=torch.float16)
    with pytest.raises((HlaError, AssertionError), match='16-bit'):
        _bwd(_call(c['geom'], lv16, 0), poses, sums, dc)
    call = _call(c['geom'], c['run_lv'], 0)
    call.cfg.keep, call.cfg.keep_stride = dummy.data_ptr(), 16
    with pytest.raises((HlaError, AssertionError), match='keep'):
        _bwd(call, poses, sums, dc)
    call = _call(c['geom'], c['run_lv'], 0)
    call.lv[0].depth = dummy.data_ptr()
    with pytest.raises((HlaError, AssertionError), match='depth'):
        _bwd(call, poses, sums, dc)
    call = _call(c['geom'], c['run_lv'], 0)
    call.cfg.deterministic = 1
    with pytest.raises((HlaError, AssertionError), match='deterministic'):
        _bwd(call, poses, sums, dc)
    with pytest.raises(HlaError, match='workspace'):
        _bwd(good, poses, sums, dc, ws_short=1)
    got = _bwd(good, poses, sums, dc)                     # and the library is fine afterwards
    assert all(torch.isfinite(t).all() for t in got)
