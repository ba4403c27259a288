"""``hla_s2g_pose_score`` (csrc/pose_score.hip: ps_accum, ps_close) against the fp64 reference of tests/pose_score_ref.py, through
the C ABI with the hand-made border levels of tests/lm_kernel_ref.py (pixels on, just inside and just outside every map border,
far-corner cells, texels), like tests/test_lm_kernels_vs_fp64.py.

Gates (none of them measured on the kernel):
  sums    |hip - ref64| <= 2e-6 * T_k, T_k = the reference's fp64 sum of the absolute values of slot k's terms (the LM kernels'
          TOL_SUM; tests/test_pose_score_ref_cpu.py shows the fp32 run of the reference itself inside it on every case used here).
          fp16 / bf16 maps are rounded on the host and the reference reads the rounded values: the same gate
  counts  slots 6 and 7 exact
  cost    |cost - f(sums_hip)| <= 4.8e-7, f = the header's formula in fp64 on the kernel's own sums; 4.8e-7 is one fp32 ulp at 4,
          the cost's upper bound
  bitwise a hypothesis alone, first or last among 70, in any K, twice: identical sums and cost"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import pose_score_ref as PS
from test_lm_kernels_vs_fp64 import _Call

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
TOL_SUM, TOL_COST = 2e-6, 4.8e-7
KC = 32                  # PS_KC of csrc/pose_score.hip: hypotheses per block (K = 33 and 70 cross it)


def _score(call, poses):
    """poses [B,K,3] -> (cost [B,K] fp32, sums [B,K,8] fp64) on the CPU, of level 0 of ``call``."""
    lib, _lib, d = call.lib, call._lib, call.dev
    p = poses.float().contiguous().to(d)
    B, K = p.shape[:2]
    assert B == call.B and p.shape[2] == 3
    cost = torch.full((B, K), float('nan'), device=d, dtype=F32)
    sums = torch.full((B, K, 8), float('nan'), device=d, dtype=F64)
    lvl = C.byref(call.lv[0])
    nbytes = lib.hla_s2g_pose_score_workspace_bytes(C.byref(call.cfg), lvl, B, K)
    assert nbytes > 0, lib.hla_last_error()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    rc = lib.hla_s2g_pose_score(C.byref(call.cfg), lvl, _lib.ptr(call.R_FL), _lib.ptr(call.T_FL), _lib.ptr(p), K, _lib.ptr(sums),
                                _lib.ptr(cost), _lib.ptr(ws), nbytes, B, _lib.stream_ptr())
    _lib.check(rc, 'hla_s2g_pose_score')
    torch.cuda.synchronize()
    return cost.cpu(), sums.cpu()


def _call(geom, lv, using_weight, inv_norm=None):
    call = _Call(geom, [lv], using_weight=using_weight, inv_norm=[inv_norm] if inv_norm is not None else None)
    call.cfg.count_in_view = 0
    return call


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _gate(tag, cost, sums, ref, using_weight):
    """Kernel outputs against the reference tuple of PS.score (fp64)."""
    rs, mags, counts, rcost, _ = ref
    got = sums[..., :6].numpy()
    assert np.isfinite(sums.numpy()).all() and np.isfinite(cost.numpy()).all(), tag
    err = np.abs(got - rs.numpy())
    m = mags.numpy()
    ratio = (err / np.where(m > 0, m, 1.0)).max()
    print(f'PS sums {tag}: worst |hip - ref64| / T_k = {ratio:.2e} (limit {TOL_SUM:.0e})')
    assert (err <= TOL_SUM * m).all(), (tag, (err / np.where(m > 0, m, 1.0)).reshape(-1, 6).max(0))
    assert np.array_equal(sums[..., 6:8].numpy(), counts.double().numpy()), (tag, sums[..., 6:8], counts)
    f = PS.cost_from_sums(sums)
    cerr = (cost.double() - f).abs().max().item()
    print(f'PS cost {tag}: |cost - f(sums)| = {cerr:.2e} (limit {TOL_COST:.1e}); |cost - ref64 cost| = {(cost.double() - rcost).abs().max():.2e}')
    assert cerr <= TOL_COST, (tag, cerr)
    if not using_weight:
        assert _same(sums[..., 3:6], sums[..., 0:3]), tag


def _gate_out_of_view(tag, cost, sums, k, using_weight):
    assert (sums[:, k][:, [0, 2, 3, 5, 6]] == 0).all(), (tag, sums[:, k])
    assert (sums[:, k, 7] > 0).all()
    if not using_weight:
        assert (cost[:, k] == 1).all(), (tag, cost[:, k])


_LEVELS = {}


def _level(ford, shape, Cn, A, B, dtype=F32):
    key = (ford, shape, Cn, A, B, dtype)
    if key not in _LEVELS:
        _LEVELS[key] = (R.make_geom(ford, B), R.make_level(ford, shape, Cn, A, B, R.case_seed(ford, shape, Cn, A, B), dtype=dtype))
    return _LEVELS[key]


def _case(ford, shape, Cn, A, B, w, dtype=F32, inv_norm=None):
    geom, lv = _level(ford, shape, Cn, A, B, dtype)
    poses = PS.hypotheses(B, PS.K_CASE, R.case_seed('ps', ford, shape, Cn, A, B, w), out_of_view=PS.OUT_K)
    ref_lv, run_lv = R.cast_level(lv, F64), lv
    if inv_norm is not None:        # deferred norms: the kernel reads raw maps and rescales its sums; the reference reads raw * inv
        run_lv = R.cast_level(lv, F32)
        for k, iv in zip(('sat', 'grd'), inv_norm):
            raw = (getattr(lv, k) / torch.tensor(iv, dtype=F32).view(-1, 1, 1, 1)).contiguous()
            setattr(run_lv, k, raw)
            setattr(ref_lv, k, raw.double() * torch.tensor(iv, dtype=F64).view(-1, 1, 1, 1))
    ref = PS.score(R.cast_geom(geom, F64), ref_lv, poses, w)
    cost, sums = _score(_call(geom, run_lv, w, inv_norm), poses)
    tag = f"{'ford' if ford else 'kitti'} {shape} C{Cn} A{A} B{B} {str(dtype)[6:]} w{w}" + (' deferred' if inv_norm else '')
    _gate(tag, cost, sums, ref, w)
    _gate_out_of_view(tag, cost, sums, PS.OUT_K, w)
    return cost, sums


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['fp32', 'fp16', 'bf16'])
@pytest.mark.parametrize('Cn', [16, 64, 128, 256])
def test_border_classes_every_width_and_map_type(Cn, dtype, using_weight):
    _case(0, 'ragged', Cn, 16, 3, using_weight, dtype)


@pytest.mark.parametrize('case', PS.GPU_CASES, ids=str)
def test_chains_shapes_and_batches(case):
    """Both chains with A = 13 and 16; fewer pixels than a tile, stored rows offset by grd_row_skip, many tiles (more than 64 per
    sample: the closing reduction's second round), B = 9 (the XCD-affine block map with idle blocks)."""
    _case(*case)


@pytest.mark.parametrize('using_weight', [0, 1])
def test_deferred_inverse_norms(using_weight):
    _case(0, 'ragged', 128, 16, 3, using_weight, inv_norm=([0.5, 3.0, 1.25], [2.0, 0.75, 1.5]))


# ----------------------------------------------------------------------------------------------------------------------
# K, chunks of hypotheses, and what a hypothesis may not depend on
# ----------------------------------------------------------------------------------------------------------------------
_K70 = {}


def _k70():
    """(geom, lv, poses [B,70,3], reference, kernel cost, kernel sums) of the 70-hypothesis case, made once."""
    if not _K70:
        ford, shape, Cn, A, B, w = 0, 'ragged', 64, 16, 3, 1
        geom, lv = _level(ford, shape, Cn, A, B)
        poses = PS.hypotheses(B, 70, 4242, out_of_view=40)
        ref = PS.score(R.cast_geom(geom, F64), R.cast_level(lv, F64), poses, w)
        cost, sums = _score(_call(geom, lv, w), poses)
        _K70.update(geom=geom, lv=lv, poses=poses, ref=ref, cost=cost, sums=sums, w=w)
    return SimpleNamespace(**_K70)


@pytest.mark.parametrize('K', [1, 2, 7, KC, KC + 1, 70])
def test_any_number_of_hypotheses(K):
    """The first K of 70 hypotheses: inside the gates, and bit for bit what they are among all 70 (K = 33 and 70 cross the
    hypotheses-per-block constant, K = 32 fills one block exactly)."""
    c = _k70()
    cost, sums = _score(_call(c.geom, c.lv, c.w), c.poses[:, :K])
    _gate(f'K{K}', cost, sums, tuple(t[:, :K] for t in c.ref), c.w)
    assert _same(cost, c.cost[:, :K]) and _same(sums, c.sums[:, :K])


def test_hypothesis_alone_first_last_and_repeated():
    c = _k70()
    call = _call(c.geom, c.lv, c.w)
    again = _score(call, c.poses)
    assert _same(again[0], c.cost) and _same(again[1], c.sums)                    # twice in a row
    for k in (0, 33, 69):
        moved = c.poses.clone()
        moved[:, 0], moved[:, 69] = c.poses[:, k], c.poses[:, k]                  # first and last among 70
        cost, sums = _score(call, moved)
        for at in (0, 69):
            assert _same(cost[:, at], c.cost[:, k]) and _same(sums[:, at], c.sums[:, k]), (k, at)
    b, k = 1, 33
    one_lv = SimpleNamespace(**vars(c.lv))
    one_lv.sat, one_lv.grd, one_lv.conf = c.lv.sat[b:b + 1].contiguous(), c.lv.grd[b:b + 1].contiguous(), c.lv.conf[b:b + 1].contiguous()
    cost, sums = _score(_call(R.make_geom(0, 1), one_lv, c.w), c.poses[b:b + 1, k:k + 1])     # alone: B = 1, K = 1
    assert _same(cost[0, 0], c.cost[b, k]) and _same(sums[0, 0], c.sums[b, k])


@pytest.mark.parametrize('ford', [0, 1])
def test_norm_sums_against_the_lm_loop(ford):
    """Second witness: slots 0 and 1 and normal_eq[0, b, 0:2] of hla_s2g_lm_solve started at the same pose, each inside the
    gate around the reference."""
    Cn, A, B, w = 64, 16, 3, 0
    geom, lv = _level(ford, 'ragged', Cn, A, B)
    poses = PS.hypotheses(B, 4, 99 + ford)
    ref = PS.score(R.cast_geom(geom, F64), R.cast_level(lv, F64), poses, w)
    call = _call(geom, lv, w)
    cost, sums = _score(call, poses)
    for k in range(4):
        _, neq = call.forward(poses[:, k], torch.zeros(1, 2, B))
        for slot in (0, 1):
            r, m = ref[0][:, k, slot].numpy(), ref[1][:, k, slot].numpy()
            e_loop, e_score = np.abs(neq[0, :, slot].numpy() - r), np.abs(sums[:, k, slot].numpy() - r)
            print(f'PS witness ford{ford} k{k} slot{slot}: loop {(e_loop / m).max():.2e}, score {(e_score / m).max():.2e} of T_k')
            assert (e_loop <= TOL_SUM * m).all() and (e_score <= TOL_SUM * m).all()


@pytest.mark.parametrize('ford', [0, 1])
@pytest.mark.parametrize('shape,Cn', [('ragged', 128), ('mid', 16)])
def test_planted_minimum(ford, shape, Cn):
    """The ground map is the satellite map sampled (fp64) at hypothesis 2's pose: its cost is <= 1e-5, every other one >= 1
    (fp64 reference: >= 1.9 but for the out-of-view one, tests/test_pose_score_ref_cpu.py)."""
    B = 2
    poses = PS.planted_poses(B)
    geom, lv = PS.planted_level(ford, shape, Cn, 16, B, R.case_seed('planted-level', ford, shape, Cn), 2, poses)
    cost, sums = _score(_call(geom, lv, 0), poses)
    others = cost[:, [k for k in range(poses.shape[1]) if k != 2]]
    print(f'PS planted ford{ford} {shape} C{Cn}: cost[2] = {cost[:, 2].max():.2e}, min other = {others.min():.4f}')
    assert (cost[:, 2] <= 1e-5).all() and (others >= 1).all()
    assert (cost.argmin(1) == 2).all()


def test_refusals():
    """A depth map and a dropout mask are refused with an error, not a crash; so is a bad channel count."""
    geom, lv = _level(0, 'ragged', 64, 16, 3)
    poses = PS.hypotheses(3, 2, 5)
    from highlyaccurate_amd._lib import HlaError
    call = _call(geom, lv, 0)
    dummy = torch.zeros(16, device=call.dev)
    call.lv[0].depth = dummy.data_ptr()
    with pytest.raises((HlaError, AssertionError), match='depth'):
        _score(call, poses)
    call = _call(geom, lv, 0)
    call.cfg.keep, call.cfg.keep_stride = dummy.data_ptr(), 16
    with pytest.raises((HlaError, AssertionError), match='keep'):
        _score(call, poses)
    call = _call(geom, lv, 0)
    call.lv[0].C = 32
    with pytest.raises((HlaError, AssertionError), match='unsupported channel count 32'):
        _score(call, poses)
    cost, sums = _score(_call(geom, lv, 0), poses)          # and the library is fine afterwards
    assert torch.isfinite(cost).all()
