"""``hla_g2s_pose_score_bwd`` (csrc/g2s_pose_score.hip: gpsb_coef, gpsb_accum in its geo, weighted and in-plane instantiations)
against the closed-form fp64 reference of tests/g2s_pose_score_bwd_ref.py, through the C ABI with the hand-made levels of
tests/test_g2s_pose_score_gpu.py.  The kernel gets the FORWARD kernel's sums, as a caller would hand them over.

Gate (not measured on the kernel): elementwise |hip - ref64| <= TOL * T, T = the reference's sum of the absolute values of the
element's terms, TOL = twice the worst ratio of the reference's own fp32 run (``g2s_pose_score_bwd_ref.REF32_WORST``,
tests/test_g2s_pose_score_bwd_ref_cpu.py); an element with T = 0 must be exactly zero.  The measured ratios are printed.
Also: every output buffer starts as a sentinel and all outputs are finite; d_sat bitwise equal across two runs and across B (a
sample alone against the same sample in its batch), d_grd and d_conf (fp32 atomics) inside the gate both times; a cotangent on the
out-of-view hypothesis alone, or none at all, leaves exact zeros; without weights d_grd_conf is not touched; refusals."""
import ctypes as C

import pytest
import torch

import g2s_geo_ref as R
import g2s_pose_score_bwd_ref as GB
import g2s_pose_score_ref as GP
from test_g2s_pose_score_gpu import _Call, _same

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
SENTINEL = 7.25
NAMES = ('d_sat', 'd_grd', 'd_conf')


def _bwd(call, l, poses, sums, d_cost, ws_short=0):
    """-> (d_sat [B,C,A,A], d_grd [B,C,h,w], d_conf [B,1,h,w]) fp32 on the CPU, of level ``l`` of ``call``.  Every output buffer
    is handed over holding SENTINEL; without weights d_conf must come back untouched and is returned as zeros."""
    lib, _lib, d = call.lib, call._lib, call.dev
    p = poses.float().contiguous().to(d)
    B, K = p.shape[:2]
    sat, grd = call.feats[0][l], call.feats[1][l]
    d_sat, d_grd = torch.full_like(sat, SENTINEL), torch.full_like(grd, SENTINEL)
    d_conf = torch.full(tuple(grd.shape[:3]), SENTINEL, device=d, dtype=F32)
    gr = _lib.S2GLevelGrad()
    gr.d_sat_feat, gr.d_grd_feat, gr.d_grd_conf = d_sat.data_ptr(), d_grd.data_ptr(), d_conf.data_ptr()
    s, dc = sums.double().contiguous().to(d), d_cost.float().contiguous().to(d)
    assert tuple(s.shape) == (B, K, 8) and tuple(dc.shape) == (B, K)
    lvl = C.byref(call.lv[l])
    nbytes = lib.hla_g2s_pose_score_bwd_workspace_bytes(C.byref(call.cfg), lvl, B, K)
    if nbytes == 0:
        _lib.check(-1, 'hla_g2s_pose_score_bwd_workspace_bytes')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    rc = lib.hla_g2s_pose_score_bwd(C.byref(call.cfg), lvl, C.byref(gr), _lib.ptr(call.Kdev), int(call.hw[0]), int(call.hw[1]),
                                    _lib.ptr(p), K, _lib.ptr(s), _lib.ptr(dc), _lib.ptr(ws), nbytes - ws_short, B, _lib.stream_ptr())
    _lib.check(rc, 'hla_g2s_pose_score_bwd')
    torch.cuda.synchronize()
    if not call.cfg.using_weight:
        assert (d_conf == SENTINEL).all()
        d_conf = torch.zeros_like(d_conf)
    return d_sat.permute(0, 3, 1, 2).cpu(), d_grd.permute(0, 3, 1, 2).cpu(), d_conf[:, None].cpu()


def _gate(tag, got, ref, T):
    worst = []
    for name, a, b, t in zip(NAMES, got, ref, T):
        assert torch.isfinite(a).all(), (tag, name)
        ratio, zeros = GB.worst_ratio(a, b, t)
        print(f'GPSB {tag} {name}: worst |hip - ref64| / T = {ratio:.2e} (limit {GB.TOL:.2e})')
        worst.append((name, ratio, zeros))
    for name, ratio, zeros in worst:
        assert zeros and ratio <= GB.TOL, (tag, name, ratio, zeros)


def _run(case):
    r = GB.reference(case)
    call = _Call(r.c, r.w)
    _, sums = call.score(r.l, r.poses)
    got = _bwd(call, r.l, r.poses, sums, r.d_cost)
    _gate(GB.case_id(case), got, r.grads, r.T)
    return r, call, sums, got


@pytest.mark.parametrize('case', GB.CASES, ids=GB.case_id)
def test_gradients_against_the_closed_form(case):
    """geo: A = 7 under one tile at C = 256 / 128 / 64, the border, behind, out, mid (many tiles), deferred and B = 9 cases with
    and without weights; in-plane: C = 16 .. 256; K = 1, 33 and 70 (across the 32-hypothesis batch); 'crowded' (runs of pixels in
    one texel cell).  d_cost has exact zeros; one hypothesis is out of view."""
    _run(case)


@pytest.mark.parametrize('case', [GB.CASES[1], GB.CROWDED], ids=GB.case_id)
def test_out_of_view_or_no_cotangent_leaves_exact_zeros(case):
    r = GB.reference(case)
    call = _Call(r.c, r.w)
    _, sums = call.score(r.l, r.poses)
    rows = GP.far_out_rows(r.c)
    assert len(rows) == r.c.B and (sums[:, r.out_k, 6] == 0).all()
    only = torch.zeros_like(r.d_cost)
    only[:, r.out_k] = 1.5
    for dc in (only, torch.zeros_like(only)):
        got = _bwd(call, r.l, r.poses, sums, dc)
        assert all((t == 0).all() for t in got)


@pytest.mark.parametrize('case', [GB.CASES[19], GB.CASES[21], GB.CROWDED], ids=GB.case_id)
def test_d_sat_is_bitwise_reproducible_and_independent_of_the_batch(case):
    """Twice in a row; then sample 1 alone (B = 1) against itself in the batch (B = 9 takes the XCD-affine block map, B = 1 does
    not).  d_grd and d_conf (fp32 atomics) are inside the gate both times."""
    r, call, sums, first = _run(case)
    again = _bwd(call, r.l, r.poses, sums, r.d_cost)
    _gate(f'{GB.case_id(case)} again', again, r.grads, r.T)
    assert _same(first[0], again[0])
    b = 1
    one = R.take(r.c, [b])
    one.proj = r.c.proj
    call1 = _Call(one, r.w)
    _, sums1 = call1.score(r.l, r.poses[b:b + 1])
    assert _same(sums1[0], sums[b])
    alone = _bwd(call1, r.l, r.poses[b:b + 1], sums1, r.d_cost[b:b + 1])
    assert _same(alone[0][0], first[0][b])
    _gate(f'{GB.case_id(case)} alone', alone, [t[b:b + 1] for t in r.grads], [t[b:b + 1] for t in r.T])


def test_refusals():
    """16-bit maps, a dropout mask, a depth map, cfg->deterministic, grd_row_skip != 0 and a workspace one byte short: an error,
    not a crash, and a good call afterwards still passes the gate."""
    from highlyaccurate_amd._lib import HLA_F16, HlaError
    case = GB.CASES[4]                                    # shape 7 x 7, C = 64, no weights
    r = GB.reference(case)
    good = _Call(r.c, r.w)
    _, sums = good.score(r.l, r.poses)
    dummy = torch.zeros(16, device=good.dev)
    call = _Call(r.c, r.w)
    call.lv[r.l].feat_dtype = HLA_F16
    with pytest.raises(HlaError, match='fp32 feature maps only'):
        _bwd(call, r.l, r.poses, sums, r.d_cost)
    call = _Call(r.c, r.w)
    call.cfg.keep, call.cfg.keep_stride = dummy.data_ptr(), 16
    with pytest.raises(HlaError, match='keep'):
        _bwd(call, r.l, r.poses, sums, r.d_cost)
    call = _Call(r.c, r.w)
    call.lv[r.l].depth = dummy.data_ptr()
    with pytest.raises(HlaError, match='depth'):
        _bwd(call, r.l, r.poses, sums, r.d_cost)
    call = _Call(r.c, r.w)
    call.cfg.deterministic = 1
    with pytest.raises(HlaError, match='deterministic'):
        _bwd(call, r.l, r.poses, sums, r.d_cost)
    call = _Call(r.c, r.w)
    call.lv[r.l].grd_row_skip = 1
    with pytest.raises(HlaError, match='grd_row_skip'):
        _bwd(call, r.l, r.poses, sums, r.d_cost)
    with pytest.raises(HlaError, match='workspace'):
        _bwd(good, r.l, r.poses, sums, r.d_cost, ws_short=1)
    got = _bwd(good, r.l, r.poses, sums, r.d_cost)
    _gate('after the refusals', got, r.grads, r.T)
