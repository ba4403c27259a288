"""``hla_g2s_pose_score`` (csrc/g2s_pose_score.hip: gps_accum in its geo, weighted and in-plane instantiations, gps_close) against
the fp64 reference of tests/g2s_pose_score_ref.py, through the C ABI with the hand-made levels of tests/g2s_geo_ref.py (per-sample
intrinsics with skew entries, pixels 2^-10 px inside and outside each border of the ground map, an in-bounds pixel behind the
camera, a sample with nothing in view, deferred norms, B = 8 / 9) and in-plane levels with C = 16 .. 256 and ragged last tiles.

Gates (from the project, none of them measured on this kernel; tests/test_g2s_pose_score_ref_cpu.py shows the reference's own fp32
run inside the sum gate on every case used here):
  sums    |hip - ref64| <= 2e-6 * T_k, T_k = the reference's fp64 sum of the absolute values of slot k's terms (TOL_SUM of every
          LM kernel suite); slot 7 the same, and bitwise equal across k
  count   slot 6 exact
  cost    |cost - f(sums_hip)| <= 4.8e-7, f = the header's formula in fp64 on the kernel's own sums; 4.8e-7 is one fp32 ulp at 4,
          the cost's upper bound; +inf compared for equality
  bitwise a hypothesis alone, first or last among 70, in any K, in B = 1 or in the batch, twice: identical sums and cost
Measured errors: EXPERIMENTS.md, "Pose search: LM_G2SP"."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import g2s_geo_ref as R
import g2s_pose_score_ref as GP

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
TOL_SUM, TOL_COST = 2e-6, 4.8e-7
KC = 32                  # GPS_KC of csrc/g2s_pose_score.hip: hypotheses per block (K = 33 and 70 cross it)


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


_NETS = {}


def _net(ranges, uw, proj):
    from highlyaccurate_amd.models_kitti import LM_G2SP
    key = (ranges, uw, proj)
    if key not in _NETS:
        _NETS[key] = LM_G2SP(R.make_args(ranges, N_iters=1, using_weight=uw, proj=proj)).to(_dev())
    return _NETS[key]


class _Call:
    """One case on the GPU: the structs ``LM_G2SP`` itself builds, handed to the C ABI."""

    def __init__(self, c, uw):
        from highlyaccurate_amd import _lib
        d = _dev()
        self._lib, self.lib, self.dev, self.c, self.B = _lib, _lib.load(), d, c, c.B
        self.geo = c.proj == 'geo'
        self.net = _net(c.ranges, uw, c.proj)
        nh = lambda t: t.permute(0, 2, 3, 1).contiguous().to(d)
        sat, grd = R.raw_maps(c)
        self.feats = ([nh(s) for s in sat], [nh(g) for g in grd],
                      [x[:, 0].contiguous().to(d) for x in c.conf] if self.geo else [None] * len(sat))
        self.K = c.K.to(d) if self.geo else None
        self.hw = c.ori_hw if self.geo else (0, 0)
        self.inv = (c.sat_inv.to(d), c.grd_inv.to(d)) if hasattr(c, 'sat_inv') else (None, None)
        self.cfg, self.lv, self.Kdev = self.net._structs(*self.feats, self.K, *self.inv)

    def raw(self, l, poses, K=None, ws_bytes=None, sums=True, cost=True, poses_ptr=True):
        """-> (rc, cost, sums, workspace bytes asked for); outputs start as NaN."""
        lib, _lib, d = self.lib, self._lib, self.dev
        p = poses.float().contiguous().to(d)
        B, Kh = p.shape[:2]
        Kh = Kh if K is None else K
        o_cost = torch.full((B, max(Kh, 1)), float('nan'), device=d, dtype=F32)
        o_sums = torch.full((B, max(Kh, 1), 8), float('nan'), device=d, dtype=F64)
        lvl = C.byref(self.lv[l])
        need = lib.hla_g2s_pose_score_workspace_bytes(C.byref(self.cfg), lvl, B, Kh)
        nbytes = need if ws_bytes is None else ws_bytes
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=d)
        rc = lib.hla_g2s_pose_score(C.byref(self.cfg), lvl, _lib.ptr(self.Kdev), int(self.hw[0]), int(self.hw[1]),
                                    _lib.ptr(p if poses_ptr else None), Kh, _lib.ptr(o_sums if sums else None),
                                    _lib.ptr(o_cost if cost else None), _lib.ptr(ws), nbytes, B, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, o_cost.cpu(), o_sums.cpu(), need

    def score(self, l, poses):
        rc, cost, sums, need = self.raw(l, poses)
        assert need > 0, self.lib.hla_last_error()
        self._lib.check(rc, 'hla_g2s_pose_score')
        return cost, sums


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _gate(tag, cost, sums, ref, using_weight):
    """Kernel outputs against the reference tuple of GP.score (fp64)."""
    rs, mags, counts, rcost, _ = ref
    assert np.isfinite(sums.numpy()).all() and not np.isnan(cost.numpy()).any(), tag
    err = np.abs(sums.numpy() - rs.numpy())
    m = mags.numpy()
    rel = err / np.where(m > 0, m, 1.0)
    print(f'GPS sums {tag}: worst |hip - ref64| / T_k = {rel.max():.2e} (limit {TOL_SUM:.0e}); per slot {np.array2string(rel.reshape(-1, 8).max(0), precision=1)}')
    assert (err <= TOL_SUM * m).all(), (tag, rel.reshape(-1, 8).max(0))
    assert np.array_equal(sums[..., 6].numpy(), counts.double().numpy()), (tag, sums[..., 6], counts)
    assert _same(sums[..., 7], sums[:, :1, 7].expand_as(sums[..., 7])), tag
    f = GP.cost_from_sums(sums)
    seen = counts > 0
    assert torch.equal(torch.isinf(cost), ~seen) and (cost[~seen] > 0).all(), (tag, cost)
    cerr = (cost.double()[seen] - f[seen]).abs().max().item() if bool(seen.any()) else 0.0
    gap = (cost.double()[seen] - rcost[seen]).abs().max().item() if bool(seen.any()) else 0.0
    print(f'GPS cost {tag}: |cost - f(sums)| = {cerr:.2e} (limit {TOL_COST:.1e}); |cost - ref64 cost| = {gap:.2e}')
    assert cerr <= TOL_COST, (tag, cerr)
    if not using_weight:
        assert _same(sums[..., 3:6], sums[..., 0:3]), tag


_REFS = {}


def _ref(c, l, poses, w, tag=''):
    key = (c.name, l, w, tag)
    if key not in _REFS:
        _REFS[key] = GP.score(c, l, poses, w, F64)
    return _REFS[key]


@pytest.mark.parametrize('run', GP.RUNS, ids=GP.run_id)
def test_sums_counts_and_cost_against_fp64(run):
    """A = 7 under one tile at C = 256 / 128 / 64, the border, behind, out, mid (154 tiles per sample at level 1: the closing
    reduction's second round), deferred and B = 8 / 9 cases with and without weights, the in-plane levels C = 16 .. 256."""
    key, l, w = run
    c = GP.get(*key)
    poses = GP.hypotheses(c, l)
    cost, sums = _Call(c, w).score(l, poses)
    _gate(GP.run_id(run), cost, sums, _ref(c, l, poses, w), w)
    rows = GP.far_out_rows(c)
    assert (sums[rows, GP.OUT_K, :7] == 0).all() and (sums[rows, GP.OUT_K, 7] > 0).all() and (cost[rows, GP.OUT_K] == float('inf')).all()
    if getattr(c, 'out', None) is not None:          # the sample with nothing in view at any pose
        assert (sums[c.out, :, :7] == 0).all() and torch.isinf(cost[c.out]).all()


# ----------------------------------------------------------------------------------------------------------------------
# K, chunks of hypotheses, and what a hypothesis may not depend on
# ----------------------------------------------------------------------------------------------------------------------
_K70 = {}


def _k70(proj):
    """(case, level, poses [B,70,3], reference, kernel cost, kernel sums) of the 70-hypothesis case, made once."""
    if proj not in _K70:
        c, l, w, poses = GP.k70(proj)
        ref = _ref(c, l, poses, w, 'k70')
        cost, sums = _Call(c, w).score(l, poses)
        _K70[proj] = SimpleNamespace(c=c, l=l, w=w, poses=poses, ref=ref, cost=cost, sums=sums)
    return _K70[proj]


@pytest.mark.parametrize('proj', ['geo', 'nn'])
@pytest.mark.parametrize('K', [1, 2, 7, KC, KC + 1, 70])
def test_any_number_of_hypotheses(K, proj):
    """The first K of 70 hypotheses: inside the gates, and bit for bit what they are among all 70 (K = 33 and 70 cross the
    hypotheses-per-block constant, K = 32 fills one block exactly)."""
    t = _k70(proj)
    cost, sums = _Call(t.c, t.w).score(t.l, t.poses[:, :K])
    _gate(f'{proj} K{K}', cost, sums, tuple(x[:, :K] for x in t.ref), t.w)
    assert _same(cost, t.cost[:, :K]) and _same(sums, t.sums[:, :K])


@pytest.mark.parametrize('proj', ['geo', 'nn'])
def test_hypothesis_alone_first_last_repeated_and_in_any_batch(proj):
    t = _k70(proj)
    call = _Call(t.c, t.w)
    again = call.score(t.l, t.poses)
    assert _same(again[0], t.cost) and _same(again[1], t.sums)                    # twice in a row
    for k in (0, 33, 69):
        moved = t.poses.clone()
        moved[:, 0], moved[:, 69] = t.poses[:, k], t.poses[:, k]                  # first and last among 70
        cost, sums = call.score(t.l, moved)
        for at in (0, 69):
            assert _same(cost[:, at], t.cost[:, k]) and _same(sums[:, at], t.sums[:, k]), (k, at)
    b, k = 1, 33
    one = R.take(t.c, [b])
    one.proj = t.c.proj
    cost, sums = _Call(one, t.w).score(t.l, t.poses[b:b + 1, k:k + 1])            # alone: B = 1, K = 1
    assert _same(cost[0, 0], t.cost[b, k]) and _same(sums[0, 0], t.sums[b, k])
    if t.c.B == 9:                                                                # another slot, another XCD, the second octet
        idx = [8, 7, 6, 5, 0, 3, 2, 1, 4]
        perm = R.take(t.c, idx)
        perm.proj = t.c.proj
        cost, sums = _Call(perm, t.w).score(t.l, t.poses[idx])
        assert _same(cost, t.cost[idx]) and _same(sums, t.sums[idx])


def test_score_poses_is_the_c_abi_call():
    """``LM_G2SP.score_poses`` with shared [K,3] poses and with per-sample ones: bitwise what the C ABI gives."""
    c, l, w = GP.get('deferred'), 1, 1
    poses = GP.hypotheses(c, l)
    call = _Call(c, w)
    cost, sums = call.score(l, poses)
    got = call.net.score_poses(*call.feats, call.K, call.hw, poses, l, sat_inv_norm=call.inv[0], grd_inv_norm=call.inv[1])
    assert got[0].dtype == F32 and got[1].dtype == F64 and tuple(got[1].shape) == (c.B, GP.K_CASE, 8)
    assert _same(got[0].cpu(), cost) and _same(got[1].cpu(), sums)
    shared = poses[0]
    got = call.net.score_poses(*call.feats, call.K, call.hw, shared, l, sat_inv_norm=call.inv[0], grd_inv_norm=call.inv[1])
    want = call.score(l, shared[None].expand(c.B, -1, -1))
    assert _same(got[0].cpu(), want[0]) and _same(got[1].cpu(), want[1])


@pytest.mark.parametrize('proj', ['geo', 'nn'])
def test_planted_minimum(proj):
    """The satellite map is the ground map projected (fp64) at hypothesis 2's pose wherever that is in view: its cost is <= 1e-5,
    every other hypothesis that sees anything >= 1 (fp64 reference: >= 1.5, tests/test_g2s_pose_score_ref_cpu.py)."""
    c, l, poses = GP.planted(proj)
    cost, sums = _Call(c, 0).score(l, poses)
    others = cost[:, [k for k in range(poses.shape[1]) if k != GP.PLANTED_K]]
    print(f'GPS planted {proj}: cost[2] = {cost[:, GP.PLANTED_K].max():.2e}, min other = {others.min():.4f}')
    assert (cost[:, GP.PLANTED_K] <= 1e-5).all() and (others >= 1).all()
    assert (cost.argmin(1) == GP.PLANTED_K).all() and (cost[:, GP.OUT_K] == float('inf')).all()


def test_non_finite_poses_see_nothing():
    """NaN and infinite pose components: every in-bounds test fails in fp64, nothing is in view, nothing is read."""
    c, l = GP.get('mid'), 0
    poses = GP.hypotheses(c, l).clone()
    poses[:, 1] = torch.tensor([float('nan'), 0.0, 0.0])
    poses[:, 2] = torch.tensor([0.0, float('inf'), 0.0])
    poses[:, 4] = torch.tensor([0.1, 0.1, float('-inf')])
    cost, sums = _Call(c, 1).score(l, poses)
    ref = GP.hypotheses(c, l)
    want = _Call(c, 1).score(l, ref)
    for k in (1, 2, 4):
        assert (sums[:, k, :7] == 0).all() and (cost[:, k] == float('inf')).all()
    for k in (0, 3, 5, 6):
        assert _same(cost[:, k], want[0][:, k]) and _same(sums[:, k], want[1][:, k])


def test_refusals():
    """Bad arguments come back as a status with a message, not a crash, and the library works afterwards."""
    from highlyaccurate_amd._lib import HLA_F16, HlaError
    c, l = GP.get('mid'), 0
    poses = GP.hypotheses(c, l)
    call = _Call(c, 0)
    err = lambda: call.lib.hla_last_error().decode()
    for kw in (dict(poses_ptr=False), dict(sums=False), dict(cost=False)):
        rc, _, _, _ = call.raw(l, poses, **kw)
        assert rc != 0 and 'null argument' in err(), (kw, err())
    rc, _, _, need = call.raw(l, poses, K=0)
    assert rc != 0 and need == 0 and 'K >= 1' in err()
    rc, _, _, need = call.raw(l, poses, ws_bytes=256)
    assert need > 256 and rc != 0 and 'workspace' in err()
    call16 = _Call(c, 0)
    call16.lv[l].feat_dtype = HLA_F16
    rc, _, _, need = call16.raw(l, poses)
    assert rc != 0 and need == 0 and 'fp32 feature maps only' in err()
    nn = _Call(GP.get('nn', 64, 3), 0)
    nn.cfg.using_weight = 1
    rc, _, _, need = nn.raw(0, GP.hypotheses(nn.c, 0))
    assert rc != 0 and need == 0 and 'no weighted variant' in err()
    with pytest.raises(ValueError, match='inconsistent feature maps'):      # the host layer refuses 16-bit maps before the library
        call.net.score_poses([t.half() for t in call.feats[0]], call.feats[1], call.feats[2], call.K, call.hw, poses, l)
    with pytest.raises(HlaError, match='HIP device'):
        call.net.score_poses([t.cpu() for t in call.feats[0]], call.feats[1], call.feats[2], call.K, call.hw, poses, l)
    cost, _ = call.score(l, poses)
    assert torch.isfinite(cost[:, 0]).all()
