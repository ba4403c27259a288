"""Closed-form reference of ``hla_g2s_pose_score_bwd`` (include/hla.h): the gradients of sum_bk d_cost[b,k] cost[b,k] with respect to
the (normalised) satellite map, the ground map and the ground confidence of ONE level, poses held constant, for both projections.
Built on ``g2s_pose_score_ref.uv_of`` / ``in_view`` (the oracle's projections) and the oracle's sampling rules
(``oracle.ref_cpu.grid_sample``: clamped corners, hard in-bounds mask); runs in the dtype of its inputs, so the same code on fp32
inputs is the "ref32" that sizes the gate.

With f the ground feature sampled where satellite pixel p projects, s the satellite feature, w the projected confidence
(using_weight) or 1, N = sums[0], S = sums[1], a = sums[3], e = sums[4], c = sums[5], nf = max(sqrt N, 1e-6), ns alike, per pixel
in view and per channel:
    d cost/d f = 2 w f/nf^2 - 2 a f/nf^4 - 2 w s/(nf ns) + 2 c f/(nf^3 ns)      spread to the four ground taps
    d cost/d s = 2 w s/ns^2 - 2 e s/ns^4 - 2 w f/(nf ns) + 2 c s/(ns^3 nf)      on the satellite pixel itself
    d cost/d w = sum_channels (f/nf - s/ns)^2                                   spread to the same four taps of the confidence
(a clamped norm is a constant: its second and fourth term are absent).  Next to every output element the reference returns T, the
same sum with every term's absolute value -- a term is each product written above (per channel for the confidence), times
|tap weight| and |d_cost|: the scale the gates are stated on."""
from types import SimpleNamespace

import numpy as np
import torch

import g2s_geo_ref as R
import g2s_pose_score_ref as GP
from pose_score_bwd_ref import cost_clamp_const, d_costs, worst_ratio  # noqa: F401  (shared with the S2G reference)

F64, F32 = torch.float64, torch.float32

# The GPU gate, |hip - ref64| <= TOL * T: twice the worst ratio of the reference's OWN fp32 run (maps, coordinates, sums and
# arithmetic in fp32) against its fp64 run over CASES, measured on the CPU by tests/test_g2s_pose_score_bwd_ref_cpu.py, which
# prints the worst ratio of every output: d_sat 5.04e-4, d_grd 4.88e-3, d_conf 4.98e-3, all three on the geo 'border' case (the
# fp32 run forms the bilinear weights from fp32 coordinates, and a satellite pixel close in front of the camera has a (u, v) that
# fp32 holds to a small fraction of a texel only; T takes |f| of the sampled value, not the sum of its taps' magnitudes).  The
# in-plane cases reach 1.6e-4, 'crowded' 1.1e-5.  The margin of 2: the kernel forms its coordinates in fp64, so it should sit well
# inside what the all-fp32 reference reaches.  Not derived from the kernel.
REF32_WORST = 4.98e-3
TOL = 2 * REF32_WORST


def _taps(uv, m, hw, dt):
    """The four clamped-corner taps of ``oracle.ref_cpu.grid_sample`` at uv [B,A,A,2] with the in-view mask m [B,A,A]:
    [(flat texel index [B,1,P] int64, weight [B,1,P] dt, zero out of view)] and the cell (x0, y0) [B,P] of every pixel."""
    h, w = hw
    B = uv.shape[0]
    md = m.reshape(B, 1, -1)
    zero = torch.zeros((), dtype=dt)
    ix = torch.where(md, uv[..., 0].reshape(B, 1, -1), zero)
    iy = torch.where(md, uv[..., 1].reshape(B, 1, -1), zero)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x0c, x1c = x0.clamp(0, w - 1), (x0 + 1).clamp(0, w - 1)
    y0c, y1c = y0.clamp(0, h - 1), (y0 + 1).clamp(0, h - 1)
    inb = md.to(dt)
    wx0, wx1, wy0, wy1 = x1c - ix, ix - x0c, y1c - iy, iy - y0c
    taps = [(y0c, x0c, wx0 * wy0 * inb), (y0c, x1c, wx1 * wy0 * inb), (y1c, x0c, wx0 * wy1 * inb), (y1c, x1c, wx1 * wy1 * inb)]
    return [((yy * w + xx).long(), wgt) for yy, xx, wgt in taps], (x0[:, 0].long(), y0[:, 0].long())


def grads(c, l, poses, using_weight, sums, d_cost, dt=F64, maps=None):
    """Level ``l`` of case ``c`` (g2s_pose_score_ref) at ``poses`` [B,K,3]; sums [B,K,>=6] and d_cost [B,K] (used in dt); maps as
    in ``g2s_pose_score_ref.score``.  -> (d_sat [B,C,A,A], d_grd [B,C,h,w], d_conf [B,1,h,w]), (T_sat, T_grd, T_conf) of the same
    shapes, all in dt; d_conf is zero without weights."""
    sat, grd, conf = maps if maps is not None else R.cast(c, dt)
    sat, grd, conf = sat[l].detach(), grd[l].detach(), conf[l].detach() if conf[l] is not None else None
    B, K = poses.shape[:2]
    A, Cn, (h, w) = c.levels[l]
    sums, d_cost = sums.to(dt), d_cost.to(dt)
    s = sat.reshape(B, Cn, A * A)
    gflat = grd.reshape(B, Cn, h * w)
    cflat = conf.reshape(B, 1, h * w) if using_weight else None
    d_sat, T_sat = torch.zeros_like(s), torch.zeros_like(s)
    d_grd, T_grd = [torch.zeros(B * h * w, Cn, dtype=dt) for _ in range(2)]
    d_conf, T_conf = [torch.zeros(B * h * w, 1, dtype=dt) for _ in range(2)]
    base = (torch.arange(B) * h * w).view(B, 1)
    for k in range(K):
        uv = GP.uv_of(c, l, poses[:, k], dt)
        m = GP.in_view(uv, (h, w))
        taps, _ = _taps(uv, m, (h, w), dt)
        md = m.reshape(B, 1, -1).to(dt)
        f = sum(torch.gather(gflat, 2, idx.expand(B, Cn, -1)) * wgt for idx, wgt in taps)
        wt = sum(torch.gather(cflat, 2, idx) * wgt for idx, wgt in taps) if using_weight else torch.ones_like(md)
        N, S, a, e, cc = [sums[:, k, i].view(B, 1, 1) for i in (0, 1, 3, 4, 5)]
        rf, rs = torch.sqrt(N), torch.sqrt(S)
        ff, fs = (rf >= 1e-6).to(dt), (rs >= 1e-6).to(dt)
        nf, ns = torch.clamp(rf, min=1e-6), torch.clamp(rs, min=1e-6)
        dc = d_cost[:, k].view(B, 1, 1)
        tf = [2 * wt * f / nf ** 2, -ff * 2 * a * f / nf ** 4, -2 * wt * s / (nf * ns), ff * 2 * cc * f / (nf ** 3 * ns)]
        ts = [2 * wt * s / ns ** 2, -fs * 2 * e * s / ns ** 4, -2 * wt * f / (nf * ns), fs * 2 * cc * s / (ns ** 3 * nf)]
        d_sat += sum(ts) * md * dc
        T_sat += sum(t.abs() for t in ts) * md * dc.abs()
        df, Tf = sum(tf) * md * dc, sum(t.abs() for t in tf) * md * dc.abs()
        q = md * ((f / nf - s / ns) ** 2).sum(1, keepdim=True) if using_weight else None
        for idx, wgt in taps:
            at = (base + idx[:, 0]).reshape(-1)
            d_grd.index_add_(0, at, (df * wgt).permute(0, 2, 1).reshape(-1, Cn))
            T_grd.index_add_(0, at, (Tf * wgt.abs()).permute(0, 2, 1).reshape(-1, Cn))
            if using_weight:
                d_conf.index_add_(0, at, (q * dc * wgt).permute(0, 2, 1).reshape(-1, 1))
                T_conf.index_add_(0, at, (q * dc.abs() * wgt.abs()).permute(0, 2, 1).reshape(-1, 1))
    nchw = lambda t, n: t.reshape(B, h, w, n).permute(0, 3, 1, 2).contiguous()
    sq = lambda t: t.reshape(B, Cn, A, A)
    return (sq(d_sat), nchw(d_grd, Cn), nchw(d_conf, 1)), (sq(T_sat), nchw(T_grd, Cn), nchw(T_conf, 1))


def shared_cells(c, l, pose):
    """Per sample, over the row-major neighbouring pairs of satellite pixels that are both in view at ``pose`` [B,3] (fp64):
    -> (pairs that fall into the same texel cell [B], pairs that do not [B])."""
    hw = c.levels[l][2]
    uv = GP.uv_of(c, l, pose, F64)
    m = GP.in_view(uv, hw)
    _, (x0, y0) = _taps(uv, m, hw, F64)
    mf = m.reshape(c.B, -1)
    both = mf[:, 1:] & mf[:, :-1]
    same = (x0[:, 1:] == x0[:, :-1]) & (y0[:, 1:] == y0[:, :-1])
    return (both & same).sum(1), (both & ~same).sum(1)


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
CROWDED_LEVEL = (16, 64, (3, 4))        # A = 16, C = 64 on a ground map of 3 x 4 texels: runs of satellite pixels share a cell


def crowded_case():
    """geo, B = 2, with weights: 256 satellite pixels over the six cells of a 3 x 4 ground map."""
    rs = np.random.RandomState(R._seed('gpsb crowded'))
    c = R._case('crowded', [CROWDED_LEVEL], 2, R.ordinary_K(rs, 2), 1, R._rand_pose(rs, 2))
    c.proj = 'geo'
    return c


_CASES = {}


def get(key):
    if key == ('crowded',):
        if key not in _CASES:
            _CASES[key] = crowded_case()
        return _CASES[key]
    return GP.get(*key)


# (case key, level, using_weight, K): K = K_CASE with hypothesis OUT_K out of view; K = 1, 33, 70 are the first K of the 70
# hypotheses of g2s_pose_score_ref.k70 (hypothesis 40 out of view; 33 and 70 cross the 32-hypothesis coefficient batch)
GEO_RUNS = [(('shape', 7, 256), 0), (('shape', 7, 128), 0), (('shape', 7, 64), 0), (('border',), 0), (('behind',), 0), (('out',), 0),
            (('mid',), 0), (('mid',), 1), (('deferred',), 0), (('octet9',), 0)]
CASES = [(k, l, w, GP.K_CASE) for k, l in GEO_RUNS for w in (0, 1)] + \
        [(k, l, 0, GP.K_CASE) for k, l in GP.NN_RUNS] + \
        [GP.K70[p] + (K,) for p in ('geo', 'nn') for K in (1, 33, 70)] + \
        [(('crowded',), 0, 1, GP.K_CASE)]
CROWDED = CASES[-1]


def case_id(case):
    key, l, w, K = case
    return '-'.join(str(x) for x in key) + f'-L{l}-w{w}-K{K}'


def case_inputs(case):
    """-> (case object, level, using_weight, poses [B,K,3] fp32, d_cost [B,K] fp32, out-of-view hypothesis or None)."""
    key, l, w, K = case
    c = get(key)
    if K == GP.K_CASE:
        poses, out_k = GP.hypotheses(c, l), GP.OUT_K
    else:
        poses = GP.k70('geo' if c.proj == 'geo' else 'nn')[3][:, :K]
        out_k = GP.K70_OUT if K > GP.K70_OUT else None
    dc = d_costs(c.B, K, R._seed('gpsb-dc', c.name, l, w, K), keep=() if out_k is None else (out_k,))
    return c, l, w, poses, dc, out_k


_REF = {}


def reference(case):
    """The fp64 reference of a case, computed once per process: SimpleNamespace(c, l, w, poses, d_cost, out_k, sums [B,K,8],
    counts [B,K], cost, grads (d_sat, d_grd, d_conf), T (the three scales))."""
    if case not in _REF:
        c, l, w, poses, dc, out_k = case_inputs(case)
        sums, _, counts, cost, _ = GP.score(c, l, poses, w, F64)
        g, T = grads(c, l, poses, w, sums, dc, F64)
        _REF[case] = SimpleNamespace(c=c, l=l, w=w, poses=poses, d_cost=dc, out_k=out_k, sums=sums, counts=counts, cost=cost,
                                     grads=g, T=T)
    return _REF[case]
