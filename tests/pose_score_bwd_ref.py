"""Closed-form reference of ``hla_s2g_pose_score_bwd`` (include/hla.h): the gradients of sum_bk d_cost[b,k] cost[b,k] with respect to
the (normalised) satellite map, the ground map and the ground confidence of ONE level, poses held constant.  Built on
``lm_kernel_ref.level_uv`` (the oracle's projections) and the oracle's sampling rules (``oracle.ref_cpu.grid_sample``: clamped
corners, hard in-bounds mask), like tests/pose_score_ref.py; runs in the dtype of its inputs, so the same code on fp32 inputs is
the "ref32" that sizes the gate.

With s, g the masked values, N = sums[0], G = sums[1], a = sums[3], e = sums[4], c = sums[5], ns = max(sqrt N, 1e-6), ng alike,
w = conf x ground mask (using_weight) or the ground mask:
    d cost/d s    = 2 w s/ns^2 - 2 a s/ns^4 - 2 w g/(ns ng) + 2 c s/(ns^3 ng)      pixels in view, spread to the four taps
    d cost/d g    = 2 w g/ng^2 - 2 e g/ng^4 - 2 w s/(ns ng) + 2 c g/(ng^3 ns)      pixels with the ground mask
    d cost/d conf = ground mask x sum_channels (s/ns - g/ng)^2
(a clamped norm is a constant: its second and fourth term are absent).  Next to every output element the reference returns T, the
same sum with every term's absolute value -- a term is each product written above (per channel for conf), times |tap weight| and
|d_cost|: the scale the gates are stated on."""
import numpy as np
import torch

import lm_kernel_ref as R
import pose_score_ref as PS

# The GPU gate, |hip - ref64| <= TOL * T.  The project's TOL_SUM = 2e-6 does not hold for the reference's OWN fp32 run on this scale
# (T takes |s| of the sampled value, not the sum of its taps' magnitudes, and the fp32 run forms the bilinear weights from fp32
# coordinates): its worst ratio over CASES is 3.06e-4 (d_sat, K = 33; d_grd 5.7e-5, d_conf 1.8e-6;
# tests/test_pose_score_bwd_ref_cpu.py prints all of them), so the gate is twice that.  Not derived from the kernel.
REF32_WORST = 3.06e-4
TOL = 2 * REF32_WORST


def grads(geom, lv, poses, using_weight, sums, d_cost):
    """geom / lv as in lm_kernel_ref (maps in dtype dt, channels first); poses [B,K,3]; sums [B,K,>=6] and d_cost [B,K] (used in
    dt).  -> (d_sat [B,C,A,A], d_grd [B,C,h,w], d_conf [B,1,h,w]), (T_sat, T_grd, T_conf) of the same shapes, all in dt; rows above
    row0 of the ground outputs are zero, d_conf is zero without weights."""
    dt = lv.sat.dtype
    B, K = poses.shape[:2]
    Cn, A, r0 = lv.sat.shape[1], lv.A, lv.row0
    sums, d_cost = sums.to(dt), d_cost.to(dt)
    flat = lv.sat.reshape(B, Cn, A * A)
    out = [torch.zeros(B * A * A, Cn, dtype=dt) for _ in range(2)] + [torch.zeros_like(lv.grd) for _ in range(2)] + \
          [torch.zeros_like(lv.conf) for _ in range(2)]
    d_sat, T_sat, d_grd, T_grd, d_conf, T_conf = out
    base = (torch.arange(B) * A * A).view(B, 1)
    for k in range(K):
        uv, _, mask = R.level_uv(geom, lv, R.pose_cols(poses[:, k].to(dt), dt))
        m = mask.expand(B, -1, -1)[:, r0:].reshape(B, 1, -1)
        ix, iy = uv[:, r0:, :, 0].reshape(B, 1, -1), uv[:, r0:, :, 1].reshape(B, 1, -1)
        x0, y0 = torch.floor(ix), torch.floor(iy)
        x0c, x1c = x0.clamp(0, A - 1), (x0 + 1).clamp(0, A - 1)
        y0c, y1c = y0.clamp(0, A - 1), (y0 + 1).clamp(0, A - 1)
        inb = ((ix >= 0) & (ix <= A - 1) & (iy >= 0) & (iy <= A - 1)).to(dt) * m
        wx0, wx1, wy0, wy1 = x1c - ix, ix - x0c, y1c - iy, iy - y0c
        taps = [(y0c, x0c, wx0 * wy0 * inb), (y0c, x1c, wx1 * wy0 * inb), (y1c, x0c, wx0 * wy1 * inb), (y1c, x1c, wx1 * wy1 * inb)]
        taps = [((yy * A + xx).long(), wgt) for yy, xx, wgt in taps]
        s = sum(torch.gather(flat, 2, idx.expand(B, Cn, -1)) * wgt for idx, wgt in taps)
        g = lv.grd[:, :, r0:].reshape(B, Cn, -1) * m
        w = (lv.conf[:, :, r0:].reshape(B, 1, -1) if using_weight else torch.ones_like(m)) * m
        N, G, a, e, c = [sums[:, k, i].view(B, 1, 1) for i in (0, 1, 3, 4, 5)]
        rs, rg = torch.sqrt(N), torch.sqrt(G)
        fs, fg = (rs >= 1e-6).to(dt), (rg >= 1e-6).to(dt)
        ns, ng = torch.clamp(rs, min=1e-6), torch.clamp(rg, min=1e-6)
        dc = d_cost[:, k].view(B, 1, 1)
        ts = [2 * w * s / ns ** 2, -fs * 2 * a * s / ns ** 4, -2 * w * g / (ns * ng), fs * 2 * c * s / (ns ** 3 * ng)]
        tg = [2 * w * g / ng ** 2, -fg * 2 * e * g / ng ** 4, -2 * w * s / (ns * ng), fg * 2 * c * g / (ng ** 3 * ns)]
        ds, Ts = sum(ts) * dc, sum(t.abs() for t in ts) * dc.abs()
        for idx, wgt in taps:
            at = (base + idx[:, 0]).reshape(-1)
            d_sat.index_add_(0, at, (ds * wgt).permute(0, 2, 1).reshape(-1, Cn))
            T_sat.index_add_(0, at, (Ts * wgt.abs()).permute(0, 2, 1).reshape(-1, Cn))
        shape = (B, Cn, lv.h - r0, lv.w)
        d_grd[:, :, r0:] += (sum(tg) * dc).reshape(shape)
        T_grd[:, :, r0:] += (sum(t.abs() for t in tg) * dc.abs()).reshape(shape)
        if using_weight:
            q = (m * ((s / ns - g / ng) ** 2).sum(1, keepdim=True)).reshape(B, 1, lv.h - r0, lv.w)
            d_conf[:, :, r0:] += q * dc.view(B, 1, 1, 1)
            T_conf[:, :, r0:] += q * dc.abs().view(B, 1, 1, 1)
    nchw = lambda t: t.reshape(B, A, A, Cn).permute(0, 3, 1, 2).contiguous()
    return (nchw(d_sat), d_grd, d_conf), (nchw(T_sat), T_grd, T_conf)


def cost_clamp_const(sums):
    """``pose_score_ref.cost_from_sums`` with max(sqrt(x), 1e-6) written as `sqrt(x) where that is at least 1e-6, else the constant
    1e-6`: the same values, and an autograd that is finite where x = 0 (autograd of clamp(sqrt(x)) is 0 x inf = NaN there)."""
    def norm(x):
        big = torch.sqrt(x.detach()) >= 1e-6
        return torch.where(big, torch.sqrt(torch.where(big, x, torch.ones_like(x))), torch.full_like(x, 1e-6))
    ns, ng = norm(sums[..., 0]), norm(sums[..., 1])
    return sums[..., 3] / (ns * ns) + sums[..., 4] / (ng * ng) - 2 * sums[..., 5] / (ns * ng)


def d_costs(B, K, seed, keep=()):
    """[B,K] fp32 cotangents of either sign, about a third of them exactly 0 (never the hypotheses in ``keep``)."""
    rs = np.random.RandomState(seed)
    d = rs.standard_normal((B, K)).astype(np.float32)
    zero = rs.uniform(size=(B, K)) < 0.33
    for k in keep:
        zero[:, k] = False
    d[zero] = 0
    return torch.from_numpy(d)


DEFERRED = ([0.5, 3.0, 1.25], [2.0, 0.75, 1.5])      # inverse norms (sat, grd) of the deferred-norm case, B = 3
# (ford, shape, C, A, B, using_weight, K, out-of-view hypothesis, deferred norms) of every run of tests/test_pose_score_bwd_gpu.py
CASES = [(0, 'ragged', C, 16, 3, w, PS.K_CASE, PS.OUT_K, False) for C in (16, 64, 128, 256) for w in (0, 1)] + \
        [c + (PS.K_CASE, PS.OUT_K, False) for c in PS.GPU_CASES] + \
        [(0, 'ragged', 64, 16, 3, 1, K, (40 if K > 40 else None), False) for K in (1, 33, 70)] + \
        [(0, 'ragged', 128, 16, 3, w, PS.K_CASE, PS.OUT_K, True) for w in (0, 1)]


# The same tuples with a tenth field 'coherent': on the coherent table of lm_kernel_ref (cell runs that psb_accum merges before its
# atomics), every run of tests/test_cell_runs_vs_fp64.py.  The out-of-view hypothesis clears these tables too
# (tests/test_cell_runs_cpu.py).
RUN_CASES = [(0, 'ragged', C, 16, 3, w, PS.K_CASE, PS.OUT_K, False, 'coherent') for C in (16, 64, 128, 256) for w in (0, 1)] + \
            [(0, 'mid', 64, 16, 2, 1, 33, None, False, 'coherent'), (1, 'mid', 16, 13, 2, 1, PS.K_CASE, PS.OUT_K, False, 'coherent')]


# case -> salt of its hypotheses' seed (0 where not listed): see lm_kernel_ref.COHERENT_SALT
RUN_POSE_SALT = {RUN_CASES[1]: 1, RUN_CASES[4]: 8, RUN_CASES[5]: 9}


def case_inputs(case):
    """-> (geom, lv32 as the kernel reads it (raw maps when deferred), inv_norm or None, lv64 the reference reads (normalised maps),
    poses [B,K,3] fp32, d_cost [B,K] fp32)."""
    ford, shape, Cn, A, B, w, K, out_k, deferred = case[:9]
    geom = R.make_geom(ford, B)
    if len(case) > 9:
        assert case[9] == 'coherent'
        lv = R.coherent_level(ford, shape, Cn, A, B)[1]
    else:
        lv = R.make_level(ford, shape, Cn, A, B, R.case_seed(ford, shape, Cn, A, B))
    # (coherent: poses within 1.2 px and 1 degree of the zero pose, so that every hypothesis keeps the table's cell runs)
    salt = (RUN_POSE_SALT.get(case, 0),) if len(case) > 9 else ()
    poses = PS.hypotheses(B, K, R.case_seed('psb', ford, shape, Cn, A, B, w, K, *salt), out_of_view=out_k, lim=0.1 if len(case) > 9 else 0.3)
    dc = d_costs(B, K, R.case_seed('psb-dc', ford, shape, Cn, A, B, w, K), keep=() if out_k is None else (out_k,))
    ref_lv, run_lv, inv = R.cast_level(lv, torch.float64), lv, None
    if deferred:
        inv = DEFERRED
        run_lv = R.cast_level(lv, torch.float32)
        for k, iv in zip(('sat', 'grd'), inv):
            raw = (getattr(lv, k) / torch.tensor(iv, dtype=torch.float32).view(-1, 1, 1, 1)).contiguous()
            setattr(run_lv, k, raw)
            setattr(ref_lv, k, raw.double() * torch.tensor(iv, dtype=torch.float64).view(-1, 1, 1, 1))
    return geom, run_lv, inv, ref_lv, poses, dc


_REF = {}


def reference(case):
    """The fp64 reference of a case, computed once per process: dict(geom, run_lv, inv, ref_lv, poses, d_cost, sums [B,K,6],
    counts, grads (d_sat, d_grd, d_conf), T (the three scales))."""
    if case not in _REF:
        geom, run_lv, inv, ref_lv, poses, dc = case_inputs(case)
        g64 = R.cast_geom(geom, torch.float64)
        sums, _, counts, cost, _ = PS.score(g64, ref_lv, poses, case[5])
        g, T = grads(g64, ref_lv, poses, case[5], sums, dc)
        _REF[case] = dict(geom=geom, run_lv=run_lv, inv=inv, ref_lv=ref_lv, poses=poses, d_cost=dc, sums=sums, counts=counts,
                          cost=cost, grads=g, T=T)
    return _REF[case]


def worst_ratio(got, ref, T):
    """max |got - ref| / T over the elements with T > 0, and whether every element with T == 0 is exactly zero in ``got``."""
    got, ref, T = got.double(), ref.double(), T.double()
    pos = T > 0
    ratio = float(((got - ref).abs()[pos] / T[pos]).max()) if bool(pos.any()) else 0.0
    return ratio, bool((got[~pos] == 0).all())
