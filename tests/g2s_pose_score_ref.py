"""fp64-capable reference of ``hla_g2s_pose_score`` (include/hla.h): LM_G2SP's matching term at K candidate poses per sample on
one level, for both projections.  Built from ``oracle.ref_cpu.g2s_pose_to_uv`` (through the case handling of tests/g2s_geo_ref.py)
or ``g2s_nn_ref.inplane_pose_to_uv`` and ``oracle.ref_cpu.grid_sample``; the in-view mask comes from the (u, v) themselves, not
from ``f != 0``.  Runs in the dtype of its inputs, so the same code on fp32 inputs is the "ref32" that shows the gate's headroom.

``O.grid_sample`` asserts when no pixel of its batch is in view (jacobian.py:172), so every hypothesis is evaluated in a batch that
also holds a 2 x 2 guard map sampled at its centre; the guard rows are dropped.

Also here: the hypothesis builders and the list of cases tests/test_g2s_pose_score_gpu.py runs; tests/test_g2s_pose_score_ref_cpu.py
asserts on the reference alone every property those cases exist for."""
from types import SimpleNamespace

import numpy as np
import torch

import g2s_geo_ref as R
import g2s_nn_ref as NN
from oracle import ref_cpu as O

F64, F32 = torch.float64, torch.float32
N_SLOTS = 8
K_CASE = 7                      # hypotheses per case; hypothesis 0 is the case's own starting pose
OUT_K = 3                       # the hypothesis with nothing in view
FAR_OUT = (50.0, 50.0, 0.0)     # 1000 m away: behind the camera (geo), 100 and more pixels off the map (in-plane)
NN_RANGES = (20.0, 20.0, 30.0)
# in-plane levels (A, C, (h, w)): C = 16 with 256-pixel tiles (324 pixels: a ragged last tile of 68), 64 (729 pixels: 12 tiles, the
# last of 25), 128 and 256 under and over one tile, ground maps larger and smaller than the satellite map
NN_LEVELS = {16: (18, 16, (18, 18)), 64: (27, 64, (25, 30)), 128: (9, 128, (11, 8)), 256: (6, 256, (5, 9))}


def uv_of(c, l, pose, dt):
    """(u, v) [B,A,A] of level ``l`` of case ``c`` at ``pose`` [B,3], in dtype dt."""
    A, _, (h, w) = c.levels[l]
    su, sv, th = R.cols(pose, dt)
    if c.proj == 'nn':
        uv, _ = NN.inplane_pose_to_uv(R.make_args(c.ranges), A, su, sv, th)
    else:
        uv, _, _ = O.g2s_pose_to_uv(R.make_args(c.ranges), A, su, sv, th, c.K, h, w, *c.ori_hw, require_jac=False)
    return uv


def in_view(uv, hw):
    h, w = hw
    u, v = uv[..., 0], uv[..., 1]
    return (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)


def min_dist(uv, hw):
    """How far the closest pixel of each sample is from changing its cell or its in-view decision -- ``pixel_classes.min_dist`` of
    tests/g2s_geo_ref.py for any projection: in view the distance of u and v to the nearest texel line (u == 0 or v == 0 exactly is
    not counted), out of view the largest border violation.  uv [B,A,A,2] -> [B]."""
    h, w = hw
    B = uv.shape[0]
    u, v = uv[..., 0].reshape(B, -1).double(), uv[..., 1].reshape(B, -1).double()
    inb = in_view(uv, hw).reshape(B, -1)
    inf = torch.full_like(u, float('inf'))
    du = torch.where(u == 0, inf, (u - torch.round(u)).abs())
    dv = torch.where(v == 0, inf, (v - torch.round(v)).abs())
    viol = torch.stack([-u, u - (w - 1), -v, v - (h - 1)], 0).max(0)[0]
    return torch.where(inb, torch.minimum(du, dv), viol).min(1)[0]


def _guarded_sample(img, uv):
    """O.grid_sample(img, uv)[0] for a batch that may have nothing in view: a constant extra sample is sampled at (0.5, 0.5)."""
    B, Cn, h, w = img.shape
    guard_img = torch.zeros(1, Cn, h, w, dtype=img.dtype)
    guard_uv = torch.full((1,) + tuple(uv.shape[1:]), 0.5, dtype=uv.dtype)
    return O.grid_sample(torch.cat([img, guard_img]), torch.cat([uv, guard_uv]))[0][:B]


def cost_from_sums(sums):
    """The kernel's closing formula on [..., 8] sums, in their dtype; +inf where nothing is in view."""
    nf = torch.clamp(torch.sqrt(sums[..., 0]), min=1e-6)
    ns = torch.clamp(torch.sqrt(sums[..., 1]), min=1e-6)
    c = sums[..., 3] / (nf * nf) + sums[..., 4] / (ns * ns) - 2 * sums[..., 5] / (nf * ns)
    return torch.where(sums[..., 6] == 0, torch.full_like(c, float('inf')), c)


def score(c, l, poses, using_weight, dt=F64, maps=None):
    """Level ``l`` of case ``c`` at ``poses`` [B,K,3], everything in dtype ``dt`` (maps = (sat, grd, conf) NCHW lists in dt, by
    default ``g2s_geo_ref.cast(c, dt)``: with deferred norms the raw maps x inv).
    -> sums [B,K,8] dt, mags [B,K,8] fp64 (sums of the absolute values of the terms), counts [B,K] int64, cost [B,K] dt by the
    kernel's formula, direct [B,K] dt = sum w (f/nf - s/ns)^2 over the pixels in view (+inf with none)."""
    sat, grd, conf = maps if maps is not None else R.cast(c, dt)
    sat, grd, conf = sat[l], grd[l], conf[l]
    B, Kh = poses.shape[:2]
    hw = c.levels[l][2]
    out = [[] for _ in range(4)]
    for k in range(Kh):
        uv = uv_of(c, l, poses[:, k], dt)
        m = in_view(uv, hw)                                           # [B,A,A]
        f = _guarded_sample(grd, uv)                                  # zero out of view
        w = _guarded_sample(conf, uv) if using_weight else torch.ones(B, 1, *m.shape[1:], dtype=dt)
        md = m[:, None].to(dt)
        s_in = sat * md
        terms = [f * f, s_in * s_in, f * s_in, w * f * f, w * s_in * s_in, w * f * s_in]
        flat = [t.reshape(B, -1) for t in terms]
        cnt = m.reshape(B, -1).sum(1)
        s_all = (sat * sat).reshape(B, -1)
        sums = torch.stack([t.sum(1) for t in flat] + [cnt.to(dt), s_all.sum(1)], 1)
        out[0].append(sums)
        out[1].append(torch.stack([t.abs().double().sum(1) for t in flat] + [cnt.double(), s_all.abs().double().sum(1)], 1))
        out[2].append(cnt)
        nf = torch.clamp(torch.sqrt(sums[:, 0]), min=1e-6).view(B, 1, 1, 1)
        ns = torch.clamp(torch.sqrt(sums[:, 1]), min=1e-6).view(B, 1, 1, 1)
        direct = (w * md * (f / nf - sat / ns) ** 2).reshape(B, -1).sum(1)
        out[3].append(torch.where(cnt == 0, torch.full_like(direct, float('inf')), direct))
    sums, mags, counts, direct = [torch.stack(o, 1) for o in out]
    return sums, mags, counts, cost_from_sums(sums), direct


# ----------------------------------------------------------------------------------------------------------------------
# cases: those of tests/g2s_geo_ref.py, and in-plane ones made with its builders
# ----------------------------------------------------------------------------------------------------------------------
_CASES = {}


def nn_case(Cn, B):
    rs = np.random.RandomState(R._seed('gps nn', Cn, B))
    c = R._case(f'nn C{Cn} B{B}', [NN_LEVELS[Cn]], B, torch.zeros(B, 3, 3), 1, R._rand_pose(rs, B, 0.6), ranges=NN_RANGES)
    return c


def get(name, *a):
    """A case of g2s_geo_ref (proj 'geo') or ``nn_case`` (name 'nn'), made once, with ``proj`` set."""
    key = (name,) + a
    if key not in _CASES:
        c = nn_case(*a) if name == 'nn' else R.get(name, *a)
        c = SimpleNamespace(**vars(c))
        c.proj = 'nn' if name == 'nn' else 'geo'
        _CASES[key] = c
    return _CASES[key]


def far_out_rows(c):
    """The samples FAR_OUT puts out of view: all but the 'behind' case's special one."""
    return [b for b in range(c.B) if b != getattr(c, 'behind', None)]


def fp32_headroom(c, l, poses, using_weight):
    """max over samples, hypotheses and slots of |ref32 - ref64| / T_k: what the reference's own fp32 run uses of a gate."""
    s64, mags, _, _, _ = score(c, l, poses, using_weight, F64)
    s32 = score(c, l, poses, using_weight, F32)[0].double()
    return float(((s32 - s64).abs() / torch.where(mags > 0, mags, torch.ones_like(mags))).max())


_HYP = {}


def hypotheses(c, l, Kh=K_CASE, out_k=OUT_K, lim=0.3, tag=''):
    """[B,Kh,3] fp32, made once: hypothesis 0 is the case's starting pose (what its intrinsics were made for), hypothesis
    ``out_k`` FAR_OUT, the others random in [-lim, lim].  A drawn pose is a condition on the INPUTS, decided on the reference
    alone: it is redrawn until every sample keeps 64 GUARD from every texel line and border (fp32 and fp64 agree on every cell and
    every in-view decision) and the reference's fp32 run of it uses at most half of the sum gate 2e-6 T_k -- a satellite pixel just
    in front of the camera has z near 0 and a (u, v) that fp32 cannot hold to the fraction of a texel the gate assumes."""
    key = (c.name, l, Kh, out_k, lim, tag)
    if key in _HYP:
        return _HYP[key]
    rs = np.random.RandomState(R._seed('gps hyp', c.name, l, Kh, tag))
    hw = c.levels[l][2]
    P = torch.zeros(c.B, Kh, 3)
    P[:, 0] = R.start_pose(c)
    for k in range(1, Kh):
        if k == out_k:
            P[:, k] = torch.tensor(FAR_OUT)
            continue
        for _ in range(50):
            p = torch.from_numpy(rs.uniform(-lim, lim, size=(c.B, 3)).astype(np.float32))
            if float(min_dist(uv_of(c, l, p, F64), hw).min()) > 64 * R.GUARD and \
                    all(fp32_headroom(c, l, p[:, None], w) <= 1e-6 for w in ((0, 1) if c.proj == 'geo' else (0,))):
                break
        else:
            raise AssertionError(f'no well-conditioned hypothesis for {c.name} level {l}')
        P[:, k] = p
    _HYP[key] = P
    return P


# (case key, level) of the sums-against-fp64 runs; every one with and without weights where the projection has weights
GEO_RUNS = [(('shape', 7, 256), 0), (('shape', 7, 128), 0), (('shape', 7, 64), 0), (('border',), 0), (('behind',), 0), (('out',), 0),
            (('mid',), 0), (('mid',), 1), (('deferred',), 0), (('deferred',), 1), (('octet8',), 0), (('octet9',), 0), (('octet9',), 1)]
NN_RUNS = [(('nn', 16, 9), 0), (('nn', 64, 3), 0), (('nn', 128, 2), 0), (('nn', 256, 2), 0)]
RUNS = [(k, l, w) for k, l in GEO_RUNS for w in (0, 1)] + [(k, l, 0) for k, l in NN_RUNS]


def run_id(r):
    key, l, w = r
    return '-'.join(str(x) for x in key) + f'-L{l}-w{w}'


K70 = {'geo': (('octet9',), 0, 1), 'nn': (('nn', 64, 3), 0, 0)}       # (case key, level, using_weight) of the 70-hypothesis runs
K70_OUT = 40


def k70(proj):
    """-> (case, level, using_weight, poses [B,70,3]); hypothesis 40 is FAR_OUT."""
    key, l, w = K70[proj]
    c = get(*key)
    return c, l, w, hypotheses(c, l, Kh=70, out_k=K70_OUT, tag='k70')


# ----------------------------------------------------------------------------------------------------------------------
# the planted minimum
# ----------------------------------------------------------------------------------------------------------------------
PLANTED = {'geo': ('mid', 1), 'nn': ('nn', 64, 3)}            # (case key..., level for geo)
PLANTED_POSES = [(0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (-0.15, 0.25, 0.4), FAR_OUT, (0.0, -0.3, 0.0), (0.3, 0.3, -0.5), (-0.3, -0.3, 0.6)]
PLANTED_K = 2


def planted(proj):
    """-> (case, level, poses [B,7,3]): a copy of a case whose satellite map IS the ground map projected (fp64) at hypothesis 2
    where that projection is in view, and stays random elsewhere: hypothesis 2 scores 0 up to the rounding of the map to fp32."""
    if proj == 'nn':
        base, l = get(*PLANTED['nn']), 0
    else:
        base, l = get(PLANTED['geo'][0]), PLANTED['geo'][1]
    c = SimpleNamespace(**vars(base))
    c.name = base.name + ' planted'
    poses = torch.tensor(PLANTED_POSES, dtype=F32)[None].repeat(c.B, 1, 1)
    _, grd, _ = R.cast(base, F64)
    uv = uv_of(c, l, poses[:, PLANTED_K], F64)
    m = in_view(uv, c.levels[l][2])[:, None]
    f = _guarded_sample(grd[l], uv)
    c.sat = list(base.sat)
    c.sat[l] = torch.where(m, f, base.sat[l].double()).float().contiguous()
    return c, l, poses
