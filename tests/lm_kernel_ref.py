"""fp64-capable reference of ONE step of the satellite->ground LM pose loop with free geometry, and the seeded inputs of
``tests/test_lm_kernel_ref_cpu.py`` / ``tests/test_lm_kernels_vs_fp64.py``.

``oracle.ref_cpu`` derives the satellite map's metres-per-pixel and centre from its side A and takes the ground points from the
camera model; the C ABI (``hla_s2g_lm_solve`` / ``hla_s2g_lm_solve_bwd``) takes any ``h, w, row0, grd_row_skip, A, C,
meter_per_pixel, centre`` and any ``xyz`` table.  The projections here are the oracle's formulas with ``mpp`` and ``centre`` as
arguments, so that a test can put a ground pixel exactly where it wants it on the satellite map: on a border, one ulp-ish step to
either side of it, on a texel, in a clamped far-corner cell.  Sampling (``O.grid_sample``) and the update (``O.lm_update``) are the
oracle's own, unchanged.  Everything runs in the dtype of its inputs (the fp32 table is upcast, as in the kernels): the same code
on ``torch.float32`` inputs is the "ref32" that sizes the gates.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ref_cpu as O

RANGES = (6.0, 6.0, 10.0)            # shift_range_lat, shift_range_lon (m), rotation_range (deg) of every case
FORD_R = [[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]      # the usual camera -> body axis permutation
FORD_T = [-2.0, 0.5, 0.25]           # dyadic: X + T is exact
EPS = 2.0 ** -12                     # border offsets: (A - 1 +- EPS - centre) * mpp is exact in fp32 for A <= 16


# ----------------------------------------------------------------------------------------------------------------------
# projections: oracle.ref_cpu.kitti_pose_to_uv / ford_pose_to_uv with mpp and centre as arguments
# ----------------------------------------------------------------------------------------------------------------------
def _table4(table):
    return table if table.dim() == 4 else table[None]


def pose_to_uv_kitti(table, su, sv, th, A, mpp, centre, ranges):
    """table [h,w,3] fp32; pose tensors [B,1]; ranges = (lat, lon, rot).  -> uv [B,h,w,2], (jac_u, jac_v, jac_theta), mask [1,h,w]."""
    lat, lon, rot = ranges
    dt = su.dtype
    B = th.shape[0]
    xyz_grd = _table4(table)
    k = rot / 180 * np.pi
    ang = th * k
    u_m, v_m = su * lon, sv * lat
    c, s = torch.cos(ang), torch.sin(ang)
    z, o = torch.zeros_like(c), torch.ones_like(c)
    R = torch.cat([c, z, -s, z, o, z, s, z, c], -1).view(B, 3, 3)
    T0 = torch.cat([v_m, O.CAMERA_HEIGHT * o, -u_m], -1)
    T = -(R * T0[:, None, :]).sum(-1)
    X = xyz_grd.to(dt).expand(B, -1, -1, -1)
    xyz = (R[:, None, None] * X[:, :, :, None, :]).sum(-1) + T[:, None, None, :]
    uv = torch.stack([xyz[..., 2], xyz[..., 0]], -1) / mpp + centre
    dR = k * torch.cat([-s, z, -c, z, z, z, c, z, -s], -1).view(B, 3, 3)
    h, w = X.shape[1:3]
    e_u = torch.tensor([0.0, 0.0, -1.0], dtype=dt) * lon
    e_v = torch.tensor([1.0, 0.0, 0.0], dtype=dt) * lat
    d_u = -(R * e_u.view(1, 1, 3)).sum(-1)[:, None, None, :].expand(B, h, w, 3)
    d_v = -(R * e_v.view(1, 1, 3)).sum(-1)[:, None, None, :].expand(B, h, w, 3)
    d_t = (dR[:, None, None] * X[:, :, :, None, :]).sum(-1) - (dR * T0[:, None, :]).sum(-1)[:, None, None, :]
    pick = lambda d: torch.stack([d[..., 2], d[..., 0]], -1) / mpp
    return uv, (pick(d_u), pick(d_v), pick(d_t)), (xyz_grd[..., 2] > 0).to(dt)


def pose_to_uv_ford(table, R_FL, T_FL, su, sv, th, A, mpp, centre, ranges):
    """R_FL [B,3,3], T_FL [B,3]; otherwise as ``pose_to_uv_kitti``."""
    lat, lon, rot = ranges
    dt = su.dtype
    B = su.shape[0]
    xyz_grd = _table4(table)
    Xc = xyz_grd.to(dt).expand(B, -1, -1, -1)
    Xb = (R_FL.to(dt)[:, None, None] * Xc[:, :, :, None, :]).sum(-1) + T_FL.to(dt)[:, None, None, :]
    su_m, sv_m = lat * su, lon * sv
    Tw = torch.cat([sv_m, -su_m, torch.zeros_like(sv_m)], -1)
    k = rot / 180 * np.pi
    yaw = th * k
    c, s = torch.cos(yaw), torch.sin(yaw)
    z, o = torch.zeros_like(c), torch.ones_like(c)
    Rw = torch.cat([c, s, z, -s, c, z, z, z, o], -1).view(B, 3, 3)
    P = Xb + Tw[:, None, None, :]
    Xw = (Rw[:, None, None] * P[:, :, :, None, :]).sum(-1)
    Rs = torch.tensor([0, 1, 0, -1, 0, 0, 0, 0, 1], dtype=dt).view(1, 3, 3).expand(B, 3, 3)
    Xs = (Rs[:, None, None] * Xw[:, :, :, None, :]).sum(-1)
    uv = Xs[..., :2] / mpp + centre
    h, w = Xc.shape[1:3]
    dRw = k * torch.cat([-s, c, z, -c, -s, z, z, z, z], -1).view(B, 3, 3)
    e_u = lat * torch.tensor([0.0, -1.0, 0.0], dtype=dt)
    e_v = lon * torch.tensor([1.0, 0.0, 0.0], dtype=dt)
    dXw_t = (dRw[:, None, None] * P[:, :, :, None, :]).sum(-1)
    dXw_u = (Rw * e_u.view(1, 1, 3)).sum(-1)
    dXw_v = (Rw * e_v.view(1, 1, 3)).sum(-1)
    dXs_t = (Rs[:, None, None] * dXw_t[:, :, :, None, :]).sum(-1)
    dXs_u = (Rs * dXw_u[:, None, :]).sum(-1)[:, None, None, :].expand(B, h, w, 3)
    dXs_v = (Rs * dXw_v[:, None, :]).sum(-1)[:, None, None, :].expand(B, h, w, 3)
    return uv, (dXs_u[..., :2] / mpp, dXs_v[..., :2] / mpp, dXs_t[..., :2] / mpp), (xyz_grd[..., 2] > 0).to(dt)


def level_uv(geom, lv, pose):
    """uv, jac, mask of level ``lv`` (fields table, A, mpp, centre) under ``geom`` (fields ford, ranges, R_FL, T_FL)."""
    su, sv, th = pose
    if geom.ford:
        return pose_to_uv_ford(lv.table, geom.R_FL, geom.T_FL, su, sv, th, lv.A, lv.mpp, lv.centre, geom.ranges)
    return pose_to_uv_kitti(lv.table, su, sv, th, lv.A, lv.mpp, lv.centre, geom.ranges)


# ----------------------------------------------------------------------------------------------------------------------
# one step
# ----------------------------------------------------------------------------------------------------------------------
def _operands(sat, grd, conf, uv, jac, mask, row0, keep):
    """Sampled features f, ground features g, weight map gc (all masked, rows row0.., dropped pixels zeroed) and J [3,B,C,h',w]."""
    B = sat.shape[0]
    m = mask.expand(B, -1, -1)
    f, J = O.grid_sample(sat, uv, torch.stack(jac, 0))
    f, J = f * m[:, None], J * m[None, :, None]
    g = grd * m[:, None]
    gc = (conf if conf is not None else torch.ones_like(grd[:, :1])) * m[:, None]
    f, g, gc, J = f[:, :, row0:], g[:, :, row0:], gc[:, :, row0:], J[:, :, :, row0:]
    if keep is not None:
        k = keep.reshape(1, 1, *f.shape[-2:]).to(f.dtype)
        f, g, J = f * k, g * k, J * k[None]
    return f, g, gc, J


def step_sums(sat, grd, conf, uv, jac, mask, A, row0, using_weight, keep=None):
    """The 14 sums of ``normal_eq`` -- ||s||^2, ||g||^2, H(6), J^T W s (3), J^T W g (3) -- [B,14], the sums of the absolute values
    of their terms [B,14], and the number of pixels of the WHOLE map (every row, whatever its mask) inside the satellite map [B].
    sat [B,C,A,A], grd [B,C,h,w], conf [B,1,h,w] or None, keep [(h - row0) * w] bool or None."""
    f, g, gc, J = _operands(sat, grd, conf, uv, jac, mask, row0, keep)
    B = f.shape[0]
    s_, g_, J = f.reshape(B, -1), g.reshape(B, -1), J.reshape(3, B, -1)
    W = (gc if using_weight else torch.ones_like(gc)).expand(-1, f.shape[1], -1, -1).reshape(B, -1)
    terms = [s_ * s_, g_ * g_]
    terms += [W * J[p] * J[q] for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    terms += [W * J[p] * s_ for p in range(3)] + [W * J[p] * g_ for p in range(3)]
    sums = torch.stack([t.sum(1) for t in terms], 1)
    mags = torch.stack([t.abs().double().sum(1) for t in terms], 1)
    u, v = uv[..., 0].reshape(B, -1), uv[..., 1].reshape(B, -1)
    count = ((u >= 0) & (u <= A - 1) & (v >= 0) & (v <= A - 1)).sum(1)
    return sums, mags, count


def update_args(ranges=RANGES, damping=1.0, use_hessian=0, train_damping=0):
    lat, lon, rot = ranges
    return O.default_args(shift_range_lat=lat, shift_range_lon=lon, rotation_range=rot, damping=damping, use_hessian=use_hessian,
                          train_damping=train_damping, dropout=0)


def step(args, ford, sat, grd, conf, uv, jac, mask, row0, pose, using_weight, rand_uv, damping_param=None, keep=None):
    """``O.lm_update`` on this level's operands: pose (su, sv, th) -> the pose after the step.  rand_uv = (ru, rv), each [B,1]."""
    f, g, gc, J = _operands(sat, grd, conf, uv, jac, mask, row0, keep)
    su, sv, th = pose
    return O.lm_update(args, damping_param, su, sv, th, f, g, gc, J, using_weight, ford=ford, rand_uv=rand_uv)


# ----------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = {                     # h, w, row0, grd_row_skip
    'sub_tile': (7, 37, 5, 0),       # 74 px: less than one tile, ragged in every pixels-per-wave count
    'ragged': (7, 37, 0, 0),         # 259 px: 3 forward / backward tiles, the last one 3 px
    'skip': (9, 20, 4, 3),           # stored rows offset by grd_row_skip
    'mid': (33, 131, 1, 0),          # 4192 px: 256-px tiles, the last one 96 px
    'many': (129, 257, 0, 0),        # 33153 px: forward 65 tiles (the last one 385 px), backward 130
    'octet': (7, 37, 0, 0),          # run with B = 8 and 9: the XCD-affine block map, B = 9 with seven idle blocks per tile
}
# (ford, shape, C, A, B) of every pose-0 case tests/test_lm_kernels_vs_fp64.py runs, forward or backward
BORDER_CASES = [(0, 'ragged', C, 16, 3) for C in (16, 64, 128, 256)] + [
    (1, 'ragged', 64, 16, 3), (0, 'ragged', 64, 13, 3), (1, 'ragged', 64, 13, 3), (0, 'sub_tile', 256, 16, 1), (0, 'skip', 128, 16, 2),
    (0, 'mid', 64, 16, 2), (0, 'many', 16, 16, 2), (0, 'octet', 64, 16, 8), (0, 'octet', 64, 16, 9)]
# (ford, level_first, dropout keep masks, using_weight) of the two-level random-pose cases
RANDOM_CASES = [(0, 0, 0, 1), (0, 1, 1, 0), (1, 0, 0, 0), (1, 1, 0, 1)]


def case_seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode()) % 100000
BORDER_CLASSES = ('on0', 'below0', 'above0', 'onlim', 'abovelim', 'belowlim', 'texel', 'half', 'farcell', 'mid')


def border_values(A):
    """The ten values of one coordinate, in the order of BORDER_CLASSES."""
    i = A // 2 + 1
    return [0.0, -EPS, EPS, A - 1.0, A - 1 + EPS, A - 1 - EPS, float(i), i + 0.5, A - 2 + 0.75, A / 2]


def centre_of(ford, A):
    return float(A // 2) if ford else A / 2.0


def table_from_targets(ford, tu, tv, mpp, centre):
    """The fp32 table entries that put a pixel on (tu, tv) at pose 0 (fp64 arithmetic, then rounded to fp32)."""
    if ford:       # u = (X + T1) / mpp + c,  v = -(Z + T0) / mpp + c
        X, Z = (tu - centre) * mpp - FORD_T[1], -(tv - centre) * mpp - FORD_T[0]
    else:          # u = Z / mpp + c,  v = X / mpp + c
        X, Z = (tv - centre) * mpp, (tu - centre) * mpp
    return np.stack([X, np.full_like(X, O.CAMERA_HEIGHT), Z], -1).astype(np.float32)


def targets_from_table(ford, table, mpp, centre):
    """Pose-0 satellite coordinates of a table, in fp64 from its fp32 entries, by the plain formulas."""
    t = np.asarray(table, np.float64)
    if ford:
        return (t[..., 0] + FORD_T[1]) / mpp + centre, -(t[..., 2] + FORD_T[0]) / mpp + centre
    return t[..., 2] / mpp + centre, t[..., 0] / mpp + centre


def border_table(ford, A, h, w, row0, seed, mpp=0.5):
    """-> (table [h,w,3] fp32, target u [h,w], target v [h,w], class index u / v [h,w], -1 for the random fill).
    The 100 pairs of ``border_values`` first -- those with z > 0 before the masked ones --, then random targets in [-2, A + 1]
    on a 2^-10 grid (exact in fp32 too); the list starts at the first pixel the loop reads, (row0, 0), and wraps."""
    centre = centre_of(ford, A)
    vals = np.array(border_values(A))
    cu, cv = [a.reshape(-1) for a in np.meshgrid(np.arange(10), np.arange(10), indexing='ij')]
    n = h * w
    rs = np.random.RandomState(seed)
    fill = np.round(rs.uniform(-2.0, A + 1.0, size=(2, n - 100)) * 1024) / 1024
    tu = np.concatenate([vals[cu], fill[0]])
    tv = np.concatenate([vals[cv], fill[1]])
    ku, kv = np.concatenate([cu, -np.ones(n - 100, int)]), np.concatenate([cv, -np.ones(n - 100, int)])
    z = table_from_targets(ford, tu[:100], tv[:100], mpp, centre)[:, 2]
    order = np.concatenate([np.argsort(~(z > 0), kind='stable'), np.arange(100, n)])
    pos = (row0 * w + np.arange(n)) % n
    out = [np.empty(n) for _ in range(2)] + [np.empty(n, int) for _ in range(2)]
    for dst, src in zip(out, (tu, tv, ku, kv)):
        dst[pos] = src[order]
    tu, tv, ku, kv = [a.reshape(h, w) for a in out]
    return torch.from_numpy(table_from_targets(ford, tu, tv, mpp, centre)), tu, tv, ku, kv


def make_level(ford, shape, C, A, B, seed, mpp=0.5, dtype=torch.float32):
    """One level of a case (``shape``: a name in SHAPES or (h, w, row0, skip)): border table + unit-norm-ish random maps.  ``dtype`` bf16 / fp16: the maps are rounded to it here (on
    the host) and the reference reads the rounded values."""
    h, w, row0, skip = SHAPES[shape] if isinstance(shape, str) else shape
    rs = np.random.RandomState(seed + 1000)
    table, tu, tv, ku, kv = border_table(ford, A, h, w, row0, seed, mpp)
    npix = (h - row0) * w
    sat = torch.from_numpy((rs.standard_normal((B, C, A, A)) / np.sqrt(C * A * A)).astype(np.float32)).to(dtype)
    grd = torch.from_numpy((rs.standard_normal((B, C, h, w)) / np.sqrt(C * npix)).astype(np.float32)).to(dtype)
    conf = torch.from_numpy(rs.uniform(0.27, 0.5, size=(B, 1, h, w)).astype(np.float32))
    grd[:, :, :skip] = 0      # rows the caller does not store
    conf[:, :, :skip] = 0
    return SimpleNamespace(shape=shape, h=h, w=w, row0=row0, skip=skip, C=C, A=A, mpp=mpp, centre=centre_of(ford, A), table=table,
                           sat=sat, grd=grd, conf=conf, dtype=dtype, tu=tu, tv=tv, ku=ku, kv=kv)


def make_geom(ford, B):
    g = SimpleNamespace(ford=ford, ranges=RANGES, R_FL=None, T_FL=None)
    if ford:
        g.R_FL = torch.tensor([FORD_R]).repeat(B, 1, 1)
        g.T_FL = torch.tensor([FORD_T]).repeat(B, 1)
    return g


def cast_level(lv, dt, requires_grad=False):
    """The level's maps in ``dt`` (fp64 / fp32), as fresh leaves when ``requires_grad``; table and geometry shared."""
    o = SimpleNamespace(**vars(lv))
    for k in ('sat', 'grd', 'conf'):
        setattr(o, k, getattr(lv, k).to(dt).clone().requires_grad_(requires_grad))
    return o


def cast_geom(g, dt):
    o = SimpleNamespace(**vars(g))
    if g.ford:
        o.R_FL, o.T_FL = g.R_FL.to(dt), g.T_FL.to(dt)
    return o


def pose_cols(p, dt):
    p = torch.as_tensor(p)
    return tuple(p[:, i:i + 1].to(dt) for i in range(3))


def level_sums(geom, lv, pose, using_weight, keep=None):
    uv, jac, mask = level_uv(geom, lv, pose)
    return step_sums(lv.sat, lv.grd, lv.conf if using_weight else None, uv, jac, mask, lv.A, lv.row0, using_weight, keep)


def level_step(args, geom, lv, pose, using_weight, rand_uv, damping_param=None, keep=None):
    uv, jac, mask = level_uv(geom, lv, pose)
    return step(args, geom.ford, lv.sat, lv.grd, lv.conf, uv, jac, mask, lv.row0, pose, using_weight, rand_uv, damping_param, keep)


def step_order(L, N, level_first):
    """(iteration, level) of every step in execution order."""
    return [(i, l) for l in range(L) for i in range(N)] if level_first else [(i, l) for i in range(N) for l in range(L)]


# the two-level cases: levels differ in C, shape, A and mpp (forward nt = 3 and 17: the coarser level leaves part_ld > nt)
TWO_LEVELS = (('ragged', 128, 16, 0.5), ('mid', 16, 13, 0.75))
OUT_OF_VIEW_POSE = (2.4, 0.125, -0.25)       # shift_u = 2.4 x 6 m = 19 px or more: every pixel leaves the map


def make_two_level_case(ford, seed, B=3, out_sample=1):
    """-> (geom, levels, pose0 [B,3] fp32, rand_uv [steps,2,B] fp32, keep [steps, max npix] uint8) for 2 levels x 2 iterations.
    Sample ``out_sample`` starts out of view (None: no such sample)."""
    levels = [make_level(ford, s, C, A, B, seed + 10 * l, mpp) for l, (s, C, A, mpp) in enumerate(TWO_LEVELS)]
    rs = np.random.RandomState(seed + 77)
    p0 = rs.uniform(-0.3, 0.3, size=(B, 3)).astype(np.float32)
    if out_sample is not None:
        p0[out_sample] = OUT_OF_VIEW_POSE
    rand_uv = rs.uniform(-1, 1, size=(4, 2, B)).astype(np.float32)
    npix = [(lv.h - lv.row0) * lv.w for lv in levels]
    keep = (rs.uniform(size=(4, max(npix))) < 0.5).astype(np.uint8)
    return make_geom(ford, B), levels, torch.from_numpy(p0), torch.from_numpy(rand_uv), torch.from_numpy(keep)


def drop_sample(geom, levels, p0, rand_uv, b):
    """The same case without sample b."""
    sel = [i for i in range(p0.shape[0]) if i != b]
    g = SimpleNamespace(**vars(geom))
    if geom.ford:
        g.R_FL, g.T_FL = geom.R_FL[sel], geom.T_FL[sel]
    lvs = []
    for lv in levels:
        o = SimpleNamespace(**vars(lv))
        o.sat, o.grd, o.conf = lv.sat[sel].contiguous(), lv.grd[sel].contiguous(), lv.conf[sel].contiguous()
        lvs.append(o)
    return g, lvs, p0[sel].contiguous(), rand_uv[:, :, sel].contiguous()
