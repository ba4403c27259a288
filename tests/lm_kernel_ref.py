"""fp64-capable reference of ONE step of the satellite->ground LM pose loop with free geometry, and the seeded inputs of
``tests/test_lm_kernel_ref_cpu.py`` / ``tests/test_lm_kernels_vs_fp64.py``; at the end, the rule of the reach flag and the inputs of
``tests/test_lm_reach_ref_cpu.py`` / ``tests/test_lm_reach_vs_fp64.py``.

``oracle.ref_cpu`` derives the satellite map's metres-per-pixel and centre from its side A and takes the ground points from the
camera model; the C ABI (``hla_s2g_lm_solve`` / ``hla_s2g_lm_solve_bwd``) takes any ``h, w, row0, grd_row_skip, A, C,
meter_per_pixel, centre`` and any ``xyz`` table.  The projections here are the oracle's formulas with ``mpp`` and ``centre`` as
arguments, so that a test can put a ground pixel exactly where it wants it on the satellite map: on a border, one ulp-ish step to
either side of it, on a texel, in a clamped far-corner cell.  Sampling (``O.grid_sample``) and the update (``O.lm_update``) are the
oracle's own, unchanged.  Everything runs in the dtype of its inputs (the fp32 table is upcast, as in the kernels): the same code
on ``torch.float32`` inputs is the "ref32" that sizes the gates.

Two kinds of table: ``border_table`` (every border class, then random targets: next to every pixel in a texel cell of its own) and
``coherent_table`` (targets linear along each row: runs of pixels in one cell, which lm_bwd_accum and psb_accum merge in registers
before their atomics), with ``run_stats``, the CPU mirror of that merge, for ``tests/test_cell_runs_cpu.py`` /
``tests/test_cell_runs_vs_fp64.py``.
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
# How the two backward kernels that merge texel-cell runs deal a level's pixels to their lane groups (``run_stats`` mirrors it; the
# kernels' own statements are lm_pick_tile_bwd in csrc/lm_backward.hip and psb_tile / PSB_NPL in csrc/pose_score.hip).  A block
# has 4 waves, a pixel takes C / 4 lanes, so a block has 4 * (256 / C) lane groups; each walks RUN consecutive pixels of the tile.
def lm_bwd_tile(npix):
    return 256 if npix >= 4096 else 128         # lm_pick_tile_bwd


PSB_RUN = 8                                      # PSB_NPL


def lane_groups(C):
    return 4 * (256 // C)


def psb_tile(C):
    return lane_groups(C) * PSB_RUN              # psb_tile


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


# ----------------------------------------------------------------------------------------------------------------------
# coherent tables: neighbouring ground pixels fall into the same texel cell, as at real geometry (the border table's random fill
# gives every pixel a cell of its own, so the backward kernels' merge of a cell run in registers is next to never taken there)
# ----------------------------------------------------------------------------------------------------------------------
# Step of the swept coordinate per pixel, by row: the cycle 1/16, 3/32, 1/8, 3/16, 5/16, 1/2, 1, 0 in an order that brings both
# extremes (one pixel per cell, a whole row in one cell) into the first seven rows, the height of the smallest shapes.
COHERENT_STEPS = (1 / 16, 3 / 32, 1 / 8, 0.0, 5 / 16, 1.0, 1 / 2, 3 / 16)
COHERENT_DRIFT = 1 / 64                # of the other coordinate, per pixel
HOLE_PERIOD = 12                       # one pixel in twelve of every row is a hole
OUTSIDE = 3.0                          # no target lies further than this from the map: OUT_OF_VIEW_POSE clears these tables too


def coherent_table(ford, A, h, w, row0, seed, mpp=0.5):
    """-> the tuple of ``border_table`` (class indices all -1).  Pose-0 targets vary linearly along every row, on the 2^-10 grid.
    Row k counted from row0 (wrapping): k even sweeps v, k odd sweeps u, by COHERENT_STEPS[j % 8] per pixel (j = k, less one after
    the copied row) while the other coordinate drifts by 1/64 per pixel.
      k = 0   u == A - 1 exactly, v sweeping: a run in a clamped cell with dxo == 0
      k = 1   v == A - 1 exactly, u sweeping: dyo == 0 (Ford: z <= 0 on that line at these constants, the row is masked)
      k = 3   row 2 again, moved by 1/32 in both coordinates: two rows that share their cells
      step 0  a whole row in as few cells as the drift allows (one cell for w <= 48)
    The other rows start and run as drawn from ``seed``: inside the visible part of the map (KITTI: u > centre, Ford: v < centre
    + 4), entering it from outside the map, or leaving it; a row that has left stays OUTSIDE px from the border.
    Holes: column c of row k with (c + 5 k) % 12 == 7 is moved out of the map (by OUTSIDE) or, every second one, onto a masked
    target inside the map (z <= 0)."""
    centre = centre_of(ford, A)
    lim = A - 1.0
    q = lambda x: np.round(np.asarray(x, np.float64) * 1024) / 1024
    zero_v = centre - FORD_T[0] / mpp      # Ford: z > 0 is v < zero_v (centre + 4 at mpp = 0.5)
    vis = {'u': (0.0, lim) if ford else (centre + 0.25, lim), 'v': (0.0, min(lim, zero_v - 0.25)) if ford else (0.0, lim)}
    # the map border a row can enter or leave through with z > 0 on both sides of it
    open_side = {'u': (-1, +1) if ford else (+1,), 'v': (-1,) if ford else (-1, +1)}
    rs = np.random.RandomState(seed)
    cols = np.arange(w)
    tu, tv = np.empty((h, w)), np.empty((h, w))
    for k in range(h):
        r = (row0 + k) % h
        j = k if k < 3 else k - 1
        step = COHERENT_STEPS[j % 8]
        sw, ot = ('v', 'u') if k % 2 == 0 else ('u', 'v')
        span, dspan = step * (w - 1), COHERENT_DRIFT * (w - 1)
        (lo, hi), (olo, ohi) = vis[sw], vis[ot]
        mode, sign, side, f0, f1 = rs.randint(3), rs.choice((-1, 1)), rs.randint(2), rs.uniform(), rs.uniform()   # (drawn for every row)
        if k == 3:
            tu[r], tv[r] = tu[(row0 + 2) % h] + 1 / 32, tv[(row0 + 2) % h] + 1 / 32
            continue
        side = open_side[sw][side % len(open_side[sw])]
        n_out = min(5, w // 4) + 0.5
        if step == 0 or (k < 3 and span <= hi - lo) or (mode == 0 and span <= hi - lo):      # inside
            s0 = lo + f0 * (hi - lo - span)
            s0, d = (s0, step) if sign > 0 else (s0 + span, -step)
        elif mode == 1 or k < 3:                                                           # enters through `side`
            s0 = (lim + n_out * step) if side > 0 else -n_out * step
            d = -side * step
        else:                                                                              # leaves through `side`
            s0 = ((lim + n_out * step) if side > 0 else -n_out * step) - side * span
            d = side * step
        if step == 0 and dspan < 0.75:          # the drift stays inside one cell
            o0 = np.ceil(olo) + np.floor(f1 * (np.floor(ohi) - np.ceil(olo))) + 0.125
        else:
            o0 = olo + f1 * max(ohi - olo - dspan, 0.0)
        s, o = q(s0) + d * cols, q(o0) + COHERENT_DRIFT * cols
        if k == 0:
            o = np.full(w, lim)                 # sw = 'v': u == A - 1
        if k == 1:
            o = np.full(w, lim)                 # sw = 'u': v == A - 1
        tu[r], tv[r] = (o, s) if sw == 'v' else (s, o)
    tu, tv = np.clip(tu, -OUTSIDE, lim + OUTSIDE), np.clip(tv, -OUTSIDE, lim + OUTSIDE)
    for k in range(h):
        r = (row0 + k) % h
        for n, c in enumerate(cols[(cols + 5 * k) % HOLE_PERIOD == 7]):
            if (n + k) % 2 == 0:                # out of the map, z > 0
                if ford:
                    tv[r, c] = -OUTSIDE
                else:
                    tu[r, c] = lim + OUTSIDE
            elif ford:                          # inside the map, z <= 0
                tv[r, c] = zero_v + 0.5
            else:
                tu[r, c] = centre - 1.5
    tu, tv = q(tu), q(tv)
    none = -np.ones((h, w), int)
    return torch.from_numpy(table_from_targets(ford, tu, tv, mpp, centre)), tu, tv, none, none.copy()


def pixel_cells(lv, pose, keep=None):
    """What lm_pixel (csrc/lm_common.h) makes of the pixels the loop reads, for ONE sample at ``pose`` = (su, sv, th) floats, in
    fp64: live [npix] bool (ground mask, in view, kept) and cell [npix,4] int = (x0, y0, dx, dy), dx / dy = 0 in a clamped cell."""
    one = lambda x: torch.tensor([[float(x)]], dtype=torch.float64)
    uv, _, mask = level_uv(cast_geom(make_geom(lv.ford, 1), torch.float64), lv, tuple(one(x) for x in pose))
    u, v = [uv[0, lv.row0:, :, i].reshape(-1).numpy() for i in range(2)]
    lim = lv.A - 1
    live = (u >= 0) & (u <= lim) & (v >= 0) & (v <= lim) & (mask[0, lv.row0:].reshape(-1).numpy() > 0)
    if keep is not None:
        live &= np.asarray(keep).reshape(-1)[:len(live)].astype(bool)
    x0, y0 = np.floor(u), np.floor(v)
    cell = np.stack([x0, y0, np.minimum(x0 + 1, lim) - x0, np.minimum(y0 + 1, lim) - y0], 1).astype(int)
    return live, cell


def run_stats(lv, pose, C, kind, keep=None):
    """The CPU mirror of how ``kind`` = 'lm_bwd' (lm_bwd_accum) or 'psb' (psb_accum) merges texel-cell runs, for one sample at
    ``pose``: a lane group walks RUN consecutive pixels of its tile; a live pixel in another cell than the open one flushes it; a
    pixel that is not live (a hole) leaves it open.  -> dict:
      live         pixels that reach the satellite map          merged      those in runs of 2 or more
      longest      the longest run                               run         RUN of the (full) tile
      across_hole  runs that go on in the same cell after a hole             open_hole   holes met with a cell open
      clamped      runs of 2 or more in a cell with dxo == 0 or dyo == 0     tiles       tiles of the level
      multi_group / multi_tile   texels flushed to by at least 2 lane groups / by lane groups of at least 2 tiles
      merged_pixels              the indices (from row0 on) of the merged pixels"""
    live, cell = pixel_cells(lv, pose, keep)
    tp = lm_bwd_tile(len(live)) if kind == 'lm_bwd' else psb_tile(C)
    return group_stats(live, cell, lane_groups(C), tp, None if kind == 'lm_bwd' else PSB_RUN)


def group_stats(live, cell, groups, tp, fixed_run=None):
    """``run_stats`` on given pixels: live [npix] bool, cell [npix,4] int, ``groups`` lane groups per block, tiles of ``tp`` pixels,
    RUN = ``fixed_run`` or, if None, ceil(pixels of the tile / groups)."""
    npix = len(live)
    nt = (npix + tp - 1) // tp
    out = dict(live=int(live.sum()), merged=0, longest=0, across_hole=0, open_hole=0, clamped=0, tiles=nt,
               run=fixed_run or (min(tp, npix) + groups - 1) // groups, merged_pixels=[])
    writers = {}

    def flush(c, n, who, pix):
        if c is None:
            return
        out['merged'] += n if n >= 2 else 0
        out['merged_pixels'] += pix if n >= 2 else []
        out['longest'] = max(out['longest'], n)
        out['clamped'] += int(n >= 2 and (c[2] == 0 or c[3] == 0))
        for t in {(c[1], c[0]), (c[1], c[0] + c[2]), (c[1] + c[3], c[0]), (c[1] + c[3], c[0] + c[2])}:
            writers.setdefault(t, set()).add(who)

    for tile in range(nt):
        p0 = tile * tp
        n_p = min(tp, npix - p0)
        run = fixed_run or (n_p + groups - 1) // groups
        for g in range(groups):
            cur, n, hole, counted, pix = None, 0, False, False, []
            for i in range(g * run, min((g + 1) * run, n_p)):
                p = p0 + i
                if not live[p]:
                    out['open_hole'] += int(cur is not None)
                    hole = cur is not None
                    continue
                c = tuple(cell[p])
                if c != cur:
                    flush(cur, n, (tile, g), pix)
                    cur, n, counted, pix = c, 0, False, []
                elif hole and not counted:
                    out['across_hole'] += 1
                    counted = True
                n, hole = n + 1, False
                pix.append(p)
            flush(cur, n, (tile, g), pix)
    out['multi_group'] = sum(len(s) >= 2 for s in writers.values())
    out['multi_tile'] = sum(len({t for t, _ in s}) >= 2 for s in writers.values())
    return out


# (ford, shape, C, A, B) of the one-level coherent cases of tests/test_cell_runs_vs_fp64.py, each run at pose 0 and COHERENT_POSE
COHERENT_CASES = [(0, 'ragged', C, 16, 3) for C in (16, 64, 128, 256)] + [
    (1, 'ragged', 64, 16, 3), (0, 'ragged', 64, 13, 3), (1, 'ragged', 64, 13, 3), (0, 'mid', 64, 16, 2), (0, 'skip', 128, 16, 2),
    (0, 'octet', 64, 16, 9)]
COHERENT_POSE = (0.05, -0.03, 0.4)
# (ford, level_first, dropout keep masks, using_weight) of the two-level coherent cases
COHERENT_TWO_LEVEL_CASES = [(f, lf, kp, (f + lf + kp) % 2) for f in (0, 1) for lf in (0, 1) for kp in (0, 1)]
# Seeds.  tests/test_cell_runs_cpu.py states what a case's inputs must reach at every pose it is run at (a full lane group of 8
# live pixels in one cell, a run across a hole, ...) and holds the references' own fp32 runs inside the gates; on a level of seven
# rows of 37 pixels, two or three in a hundred (pose, condition) pairs miss by chance.  The salts are the FIRST ones, counted
# from 0, under which every condition of that file holds: found on the CPU, on the inputs and the references alone.
COHERENT_SALT = {}                     # (ford, shape, C, A, B) -> salt (0 where not listed: every table is its first one)
COHERENT_TWO_LEVEL_SALT = {(1, 0): 1}  # (ford, level_first) -> salt
_COHERENT = {}


def coherent_level(ford, shape, C, A, B, dtype=torch.float32):
    """(geom, level) of a coherent case, made once per process and never modified."""
    key = (ford, shape, C, A, B, dtype)
    if key not in _COHERENT:
        _COHERENT[key] = (make_geom(ford, B), make_level(ford, shape, C, A, B, case_seed('coherent', ford, shape, C, A, B,
                                                                                            COHERENT_SALT.get(key[:5], 0)),
                                                         dtype=dtype, table='coherent'))
    return _COHERENT[key]


def coherent_two_level_case(ford, level_first):
    """``make_two_level_case`` on coherent tables; the dropout masks drop one pixel in six (holes inside open cells)."""
    salt = COHERENT_TWO_LEVEL_SALT.get((ford, level_first), 0)
    return make_two_level_case(ford, case_seed('coherent2', ford, level_first, salt), table='coherent', keep_p=5 / 6)


def make_level(ford, shape, C, A, B, seed, mpp=0.5, dtype=torch.float32, table='border'):
    """One level of a case (``shape``: a name in SHAPES or (h, w, row0, skip)): border table + unit-norm-ish random maps.  ``dtype`` bf16 / fp16: the maps are rounded to it here (on
    the host) and the reference reads the rounded values.  table = 'coherent': ``coherent_table`` instead of ``border_table``
    (the maps are the same bytes either way)."""
    h, w, row0, skip = SHAPES[shape] if isinstance(shape, str) else shape
    rs = np.random.RandomState(seed + 1000)
    table, tu, tv, ku, kv = {'border': border_table, 'coherent': coherent_table}[table](ford, A, h, w, row0, seed, mpp)
    npix = (h - row0) * w
    sat = torch.from_numpy((rs.standard_normal((B, C, A, A)) / np.sqrt(C * A * A)).astype(np.float32)).to(dtype)
    grd = torch.from_numpy((rs.standard_normal((B, C, h, w)) / np.sqrt(C * npix)).astype(np.float32)).to(dtype)
    conf = torch.from_numpy(rs.uniform(0.27, 0.5, size=(B, 1, h, w)).astype(np.float32))
    grd[:, :, :skip] = 0      # rows the caller does not store
    conf[:, :, :skip] = 0
    return SimpleNamespace(shape=shape, h=h, w=w, row0=row0, skip=skip, C=C, A=A, mpp=mpp, centre=centre_of(ford, A), table=table,
                           sat=sat, grd=grd, conf=conf, dtype=dtype, tu=tu, tv=tv, ku=ku, kv=kv, ford=int(ford))


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


def make_two_level_case(ford, seed, B=3, out_sample=1, table='border', keep_p=0.5):
    """-> (geom, levels, pose0 [B,3] fp32, rand_uv [steps,2,B] fp32, keep [steps, max npix] uint8) for 2 levels x 2 iterations.
    Sample ``out_sample`` starts out of view (None: no such sample); keep_p: the share of pixels a dropout mask keeps."""
    levels = [make_level(ford, s, C, A, B, seed + 10 * l, mpp, table=table) for l, (s, C, A, mpp) in enumerate(TWO_LEVELS)]
    rs = np.random.RandomState(seed + 77)
    p0 = rs.uniform(-0.3, 0.3, size=(B, 3)).astype(np.float32)
    if out_sample is not None:
        p0[out_sample] = OUT_OF_VIEW_POSE
    rand_uv = rs.uniform(-1, 1, size=(4, 2, B)).astype(np.float32)
    npix = [(lv.h - lv.row0) * lv.w for lv in levels]
    keep = (rs.uniform(size=(4, max(npix))) < keep_p).astype(np.uint8)
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


# ----------------------------------------------------------------------------------------------------------------------
# the reach flag (hla_s2g_config.reach_mode = 1): the rule, and inputs with pixels exactly on the column border
# ----------------------------------------------------------------------------------------------------------------------
def reach_pixels(geom, lv, pose, keep=None):
    """The pixels of one step that can set the flag, and their u: rows >= row0, kept, table z > 0, inside the map.
    pose = (su, sv, th), each [B,1], in the precision to compute in; keep [(h - row0) * w] or None.  -> part, u: [B, (h - row0) * w]."""
    uv, _, mask = level_uv(cast_geom(geom, pose[0].dtype), lv, pose)
    u, v = uv[:, lv.row0:, :, 0], uv[:, lv.row0:, :, 1]
    lim = lv.A - 1
    part = (u >= 0) & (u <= lim) & (v >= 0) & (v <= lim) & (mask[:, lv.row0:] > 0)
    if keep is not None:
        part = part & torch.as_tensor(keep).bool().reshape(1, lv.h - lv.row0, lv.w)
    B = u.shape[0]
    return part.reshape(B, -1), u.reshape(B, -1)


def _step_keep(keep, k, lv):
    return None if keep is None else keep[k, :(lv.h - lv.row0) * lv.w]


def reach_flags(geom, levels, poses_per_step, col0, keep=None):
    """flag[b] = 1 iff in some step a pixel that is read (rows >= row0), kept by that step's dropout mask, has table z > 0 and lies
    inside the map has u < col0[level].  A pixel with zero confidence counts (its taps are read all the same).
    poses_per_step: [(level index, (su, sv, th))] in execution order, the pose every sample has when the step starts;
    keep [steps, max npix] or None.  -> int32 [B]."""
    flag = None
    for k, (l, pose) in enumerate(poses_per_step):
        part, u = reach_pixels(geom, levels[l], pose, _step_keep(keep, k, levels[l]))
        hit = (part & (u < col0[l])).any(1)
        flag = hit if flag is None else flag | hit
    return flag.to(torch.int32)


def reach_margin(geom, levels, poses_per_step, col0, keep=None):
    """min |u - col0[level]| over the steps and the pixels ``reach_flags`` looks at, per sample [B] (inf: no such pixel)."""
    best = None
    for k, (l, pose) in enumerate(poses_per_step):
        part, u = reach_pixels(geom, levels[l], pose, _step_keep(keep, k, levels[l]))
        d = torch.where(part, (u - col0[l]).abs().double(), torch.full_like(u, float('inf'), dtype=torch.float64)).min(1).values
        best = d if best is None else torch.minimum(best, d)
    return best


# KITTI chain, A = 16, mpp = 0.5: the ground mask z > 0 is u > A / 2 = 8 at theta = 0, so a pixel that takes part AND lies left of
# the first valid column needs that column right of the centre.
REACH_A, REACH_COL0 = 16, 10
REACH_LEFT = (-EPS, -1.0, -1.0 + EPS)          # offsets from col0 of the targets that must set the flag
# Samples differ by pose only.  At theta = 0 a dyadic shift_u = s moves every u by exactly 12 s px (lon = 6 m, mpp = 0.5) and
# leaves v alone; shift_v = 0.25 moves every v by exactly -3 px and leaves u alone (fp32 and fp64 alike).
REACH_SHIFT = 2.0 ** -14                       # 3 EPS in u
REACH_POSES = ((0.0, 0.0, 0.0), (-REACH_SHIFT, 0.0, 0.0), (REACH_SHIFT, 0.0, 0.0), (0.0, 0.25, 0.0))


def reach_table(h, w, row0, seed, col0=REACH_COL0, A=REACH_A, extra=(), mpp=0.5):
    """-> (table [h,w,3] fp32, target u [h,w], target v [h,w]) of a KITTI level whose smallest u among the pixels that take part at
    pose 0 is EXACTLY col0.  From the first pixel read, (row0, 0), on:
      {col0, col0 + EPS} x the ten border classes of v                                  (in view: on / just right of the column)
      {col0 - EPS, col0 - 1, col0 - 1 + EPS} x {-EPS, A - 1 + EPS} in v                 (left of it, but outside the map in v)
      {A / 2, A / 2 - 1.5, -EPS} x {A / 2, 1.25} in v                                   (left of it, but z <= 0; the last one u < 0 too)
    then random targets right of the column: u in [col0 + 2^-10, A + 1], v in [-2, A + 1], on a 2^-10 grid.
    extra: ((row, column), u, v) targets written over that list afterwards."""
    centre = centre_of(0, A)
    vals = border_values(A)
    tu = [col0 + d for d in (0.0, EPS) for _ in vals] + [col0 + d for d in REACH_LEFT for _ in range(2)] + \
         [x for x in (A / 2, A / 2 - 1.5, -EPS) for _ in range(2)]
    tv = vals * 2 + [-EPS, A - 1 + EPS] * 3 + [A / 2, 1.25] * 3
    n, m = h * w, len(tu)
    rs = np.random.RandomState(seed)
    fu = np.round(rs.uniform(col0 + 2.0 ** -10, A + 1.0, size=n - m) * 1024) / 1024
    fv = np.round(rs.uniform(-2.0, A + 1.0, size=n - m) * 1024) / 1024
    pos = (row0 * w + np.arange(n)) % n
    U, V = np.empty(n), np.empty(n)
    U[pos], V[pos] = np.concatenate([tu, fu]), np.concatenate([tv, fv])
    U, V = U.reshape(h, w), V.reshape(h, w)
    for (r, c), eu, ev in extra:
        U[r, c], V[r, c] = eu, ev
    return torch.from_numpy(table_from_targets(0, U, V, mpp, centre)), U, V


def make_reach_level(shape, C, B, seed, extra=(), dtype=torch.float32, col0=REACH_COL0, A=REACH_A, mpp=0.5):
    """``make_level``'s maps on a ``reach_table``."""
    lv = make_level(0, shape, C, A, B, seed, mpp, dtype)
    lv.table, lv.tu, lv.tv = reach_table(lv.h, lv.w, lv.row0, seed, col0, A, extra, mpp)
    lv.ku = lv.kv = None
    return lv


def nan_strip(lv, col0):
    """The level with the satellite map's columns left of col0 set to NaN: what a trimmed extractor leaves there at worst."""
    o = SimpleNamespace(**vars(lv))
    o.sat = lv.sat.clone()
    o.sat[..., :col0] = float('nan')
    return o


def reach_poses(idx):
    """pose0 [B,3] fp32 from indices into REACH_POSES."""
    return torch.tensor([REACH_POSES[i] for i in idx], dtype=torch.float32)


# The moving-pose cases: two levels that differ in C, shape, A, mpp AND first valid column, 2 iterations.  Per level six pixels sit
# REACH2_GAP px right of the column, in a band of v of their own, and every other pixel at least half a pixel further right: so
# whether a sample crosses at a level is decided by how far its shift_u travels (12 px / 8 px per unit at the two levels) and by
# whether its shift_v has moved that level's six out of the map (shift_v = -0.25: +3 px / +2 px in v).
#                 shape    C    A   mpp  col0  v band of the six
REACH2_LEVELS = (('ragged', 128, 16, 0.5, 10, (12.5, 14.5)), ('mid', 16, 13, 0.75, 8, (2.0, 6.0)))
REACH2_COL0 = tuple(v[4] for v in REACH2_LEVELS)
REACH2_GAP = 0.5


def reach2_table(h, w, row0, seed, col0, A, mpp, band):
    """Six pixels among the rows read AT u = col0 + REACH2_GAP, v spread over ``band``; random targets for the others: u in
    [col0 + REACH2_GAP + 0.5, A + 1], v in [-2, A + 1] (2^-10 grid), every eighth of them masked (u <= A / 2)."""
    n = h * w
    rs = np.random.RandomState(seed)
    U = np.round(rs.uniform(col0 + REACH2_GAP + 0.5, A + 1.0, size=n) * 1024) / 1024
    V = np.round(rs.uniform(-2.0, A + 1.0, size=n) * 1024) / 1024
    U[::8] = np.round(rs.uniform(-2.0, A / 2, size=len(U[::8])) * 1024) / 1024
    near = row0 * w + 5 + 29 * np.arange(6)
    U[near], V[near] = col0 + REACH2_GAP, np.linspace(band[0], band[1], 6)
    U, V = U.reshape(h, w), V.reshape(h, w)
    return torch.from_numpy(table_from_targets(0, U, V, mpp, centre_of(0, A))), U, V


def make_reach2_case(seed, p0):
    """-> (geom, levels, pose0 [B,3] fp32, rand_uv [4,2,B] fp32, keep [4, max npix] uint8) of the moving-pose cases (KITTI)."""
    p0 = torch.tensor(p0, dtype=torch.float32)
    B = p0.shape[0]
    levels = []
    for l, (s, C, A, mpp, col0, band) in enumerate(REACH2_LEVELS):
        lv = make_level(0, s, C, A, B, seed + 10 * l, mpp)
        lv.table, lv.tu, lv.tv = reach2_table(lv.h, lv.w, lv.row0, seed + 10 * l + 5, col0, A, mpp, band)
        lv.ku = lv.kv = None
        levels.append(lv)
    rs = np.random.RandomState(seed + 77)
    rand_uv = rs.uniform(-1, 1, size=(4, 2, B)).astype(np.float32)
    npix = [(lv.h - lv.row0) * lv.w for lv in levels]
    keep = (rs.uniform(size=(4, max(npix))) < 0.5).astype(np.uint8)
    return make_geom(0, B), levels, p0, torch.from_numpy(rand_uv), torch.from_numpy(keep)


def trajectory(geom, levels, p0, rand_uv, N, level_first, using_weight, keep, dt):
    """The reference's own trajectory in ``dt``: [(level, pose at the start of the step)], and the pose after the last step."""
    args = update_args()
    g, lvs = cast_geom(geom, dt), [cast_level(lv, dt) for lv in levels]
    pose = pose_cols(p0, dt)
    out = []
    for k, (i, l) in enumerate(step_order(len(levels), N, level_first)):
        out.append((l, pose))
        kp = _step_keep(keep, k, lvs[l])
        pose = level_step(args, g, lvs[l], pose, using_weight, tuple(rand_uv[k, j][:, None].to(dt) for j in range(2)),
                          keep=None if kp is None else kp.bool())
    return out, pose


# level_first -> (dropout keep masks, pose0).  Sample 0 never crosses (though at level 1 it reads left of col0[0] = 10 all the time);
# sample 1 crosses under col0[0] at level 0 and never under col0[1]; sample 2 (a whole map's width to the left) in every step;
# sample 3 -- shift_v = -0.25 has moved level 0's six pixels out of the map -- only at level 1 and only in iteration 2, when its
# shift_u has drifted past -REACH2_GAP / 8.  Found by sweeping shift_u over the fp64 reference's own trajectory for the largest
# distance from the column (tests/test_lm_reach_ref_cpu.py asserts the pattern and the margin).
REACH2_CASES = {
    0: (0, [[0.05, 0.01, -0.02], [-0.046, 0.0, 0.0], [-1.0, 0.0, 0.0], [-481 / 8192, -0.25, 0.0]]),
    1: (1, [[0.05, 0.01, -0.02], [-0.0435, 0.0, 0.0], [-1.0, 0.0, 0.0], [-371 / 8192, -0.25, 0.0]]),
}
REACH2_STEP_FLAGS = {      # [sample][step in execution order], level_first 0: levels 0 1 0 1, level_first 1: levels 0 0 1 1
    0: [[0, 0, 0, 0], [1, 0, 1, 0], [1, 1, 1, 1], [0, 0, 0, 1]],
    1: [[0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1], [0, 0, 0, 1]],
}


def reach2_case(level_first):
    use_keep, p0 = REACH2_CASES[level_first]
    geom, levels, p0, rand_uv, keep = make_reach2_case(case_seed('reach2', level_first), p0)
    return geom, levels, p0, rand_uv, (keep if use_keep else None)


def pose_allowance_px(levels, p64, p32, tol_pose=1e-6):
    """The largest pixel displacement at any of ``levels`` that the pose gate of tests/test_lm_kernels_vs_fp64.py --
    max(tol_pose, 2 |ref32 - ref64|) per component -- lets a pose error cause: (lon / mpp) d_su + (lat / mpp) d_sv + rotation x radius,
    with the map's side A as a (generous) radius.  p64 / p32: the pose after one step in the two precisions, (su, sv, th) of [B,1]."""
    lat, lon, rot = RANGES
    a, b = torch.cat(p64, 1).double(), torch.cat(p32, 1).double()
    allow = torch.clamp(2 * (a - b).abs(), min=tol_pose)
    return max(float((lon / lv.mpp * allow[:, 0] + lat / lv.mpp * allow[:, 1] + rot / 180 * np.pi * allow[:, 2] * lv.A).max())
               for lv in levels)


# The one-level reach cases: name -> (shape, crossing pixel or None, indices into REACH_POSES of the samples, special).  The crossing
# pixel is ((row, column) -- negative values count from the end --, offset of u from col0, v); special: 'drop' -- a dropout mask
# that drops it (and every second other pixel), 'conf0' -- its confidence is zero.
_V = dict(zip(BORDER_CLASSES, border_values(REACH_A)))
REACH_CASES = {
    'clean': ('ragged', None, (0, 1, 2, 3), None),
    'first': ('ragged', (('row0', 0), REACH_LEFT[0], _V['on0']), (0, 2, 1), None),             # the first pixel read
    'last': ('ragged', ((-1, -1), REACH_LEFT[2], _V['onlim']), (0, 2, 1), None),               # the last pixel of the 3-px last tile
    'many_last': ('many', ((-1, -2), REACH_LEFT[1], _V['texel']), (0, 2), None),               # in the last of 65 tiles
    'not_read': ('skip', (('row0-1', 5), REACH_LEFT[0], _V['mid']), (0, 2), None),             # a stored row above row0
    'dropped': ('ragged', (('row0', 0), REACH_LEFT[0], _V['half']), (0, 2, 1), 'drop'),
    'conf0': ('ragged', (('row0', 0), REACH_LEFT[0], _V['farcell']), (0, 2, 1), 'conf0'),
    'idle_blocks': ('octet', None, (0, 2, 0, 2, 0, 2, 0, 2, 1), None),                         # B = 9, the crossing sample last
    'two_groups': ('octet', None, (1, 0, 2, 0, 2, 0, 2, 0, 2, 0, 2, 0, 2, 0, 2, 1, 1), None),  # B = 17: 0, 15 | 16 cross
}


def reach_case(name, C=64, dtype=torch.float32):
    """-> (geom, level, pose0 [B,3] fp32, keep [1, npix] uint8 or None, (row, column) of the crossing pixel or None)."""
    shape, cross, idx, special = REACH_CASES[name]
    h, w, row0, _ = SHAPES[shape]
    B = len(idx)
    seed = case_seed('reach', name)
    extra, rc = (), None
    if cross is not None:
        (r, c), du, v = cross
        r = {'row0': row0, 'row0-1': row0 - 1}.get(r, r)
        rc = (r % h, c % w)
        extra = ((rc, REACH_COL0 + du, v),)
    lv = make_reach_level(shape, C, B, seed, extra, dtype)
    keep = None
    if special == 'drop':
        keep = (np.random.RandomState(seed + 5).uniform(size=(1, (h - row0) * w)) < 0.5).astype(np.uint8)
        keep[0, (rc[0] - row0) * w + rc[1]] = 0
        keep = torch.from_numpy(keep)
    if special == 'conf0':
        lv.conf[:, 0, rc[0], rc[1]] = 0
    return make_geom(0, B), lv, reach_poses(idx), keep, rc
