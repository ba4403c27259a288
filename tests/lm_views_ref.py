"""fp64-capable reference of ONE step of the multi-view LM loop (``hla_s2g_lm_solve_views``), on top of ``tests/lm_kernel_ref.py``:
the reference's ``LM_update`` applied to the UNION of the views' pixels.  The satellite map is projected into every view with that
view's table and (R_v, T_v) at the common pose (``R.pose_to_uv_ford``), the views' rows from row0 on are concatenated, and
``R.step`` / ``R.step_sums`` run once with row0 = 0, i.e. ``O.lm_update`` on the union.  Everything runs in the dtype of its inputs:
the same code on fp32 inputs is the "ref32" that sizes the gates.

A views level is a ``lm_kernel_ref`` level whose ground map, confidence and table carry the pseudo-batch B * V (view v of sample
b at index b * V + v; ``table`` [V,h,w,3]) next to a satellite map of batch B; a views geometry has R_FL [B,V,3,3], T_FL [B,V,3].
"""
from types import SimpleNamespace

import numpy as np
import torch

import lm_kernel_ref as R
from oracle import ref_cpu as O

# dyadic offsets added to FORD_T per view: X + T stays exact
VIEW_T_OFFSETS = ((0.0, 0.0, 0.0), (0.5, -0.25, 0.0), (-0.75, 0.5, 0.125), (0.25, 0.25, -0.125),
                  (-0.5, -0.5, 0.0), (1.0, 0.0, 0.25), (0.0, -0.75, 0.0), (-0.25, 0.75, 0.5))


def make_views_geom(B, V):
    g = SimpleNamespace(ford=1, ranges=R.RANGES)
    g.R_FL = torch.tensor(R.FORD_R).repeat(B, V, 1, 1)
    T = torch.tensor([[R.FORD_T[i] + VIEW_T_OFFSETS[v][i] for i in range(3)] for v in range(V)])
    g.T_FL = T[None].repeat(B, 1, 1).contiguous()
    return g


def make_views_level(shape, C, A, B, V, seed, mpp=0.5, dtype=torch.float32):
    """``R.make_level(True, ...)`` with batch B * V for ground map and confidence, a table seed per view, and the satellite maps
    of the first B samples."""
    lv = R.make_level(1, shape, C, A, B * V, seed, mpp, dtype)
    lv.sat = lv.sat[:B].contiguous()
    lv.table = torch.stack([R.border_table(1, A, lv.h, lv.w, lv.row0, seed + 101 * v, mpp)[0] for v in range(V)])
    lv.V = V
    return lv


def cast_views_geom(g, dt):
    o = SimpleNamespace(**vars(g))
    o.R_FL, o.T_FL = g.R_FL.to(dt), g.T_FL.to(dt)
    return o


def select_views(geom, lv, views):
    """The same case with the views ``views`` (a list of indices; repeats allowed), in that order."""
    V, B = lv.V, lv.sat.shape[0]
    g = SimpleNamespace(**vars(geom))
    g.R_FL, g.T_FL = geom.R_FL[:, views].contiguous(), geom.T_FL[:, views].contiguous()
    o = SimpleNamespace(**vars(lv))
    pick = lambda t: t.reshape(B, V, *t.shape[1:])[:, views].reshape(B * len(views), *t.shape[1:]).contiguous()
    o.grd, o.conf, o.table, o.V = pick(lv.grd), pick(lv.conf), lv.table[views].contiguous(), len(views)
    return g, o


def select_samples(geom, lv, samples):
    V = lv.V
    g = SimpleNamespace(**vars(geom))
    g.R_FL, g.T_FL = geom.R_FL[samples].contiguous(), geom.T_FL[samples].contiguous()
    o = SimpleNamespace(**vars(lv))
    rows = [b * V + v for b in samples for v in range(V)]
    o.sat, o.grd, o.conf = lv.sat[samples].contiguous(), lv.grd[rows].contiguous(), lv.conf[rows].contiguous()
    return g, o


def masked_table(table):
    """A table no point of which has z > 0: the view contributes fourteen exact zeros."""
    t = table.clone()
    t[..., 2] = -t[..., 2].abs() - 1.0
    return t


def view_operands(geom, lv, pose, v):
    """sat, grd, conf, uv, jac, mask of view v alone (full maps: rows are cut by the caller's row0)."""
    B = lv.sat.shape[0]
    su, sv, th = pose
    uv, jac, mask = R.pose_to_uv_ford(lv.table[v], geom.R_FL[:, v], geom.T_FL[:, v], su, sv, th, lv.A, lv.mpp, lv.centre, geom.ranges)
    return lv.sat, lv.grd[v::lv.V], lv.conf[v::lv.V], uv, jac, mask


def union_operands(geom, lv, pose):
    """The views' rows from row0 on, concatenated: what ``R.step`` / ``R.step_sums`` take with row0 = 0."""
    r0 = lv.row0
    ops = [view_operands(geom, lv, pose, v) for v in range(lv.V)]
    grd = torch.cat([o[1][:, :, r0:] for o in ops], 2)
    conf = torch.cat([o[2][:, :, r0:] for o in ops], 2)
    uv = torch.cat([o[3][:, r0:] for o in ops], 1)
    jac = tuple(torch.cat([o[4][i][:, r0:] for o in ops], 1) for i in range(3))
    mask = torch.cat([o[5][:, r0:] for o in ops], 1)
    return lv.sat, grd, conf, uv, jac, mask


def views_sums(geom, lv, pose, using_weight):
    """The 14 sums of the union [B,14] and the sums of the absolute values of their terms [B,14]."""
    sat, grd, conf, uv, jac, mask = union_operands(geom, lv, pose)
    sums, mags, _ = R.step_sums(sat, grd, conf if using_weight else None, uv, jac, mask, lv.A, 0, using_weight)
    return sums, mags


def one_view_sums(geom, lv, pose, v, using_weight):
    sat, grd, conf, uv, jac, mask = view_operands(geom, lv, pose, v)
    sums, mags, _ = R.step_sums(sat, grd, conf if using_weight else None, uv, jac, mask, lv.A, lv.row0, using_weight)
    return sums, mags


def views_step(args, geom, lv, pose, using_weight, rand_uv, gauss_newton=False):
    """``O.lm_update`` on the union: pose (su, sv, th) -> the pose after the step."""
    sat, grd, conf, uv, jac, mask = union_operands(geom, lv, pose)
    if not gauss_newton:
        return R.step(args, True, sat, grd, conf, uv, jac, mask, 0, pose, using_weight, rand_uv)
    f, g, gc, J = R._operands(sat, grd, conf, uv, jac, mask, 0, None)      # (R.step has no GN switch: its own two lines)
    return O.lm_update(args, None, *pose, f, g, gc, J, using_weight, ford=True, rand_uv=rand_uv, gauss_newton=True)


def step_from_sums(S, pose, lam=1.0):
    """The damped solve from 14 de-normalised sums [B,14] (fp64): what the closing kernel does with the total."""
    S = np.asarray(S, np.float64)
    out = []
    for b in range(S.shape[0]):
        s = S[b]
        ns, ng = max(np.sqrt(s[0]), 1e-6), max(np.sqrt(s[1]), 1e-6)
        H = np.array([[s[2], s[3], s[4]], [s[3], s[5], s[6]], [s[4], s[6], s[7]]]) / ns ** 2
        g = s[8:11] / ns ** 2 - s[11:14] / (ns * ng)
        out.append(-np.linalg.solve(H + lam * np.eye(3), g))
    return np.asarray(pose, np.float64) + np.stack(out)


def step_per_view_normalised(Sv, pose, lam=1.0):
    """The PLANTED variant the feature must not be: every view's H and right-hand side normalised by that view's own norms,
    then added.  Sv: list of [B,14]."""
    Sv = [np.asarray(s, np.float64) for s in Sv]
    out = []
    for b in range(Sv[0].shape[0]):
        H, g = np.zeros((3, 3)), np.zeros(3)
        for S in Sv:
            s = S[b]
            ns, ng = max(np.sqrt(s[0]), 1e-6), max(np.sqrt(s[1]), 1e-6)
            H += np.array([[s[2], s[3], s[4]], [s[3], s[5], s[6]], [s[4], s[6], s[7]]]) / ns ** 2
            g += s[8:11] / ns ** 2 - s[11:14] / (ns * ng)
        out.append(-np.linalg.solve(H + lam * np.eye(3), g))
    return np.asarray(pose, np.float64) + np.stack(out)


def random_pose(B, seed, scale=0.3):
    rs = np.random.RandomState(seed)
    p0 = torch.from_numpy(rs.uniform(-scale, scale, size=(B, 3)).astype(np.float32))
    return p0


def random_draws(steps, B, seed):
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, size=(steps, 2, B)).astype(np.float32))
