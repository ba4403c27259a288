"""Pose scoring and pose search as both directions run them (satellite->ground: ``S2GPBase``, _s2gp.py; ground->satellite:
``LM_G2SP``, _g2sp.py): the pose-list arguments, the calls of ``hla_{s2g,g2s}_pose_score[_bwd]`` (include/hla.h), the top-m search
around the LM loop and the triplet-form loss on the score surface.  A direction's method builds its structs and names its entry
point and its own C arguments; the rest is here."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def pose_grid(n_u: int, n_v: int, n_theta: int, span=(1., 1., 1.)):
    """Candidate poses for ``forward_search``: a centred lattice over [-span, span] per component, in the normalised units of the
    pose (1 = shift_range / rotation_range), [n_u * n_v * n_theta, 3] fp32 (shift_u, shift_v, theta).  The counts are odd so that
    the zero pose is on the lattice; it is candidate 0, the others follow with shift_u outermost and theta innermost."""
    axes = []
    for name, n, s in zip(('n_u', 'n_v', 'n_theta'), (n_u, n_v, n_theta), span):
        if int(n) != n or n < 1 or n % 2 == 0:
            raise ValueError(f'{name} must be a positive odd count (the lattice is centred on the zero pose), got {n}')
        half = (int(n) - 1) // 2
        axes.append(torch.tensor([float(s) * i / half if half else 0.0 for i in range(-half, half + 1)], dtype=torch.float32))
    grid = torch.cartesian_prod(*axes).reshape(-1, 3)
    zero = (len(axes[0]) // 2 * len(axes[1]) + len(axes[1]) // 2) * len(axes[2]) + len(axes[2]) // 2
    order = [zero] + [i for i in range(grid.shape[0]) if i != zero]
    return grid[order].contiguous()


def eligible_cost(cost, sums, min_in_view):
    """The ranking rule of ``forward_search``: a candidate is eligible when its pixels in view (``sums[..., 6]``) reach
    ``min_in_view`` times the sample's maximum over its candidates; the others get +inf.  (A pose with nothing in view scores 1,
    below the ~2 of a mismatch, and would otherwise win.)  A sample without any eligible candidate keeps candidate 0.
    cost [B,K], sums [B,K,8] -> [B,K] in cost's dtype."""
    in_view = sums[..., 6]
    ok = in_view >= float(min_in_view) * in_view.max(dim=1, keepdim=True).values
    out = torch.where(ok, cost, torch.full_like(cost, float('inf')))
    none = ~ok.any(dim=1)
    out[:, 0] = torch.where(none, torch.zeros_like(cost[:, 0]), out[:, 0])
    return out


def _poses_arg(poses, B: int, name: str = 'poses'):
    """[K,3] (shared) or [B,K,3] -> [B,K,3] fp32, K >= 1."""
    p = torch.as_tensor(poses, dtype=torch.float32)
    if p.dim() == 2 and p.shape[1] == 3 and p.shape[0] >= 1:
        return p[None].expand(B, -1, -1)
    if p.dim() == 3 and p.shape[0] == B and p.shape[2] == 3 and p.shape[1] >= 1:
        return p
    raise ValueError(f'{name} must be [K,3] or [B,K,3] with B = {B} and K >= 1, got {tuple(p.shape)}')


def levels_arg(levels, n: int):
    """``levels`` of ``score_candidates`` / ``score_loss`` -> a tuple of distinct indices in [0, n) (None: all of them)."""
    lvls = tuple(range(n)) if levels is None else tuple(int(l) for l in levels)
    if not lvls or len(set(lvls)) != len(lvls) or not all(0 <= l < n for l in lvls):
        raise ValueError(f'levels must be distinct indices in [0, {n}), got {levels}')
    return lvls


def true_pose_first(gt_pose, candidates, B: int, device):
    """The pose list of ``score_loss``: (shift_u, shift_v, heading) of the true pose, each [B] or [B,1], then ``candidates``
    ([K,3] or [B,K,3]) -> [B,K+1,3] fp32 on ``device``, entry 0 the true pose."""
    cand = _poses_arg(candidates, B, 'candidates').to(device)
    gt = torch.stack([torch.as_tensor(g, dtype=torch.float32).detach().to(device).reshape(B) for g in gt_pose], dim=1)
    return torch.cat([gt[:, None, :], cand], dim=1).contiguous()


def _checked(structs, sat_feats, poses, level):
    """The argument checks of ``score_poses`` / ``score_poses_bwd``, then the direction's structs: ``structs()`` -> (cfg, lv,
    extra); ``extra``: what its entry points take between the level and the poses, tensors (or None) and ints.
    -> (cfg, the level's struct by reference, extra as C arguments, poses [B,K,3] on the device, the level's index); the tensors of
    ``extra`` and the struct array stay alive in ``keep``, the last element, until the caller returns."""
    B, L = sat_feats[0].shape[0], len(sat_feats)
    p = _poses_arg(poses, B)
    if not 0 <= int(level) < L:
        raise ValueError(f'level must be in [0, {L}), got {level}')
    _lib.require_gpu(sat_feats[0], 'sat_feats')
    cfg, lv, extra = structs()
    args = [a if isinstance(a, int) else _lib.ptr(a) for a in extra]
    return cfg, C.byref(lv[int(level)]), args, p.to(sat_feats[0].device).contiguous(), int(level), (lv, extra)


def _workspace(entry, cfg, one, B, K, dev):
    nbytes = getattr(_lib.load(), entry + '_workspace_bytes')(C.byref(cfg), one, B, K)
    if nbytes == 0:
        _lib.check(-1, entry + '_workspace_bytes')
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def score_poses(entry, structs, sat_feats, poses, level):
    """``entry`` = 'hla_{s2g,g2s}_pose_score' at ``poses`` on level ``level`` -> (cost [B,K] fp32, sums [B,K,8] fp64)."""
    cfg, one, args, p, _, keep = _checked(structs, sat_feats, poses, level)
    dev = p.device
    B, K = p.shape[:2]
    cost = torch.empty(B, K, device=dev, dtype=torch.float32)
    sums = torch.empty(B, K, 8, device=dev, dtype=torch.float64)
    ws, nbytes = _workspace(entry, cfg, one, B, K, dev)
    rc = getattr(_lib.load(), entry)(C.byref(cfg), one, *args, _lib.ptr(p), K, _lib.ptr(sums), _lib.ptr(cost), _lib.ptr(ws), nbytes, B,
                                     _lib.stream_ptr())
    _lib.check(rc, entry)
    return cost, sums


def score_poses_bwd(entry, structs, sat_feats, grd_feats, grd_confs, poses, level, sums, d_cost):
    """``entry`` = 'hla_{s2g,g2s}_pose_score_bwd': ``sums`` [B,K,8] of the forward and ``d_cost`` [B,K] -> (d_sat, d_grd, d_conf or
    None) of level ``level``, fp32 NHWC, all three written by the call."""
    cfg, one, args, p, l, keep = _checked(structs, sat_feats, poses, level)
    dev = p.device
    B, K = p.shape[:2]
    if tuple(sums.shape) != (B, K, 8) or sums.dtype != torch.float64 or tuple(d_cost.shape) != (B, K):
        raise ValueError(f'expected sums [B,K,8] fp64 and d_cost [B,K] with B = {B}, K = {K}, got {tuple(sums.shape)} '
                         f'{sums.dtype} and {tuple(d_cost.shape)}')
    sums, dc = sums.to(dev).contiguous(), d_cost.to(dev).float().contiguous()
    d_sat, d_grd = torch.empty_like(sat_feats[l], dtype=torch.float32), torch.empty_like(grd_feats[l], dtype=torch.float32)
    d_conf = torch.empty_like(grd_confs[l]) if cfg.using_weight else None
    gr = _lib.S2GLevelGrad()
    gr.d_sat_feat, gr.d_grd_feat, gr.d_grd_conf = d_sat.data_ptr(), d_grd.data_ptr(), d_conf.data_ptr() if d_conf is not None else 0
    ws, nbytes = _workspace(entry, cfg, one, B, K, dev)
    rc = getattr(_lib.load(), entry)(C.byref(cfg), one, C.byref(gr), *args, _lib.ptr(p), K, _lib.ptr(sums), _lib.ptr(dc), _lib.ptr(ws),
                                     nbytes, B, _lib.stream_ptr())
    _lib.check(rc, entry)
    return d_sat, d_grd, d_conf


def score_level_grads(model, bwd, levels, d_out, sat_feats, grd_feats, grd_confs):
    """The map gradients of a ``score_candidates`` backward in either direction: ``bwd(n, l)`` -> (d_sat, d_grd, d_conf) of the
    n-th scored level l; a level that was not scored, or whose cost was not used downstream (``d_out[n]`` None), takes no part:
    zeros.  -> (d_sat[l], d_grd[l], d_conf[l] or None when the confidence heads take no part)."""
    L = len(sat_feats)
    use_w = bool(model.using_weight) and all(c is not None for c in grd_confs)
    d_sat, d_grd, d_conf = [None] * L, [None] * L, [None] * L
    for n, l in enumerate(levels):
        if d_out[n] is not None:
            d_sat[l], d_grd[l], d_conf[l] = bwd(n, l)
    for l in range(L):
        if d_sat[l] is None:
            d_sat[l], d_grd[l] = torch.zeros_like(sat_feats[l]), torch.zeros_like(grd_feats[l])
        if use_w and d_conf[l] is None:
            d_conf[l] = torch.zeros_like(grd_confs[l])
    return d_sat, d_grd, d_conf if use_w else None


def search(model, cand, top_m: int, score, solve, score_level, finest: int, min_in_view):
    """The top-m search of ``forward_search`` in both directions, on feature maps the caller extracted (under no_grad):
    ``score(poses, level)`` -> (cost, sums) scores ``cand`` [B,K,3] at ``score_level``; ``solve(init_pose)`` -> trace runs the LM
    loop from each of the ``top_m`` best eligible ones (``eligible_cost``); the final pose that scores best at level ``finest``
    is returned, [B,3] in the trace's order.  ``model.last_search`` keeps cost, sums, start_index, traces, final_cost, best."""
    cost, sums = score(cand, score_level)
    start_index = torch.topk(eligible_cost(cost, sums, min_in_view), top_m, dim=1, largest=False, sorted=True).indices
    starts = cand.gather(1, start_index[:, :, None].expand(-1, -1, 3))
    traces = torch.stack([solve(starts[:, m].contiguous()) for m in range(top_m)], dim=1)
    finals = traces[:, :, -1, -1, :].contiguous()
    final_cost, _ = score(finals, finest)
    best = final_cost.argmin(dim=1)
    model.last_search = dict(cost=cost, sums=sums, start_index=start_index, traces=traces, final_cost=final_cost, best=best)
    return finals.gather(1, best[:, None, None].expand(-1, 1, 3))[:, 0]


def search_candidates(candidates, top_m, sat_map):
    """``candidates`` ([K,3] or [B,K,3]) and ``top_m`` of ``forward_search`` -> ([B,K,3] on sat_map's device, int top_m)."""
    cand = _poses_arg(candidates, sat_map.shape[0], 'candidates').to(sat_map.device)
    if not 1 <= int(top_m) <= cand.shape[1]:
        raise ValueError(f'top_m must be in [1, {cand.shape[1]}] (the number of candidates), got {top_m}')
    return cand, int(top_m)


def score_loss_tail(model, costs, sums, min_in_view):
    """The loss of ``score_loss`` in both directions, from the costs [B,K+1] and sums [B,K+1,8] of the scored levels (entry 0:
    the true pose); ``model.last_score_loss`` keeps them."""
    loss = 0
    for cost, s in zip(costs, sums):
        B, K = cost.shape[0], cost.shape[1] - 1
        # eligible_cost's in-view rule over the K + 1 entries; an ineligible negative contributes exactly zero
        in_view = s[..., 6]
        ok = (in_view >= float(min_in_view) * in_view.max(dim=1, keepdim=True).values)[:, 1:]
        # models_kitti.py:592, 1622: log(1 + exp(10 (pos - neg))), averaged; cost <= 4 keeps the exponent below 40
        t = torch.log(1 + torch.exp(10.0 * (cost[:, :1] - cost[:, 1:])))
        loss = loss + torch.where(ok, t, torch.zeros_like(t)).sum() / (B * K)     # models_kitti.py:595: summed over the levels
    model.last_score_loss = dict(costs=[c.detach() for c in costs], sums=sums)
    return loss
