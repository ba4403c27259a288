"""Host logic of ``LM_S2GP.orien_corr`` (models_kitti.py:1494-1624), the coarse heading search: the satellite maps are resampled
to polar form, the ground maps slide over them along the heading axis, and the normalised correlation of every shift comes back
(``mode='test'``: the argmin heading of the last level; ``mode='train'``: the triplet loss over all levels).

Per level the device path is: ``hla_grid_sample`` on the WINDOW of the polar grid the shifts read (sampling the window equals
sampling the whole 4W-wide polar map and slicing it; at rotation_range = 10 three quarters of that map are never read) ->
``hla_orien_corr`` -> ``hla_orien_triplet_loss``; backwards ``hla_orien_triplet_loss_bwd`` -> ``hla_orien_corr_bwd`` ->
``hla_orien_window_bwd`` (the sampler's backward to the map, summed in fp64) -> ``hla_vgg_backward`` of both extractors.  The
window ``P1`` [B,H,W+S-1,C] is kept for the backward (656 MB at B = 32 at the finest KITTI level)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .VGG import vgg_forward_nhwc, vgg_backward_nhwc

SAT_SIDE = 512          # polar_coordinates builds its grids for a 512 x 512 satellite image (models_kitti.py:1522)
CHANNELS = (16, 64, 128, 256)


def polar_coordinates(meters_per_pixel, level):
    """models_kitti.py:1518-1541, the same fp32 op sequence (bit-identical): [1, A//2, 8A, 2] pixel coordinates (x, y) into the
    level's A x A satellite map, A = 512 / 2^(3-level): row v is a range that falls from 40 m, column u a bearing, one turn
    per 2A columns (the grid holds four turns)."""
    A = SAT_SIDE / 2 ** (3 - level)
    grd_H = A // 2
    grd_W = A * 2
    v, u = torch.meshgrid(torch.arange(0, grd_H, dtype=torch.float32), torch.arange(0, 4 * grd_W, dtype=torch.float32), indexing='ij')
    theta = u / grd_W * np.pi * 2
    radius = (1 - v / grd_H) * 40 / meters_per_pixel
    us = A / 2 + radius * torch.cos(np.pi / 4 - theta)
    vs = A / 2 - radius * torch.sin(np.pi / 4 - theta)
    return torch.stack([us, vs], dim=-1).unsqueeze(dim=0)


def window_columns(sat_W: int, W: int, n: int):
    """The polar-map columns of the reference's ``polar_sat1`` (models_kitti.py:1582-1585), slice for slice: for 0 < n <= sat_W they
    are -n .. W+n-1 modulo sat_W in either ``cat`` case, S = 2n + 1 shifts.  The slices clamp like Python's: n = 0 makes
    ``[-0:]`` the WHOLE map (S = sat_W + 1 shifts, not 1), and n > sat_W makes ``[-n:]`` the whole map as well."""
    cols = list(range(sat_W))
    if sat_W - W < n:
        return cols[-n:] + cols + cols[:n - sat_W + W]
    return cols[-n:] + cols[:W + n]


def shifts(rotation_range: float, W: int):
    """(degree_per_pixel, n) of models_kitti.py:1579-1580."""
    deg = 90 / W
    return deg, int(np.ceil(rotation_range / deg))


def corr_forward(P1, grd, p1_inv, grd_inv):
    """``hla_orien_corr`` on P1 [B,H,W+S-1,C] and grd [B,H,W,C] (NHWC fp32; raw with their [B] fp64 inverse norms, or normalised with
    None).  Returns (corr [B,S] fp32, (dot, E, gnorm) fp64 for the backward)."""
    _lib.require_gpu(P1, 'orien_corr P1')
    _lib.require_gpu(grd, 'orien_corr grd_feat')
    lib = _lib.load()
    B, H, W, Cn = grd.shape
    if P1.dim() != 4 or P1.shape[0] != B or P1.shape[1] != H or P1.shape[3] != Cn or P1.shape[2] < W:
        raise ValueError(f'orien_corr: P1 {tuple(P1.shape)} does not match grd_feat {tuple(grd.shape)}')
    if P1.dtype != torch.float32 or grd.dtype != torch.float32 or not (P1.is_contiguous() and grd.is_contiguous()):
        raise ValueError('orien_corr: P1 and grd_feat must be contiguous fp32 NHWC tensors')
    S = P1.shape[2] - W + 1
    dev = grd.device
    dot = torch.empty(B, S, device=dev, dtype=torch.float64)
    E = torch.empty(B, S, device=dev, dtype=torch.float64)
    gnorm = torch.empty(B, device=dev, dtype=torch.float64)
    corr = torch.empty(B, S, device=dev, dtype=torch.float32)
    nbytes = lib.hla_orien_corr_workspace_bytes(B, H, W, Cn, S)
    if nbytes == 0:
        raise _lib.HlaError('hla_orien_corr_workspace_bytes: ' + lib.hla_last_error().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.hla_orien_corr(_lib.ptr(P1), _lib.ptr(grd), _lib.ptr(p1_inv), _lib.ptr(grd_inv), _lib.ptr(dot), _lib.ptr(E), _lib.ptr(gnorm),
                            _lib.ptr(corr), _lib.ptr(ws), nbytes, B, H, W, Cn, S, _lib.stream_ptr())
    _lib.check(rc, 'hla_orien_corr')
    return corr, (dot, E, gnorm)


def corr_backward(P1, grd, p1_inv, grd_inv, saved, d_corr):
    """``hla_orien_corr_bwd``: (d_P1 w.r.t. p1_inv * P1, d_grd w.r.t. grd_inv * grd), both written without atomics."""
    lib = _lib.load()
    B, H, W, Cn = grd.shape
    S = P1.shape[2] - W + 1
    dot, E, gnorm = saved
    d_corr = d_corr.float().contiguous()
    d_P1, d_grd = torch.empty_like(P1), torch.empty_like(grd)
    nbytes = lib.hla_orien_corr_workspace_bytes(B, H, W, Cn, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=grd.device)
    rc = lib.hla_orien_corr_bwd(_lib.ptr(P1), _lib.ptr(grd), _lib.ptr(p1_inv), _lib.ptr(grd_inv), _lib.ptr(dot), _lib.ptr(E),
                                _lib.ptr(gnorm), _lib.ptr(d_corr), _lib.ptr(d_P1), _lib.ptr(d_grd), _lib.ptr(ws), nbytes, B, H, W, Cn, S,
                                _lib.stream_ptr())
    _lib.check(rc, 'hla_orien_corr_bwd')
    return d_P1, d_grd


def sample_window(sat_feat, grid):
    """``hla_grid_sample`` of sat_feat [B,A,A,C] (NHWC fp32) at grid [B,H,Wp,2] -> P1 [B,H,Wp,C]."""
    B, A, A2, Cn = sat_feat.shape
    _, H, Wp, _ = grid.shape
    P1 = torch.empty(B, H, Wp, Cn, device=sat_feat.device, dtype=torch.float32)
    rc = _lib.load().hla_grid_sample(_lib.ptr(sat_feat), _lib.ptr(grid), None, _lib.ptr(P1), None, B, Cn, A, A2, H, Wp, 0, _lib.stream_ptr())
    _lib.check(rc, 'hla_grid_sample')
    return P1


def sample_window_bwd(sat_feat, grid, d_P1):
    """d(sat map) [B,A,A,C] of ``sample_window`` (``hla_orien_window_bwd``: summed in an fp64 scratch image of the map's size and
    rounded once -- the texels at the centre of the polar fan collect about a thousand cancelling terms each)."""
    B, A, A2, Cn = sat_feat.shape
    _, H, Wp, _ = grid.shape
    d_sat = torch.empty_like(sat_feat)
    acc = torch.empty(sat_feat.shape, device=sat_feat.device, dtype=torch.float64)
    rc = _lib.load().hla_orien_window_bwd(_lib.ptr(grid), _lib.ptr(d_P1), _lib.ptr(acc), _lib.ptr(d_sat), B, Cn, A, A2, H, Wp,
                                          _lib.stream_ptr())
    _lib.check(rc, 'hla_orien_window_bwd')
    return d_sat


def triplet_loss(corr, gt_heading, rotation_range, deg, loss, accumulate):
    B, S = corr.shape
    rc = _lib.load().hla_orien_triplet_loss(_lib.ptr(corr), _lib.ptr(gt_heading), gt_heading.stride(0), float(rotation_range), float(deg),
                                            _lib.ptr(loss), 1 if accumulate else 0, B, S, _lib.stream_ptr())
    _lib.check(rc, 'hla_orien_triplet_loss')


def triplet_loss_bwd(corr, gt_heading, rotation_range, deg, g_loss):
    B, S = corr.shape
    d_corr = torch.empty_like(corr)
    rc = _lib.load().hla_orien_triplet_loss_bwd(_lib.ptr(corr), _lib.ptr(gt_heading), gt_heading.stride(0), float(rotation_range),
                                                float(deg), _lib.ptr(g_loss), _lib.ptr(d_corr), B, S, _lib.stream_ptr())
    _lib.check(rc, 'hla_orien_triplet_loss_bwd')
    return d_corr


def _gt_column(gt_heading, device):
    """gt_heading [B,1] (or [B]) -> the fp32 device tensor whose column 0 the loss reads (models_kitti.py:1608,1615)."""
    g = gt_heading.to(device=device, dtype=torch.float32)
    return g[:, 0] if g.dim() == 2 else g


def levels_forward(model, sat_feats, sat_inv, grd_feats, grd_inv):
    """Every level of orien_corr on the extractors' raw NHWC maps -> [(corr, deg, n, P1, grid, saved)]."""
    out = []
    rr = float(model.args.rotation_range)
    for l in range(len(sat_feats)):
        B, H, W, Cn = grd_feats[l].shape
        A = sat_feats[l].shape[1]
        if Cn not in CHANNELS:
            raise _lib.HlaError(f'orien_corr: unsupported channel count {Cn} at level {l} (supported: {CHANNELS})')
        if H != A // 2:
            raise ValueError(f'orien_corr: level {l} ground map has {H} rows, the polar satellite map {A // 2} (the reference correlates '
                             'them row for row: the ground image must be 256 rows high)')
        deg, n = shifts(rr, W)
        grid = model._polar_window(l, n, W, B, sat_feats[l].device)
        P1 = sample_window(sat_feats[l], grid)
        corr, saved = corr_forward(P1, grd_feats[l], sat_inv[l], grd_inv[l])
        out.append((corr, deg, n, P1, grid, saved))
    return out


class _OrienCorrFn(torch.autograd.Function):
    """mode='train': the triplet loss (a scalar) whose backward is the HIP backward pass through both extractors."""

    @staticmethod
    def forward(ctx, model, names, sat_map, grd_img, gt, *params):
        sat_feats, _, sat_inv, cs = vgg_forward_nhwc(model.SatFeatureNet, sat_map, want_conf=False, defer_norm=True, save_for_backward=True)
        grd_feats, _, grd_inv, cg = vgg_forward_nhwc(model.GrdFeatureNet, grd_img, want_conf=False, defer_norm=True, save_for_backward=True)
        lv = levels_forward(model, sat_feats, sat_inv, grd_feats, grd_inv)
        loss = torch.empty(1, device=sat_map.device, dtype=torch.float32)
        for l, (corr, deg, *_) in enumerate(lv):
            triplet_loss(corr, gt, model.args.rotation_range, deg, loss, l > 0)
        model.last_orien_corr = [(c.detach(), deg) for c, deg, *_ in lv]
        ctx.model, ctx.names, ctx.gt = model, names, gt
        ctx.state = (sat_feats, sat_inv, grd_feats, grd_inv, cs, cg, lv)
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        model = ctx.model
        if ctx.state is None:
            raise RuntimeError('backward through the same orien_corr forward twice: the saved activations are released after the first')
        sat_feats, sat_inv, grd_feats, grd_inv, cs, cg, lv = ctx.state
        g = g_loss.float().reshape(1).contiguous()
        d_sat, d_grd = [], []
        for l, (corr, deg, n, P1, grid, saved) in enumerate(lv):
            d_corr = triplet_loss_bwd(corr, ctx.gt, model.args.rotation_range, deg, g)
            d_P1, dg = corr_backward(P1, grd_feats[l], sat_inv[l], grd_inv[l], saved, d_corr)
            d_sat.append(sample_window_bwd(sat_feats[l], grid, d_P1))
            d_grd.append(dg)
        g_sat = vgg_backward_nhwc(model.SatFeatureNet, cs, d_sat)
        g_grd = vgg_backward_nhwc(model.GrdFeatureNet, cg, d_grd)
        grads = {'SatFeatureNet.' + k: v for k, v in g_sat.items()}
        grads.update({'GrdFeatureNet.' + k: v for k, v in g_grd.items()})
        ctx.state = None
        return (None,) * 5 + tuple(grads.get(n) for n in ctx.names)


@_lib.on_device(lambda model, sat_map, *a, **k: sat_map)
def orien_corr(model, sat_map, grd_img, gt_heading, mode):
    _lib.require_gpu(sat_map, 'orien_corr sat_map')
    _lib.require_gpu(grd_img, 'orien_corr grd_img_left')
    if sat_map.dim() != 4 or grd_img.dim() != 4 or sat_map.shape[0] != grd_img.shape[0] or sat_map.shape[1] != 3 or grd_img.shape[1] != 3:
        raise ValueError(f'expected sat_map [B,3,A,A] and grd_img [B,3,H,W] with one B, got {tuple(sat_map.shape)} and {tuple(grd_img.shape)}')
    if tuple(sat_map.shape[-2:]) != (SAT_SIDE, SAT_SIDE):
        raise ValueError(f'orien_corr: sat_map must be {SAT_SIDE} x {SAT_SIDE}, got {tuple(sat_map.shape[-2:])}: the polar grids are built '
                         f'for that size, as in the reference (models_kitti.py:1522), whose conv shapes stop matching for any other')
    _lib.same_device(('sat_map', sat_map), ('grd_img', grd_img), ('parameters', model.damping))
    train = mode == 'train'
    if train:
        if gt_heading is None:
            raise ValueError("orien_corr(mode='train') needs gt_heading")
        gt = _gt_column(gt_heading, sat_map.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters()):
            names = [k for k, _ in model.named_parameters()]
            params = [p for _, p in model.named_parameters()]
            return _OrienCorrFn.apply(model, names, sat_map, grd_img, gt, *params)
    sat_feats, _, sat_inv = vgg_forward_nhwc(model.SatFeatureNet, sat_map, want_conf=False, defer_norm=True)
    grd_feats, _, grd_inv = vgg_forward_nhwc(model.GrdFeatureNet, grd_img, want_conf=False, defer_norm=True)
    lv = levels_forward(model, sat_feats, sat_inv, grd_feats, grd_inv)
    model.last_orien_corr = [(c, deg) for c, deg, *_ in lv]
    if train:
        loss = torch.empty(1, device=sat_map.device, dtype=torch.float32)
        for l, (corr, deg, *_) in enumerate(lv):
            triplet_loss(corr, gt, model.args.rotation_range, deg, loss, l > 0)
        return loss[0]
    corr, deg, n = lv[-1][:3]
    return (torch.argmin(corr, dim=-1) - n) * deg          # the LAST level's heading [B], degrees (models_kitti.py:1596-1597,1605)
