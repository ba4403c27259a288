"""Host logic of ``LM_G2SP.corr`` (models_kitti.py:501-595), the dense translation search: per level the ground map is projected
onto the satellite plane at the zero pose, centre-cropped by the shift ranges, L2-normalised and slid over the satellite map in
both axes; the normalised correlation of every shift comes back (``mode='train'``: the triplet loss over all levels; any other
mode: the argmin shift of the last level, in metres).

Per level the device path is: ``hla_grid_sample`` at the crop's zero-pose coordinates (sampling the crop equals projecting the
whole A x A map and cropping it) -> ``hla_g2s_corr`` (fp32-input MFMA) -> ``hla_g2s_corr_triplet_loss``; backwards
``hla_g2s_corr_triplet_loss_bwd`` -> ``hla_g2s_corr_bwd`` -> ``hla_orien_window_bwd`` (the sampler's backward to the ground map)
-> ``hla_vgg_backward`` of both extractors.  The sampler's backward is the fp64-summed one, not ``hla_grid_sample_bwd``: towards
the horizon many satellite pixels land on the same few ground texels, and the triplet loss's cotangent sums to zero over the
shifts, so a texel collects many cancelling terms -- the case that entry point was written for; it also makes the ground
gradient reproducible to the last bit but for 1e-16 relative."""
from __future__ import annotations

import torch

from . import _lib, utils
from ._autograd import extract_saved, extractor_grads, grad_params, take_state

CHANNELS = (16, 64, 128, 256)


def level_mpp(level: int) -> float:
    """``self.meters_per_pixel[level]`` (its constructor): fixed per level, whatever the map's size."""
    return utils.get_meter_per_pixel() * 2 ** (3 - level)


def crop_plan(A: int, level: int, args):
    """(Hc, Wc, top, left) of models_kitti.py:546-548: crop_H = int(A - shift_range_lat * 2 / mpp), crop_W likewise with
    shift_range_lon, and torchvision's center_crop offsets int(round((A - crop) / 2.0)) (Python's round: half to even)."""
    mpp = level_mpp(level)
    Hc = int(A - args.shift_range_lat * 2 / mpp)
    Wc = int(A - args.shift_range_lon * 2 / mpp)
    if Hc < 1 or Wc < 1:
        raise ValueError(f'corr: level {level}: the shift ranges ({args.shift_range_lat} m, {args.shift_range_lon} m) leave a '
                         f'{Hc} x {Wc} crop of the {A} x {A} map ({mpp:.4f} m per pixel): the ranges are too large for the map')
    return Hc, Wc, int(round((A - Hc) / 2.0)), int(round((A - Wc) / 2.0))


def zero_pose_grid(camera_k, A: int, hw_feat, ori_hw, plan):
    """The reference's ``uv`` (get_warp_sat2real + seq_warp_real2camera, models_kitti.py:53-161, at shift = heading = 0) of the
    crop's pixels: [B,Hc,Wc,2] fp32 (x, y) coordinates into the hw_feat ground feature map.  Computed on camera_k's device in
    fp64 and rounded once.  A point behind the camera has its depth clamped at 1e-6 and lands far out of bounds (it samples 0)."""
    Hc, Wc, top, left = plan
    dev = camera_k.device
    f64 = torch.float64
    mpp = utils.get_meter_per_pixel() * utils.get_process_satmap_sidelength() / A          # 71-72: of the A x A map
    X = (torch.arange(top, top + Hc, device=dev, dtype=f64) - (A // 2)) * mpp               # the map's row -> camera X
    Z = (torch.arange(left, left + Wc, device=dev, dtype=f64) - (A // 2)) * mpp             # the map's column -> camera Z
    X, Z = X.view(1, Hc, 1).expand(1, Hc, Wc), Z.view(1, 1, Wc).expand(1, Hc, Wc)
    Y = torch.full_like(X, utils.get_camera_height())
    K = camera_k.to(f64).clone()
    K[:, 0, :] *= hw_feat[1] / ori_hw[1]                                                    # 111-113
    K[:, 1, :] *= hw_feat[0] / ori_hw[0]
    P = torch.stack([X, Y, Z], dim=-1)                                                      # [1,Hc,Wc,3]
    uv1 = (K[:, None, None, :, :] * P[:, :, :, None, :]).sum(-1)                            # [B,Hc,Wc,3]
    last = uv1[..., 2:].clamp_min(1e-6)
    return (uv1[..., :2] / last).float().contiguous()


def _shapes(sat, g2s):
    if sat.dim() != 4 or g2s.dim() != 4 or sat.shape[1] != sat.shape[2] or sat.shape[0] != g2s.shape[0] or sat.shape[3] != g2s.shape[3]:
        raise ValueError(f'g2s_corr: sat {tuple(sat.shape)} must be [B,A,A,C] and g2s {tuple(g2s.shape)} [B,Hc,Wc,C]')
    if sat.dtype != torch.float32 or g2s.dtype != torch.float32 or not (sat.is_contiguous() and g2s.is_contiguous()):
        raise ValueError('g2s_corr: sat and g2s must be contiguous fp32 NHWC tensors')
    B, A, _, Cn = sat.shape
    return B, A, g2s.shape[1], g2s.shape[2], Cn


def _workspace(lib, B, A, Hc, Wc, Cn, dev, nbytes=None):
    n = lib.hla_g2s_corr_workspace_bytes(B, A, Hc, Wc, Cn)
    if n == 0:
        raise _lib.HlaError('hla_g2s_corr_workspace_bytes: ' + lib.hla_last_error().decode())
    n = n if nbytes is None else nbytes
    return torch.empty(max(n, 1), dtype=torch.uint8, device=dev), n


def corr_forward(sat, g2s, sat_inv, g2s_inv, out=None, workspace_bytes=None):
    """``hla_g2s_corr`` on sat [B,A,A,C] and g2s [B,Hc,Wc,C] (NHWC fp32; raw with their [B] fp64 inverse norms, or normalised with
    None).  Returns (corr [B,Ny,Nx] fp32, (dot, E, gnorm) fp64 for the backward).  ``out`` = (dot, E, gnorm, corr) to write into
    and ``workspace_bytes`` (a size to hand over instead of the required one) serve the tests."""
    _lib.require_gpu(sat, 'g2s_corr sat')
    _lib.require_gpu(g2s, 'g2s_corr g2s')
    lib = _lib.load()
    B, A, Hc, Wc, Cn = _shapes(sat, g2s)
    dev = sat.device
    ws, nbytes = _workspace(lib, B, A, Hc, Wc, Cn, dev, workspace_bytes)
    Ny, Nx = A - Hc + 1, A - Wc + 1
    if out is None:
        out = (torch.empty(B, Ny, Nx, device=dev, dtype=torch.float64), torch.empty(B, Ny, Nx, device=dev, dtype=torch.float64),
               torch.empty(B, device=dev, dtype=torch.float64), torch.empty(B, Ny, Nx, device=dev, dtype=torch.float32))
    dot, E, gnorm, corr = out
    rc = lib.hla_g2s_corr(_lib.ptr(sat), _lib.ptr(g2s), _lib.ptr(sat_inv), _lib.ptr(g2s_inv), _lib.ptr(dot), _lib.ptr(E), _lib.ptr(gnorm),
                          _lib.ptr(corr), _lib.ptr(ws), nbytes, B, A, Hc, Wc, Cn, _lib.stream_ptr())
    _lib.check(rc, 'hla_g2s_corr')
    return corr, (dot, E, gnorm)


def corr_backward(sat, g2s, sat_inv, g2s_inv, saved, d_corr, out=None):
    """``hla_g2s_corr_bwd``: (d_sat w.r.t. sat_inv * sat, d_g2s w.r.t. g2s_inv * g2s), both written without atomics."""
    lib = _lib.load()
    B, A, Hc, Wc, Cn = _shapes(sat, g2s)
    dot, E, gnorm = saved
    d_corr = d_corr.float().contiguous()
    d_sat, d_g2s = out if out is not None else (torch.empty_like(sat), torch.empty_like(g2s))
    ws, nbytes = _workspace(lib, B, A, Hc, Wc, Cn, sat.device)
    rc = lib.hla_g2s_corr_bwd(_lib.ptr(sat), _lib.ptr(g2s), _lib.ptr(sat_inv), _lib.ptr(g2s_inv), _lib.ptr(dot), _lib.ptr(E),
                              _lib.ptr(gnorm), _lib.ptr(d_corr), _lib.ptr(d_sat), _lib.ptr(d_g2s), _lib.ptr(ws), nbytes, B, A, Hc, Wc, Cn,
                              _lib.stream_ptr())
    _lib.check(rc, 'hla_g2s_corr_bwd')
    return d_sat, d_g2s


def sample_crop(grd_feat, grid):
    """``hla_grid_sample`` of grd_feat [B,h,w,C] (NHWC fp32) at grid [B,Hc,Wc,2] -> [B,Hc,Wc,C]."""
    B, h, w, Cn = grd_feat.shape
    _, Hc, Wc, _ = grid.shape
    out = torch.empty(B, Hc, Wc, Cn, device=grd_feat.device, dtype=torch.float32)
    rc = _lib.load().hla_grid_sample(_lib.ptr(grd_feat), _lib.ptr(grid), None, _lib.ptr(out), None, B, Cn, h, w, Hc, Wc, 0, _lib.stream_ptr())
    _lib.check(rc, 'hla_grid_sample')
    return out


def sample_crop_bwd(grd_feat, grid, d_g2s):
    """d(ground map) [B,h,w,C] of ``sample_crop`` (``hla_orien_window_bwd``: summed in an fp64 image of the map's size, rounded once)."""
    B, h, w, Cn = grd_feat.shape
    _, Hc, Wc, _ = grid.shape
    d_grd = torch.empty_like(grd_feat)
    acc = torch.empty(grd_feat.shape, device=grd_feat.device, dtype=torch.float64)
    rc = _lib.load().hla_orien_window_bwd(_lib.ptr(grid), _lib.ptr(d_g2s), _lib.ptr(acc), _lib.ptr(d_grd), B, Cn, h, w, Hc, Wc,
                                          _lib.stream_ptr())
    _lib.check(rc, 'hla_orien_window_bwd')
    return d_grd


def triplet_loss(corr, gt_u, gt_v, args, mpp, loss, accumulate):
    B, Ny, Nx = corr.shape
    rc = _lib.load().hla_g2s_corr_triplet_loss(_lib.ptr(corr), _lib.ptr(gt_u), gt_u.stride(0), _lib.ptr(gt_v), gt_v.stride(0),
                                               float(args.shift_range_lat), float(args.shift_range_lon), float(mpp), _lib.ptr(loss),
                                               1 if accumulate else 0, B, Ny, Nx, _lib.stream_ptr())
    _lib.check(rc, 'hla_g2s_corr_triplet_loss')


def triplet_loss_bwd(corr, gt_u, gt_v, args, mpp, g_loss):
    B, Ny, Nx = corr.shape
    d_corr = torch.empty_like(corr)
    rc = _lib.load().hla_g2s_corr_triplet_loss_bwd(_lib.ptr(corr), _lib.ptr(gt_u), gt_u.stride(0), _lib.ptr(gt_v), gt_v.stride(0),
                                                   float(args.shift_range_lat), float(args.shift_range_lon), float(mpp),
                                                   _lib.ptr(g_loss), _lib.ptr(d_corr), B, Ny, Nx, _lib.stream_ptr())
    _lib.check(rc, 'hla_g2s_corr_triplet_loss_bwd')
    return d_corr


def _gt_column(gt, device):
    """gt_shift [B,1] (or [B]) -> the fp32 device tensor whose column 0 the loss reads (models_kitti.py:587-588)."""
    g = gt.detach().to(device=device, dtype=torch.float32)
    return g[:, 0] if g.dim() == 2 else g


def levels_forward(model, sat_feats, sat_inv, grd_feats, grd_inv, camera_k, ori_hw):
    """Every level of corr on the extractors' raw NHWC maps -> [(corr, mpp, g2s, grid, saved)]."""
    out = []
    K = camera_k.to(sat_feats[0].device)
    B = sat_feats[0].shape[0]
    if tuple(K.shape) != (B, 3, 3):
        raise ValueError(f'left_camera_k must be [B,3,3], got {tuple(K.shape)}')
    for l in range(len(sat_feats)):
        A, Cn = sat_feats[l].shape[1], sat_feats[l].shape[3]
        if Cn not in CHANNELS:
            raise _lib.HlaError(f'corr: unsupported channel count {Cn} at level {l} (supported: {CHANNELS})')
        plan = crop_plan(A, l, model.args)
        grid = zero_pose_grid(K, A, grd_feats[l].shape[1:3], ori_hw, plan)
        g2s = sample_crop(grd_feats[l], grid)
        corr, saved = corr_forward(sat_feats[l], g2s, sat_inv[l], grd_inv[l])
        out.append((corr, level_mpp(l), g2s, grid, saved))
    return out


def _loss_of(model, lv, gt_u, gt_v, device):
    loss = torch.empty(1, device=device, dtype=torch.float32)
    for l, (corr, mpp, *_) in enumerate(lv):
        triplet_loss(corr, gt_u, gt_v, model.args, mpp, loss, l > 0)
    return loss


def predict(corr, mpp):
    """models_kitti.py:563-565: the argmin shift of one level -> (pred_u [B], pred_v [B]) in metres."""
    B, Ny, Nx = corr.shape
    idx = torch.argmin(corr.reshape(B, -1), dim=-1)
    pred_u = (idx % Nx - Nx / 2) * mpp
    pred_v = -(torch.div(idx, Nx, rounding_mode='floor') - Ny / 2) * mpp
    return pred_u, pred_v


class _G2sCorrFn(torch.autograd.Function):
    """mode='train': the triplet loss (a scalar) whose backward is the HIP backward pass through both extractors."""

    @staticmethod
    def forward(ctx, model, names, sat_map, grd_img, camera_k, gt_u, gt_v, *params):
        sat_feats, sat_inv, grd_feats, _, grd_inv, cs, cg = extract_saved(model, sat_map, grd_img, False)
        lv = levels_forward(model, sat_feats, sat_inv, grd_feats, grd_inv, camera_k, tuple(grd_img.shape[-2:]))
        loss = _loss_of(model, lv, gt_u, gt_v, sat_map.device)
        model.last_corr = [c.detach() for c, *_ in lv]
        ctx.model, ctx.names, ctx.gt = model, names, (gt_u, gt_v)
        ctx.state = (sat_feats, sat_inv, grd_feats, grd_inv, cs, cg, lv)
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        model = ctx.model
        sat_feats, sat_inv, grd_feats, grd_inv, cs, cg, lv = take_state(ctx, 'corr forward')
        g = g_loss.float().reshape(1).contiguous()
        d_sat, d_grd = [], []
        for l, (corr, mpp, g2s, grid, saved) in enumerate(lv):
            d_corr = triplet_loss_bwd(corr, *ctx.gt, model.args, mpp, g)
            ds, dg = corr_backward(sat_feats[l], g2s, sat_inv[l], grd_inv[l], saved, d_corr)
            d_sat.append(ds)
            d_grd.append(sample_crop_bwd(grd_feats[l], grid, dg))
        grads = extractor_grads(model, cs, cg, d_sat, d_grd)
        return (None,) * 7 + tuple(grads.get(n) for n in ctx.names)


@_lib.on_device(lambda model, sat_map, *a, **k: sat_map)
def corr(model, sat_map, grd_img, camera_k, gt_shift_u, gt_shift_v, mode):
    if model.proj == 'nn':
        # the reference would run the geometric projection on the FOLDED maps of VGGUnet_G2S: defined, plainly unintended
        raise NotImplementedError("corr with proj='nn': the reference projects the folded ground maps geometrically there; refused")
    model._check_images(sat_map, grd_img)
    dev = sat_map.device
    ori_hw = tuple(grd_img.shape[-2:])
    train = mode == 'train'
    if train:
        if gt_shift_u is None or gt_shift_v is None:
            raise ValueError("corr(mode='train') needs gt_shift_u and gt_shift_v")
        gt_u, gt_v = _gt_column(gt_shift_u, dev), _gt_column(gt_shift_v, dev)
        under = grad_params(model)
        if under:
            return _G2sCorrFn.apply(model, under[0], sat_map, grd_img, camera_k, gt_u, gt_v, *under[1])
    with torch.no_grad():
        sat_feats, sat_inv, grd_feats, _, grd_inv = model._features(sat_map, grd_img, False)
        lv = levels_forward(model, sat_feats, sat_inv, grd_feats, grd_inv, camera_k, ori_hw)
        model.last_corr = [c for c, *_ in lv]
        if train:
            return _loss_of(model, lv, gt_u, gt_v, dev)[0]
        return predict(lv[-1][0], lv[-1][1])                # the LAST level's shift, metres (models_kitti.py:563-576)
