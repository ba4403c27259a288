"""Shared host logic of the satellite->ground LM localisation models.

Mirrors the orchestration of ``models_kitti.py:1141-1316`` / ``models_ford.py:652-866`` but the whole
N_iters x levels loop is one C-ABI call (``hla_s2g_lm_solve``): no per-step host sync, no per-step
H2D copies (the reference does ~60 syncs and ~100 small uploads per forward).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib, _pose, utils
from ._autograd import _side_stream, extract_saved, extractor_grads, grad_params, take_state
from ._pose import _poses_arg, eligible_cost, pose_grid  # noqa: F401  (the models, drivers and tests import these names here)
from .VGG import VGGUnet, vgg_forward_nhwc, vgg_forward_pair_nhwc, vgg_fixup_nhwc, promised_cols

KITTI_K = [[582.9802, 0.0, 496.2420], [0.0, 482.7076, 125.0034], [0.0, 0.0, 1.0]]      # models_kitti.py:657-660
FORD_K_FL = [945.391406, 0.0, 855.502825, 0.0, 945.668274, 566.372868, 0.0, 0.0, 1.0]   # models_ford.py:116
FORD_H_FL, FORD_W_FL = 860, 1656                                                        # models_ford.py:119-120


_FEAT_DTYPES = {torch.float32: _lib.HLA_F32, torch.bfloat16: _lib.HLA_BF16, torch.float16: _lib.HLA_F16}

# Phase marks of a training step (bench.py's train.step_breakdown): when set, ``PHASE_HOOK(name)`` is called on the host right
# after the launches of phase ``name`` were enqueued on the CURRENT stream (the hook records an event there).  None: no cost.
PHASE_HOOK = None


def _phase(name: str):
    h = PHASE_HOOK
    if h is not None:
        h(name)


def _camera_rays(K_ori, grd_H, grd_W, ori_H, ori_W):
    """``xyz_w`` of grd_img2cam (models_kitti.py:657-673): K^-1 [u,v,1] with K rescaled to the level grid, [1,h,w,3] fp32."""
    K = torch.tensor(K_ori, dtype=torch.float32).reshape(1, 3, 3)
    Ks = K.clone()
    Ks[:, :1, :] = K[:, :1, :] * grd_W / ori_W
    Ks[:, 1:2, :] = K[:, 1:2, :] * grd_H / ori_H
    Kinv = torch.inverse(Ks)
    v, u = torch.meshgrid(torch.arange(0, grd_H, dtype=torch.float32),
                          torch.arange(0, grd_W, dtype=torch.float32), indexing='ij')
    uv1 = torch.stack([u, v, torch.ones_like(u)], dim=-1).unsqueeze(0)
    return torch.sum(Kinv[:, None, None, :, :] * uv1[:, :, :, None, :], dim=-1)


def ray_table(K_ori, grd_H, grd_W, ori_H, ori_W):
    """The camera rays of the pixel grid, ``xyz_grds[l][2]`` of the reference (models_kitti.py:673,682): what args.use_gt_depth
    multiplies by the depth map (741-745).  Same fp32 op sequence, bit-identical.  Returns [h,w,3] fp32 (CPU)."""
    return _camera_rays(K_ori, grd_H, grd_W, ori_H, ori_W)[0].contiguous()


def ground_plane_table(K_ori, grd_H, grd_W, ori_H, ori_W):
    """Back-project the pixel grid onto the ground plane y = camera height
    (models_kitti.py:655-682 / models_ford.py:132-155).  Same fp32 op sequence as the reference so the
    table is bit-identical.  Returns xyz [h,w,3] fp32 (CPU)."""
    xyz_w = _camera_rays(K_ori, grd_H, grd_W, ori_H, ori_W)
    y = xyz_w[..., 1:2]
    w = utils.Camera_height / torch.where(torch.abs(y) > utils.EPS, y, utils.EPS * torch.ones_like(y))
    return (xyz_w * w)[0].contiguous()


def nearest_indices(n_in: int, n_out: int):
    """Source index of every destination index under ``F.interpolate(x, size=n_out)`` in its default (nearest) mode along one
    axis: torch's own rule, min(floor(dst * fp32(n_in / n_out)), n_in - 1) with the product in fp32.  int32 [n_out] (CPU)."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(src, n_in - 1).astype(np.int32))


def polar_plane_table(grd_H, grd_W):
    """proj='polar' (grd_img2cam_polar, models_kitti.py:684-698 / models_ford.py:157-171): the level map is read as a polar fan on
    the ground plane -- column u is a bearing over 45 degrees, row v a range that falls from 30 m at the top row to 30/grd_H m at
    the bottom one.  Same fp32 op sequence as the reference so the table is bit-identical.  Every point has z > 0, so the
    reference's all-ones mask is what the kernels' z > 0 test gives.  Returns xyz [h,w,3] fp32 (CPU)."""
    v, u = torch.meshgrid(torch.arange(0, grd_H, dtype=torch.float32),
                          torch.arange(0, grd_W, dtype=torch.float32), indexing='ij')
    theta = u / grd_W * np.pi / 4
    radius = (1 - v / grd_H) * 30
    z = radius * torch.cos(np.pi / 4 - theta)
    x = -radius * torch.sin(np.pi / 4 - theta)
    y = utils.Camera_height * torch.ones_like(z)
    return torch.stack([x, y, z], dim=-1).contiguous()


def ford_K_network_input():
    """models_ford.py:116-130: K_FL rescaled from the 860x1656 sensor to the 256x1024 network input."""
    K = torch.tensor(FORD_K_FL, dtype=torch.float32).reshape(3, 3)
    out = torch.zeros_like(K)
    out[0] = K[0] / FORD_W_FL * 1024
    out[1] = K[1] / FORD_H_FL * 256
    out[2] = K[2]
    return out.tolist()


def _loss_tensor_ops(shift_lats, shift_lons, thetas, gt_shift_lat, gt_shift_lon, gt_theta, coe_shift_lat, coe_shift_lon, coe_theta):
    """models_ford.py:1073-1092 as the reference writes it (tensor ops on whatever device / dtype the inputs have)."""
    d_lat = torch.abs(shift_lats - gt_shift_lat[:, None, None]).mean(dim=0)
    d_lon = torch.abs(shift_lons - gt_shift_lon[:, None, None]).mean(dim=0)
    d_th = torch.abs(thetas - gt_theta[:, None, None]).mean(dim=0)
    losses = coe_shift_lat * d_lat + coe_shift_lon * d_lon + coe_theta * d_th
    return (losses.mean(), losses[0] - losses[-1], d_lat[0] - d_lat[-1], d_lon[0] - d_lon[-1], d_th[0] - d_th[-1],
            losses[-1], d_lat[-1], d_lon[-1], d_th[-1])


def _pose_loss_args(xs, gts, coes):
    a = _lib.PoseLossArgs()
    B, N, L = xs[0].shape
    for k in range(3):
        a.x[k], a.gt[k], a.gt_stride[k], a.coe[k] = xs[k].data_ptr(), gts[k].data_ptr(), gts[k].stride(0), float(coes[k])
        for j in range(3):
            a.x_stride[k][j] = xs[k].stride(j)
    a.B, a.N, a.L = B, N, L
    a.gt_dtype = _lib.HLA_POSE_LOSS_F64 if gts[0].dtype == torch.float64 else _lib.HLA_POSE_LOSS_F32
    return a


class _PoseLossFn(torch.autograd.Function):
    """loss_func method 0 as ONE launch forward (hla_pose_loss) and ONE backward (hla_pose_loss_bwd) instead of ~25 + ~40
    element-wise launches of 5-7 us each (0.55 ms of a training step between the LM loop and its backward).
    xs = (trace [B,N,L,3],) with ``cols`` = the trace columns holding (lat, lon, theta), or three [B,N,L] tensors (cols None)."""

    @staticmethod
    def forward(ctx, cols, coes, gt_lat, gt_lon, gt_th, *xs):
        views = [xs[0][..., c] for c in cols] if cols is not None else list(xs)
        gts = (gt_lat, gt_lon, gt_th)
        L = views[0].shape[2]
        out = torch.empty(1 + 8 * L, dtype=gt_lat.dtype, device=views[0].device)
        args = _pose_loss_args(views, gts, coes)
        _lib.check(_lib.load().hla_pose_loss(C.byref(args), _lib.ptr(out), _lib.stream_ptr()), 'hla_pose_loss')
        ctx.save_for_backward(*xs, *gts)
        ctx.cols, ctx.coes = cols, coes
        ctx.set_materialize_grads(False)
        return (out[0],) + tuple(out[1 + j * L:1 + (j + 1) * L] for j in range(8))

    @staticmethod
    @torch.autograd.function.once_differentiable       # (the gradient is piecewise constant: its own derivative is zero a.e.)
    def backward(ctx, *g):
        cols, saved = ctx.cols, ctx.saved_tensors
        nx = 1 if cols is not None else 3
        xs, gts = saved[:nx], saved[nx:]
        if cols is not None:
            d = torch.empty_like(xs[0]) if xs[0].shape[-1] == 3 and len(set(cols)) == 3 else torch.zeros_like(xs[0])
            views, dviews, grads = [xs[0][..., c] for c in cols], [d[..., c] for c in cols], (d,)
        else:
            views = list(xs)
            grads = tuple(torch.empty(x.shape, dtype=torch.float32, device=x.device) for x in xs)
            dviews = list(grads)
        args = _pose_loss_args(views, gts, ctx.coes)
        vp = C.c_void_p
        gp, keep = (vp * 9)(), []
        for j, t in enumerate(g):
            if t is not None:
                t = t.to(gts[0].dtype).contiguous()
                keep.append(t)
                gp[j] = t.data_ptr()
        dp = (vp * 3)(*[v.data_ptr() for v in dviews])
        ds = ((C.c_longlong * 3) * 3)()
        for k in range(3):
            for j in range(3):
                ds[k][j] = dviews[k].stride(j)
        _lib.check(_lib.load().hla_pose_loss_bwd(C.byref(args), gp, dp, C.byref(ds), _lib.stream_ptr()), 'hla_pose_loss_bwd')
        return (None,) * 5 + grads


def _pose_loss(cols, xs, gts, coes):
    """The nine tensors of loss_func method 0.  Device fp32 poses with fp32 / fp64 ground truth on the same device go through
    libhla (one launch each way; the batch means are summed in fp64 and rounded once, i.e. within 1 ulp of torch's fp32
    reduction, then the reference's operation order in its result type; a second backward through the gradient raises
    (once_differentiable) where the reference would return zeros); anything else (CPU tensors, other dtypes, ground truth that requires grad, tensor-valued coefficients) is evaluated
    with the reference's own tensor ops on the tensors' device -- that is the reference function, not a fallback of a kernel."""
    views = [xs[0][..., c] for c in cols] if cols is not None else list(xs)
    fused = (all(isinstance(c, (int, float)) for c in coes)
             and all(v.is_cuda and v.dtype == torch.float32 and v.dim() == 3 and v.shape == views[0].shape for v in views)
             and all(t.is_cuda and t.device == views[0].device and t.dtype == gts[0].dtype and t.dim() == 1
                     and t.shape[0] == views[0].shape[0] and not t.requires_grad for t in gts)
             and gts[0].dtype in (torch.float32, torch.float64) and 0 < views[0].shape[1] * views[0].shape[2] <= 512
             and views[0].shape[0] > 0)
    if not fused:
        return _loss_tensor_ops(*views, *gts, *coes)
    with torch.cuda.device(views[0].device):
        return _PoseLossFn.apply(cols, tuple(float(c) for c in coes), *gts, *xs)


def loss_func(loss_method, ref_feat_list, pred_feat_dict, gt_feat_dict, shift_lats, shift_lons, thetas,
              gt_shift_lat, gt_shift_lon, gt_theta, pred_uv_dict, gt_uv_dict,
              coe_shift_lat=100, coe_shift_lon=100, coe_theta=100, coe_L1=100, coe_L2=100, coe_L3=100, coe_L4=100):
    """models_ford.py:1041-1093, method 0 (the only valid one per models_ford.py:1040).  Same positional
    signature as the reference; the feature/uv dictionaries are unused by method 0 and may be None."""
    if loss_method != 0:
        raise NotImplementedError('only loss_method=0 is supported (the reference marks 1-3 as failed trials)')
    out = _pose_loss(None, (shift_lats, shift_lons, thetas), (gt_shift_lat, gt_shift_lon, gt_theta),
                     (coe_shift_lat, coe_shift_lon, coe_theta))
    return (*out, None, None, None, None)


def loss_from_trace(loss_method, trace, cols, gt_shift_lat, gt_shift_lon, gt_theta, coe_shift_lat, coe_shift_lon, coe_theta):
    """``loss_func`` for the models' own call (models_kitti.py:1304-1310, models_ford.py:848-854): the three pose tensors are
    columns ``cols`` = (lat, lon, theta) of the LM loop's trace [B,N,L,3], so the gradient comes back as ONE d_trace tensor
    instead of three column gradients that autograd would scatter into zero-filled copies and add up."""
    if loss_method != 0:
        raise NotImplementedError('only loss_method=0 is supported (the reference marks 1-3 as failed trials)')
    out = _pose_loss(tuple(cols), (trace,), (gt_shift_lat, gt_shift_lon, gt_theta), (coe_shift_lat, coe_shift_lon, coe_theta))
    return (*out, None, None, None, None)


class S2GPBase(nn.Module):
    ford = False

    # Fields of ``args`` beyond the reference's argparse namespace (all optional; a reference Namespace works unchanged):
    #   precision          'fp32' (default, exact-fp32 MFMA) | 'fp16x3' | 'bf16' | 'fp16'                       DESIGN.md 3.8
    #   lm_feat16          1: bf16 / fp16 inference hands the LM loop fp16 feature maps; 0: fp32 maps           DESIGN.md 3.3
    #   ground_crop        1: mode='test' skips the ground-image rows (and, layer by layer, the feature rows) that cannot
    #                      reach the rows the LM loop reads; 0: whole image.  Computed rows are bit-identical  DESIGN.md 3.5
    #   sat_reach_crop     1: mode='test' (KITTI, proj='geo', LM, level 3, no confidence heads, no depth map, not 'fp16x3') skips the
    #                      left columns of the satellite maps that no pose inside the configured shift / rotation range reads;
    #                      a sample whose loop leaves that reach is detected on the device and recomputed exactly, without a
    #                      host synchronisation.  0: whole maps                                                  DESIGN.md 3.5
    #   fixup_one_launch   1: that recomputation's extractor half is one launch with a workgroup per sample (bf16 / fp16); 0: ten
    #                      gated conv launches and a gated inv_norm.  Same bits (A/B and tests)                   DESIGN.md 3.5
    #   train_ground_crop  0; 1: the same for training (changes the returned confidence maps above the crop)   DESIGN.md 3.5
    #   bwd_trim           1: the backward skips rows / tiles whose gradient is exactly zero; 0: dense walk     DESIGN.md 6
    #   bwd_two_streams    1: the two extractors' backward passes run on two streams (single-GPU training)       DESIGN.md 6
    #   wgrad_two_phase    0; 1: weight gradients on the two-phase kernels (A/B and tests: HLA_VGG_BWD_WGRAD_TWO_PHASE); 2: only conv0's
    #                      from a stored map of conv2's data gradient instead of inside that kernel's epilogue (..._WGRAD0_UNFUSED)
    #   strict_errors      0; 1: reproduce jacobian.py:172's AssertionError (costs a host sync per forward)     DESIGN.md 1
    #   small_batch_two_streams  4: inference batches up to this size run the two extractors on two streams        DESIGN.md 5
    #   pair_extractor_launches  1: inference batches above small_batch_two_streams run every conv layer of the two extractors as
    #                      ONE launch of two segments (hla_vgg_forward_pair); 0: the two forwards back to back.  Same bits    DESIGN.md 3.1
    #   deterministic_backward  0; 1: lm_bwd_accum accumulates d(loss)/d(sat map) in a fixed order instead of with fp32 atomics:
    #                      the same batch twice gives bitwise equal parameter gradients
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.level = args.level
        self.N_iters = args.N_iters
        self.using_weight = args.using_weight
        self.loss_method = args.loss_method
        # level 2 = [x18, x21] with the H/4 and H/2 ground-plane tables: coherent in the Ford class only (models_ford.py:59-65;
        # the KITTI class pairs x18 with its H/8 table at level 2 and fails on the shapes)
        if args.level not in ((2, 3, 4) if self.ford else (3, 4)):
            raise NotImplementedError('args.level must be 3 (x15, x18, x21) or 4 (+ x24)' +
                                      (', or 2 (x18, x21)' if self.ford else "; the reference's KITTI model is shape-inconsistent at level 2"))
        # proj='polar' (train_kitti.py:472, train_ford.py:396): the polar table of `polar_plane_table` and the WHOLE level map in
        # every step (models_kitti.py:1194-1205, models_ford.py:738-749) instead of its bottom half.  The reference takes that
        # branch for any string other than 'geo' (an `else`); here anything else is an error.
        proj = getattr(args, 'proj', 'geo')
        if proj not in ('geo', 'polar'):
            raise NotImplementedError(f"{type(self).__name__}: proj must be 'geo' or 'polar', got {proj!r} (the reference runs its "
                                      "polar branch for any other string, 'nn' and 'CrossAttn' included: that accident is not copied)")
        self.polar = proj == 'polar'
        if self.polar and self.ford and args.level == 2:
            # models_ford.py:59-65 builds the level-2 tables with grd_img2cam whatever args.proj is, and the loop then reads the
            # whole map through the ground-plane table (rows above the horizon masked by z > 0)
            raise NotImplementedError("LM_S2GP_Ford(level=2, proj='polar'): the reference pairs the whole-map loop with the "
                                      "ground-plane tables there; that combination is not built (use level 3 or 4)")
        opt = getattr(args, 'Optimizer', 'LM')
        # KITTI (models_kitti.py:1176-1283): LM, SGD, ADAM, NN.  Ford (models_ford.py:751-788): LM, GN, NN and an SGD_update
        # (609-634, a sign-of-residual step of 0.001) that indexes its [B,3] update with three subscripts and raises as shipped.
        allowed = ('LM', 'GN') if self.ford else ('LM', 'SGD', 'ADAM')
        if opt not in allowed:
            raise NotImplementedError(f"{type(self).__name__}: Optimizer must be one of {allowed} ('NN' needs the NNrefine "
                                      f"network: out of scope; the reference's Ford SGD_update raises as shipped)")
        if getattr(args, 'estimate_depth', 0):
            raise NotImplementedError('estimate_depth (Ford height heads, VGG.py:85-118) is out of scope')
        # args.use_gt_depth only takes effect when a gt_depth tensor is passed to forward (models_kitti.py:741); neither
        # driver ever passes one (train_kitti.py:357,49).  LM_S2GP.forward then lifts every ground pixel by its depth (`_depth_arg`)
        precision = getattr(args, 'precision', 'fp32')
        self.SatFeatureNet = VGGUnet(self.level, precision=precision)
        self.GrdFeatureNet = VGGUnet(self.level, precision=precision)
        if self.ford or args.rotation_range > 0:
            self.damping = nn.Parameter(torch.zeros(size=(1, 3), dtype=torch.float32))
        else:
            self.damping = nn.Parameter(torch.zeros(size=(), dtype=torch.float32))
        self.meters_per_pixel = [utils.get_meter_per_pixel() * (2 ** (3 - l)) for l in range(4)]
        self._tables = {}
        self._reach = {}
        self._ray_tables = {}
        self._depth_idx = {}
        self.last_trace = None       # [B, N_iters, Level, 3] (shift_u, shift_v, theta) of the last forward
        self.last_normal_eq = None
        self.last_keep = None
        self.keep_normal_eq = False
        self.keep_features = False   # True: localise keeps (sat_feats, sat_inv, grd_feats, grd_inv) of its inference path in last_features
        self.last_features = None
        self.last_reach_flag = None  # int32 [B] of the last localise that ran with args.sat_reach_crop in effect (1: recomputed), else None
        self.last_search = None      # forward_search: cost, sums, start_index, traces, final_cost, best of the last call
        self.last_score_loss = None  # score_loss: costs [B,K+1] and sums [B,K+1,8] per scored level of the last call (entry 0: the true pose)
        self._view_tables = {}
        self.last_views = None       # lm_solve_views: dict(trace, normal_eq [steps,B,16], view_sums [steps,B,V,16]) of the last call

    # -- geometry tables ---------------------------------------------------------------------
    def xyz_tables(self, grd_H: int, grd_W: int, device):
        """Per-level ground-plane tables.  K is given for a 256x1024 image (models_kitti.py:657-667); the
        table of level l is grd_img2cam(H/2^(3-l), W/2^(3-l), 256, 1024): identical to the reference for its
        own 256x1024 input, and the same camera resampled for any other input size (BASELINE config 5).
        proj='polar': grd_img2cam_polar(H/2^(3-l), W/2^(3-l)) instead (models_kitti.py:626-633, models_ford.py:54-58)."""
        key = (grd_H, grd_W, str(device))
        if key not in self._tables:
            K = ford_K_network_input() if self.ford else KITTI_K
            hw = [(grd_H / 2 ** (3 - l), grd_W / 2 ** (3 - l)) for l in range(4)]
            self._tables[key] = [(polar_plane_table(h, w) if self.polar else ground_plane_table(K, h, w, 256, 1024)).to(device)
                                 for h, w in hw]
        # level 2 (Ford, models_ford.py:59-65): grd_img2cam(H / 2^(2 - l)) for l = 0, 1 = the H/4 and H/2 tables
        return self._tables[key][1:3] if self.level == 2 else self._tables[key]

    def ray_tables(self, grd_H: int, grd_W: int, device):
        """Per-level camera-ray tables (``ray_table``), sized and cached like ``xyz_tables``: what a depth map lifts."""
        key = (grd_H, grd_W, str(device))
        if key not in self._ray_tables:
            K = ford_K_network_input() if self.ford else KITTI_K
            self._ray_tables[key] = [ray_table(K, grd_H / 2 ** (3 - l), grd_W / 2 ** (3 - l), 256, 1024).to(device) for l in range(4)]
        return self._ray_tables[key][1:3] if self.level == 2 else self._ray_tables[key]

    def depth_indices(self, h: int, w: int, dH: int, dW: int, device):
        """(rows int32 [h], columns int32 [w]) on the device: ``nearest_indices`` of a [dH,dW] depth map for an h x w level map."""
        key = (h, w, dH, dW, str(device))
        if key not in self._depth_idx:
            self._depth_idx[key] = (nearest_indices(dH, h).to(device), nearest_indices(dW, w).to(device))
        return self._depth_idx[key]

    def _depth_arg(self, gt_depth, B: int, device):
        """The depth map as the kernels read it -- ``.to(device).float().contiguous()`` [B,dH,dW] -- or None."""
        if gt_depth is None:
            return None
        if self.polar:
            # the reference indexes xyz_grds[l][2], which grd_img2cam_polar does not return: IndexError there
            raise NotImplementedError("proj='polar' with a depth map: the reference's polar tables have no camera rays to lift "
                                      "(models_kitti.py:742 raises IndexError)")
        if gt_depth.dim() != 3 or gt_depth.shape[0] != B or gt_depth.shape[1] < 1 or gt_depth.shape[2] < 1:
            raise ValueError(f'gt_depth must be [B,dH,dW] with B = {B}, got {tuple(gt_depth.shape)}')
        return gt_depth.detach().to(device).float().contiguous()

    def sat_first_col32(self, A: int, grd_H: int, grd_W: int) -> int:
        """args.sat_reach_crop: the tile columns (32 px at H/4) the satellite extractor may skip for an A x A image and this
        ground geometry -- ``sat_reach`` over the configured pose range, walked back through the extractor.  Geometry only:
        cached per (A, ground size, ranges).  0 where the trim does not apply."""
        a = self.args
        if self.ford or self.polar or self.level != 3 or A % 8:
            return 0
        key = (A, grd_H, grd_W, float(a.shift_range_lat), float(a.shift_range_lon), float(a.rotation_range))
        if key not in self._reach:
            tables = [t.cpu() for t in self.xyz_tables(grd_H, grd_W, 'cpu')]
            mpp = [utils.get_meter_per_pixel() * utils.get_process_satmap_sidelength() / (A >> (3 - l)) for l in range(3)]
            cols = sat_reach(tables[:3], [A >> (3 - l) for l in range(3)], mpp, key[3], key[4], key[5])
            self._reach[key] = first_col32_of_reach(cols, A)
        return self._reach[key]

    def _levels(self, maps):
        """The extractor always computes x15, x18, x21 (x15 feeds the decoder); level 2 uses the last two (VGG.py:183-184,198-199)."""
        if self.level != 2 or maps is None:
            return maps
        return maps[1:]

    # -- LM options -> C structs -------------------------------------------------------------
    def _config(self, n_levels: int, level_first: int) -> _lib.S2GConfig:
        a = self.args
        cfg = _lib.S2GConfig()
        cfg.ford = 1 if self.ford else 0
        cfg.n_levels, cfg.n_iters, cfg.level_first = n_levels, self.N_iters, 1 if level_first else 0
        cfg.optimizer = {'LM': 0, 'SGD': 1, 'ADAM': 2, 'GN': 3}[getattr(a, 'Optimizer', 'LM')]
        # SGD_update / ADAM_update (models_kitti.py:1056-1116) read neither the confidence maps nor args.dropout;
        # GN_update (models_ford.py:534-598) reads the confidence maps but not args.dropout
        cfg.using_weight = 1 if (self.using_weight and cfg.optimizer in (0, 3)) else 0
        cfg.use_hessian = 1 if getattr(a, 'use_hessian', 0) else 0
        if self.ford:
            cfg.dof = 3
        elif a.rotation_range == 0:
            cfg.dof = 2
        elif a.shift_range_lat == 0 and a.shift_range_lon == 0:
            cfg.dof = 1
        else:
            cfg.dof = 3
        cfg.shift_range_lat, cfg.shift_range_lon = float(a.shift_range_lat), float(a.shift_range_lon)
        cfg.rotation_range = float(a.rotation_range)
        cfg.beta1, cfg.beta2 = float(getattr(a, 'beta1', 0.9)), float(getattr(a, 'beta2', 0.999))
        if getattr(a, 'train_damping', 0):
            lam = (10.0 ** (-6 + torch.sigmoid(self.damping.detach().double()) * 11.0)).reshape(-1).tolist()
        else:
            lam = [float(a.damping)] * 3
        lam = (lam + lam + lam)[:3]
        if not self.ford and cfg.dof == 1 and getattr(a, 'train_damping', 0):
            lam = [lam[0]] * 3
        for i in range(3):
            cfg.damping[i] = lam[i]
        return cfg

    def _draw_reinit(self, n_steps: int, B: int, device):
        """Reproduce the reference's global-RNG consumption: two Uniform(-1,1).sample([B,1]) draws per
        LM step (models_kitti.py:1028-1029), in step order, from torch's CPU generator."""
        return draw_reinit(n_steps, B, device)

    def _draw_dropout(self, lv, level_first, device):
        """args.dropout > 0 (models_kitti.py:968-974, models_ford.py:406-412): every LM step keeps a random half of the
        pixels, ``np.random.permutation(H*W)[:H*W//2]`` from numpy's GLOBAL generator, one draw per step in execution
        order.  Returns a uint8 [steps, stride] keep mask on the device (or None)."""
        if not getattr(self.args, 'dropout', 0) or getattr(self.args, 'Optimizer', 'LM') != 'LM':
            return None
        L, N = len(lv), self.N_iters
        order = [l for l in range(L) for _ in range(N)] if level_first else [l for _ in range(N) for l in range(L)]
        npix = [(lv[l].h - lv[l].row0) * lv[l].w for l in range(L)]
        keep = np.zeros((len(order), max(npix)), np.uint8)
        for k, l in enumerate(order):
            inds = np.random.permutation(np.arange(npix[l]))[: npix[l] // 2]
            keep[k, inds] = 1
        return torch.from_numpy(keep).to(device)

    def _lm_structs(self, sat_feats, grd_feats, grd_confs, grd_hw, extra, level_first, sat_inv_norm, grd_inv_norm, depth=None):
        """``depth``: the result of ``_depth_arg`` (the caller keeps it alive over the call), or None."""
        dev = sat_feats[0].device
        L = len(sat_feats)
        tables = self.xyz_tables(grd_hw[0], grd_hw[1], dev)
        rays = self.ray_tables(grd_hw[0], grd_hw[1], dev) if depth is not None else None
        cfg = self._config(L, level_first)
        lv = (_lib.S2GLevel * L)()
        for l in range(L):
            s, g = sat_feats[l], grd_feats[l]
            A, w, Cn = s.shape[1], g.shape[2], g.shape[3]
            h = tables[l].shape[0]                     # the level's full map height; g may hold only its last rows
            row0 = 0 if self.polar else h // 2         # first row the loop reads: the bottom half for 'geo', the whole map for 'polar'
            skip = h - g.shape[1]
            if not (s.shape[2] == A and s.shape[3] == Cn and tuple(tables[l].shape) == (h, w, 3) and 0 <= skip <= row0
                    and g.shape[0] == s.shape[0] and s.is_contiguous() and g.is_contiguous()
                    and s.dtype == g.dtype and s.dtype in _FEAT_DTYPES):
                raise ValueError(f'level {l}: inconsistent feature maps sat {tuple(s.shape)} / grd {tuple(g.shape)} '
                                 f'for a {tuple(grd_hw)} ground image')
            lv[l].sat_feat, lv[l].grd_feat, lv[l].feat_dtype = s.data_ptr(), g.data_ptr(), _FEAT_DTYPES[s.dtype]
            lv[l].grd_conf = grd_confs[l].data_ptr() if (self.using_weight and grd_confs[l] is not None) else 0
            lv[l].xyz = tables[l].data_ptr()
            if depth is not None:      # per-sample points ray * depth, mask depth != -1 (models_kitti.py:741-748; include/hla.h)
                ri, ci = self.depth_indices(h, w, depth.shape[1], depth.shape[2], dev)
                lv[l].ray, lv[l].depth, lv[l].depth_row, lv[l].depth_col = rays[l].data_ptr(), depth.data_ptr(), ri.data_ptr(), ci.data_ptr()
                lv[l].depth_h, lv[l].depth_w = depth.shape[1], depth.shape[2]
            lv[l].sat_inv_norm = sat_inv_norm[l].data_ptr() if sat_inv_norm is not None else 0
            lv[l].grd_inv_norm = grd_inv_norm[l].data_ptr() if grd_inv_norm is not None else 0
            lv[l].A, lv[l].h, lv[l].w, lv[l].C, lv[l].row0, lv[l].grd_row_skip = A, h, w, Cn, row0, skip
            if self.ford:
                lv[l].meter_per_pixel = float(extra['side_m']) / A          # models_ford.py:230
                lv[l].centre = float(A // 2)                                # models_ford.py:231
            else:
                lv[l].meter_per_pixel = utils.get_meter_per_pixel() * utils.get_process_satmap_sidelength() / A
                lv[l].centre = A / 2.0                                      # models_kitti.py:765-767
        R_FL = extra['R_FL'].to(dev).float().contiguous() if self.ford else None
        T_FL = extra['T_FL'].to(dev).float().contiguous() if self.ford else None
        return cfg, lv, R_FL, T_FL

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def lm_solve(self, sat_feats, grd_feats, grd_confs, grd_hw, extra=None, level_first=0, init_pose=None,
                 sat_inv_norm=None, grd_inv_norm=None, keep_normal_eq=None, gt_depth=None, reach=None):
        """sat_feats/grd_feats: NHWC fp32 lists (L2-normalised, or raw together with their [L,B] fp64
        inverse norms); returns trace [B,N_iters,L,3] = (shift_u, shift_v, theta).
        ``gt_depth`` [B,dH,dW] (any size): every ground pixel is lifted to ray * depth instead of onto the ground plane, with
        the mask depth != -1 (models_kitti.py:741-748); None: the flat-ground tables.
        ``reach`` = (col0, fixup): the satellite maps are only valid from column ``col0[l]`` on (a forward made with first_col32).
        The loop then reports, per sample, whether it read left of that (``self.last_reach_flag``); ``fixup(flag)`` must complete the
        maps of the flagged samples (``vgg_fixup_nhwc``), and the loop runs again for those samples alone, with the same random
        draws.  A flagged sample ends with the trace and normal equations of the loop on whole maps, bit for bit; nothing waits
        for the host."""
        lib = _lib.load()
        dev = sat_feats[0].device
        B, L = sat_feats[0].shape[0], len(sat_feats)
        depth = self._depth_arg(gt_depth, B, dev)
        cfg, lv, R_FL, T_FL = self._lm_structs(sat_feats, grd_feats, grd_confs, grd_hw, extra, level_first,
                                               sat_inv_norm, grd_inv_norm, depth)
        steps = L * self.N_iters
        reinit = (self.ford or cfg.dof == 3) and cfg.optimizer in (0, 3)
        rand_uv = self._draw_reinit(steps, B, dev) if reinit else None
        self.last_keep = self._draw_dropout(lv, level_first, dev)
        if self.last_keep is not None:
            cfg.keep, cfg.keep_stride = self.last_keep.data_ptr(), self.last_keep.shape[1]
        trace = torch.empty(B, self.N_iters, L, 3, device=dev, dtype=torch.float32)
        strict = bool(getattr(self.args, 'strict_errors', 0))
        want_neq = strict or cfg.optimizer == 3 or (self.keep_normal_eq if keep_normal_eq is None else keep_normal_eq)
        cfg.count_in_view = 1 if strict else 0
        neq = torch.empty(steps, B, 16, device=dev, dtype=torch.float64) if want_neq else None
        nbytes = lib.hla_s2g_workspace_bytes(C.byref(cfg), lv, B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p0 = init_pose.to(dev).float().contiguous() if init_pose is not None else None
        flag = None
        if reach is not None:
            flag = torch.empty(B, dtype=torch.int32, device=dev)       # (cleared by the loop's init launch)
            cfg.reach_mode, cfg.reach_flag = 1, flag.data_ptr()
            for l in range(L):
                cfg.reach_col0[l] = int(reach[0][l])
        rc = lib.hla_s2g_lm_solve(C.byref(cfg), lv, _lib.ptr(R_FL), _lib.ptr(T_FL), _lib.ptr(p0), _lib.ptr(rand_uv),
                                  _lib.ptr(trace), _lib.ptr(neq), _lib.ptr(ws), nbytes, B, _lib.stream_ptr())
        _lib.check(rc, 'hla_s2g_lm_solve')
        if reach is not None:
            # enqueued on every call, gated per sample on the device: the maps' missing columns, then the whole loop again
            reach[1](flag)
            cfg.reach_mode = 2
            rc = lib.hla_s2g_lm_solve(C.byref(cfg), lv, _lib.ptr(R_FL), _lib.ptr(T_FL), _lib.ptr(p0), _lib.ptr(rand_uv),
                                      _lib.ptr(trace), _lib.ptr(neq), _lib.ptr(ws), nbytes, B, _lib.stream_ptr())
            _lib.check(rc, 'hla_s2g_lm_solve (reach fallback)')
        self.last_reach_flag = flag
        # Error behaviour of the reference, which costs a host sync and is therefore only reproduced (a) under the ablation
        # flags that can make H + damping*D exactly singular (use_hessian / zero damping) and (b) when strict error checking
        # is asked for (args.strict_errors).  With the default flags the forward has no host sync;
        # a step whose pixels all fall outside the satellite map then leaves the pose unchanged (J = 0, r = -g).
        risky = cfg.optimizer == 3 or (cfg.optimizer == 0 and (cfg.use_hessian or min(cfg.damping[i] for i in range(3)) <= 0.0))
        if risky or strict:
            raise_like_reference(trace, neq[:, :, 14] if strict else None, level_first,
                                 gn_norm2=neq[:, :, 0] if cfg.optimizer == 3 else None)
        # a detached alias: under autograd `trace` becomes the Function's output (grad_fn -> ctx), and ctx/model must not hold it
        # or every step's ctx (8.5 GB of saved workspaces at B = 32) lives in a reference cycle until the cyclic GC runs
        self.last_trace, self.last_normal_eq = trace.detach(), neq
        return trace

    def view_tables(self, grd_H: int, grd_W: int, camera_k, device):
        """Per level, the V ground-plane tables of ``forward_views`` back to back, [V,h,w,3]: ``ground_plane_table`` with view v's
        ``camera_k[v]`` (given for a 256x1024 image, the convention of ``ford_K_network_input``), sized like ``xyz_tables``;
        proj='polar': V copies of the polar table (it has no intrinsics).  Cached per (size, matrices, device)."""
        K = torch.as_tensor(camera_k, dtype=torch.float32).cpu().reshape(-1, 3, 3)
        key = (grd_H, grd_W, K.numpy().tobytes(), str(device))
        if key not in self._view_tables:
            hw = [(grd_H / 2 ** (3 - l), grd_W / 2 ** (3 - l)) for l in range(4)]
            self._view_tables[key] = [torch.stack([polar_plane_table(h, w) if self.polar else ground_plane_table(k.tolist(), h, w, 256, 1024)
                                                   for k in K]).contiguous().to(device) for h, w in hw]
        return self._view_tables[key][1:3] if self.level == 2 else self._view_tables[key]

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def lm_solve_views(self, sat_feats, grd_feats, grd_confs, grd_hw, V, R, T, side_m, tables=None, level_first=0, init_pose=None,
                       sat_inv_norm=None, grd_inv_norm=None):
        """The LM loop over V views of one body pose (``hla_s2g_lm_solve_views``, include/hla.h): the analogue of ``lm_solve``
        for the Ford chain.  One step is the reference's LM_update on the UNION of the views' pixels: every view's normal-equation
        sums are formed at the common pose with that view's table and (R_v, T_v), added in view order, and solved once.
        sat_feats[l] [B,A,A,C]; grd_feats[l] [B*V,h',w,C] and grd_confs[l] [B*V,h',w] with view v of sample b at index b*V+v;
        R [B,V,3,3], T [B,V,3] camera -> body; ``tables[l]`` [V,h,w,3] (default: this model's ground-plane table for every view);
        sat_inv_norm[l] [B], grd_inv_norm[l] [B*V] fp64 with raw maps.  The re-initialisation draws are ``draw_reinit(steps, B)``:
        the RNG consumption of ``forward`` with batch B.  A view that lies outside the satellite map still contributes the
        norm of its ground features, as out-of-map pixels of a single view do.  Inference only: no backward exists.
        Returns the trace [B,N_iters,L,3]; ``last_views`` keeps dict(trace, normal_eq, view_sums)."""
        if not self.ford:
            raise NotImplementedError('lm_solve_views: the Ford chain only (the KITTI chain has no camera extrinsics)')
        if getattr(self.args, 'dropout', 0):
            raise NotImplementedError('lm_solve_views with args.dropout: the dropout loop is not built for several views')
        lib = _lib.load()
        dev = sat_feats[0].device
        B, L, V = sat_feats[0].shape[0], len(sat_feats), int(V)
        if tables is None:
            tables = [t[None].expand(V, -1, -1, -1).contiguous() for t in self.xyz_tables(grd_hw[0], grd_hw[1], dev)]
        R = R.to(dev).float().contiguous()
        T = T.to(dev).float().contiguous()
        if tuple(R.shape) != (B, V, 3, 3) or tuple(T.shape) != (B, V, 3):
            raise ValueError(f'R must be [B,V,3,3] and T [B,V,3] with B = {B}, V = {V}, got {tuple(R.shape)} and {tuple(T.shape)}')
        cfg = self._config(L, level_first)
        lv = (_lib.S2GLevel * L)()
        for l in range(L):
            s, g, tab = sat_feats[l], grd_feats[l], tables[l]
            A, w, Cn = s.shape[1], g.shape[2], g.shape[3]
            h = tab.shape[1]
            row0 = 0 if self.polar else h // 2
            skip = h - g.shape[1]
            if not (s.shape[2] == A and s.shape[3] == Cn and tuple(tab.shape) == (V, h, w, 3) and tab.dtype == torch.float32
                    and tab.is_contiguous() and tab.device == dev and 0 <= skip <= row0 and g.shape[0] == B * V
                    and s.is_contiguous() and g.is_contiguous() and s.dtype == g.dtype and s.dtype in _FEAT_DTYPES):
                raise ValueError(f'level {l}: inconsistent maps sat {tuple(s.shape)} / grd {tuple(g.shape)} / tables {tuple(tab.shape)} '
                                 f'for B = {B}, V = {V} and a {tuple(grd_hw)} ground image')
            lv[l].sat_feat, lv[l].grd_feat, lv[l].feat_dtype = s.data_ptr(), g.data_ptr(), _FEAT_DTYPES[s.dtype]
            lv[l].grd_conf = grd_confs[l].data_ptr() if (self.using_weight and grd_confs[l] is not None) else 0
            lv[l].xyz = tab.data_ptr()
            lv[l].sat_inv_norm = sat_inv_norm[l].data_ptr() if sat_inv_norm is not None else 0
            lv[l].grd_inv_norm = grd_inv_norm[l].data_ptr() if grd_inv_norm is not None else 0
            lv[l].A, lv[l].h, lv[l].w, lv[l].C, lv[l].row0, lv[l].grd_row_skip = A, h, w, Cn, row0, skip
            lv[l].meter_per_pixel = float(side_m) / A               # models_ford.py:230
            lv[l].centre = float(A // 2)                            # models_ford.py:231
        steps = L * self.N_iters
        rand_uv = self._draw_reinit(steps, B, dev)
        trace = torch.empty(B, self.N_iters, L, 3, device=dev, dtype=torch.float32)
        neq = torch.empty(steps, B, 16, device=dev, dtype=torch.float64)
        sums = torch.empty(steps, B, V, 16, device=dev, dtype=torch.float64)
        nbytes = lib.hla_s2g_views_workspace_bytes(C.byref(cfg), lv, B, V)
        if nbytes == 0:
            raise _lib.HlaError(f'hla_s2g_views_workspace_bytes: {lib.hla_last_error().decode()}')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p0 = init_pose.to(dev).float().contiguous() if init_pose is not None else None
        rc = lib.hla_s2g_lm_solve_views(C.byref(cfg), lv, V, _lib.ptr(R), _lib.ptr(T), _lib.ptr(p0), _lib.ptr(rand_uv), _lib.ptr(trace),
                                        _lib.ptr(neq), _lib.ptr(sums), _lib.ptr(ws), nbytes, B, _lib.stream_ptr())
        _lib.check(rc, 'hla_s2g_lm_solve_views')
        # the reference's singular-matrix error under the flags that can cause it, as in lm_solve (costs a host sync there only)
        risky = cfg.optimizer == 3 or (cfg.optimizer == 0 and (cfg.use_hessian or min(cfg.damping[i] for i in range(3)) <= 0.0))
        if risky:
            raise_like_reference(trace, None, level_first, gn_norm2=neq[:, :, 0] if cfg.optimizer == 3 else None)
        self.last_views = dict(trace=trace, normal_eq=neq, view_sums=sums)
        return trace

    def lm_grad_buffers(self, sat_feats, grd_feats, grd_confs, row0s, row_skips, grd_first_row8=0, overwrite=True, deterministic=False):
        """The buffers ``hla_s2g_lm_solve_bwd`` accumulates into, cleared where they have to be by ONE launch (``hla_zero_fill``) on
        the current stream: (d_sat[l], d_grd[l], d_conf[l] or None, d_lambda[4]).
        * d_sat: zero-filled (the scatter adds); with ``deterministic`` not at all (the closing pass writes every element).
        * d_grd: the loop only touches rows row0_l.. (h_l/2; 0 for proj='polar', where nothing is left to clear) and WRITES them
          on each level's first visit (cfg.grd_grad_overwrite): no zero-fill and no read-modify-write of half a map there.  What still has to be zero is what the consumer reads above
          them: with hla_vgg_backward(first_row8 = f) two rows (it never reads d_grd[l] above row f * 2^l - 2), else the top half.
        * d_conf: zero-filled (added to).  d_lambda: written by the call."""
        L = len(sat_feats)
        regions = []
        d_sat = [torch.empty_like(t) for t in sat_feats]
        if not deterministic:
            regions += [(d, d.numel() * 4, d.numel() * 4, 1) for d in d_sat]
        d_grd = []
        for l, t in enumerate(grd_feats):
            d = torch.empty_like(t)
            lo, hi = (max(0, (grd_first_row8 << l) - 2) if grd_first_row8 else 0), row0s[l] - row_skips[l]
            if not overwrite:
                hi = t.shape[1]
            if hi > lo:
                row = t.shape[2] * t.shape[3] * 4
                regions.append((d.data_ptr() + lo * row, (hi - lo) * row, t.shape[1] * row, t.shape[0]))
            d_grd.append(d)
        d_conf = [torch.empty_like(grd_confs[l]) if (self.using_weight and grd_confs[l] is not None) else None for l in range(L)]
        regions += [(d, d.numel() * 4, d.numel() * 4, 1) for d in d_conf if d is not None]
        d_lambda = torch.empty(4, device=sat_feats[0].device, dtype=torch.float64)
        keep = d_sat + d_grd                      # (the regions of d_grd are raw pointers into tensors that are alive here)
        for k0 in range(0, len(regions), 16):
            _lib.zero_fill(regions[k0:k0 + 16])
        del keep
        return d_sat, d_grd, d_conf, d_lambda

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def lm_backward(self, sat_feats, grd_feats, grd_confs, grd_hw, trace, normal_eq, d_trace, extra=None, level_first=0,
                    init_pose=None, sat_inv_norm=None, grd_inv_norm=None, keep=None, grd_first_row8=0, overwrite=True, gt_depth=None):
        """Backward of ``lm_solve``: d(loss)/d(trace) [B,N,L,3] -> (d_sat[l], d_grd[l], d_conf[l] or None, d_lambda[4]).
        ``keep``: the forward's dropout mask (``self.last_keep``), if args.dropout.
        Map gradients are NHWC fp32 and taken w.r.t. the L2-normalised maps (inv_norm * stored map).
        ``args.deterministic_backward``: hla_s2g_config.deterministic.  ``gt_depth``: the forward's depth map (no gradient
        is taken w.r.t. it)."""
        lib = _lib.load()
        dev = sat_feats[0].device
        B, L = sat_feats[0].shape[0], len(sat_feats)
        depth = self._depth_arg(gt_depth, B, dev)
        cfg, lv, R_FL, T_FL = self._lm_structs(sat_feats, grd_feats, grd_confs, grd_hw, extra, level_first,
                                               sat_inv_norm, grd_inv_norm, depth)
        if keep is not None:
            cfg.keep, cfg.keep_stride = keep.data_ptr(), keep.shape[1]
        det = bool(getattr(self.args, 'deterministic_backward', 0))
        cfg.deterministic = 1 if det else 0                  # (sizes the workspace: 8 B per satellite-map element)
        cfg.grd_grad_overwrite = 1 if overwrite else 0       # (0: zero-filled buffers, every step adds -- kept for callers of the C ABI)
        d_sat, d_grd, d_conf, d_lambda = self.lm_grad_buffers(sat_feats, grd_feats, grd_confs, [lv[l].row0 for l in range(L)],
                                                              [lv[l].grd_row_skip for l in range(L)], grd_first_row8, overwrite, det)
        gr = (_lib.S2GLevelGrad * L)()
        for l in range(L):
            gr[l].d_sat_feat, gr[l].d_grd_feat = d_sat[l].data_ptr(), d_grd[l].data_ptr()
            gr[l].d_grd_conf = d_conf[l].data_ptr() if d_conf[l] is not None else 0
        dtr = d_trace.to(dev).float().contiguous()
        nbytes = lib.hla_s2g_bwd_workspace_bytes(C.byref(cfg), lv, B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p0 = init_pose.to(dev).float().contiguous() if init_pose is not None else None
        # deterministic mode: 40 bits below the first visit's bound, 2^10 of room for the later visits' bounds; a batch that needs more
        # (the check costs a host sync per step: the price of this opt-in mode) is run again with 30 bits / 2^20 -- for given inputs
        # the same attempts fail and succeed, so the result stays a function of the inputs alone.  (The second attempt accumulates
        # into fresh fixed-point sums -- the call clears them -- and, with grd_grad_overwrite, rewrites d_grd; d_conf is re-cleared.)
        for attempt, bits in enumerate((1, 30) if det else (0,)):
            cfg.deterministic = bits
            if attempt:
                for t in d_conf:
                    if t is not None:
                        t.zero_()
                if not overwrite:
                    for t in d_grd:
                        t.zero_()
            rc = lib.hla_s2g_lm_solve_bwd(C.byref(cfg), lv, gr, _lib.ptr(R_FL), _lib.ptr(T_FL), _lib.ptr(p0), _lib.ptr(trace),
                                          _lib.ptr(normal_eq), _lib.ptr(dtr), _lib.ptr(d_lambda), _lib.ptr(ws), nbytes, B,
                                          _lib.stream_ptr())
            _lib.check(rc, 'hla_s2g_lm_solve_bwd')
            if not det or float(d_lambda[3]) == 0.0:
                break
        else:
            raise RuntimeError(f'deterministic_backward: the fixed-point range of d(loss)/d(sat map) was exceeded in {int(d_lambda[3])} '
                               '(step, sample) pairs even with 2^20 of head room -- the adjoints of the LM chain grow by more than that '
                               'from its last step to an earlier one; the result is not valid (run without args.deterministic_backward)')
        return d_sat, d_grd, d_conf, d_lambda[:3]

    def _score_structs(self, sat_feats, grd_feats, grd_confs, grd_hw, extra, sat_inv_norm, grd_inv_norm):
        """``_pose.score_poses``' structs: (cfg, lv, (R_FL, T_FL)), what ``hla_s2g_pose_score[_bwd]`` take."""
        cfg, lv, R_FL, T_FL = self._lm_structs(sat_feats, grd_feats, grd_confs, grd_hw, extra, 0, sat_inv_norm, grd_inv_norm)
        return cfg, lv, (R_FL, T_FL)

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def score_poses(self, sat_feats, grd_feats, grd_confs, grd_hw, poses, level, extra=None, sat_inv_norm=None, grd_inv_norm=None):
        """The LM objective at given poses, on feature maps extracted once (``hla_s2g_pose_score``, include/hla.h): low-level like
        ``lm_solve``, with the same map arguments.  ``poses`` [K,3] (shared by the samples) or [B,K,3], (shift_u, shift_v, theta)
        in normalised units; ``level`` indexes the lists.  Returns (cost [B,K] fp32, sums [B,K,8] fp64): sum s^2, sum g^2,
        sum s g, the same three weighted, pixels in view, pixels with the ground mask."""
        structs = lambda: self._score_structs(sat_feats, grd_feats, grd_confs, grd_hw, extra, sat_inv_norm, grd_inv_norm)
        return _pose.score_poses('hla_s2g_pose_score', structs, sat_feats, poses, level)

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def score_poses_bwd(self, sat_feats, grd_feats, grd_confs, grd_hw, poses, level, sums, d_cost, extra=None, sat_inv_norm=None,
                        grd_inv_norm=None):
        """Backward of ``score_poses`` (``hla_s2g_pose_score_bwd``, include/hla.h): the same map arguments (fp32 maps), ``sums``
        [B,K,8] of the forward and ``d_cost`` [B,K] -> (d_sat [B,A,A,C], d_grd like grd_feats[level], d_conf [B,h,w] or None) of
        level ``level``, fp32 NHWC, with respect to the L2-normalised maps -- what ``vgg_backward_nhwc(..., scale_invariant=True)``
        takes.  All three are written by the call (ground rows above row0 are zero); poses get no gradient.  d_grd and d_conf are
        bitwise reproducible, d_sat (fp32 atomics) is not."""
        structs = lambda: self._score_structs(sat_feats, grd_feats, grd_confs, grd_hw, extra, sat_inv_norm, grd_inv_norm)
        return _pose.score_poses_bwd('hla_s2g_pose_score_bwd', structs, sat_feats, grd_feats, grd_confs, poses, level, sums, d_cost)

    def _score_checks(self, what, sat_map, grd_img):
        if getattr(self.args, 'dropout', 0):
            raise NotImplementedError(f'{what} with args.dropout: a pose is scored on every pixel, the dropout loop on a random '
                                      'half -- their objectives differ')
        if self.level != 3:
            raise NotImplementedError(f'{what} is built for args.level = 3 (x15, x18, x21), got level {self.level}')
        _lib.image_pair(sat_map, grd_img, self.damping)

    @_lib.on_device(lambda self, sat_map, *a, **k: sat_map)
    def score_candidates(self, sat_map, grd_img, poses, levels=None, extra=None):
        """The LM objective at ``poses`` ([K,3] or [B,K,3], normalised units) on the maps of the two images, differentiable with
        respect to both extractors' parameters (not the poses): -> (costs, sums), a list of [B,K] fp32 costs and a list of
        [B,K,8] fp64 sums, one entry per level in ``levels`` (default: every level).  Under autograd it is ONE autograd.Function:
        both extractors with their activations saved, ``hla_s2g_pose_score`` per scored level; its backward runs
        ``hla_s2g_pose_score_bwd`` per scored level and ``hla_vgg_backward`` for both extractors.  ``sums`` carry no gradient.
        Without grad it is the inference extractors plus ``score_poses``.  ``extra``: the Ford dict (R_FL, T_FL, side_m)."""
        self._score_checks('score_candidates', sat_map, grd_img)
        cand = _poses_arg(poses, sat_map.shape[0]).to(sat_map.device).contiguous()
        lvls = _pose.levels_arg(levels, self.level)
        under = grad_params(self)
        if under:
            out = _ScoreFn.apply(self, under[0], sat_map, grd_img, cand, lvls, extra, *under[1])
            return list(out[:len(lvls)]), list(out[len(lvls):])
        with torch.no_grad():
            sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = self._features(sat_map, grd_img, bool(self.using_weight), False)
            res = [self.score_poses(sat_feats, grd_feats, grd_confs, grd_img.shape[-2:], cand, l, extra, sat_inv, grd_inv) for l in lvls]
        return [r[0] for r in res], [r[1] for r in res]

    def _score_loss(self, sat_map, grd_img, extra, candidates, gt_pose, levels, min_in_view):
        """``score_loss`` of both models.  gt_pose: (shift_u, shift_v, heading), each [B] or [B,1], normalised units."""
        self._score_checks('score_loss', sat_map, grd_img)
        poses = _pose.true_pose_first(gt_pose, candidates, sat_map.shape[0], sat_map.device)
        costs, sums = self.score_candidates(sat_map, grd_img, poses, levels, extra)
        return _pose.score_loss_tail(self, costs, sums, min_in_view)

    @_lib.on_device(lambda self, sat_map, *a, **k: sat_map)
    def _search(self, sat_map, grd_img, extra, candidates, top_m, score_level, min_in_view, level_first):
        """``forward_search`` of both models: extract once, score the candidates at ``score_level``, run the LM loop from the
        ``top_m`` best eligible ones, keep the final pose that scores best at the finest level.  -> trace-ordered pose [B,3]."""
        if getattr(self.args, 'dropout', 0):
            raise NotImplementedError('forward_search with args.dropout: a pose is scored on every pixel, the dropout loop on a '
                                      'random half -- their objectives differ')
        _lib.image_pair(sat_map, grd_img, self.damping)
        cand, M = _pose.search_candidates(candidates, top_m, sat_map)
        with torch.no_grad():
            sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = self._features(sat_map, grd_img, bool(self.using_weight), False)
            hw = grd_img.shape[-2:]
            score = lambda poses, level: self.score_poses(sat_feats, grd_feats, grd_confs, hw, poses, level, extra, sat_inv, grd_inv)
            solve = lambda p0: self.lm_solve(sat_feats, grd_feats, grd_confs, hw, extra, level_first, p0, sat_inv, grd_inv)
            return _pose.search(self, cand, M, score, solve, score_level, len(sat_feats) - 1, min_in_view)

    def _features(self, sat_map, grd_img, want_conf, return_confs, sat_c32=0, col_state=None, pair=True):
        """Both extractors of the inference path: (sat_feats, sat_inv, grd_feats, grd_confs, grd_inv), normalisation deferred.
        ``sat_c32`` / ``col_state``: the satellite extractor's first_col32 and the dict that receives its fix-up state.
        ``pair`` = False: never the paired launches (``forward_views``: the two batches differ in size)."""
        # Reduced-precision inference modes: the LM loop reads fp16 feature maps (written saturating by the three feature
        # layers' epilogues; also in bf16 mode: bf16's 8 significand bits moved the worst golden seed's pose 23x, fp16's 11
        # move it 1.6x).  With the gather loop written on channel PAIRS (lm_solve.hip) the accumulate kernels are VALU-bound on
        # 16-bit maps and 30 % faster than on fp32 ones: +7 % pairs/s.  args.lm_feat16 = 0 keeps fp32 maps; the fp32-class modes
        # and every training path always do.
        f16 = (self.SatFeatureNet.precision in ('bf16', 'fp16') and self.level == 3 and bool(getattr(self.args, 'lm_feat16', 1)))
        # A small batch cannot fill the chip (a B = 1 conv launch is 8-256 workgroups on 256 CUs) and the forward is then a chain of
        # ~70 dependent launches: the two extractors are independent, so the satellite branch runs on a side stream next to the
        # ground branch's (B <= args.small_batch_two_streams, default 4: B = 1 0.700 -> 0.615 ms, B = 4 1.195 -> 1.122; at B = 32, where both are dense, the same split measured
        # 2 % slower: DESIGN 3.1).
        small = sat_map.shape[0] <= int(getattr(self.args, 'small_batch_two_streams', 4))
        # (only LM_update renormalises the ground features; SGD / ADAM see the whole-map L2_norm scale, so they need every row;
        #  proj='polar' reads every row of every map, so there the flag is inert)
        dead_ok = (not return_confs and self.level == 3 and getattr(self.args, 'Optimizer', 'LM') == 'LM'
                   and bool(getattr(self.args, 'ground_crop', 1)) and not self.polar)
        skip = dead_ground_rows(grd_img.shape[-2]) if dead_ok else 0
        # a row window, passed as it lies in memory (hla_vgg_forward's x_plane): no copy
        grd_in = grd_img[:, :, skip:, :] if skip else grd_img
        # ... and inside the extractor every layer only computes the rows the LM loop's rows depend on
        f8 = ((grd_img.shape[-2] // 8) // 2 - skip // 8) if dead_ok else 0
        f8 = f8 if f8 >= 4 else 0
        # A batch that fills the chip: the two extractors are the same ten launches on two images, and each of them runs for both
        # as ONE launch (args.pair_extractor_launches, default 1; the library falls back to the two forwards where it cannot pair)
        if (pair and not small and not want_conf and self.level != 4 and bool(getattr(self.args, 'pair_extractor_launches', 1))
                and self.GrdFeatureNet.precision == self.SatFeatureNet.precision):
            (sat_feats, sat_inv), (grd_feats, grd_inv), _ = vgg_forward_pair_nhwc(
                (self.SatFeatureNet, self.GrdFeatureNet), (sat_map, grd_in), first_row8=(0, f8), feat16=f16,
                first_col32=(sat_c32, 0), col_state=col_state)
            L = self._levels
            return L(sat_feats), L(sat_inv), L(grd_feats), L([None] * 3), L(grd_inv)
        if small:
            cur = torch.cuda.current_stream()
            side = _side_stream(sat_map.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                sat_feats, _, sat_inv = vgg_forward_nhwc(self.SatFeatureNet, sat_map, want_conf=False, defer_norm=True, feat16=f16,
                                                         first_col32=sat_c32, col_state=col_state)
            sat_map.record_stream(side)
        else:
            sat_feats, _, sat_inv = vgg_forward_nhwc(self.SatFeatureNet, sat_map, want_conf=False, defer_norm=True, feat16=f16,
                                                     first_col32=sat_c32, col_state=col_state)
        grd_feats, grd_confs, grd_inv = vgg_forward_nhwc(self.GrdFeatureNet, grd_in, want_conf=want_conf, defer_norm=True,
                                                         first_row8=f8, feat16=f16)
        if small:
            cur.wait_stream(side)
            for t in list(sat_feats) + [sat_inv]:        # allocated on the side stream, consumed (LM loop) on this one
                t.record_stream(cur)
            if col_state:                                # (so is the workspace the fix-up pass works in)
                col_state['ws'].record_stream(cur)
        L = self._levels
        return L(sat_feats), L(sat_inv), L(grd_feats), L(grd_confs), L(grd_inv)

    @_lib.on_device(lambda self, sat_map, *a, **k: sat_map)
    def localise(self, sat_map, grd_img, want_conf, extra, level_first, init_pose, return_confs=True, gt_depth=None):
        """Both feature pyramids (normalisation deferred into the LM sums) + the whole LM loop.
        return_confs=False (mode='test'): the caller does not need full-size confidence maps, so the ground extractor
        only runs on the image rows that can influence the bottom half of its maps (``dead_ground_rows``).
        Under autograd (training) the same kernels run inside one autograd.Function whose backward is the HIP
        backward pass (hla_s2g_lm_solve_bwd + hla_vgg_backward for both extractors).
        ``gt_depth`` [B,dH,dW] or None: ``lm_solve``'s depth map; it gets no gradient."""
        _lib.image_pair(sat_map, grd_img, self.damping, gpu=False)
        gt_depth = self._depth_arg(gt_depth, sat_map.shape[0], sat_map.device)      # (checked before the extractors run)
        if self.polar and self.ford and level_first:
            # models_ford.py:935-950: the level-first loop has no proj branch and reads the bottom half of the polar table
            raise NotImplementedError("LM_S2GP_Ford(proj='polar') with level_first=1: the reference's level-first loop reads only "
                                      "the bottom half of the polar maps (it has no proj branch); that combination is not built")
        under = grad_params(self)
        if under:
            out = _LocaliseFn.apply(self, under[0], sat_map, grd_img, want_conf, extra, level_first, init_pose, gt_depth, *under[1])
            return out[0], list(out[1:]) if want_conf else [None] * self.level
        # (the two dense extractor passes on two streams measured 2 % slower than back to back: DESIGN.md 3.1)
        # args.sat_reach_crop: the satellite extractor skips the columns the configured pose range cannot reach;
        # the loop checks that on the device, and a sample that left the reach is completed and run again (lm_solve, `reach`)
        a = self.args
        c32 = 0
        if (bool(getattr(a, 'sat_reach_crop', 1)) and not return_confs and not want_conf and gt_depth is None and not self.ford
                and not self.polar and self.level == 3 and getattr(a, 'Optimizer', 'LM') == 'LM'
                and not getattr(a, 'strict_errors', 0) and self.SatFeatureNet.precision != 'fp16x3'):
            c32 = self.sat_first_col32(sat_map.shape[-1], grd_img.shape[-2], grd_img.shape[-1])
        state = {} if c32 else None
        sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = self._features(sat_map, grd_img, want_conf, return_confs, c32, state)
        reach = (promised_cols(c32), lambda flag: vgg_fixup_nhwc(state, flag, bool(getattr(a, 'fixup_one_launch', 1)))) if c32 else None
        trace = self.lm_solve(sat_feats, grd_feats, grd_confs, grd_img.shape[-2:], extra, level_first, init_pose,
                              sat_inv, grd_inv, gt_depth=gt_depth, reach=reach)
        if self.keep_features:
            self.last_features = (sat_feats, sat_inv, grd_feats, grd_inv)
        return trace, grd_confs


def draw_reinit(n_steps: int, B: int, device):
    """[n_steps, 2, B] = the (rand_u, rand_v) of every LM step, VALUE FOR VALUE what the reference's 2 * n_steps calls
    ``Uniform(-1, 1).sample([B, 1])`` (models_kitti.py:1028-1029) draw from torch's global CPU generator, which is left in the
    same state: ``Uniform.sample`` is ``low + torch.rand(shape) * (high - low)`` and the CPU generator fills a tensor serially,
    so one ``torch.rand`` of all of them is the same stream (``tests/test_host_logic_cpu.py`` pins both).  One call, one pinned
    staging buffer from the caching host allocator and one asynchronous copy, instead of 30 draws + a blocking upload per forward."""
    r = torch.rand(n_steps, 2, B).mul_(2.0).add_(-1.0)         # -1 + rand * 2, the same two fp32 roundings
    if torch.device(device).type == 'cuda':
        return r.pin_memory().to(device, non_blocking=True)
    return r.to(device)


def raise_like_reference(trace, in_view, level_first, gn_norm2=None):
    """The reference's two run-time errors, in the order it would hit them.  trace [B,N,L,3]; in_view [steps,B] (or None):
    per sample, the number of pixels sampled inside the map in that step (any quantity that is zero iff there is none).
    * jacobian.py:172 `assert mask.sum() > 0` fires in step k when NO pixel of the whole batch is in view (checked before
      that step's solve);
    * torch.inverse (models_kitti.py:372,1012, models_ford.py:446,578) raises in step k when any sample's matrix is exactly
      singular -- here that step's pose comes out non-finite.
    Steps after the first failure are garbage (the reference never ran them), so only the first one counts.
    gn_norm2 [steps,B] (GN_update only): ||s||^2.  GN_update divides by the UNclamped norm (models_ford.py:551-553), so a
    sample with no pixel in the compared rows gets a NaN matrix, which torch.inverse accepts: its pose is NaN from then on
    without an error of its own (the next step's assertion fires if the rest of the batch is out of view as well)."""
    B, N, L, _ = trace.shape
    steps = N * L
    tr = (trace.permute(0, 2, 1, 3) if level_first else trace).reshape(B, steps, 3)
    bad = ~torch.isfinite(tr).all(-1)                                # [B,steps]
    if gn_norm2 is not None:
        first = torch.where(bad.any(1), bad.float().argmax(1), torch.full((B,), steps - 1, device=bad.device))
        poisoned = bad.any(1) & (gn_norm2.t().gather(1, first[:, None])[:, 0] == 0)
        bad = bad & ~poisoned[:, None]
    bad = bad.any(0)                                                 # [steps]
    k_s = int(torch.nonzero(bad)[0]) if bool(bad.any()) else steps
    k_a = steps
    if in_view is not None:
        empty = in_view.sum(1) == 0
        k_a = int(torch.nonzero(empty)[0]) if bool(empty.any()) else steps
    if k_a < steps and k_a <= k_s:
        raise AssertionError(f'grid_sample: no pixel of the batch is sampled inside the map in LM step {k_a} (jacobian.py:172)')
    if k_s < steps:
        raise RuntimeError(f'linalg.inv: the normal matrix of LM step {k_s} is singular '
                           '(use_hessian / zero damping / Gauss-Newton with no Jacobian support in one pose component)')


def sat_reach(tables, sizes, mpp, shift_range_lat, shift_range_lon, rotation_range, n: int = 5):
    """Per level, the smallest satellite-map column any bilinear tap of the LM loop reads while the pose stays inside the box
    [-1, 1]^3 of (shift_u, shift_v, theta): floor(u) over the ground pixels the loop reads (rows h/2.., ground mask z > 0) that
    land inside the map, with the coefficient formulas of the loop itself (csrc/lm_common.h, lm_coefficients: KITTI chain), in
    fp64, over an n x n x n lattice of the box (n odd: corners and centres included).  ``tables[l]`` [h,w,3] ground-plane table,
    ``sizes[l]`` = A_l, ``mpp[l]`` metres per pixel.  A level nothing of which is in view gets A_l.  The camera looks towards +u,
    so the left part of every map is out of reach; the result only decides how often the exact fallback runs."""
    axis = np.linspace(-1.0, 1.0, n)
    out = []
    for t, A, m in zip(tables, sizes, mpp):
        t = np.asarray(t, dtype=np.float64)
        h = t.shape[0]
        P = t[h // 2:].reshape(-1, 3)
        P = P[P[:, 2] > 0]
        X, Z = P[:, 0], P[:, 2]
        best, im, ctr = float(A), 1.0 / m, A / 2.0
        for th in axis:
            ang = th * rotation_range / 180.0 * np.pi
            c, s = np.cos(ang), np.sin(ang)
            for su in axis * shift_range_lon:
                for sv in axis * shift_range_lat:
                    u = s * im * X + c * im * Z + (c * su - s * sv) * im + ctr
                    v = c * im * X - s * im * Z + (-c * sv - s * su) * im + ctr
                    ok = (u >= 0) & (u <= A - 1) & (v >= 0) & (v <= A - 1)
                    if ok.any():
                        best = min(best, float(np.floor(u[ok].min())))
        out.append(int(best))
    return out


def reach_walk(p0: int, p1: int, p2: int) -> dict:
    """First column each map / layer of VGGUnet.forward has to hold when the loop reads x15 / x18 / x21 from columns p0 / p1 / p2
    on (the column twin of ``dead_ground_rows``' walk): a 3x3 conv needs one more column of its input, a 2x up-sampling halves,
    a 2x2 pool doubles.  Keys: maps 'x3', 'x8', 'x15', 'x18', 'x21'; layers by their own output resolution."""
    x18 = min(p1, (p2 - 2) >> 1)              # dec2.1 [p2-1..] reads up(x18) from p2-2
    x15 = min(p0, (x18 - 2) >> 1)             # dec1.1 [x18-1..] reads up(x15) from x18-2
    x8 = min(2 * x15 - 3, x18 - 2)            # conv10 [2 x15 - 2..]; dec1.1's skip input
    x3 = min(2 * x8 - 2, p2 - 2)              # conv5 [2 x8 - 1..]; dec2.1's skip input
    return {'x21': p2, 'dec2.1': p2 - 1, 'x18': x18, 'dec1.1': x18 - 1, 'x15': x15, 'conv14': 2 * x15, 'conv12': 2 * x15 - 1,
            'conv10': 2 * x15 - 2, 'x8': x8, 'conv7': 2 * x8, 'conv5': 2 * x8 - 1, 'x3': x3, 'conv2': 2 * x3}


# columns per H/4 tile column at each layer's own resolution: a start that keeps the pools and the 32-pixel tiles aligned
_REACH_QUANTUM = {'x21': 64, 'dec2.1': 64, 'x18': 32, 'dec1.1': 32, 'x15': 16, 'conv14': 32, 'conv12': 32, 'conv10': 32, 'x8': 32,
                  'conv7': 64, 'conv5': 64, 'x3': 64, 'conv2': 128}


def first_col32_of_reach(cols, A: int) -> int:
    """The largest c for which every layer may start at its tile column c / 2c / 4c (hla_vgg_forward's first_col32) when the loop
    reads the three maps from columns ``cols`` on; at least one column of the maps stays (128 c < A)."""
    need = reach_walk(*[int(x) for x in cols])
    c = min(max(v, 0) // _REACH_QUANTUM[k] for k, v in need.items())
    return max(0, min(c, (A - 1) // 128))


def dead_ground_rows(H: int) -> int:
    """Rows at the top of the ground image that cannot influence anything the LM loop reads.
    The loop only reads rows h_l/2.. of each ground map (models_kitti.py:1194-1199, models_ford.py:739-743) and the
    per-sample L2_norm scale cancels in LM_update's own renormalisation (models_kitti.py:982-990).  Walking the
    receptive field back through VGGUnet.forward (x21 <- dec2.3 <- dec2.1 <- {up(x18), x3}, x18 <- dec1.3 <- dec1.1 <-
    {up(x15), x8}, x15 <- pool(conv14 <- conv12 <- conv10 <- x8), x8 <- pool(conv7 <- conv5 <- x3),
    x3 <- pool(conv2 <- conv0 <- image)) the first input row needed is H/2 - 34; rounding down to a multiple of 8 keeps
    the three 2x2 pools aligned.  The rows that ARE computed are bit-identical to the full-image run."""
    return max(0, ((H // 2 - 34) // 8) * 8)


def _bwd_first_row8(model, grd_hw, x21_rows: int) -> int:
    """hla_vgg_backward's first_row8 for the ground branch: the ground maps' gradient lives in rows h_l/2.. (all the LM loop reads),
    so the backward skips the rows above its support (level 3, LM_update, args.bwd_trim)."""
    inv = getattr(model.args, 'Optimizer', 'LM') == 'LM' and not model.polar      # (proj='polar': every row carries gradient)
    f8 = (grd_hw[0] // 8) // 2 - (grd_hw[0] - x21_rows * 2) // 8
    return f8 if (inv and f8 >= 4 and model.level == 3 and bool(getattr(model.args, 'bwd_trim', 1))) else 0


class _LocaliseFn(torch.autograd.Function):
    """forward: trace [B,N,L,3] (+ the three ground confidence maps); backward: parameter gradients from HIP kernels."""

    @staticmethod
    def forward(ctx, model, names, sat_map, grd_img, want_conf, extra, level_first, init_pose, gt_depth, *params):
        sat_feats, _, sat_inv, cs = vgg_forward_nhwc(model.SatFeatureNet, sat_map, want_conf=False, defer_norm=True,
                                                     save_for_backward=True)
        _phase('fwd_sat')
        # args.train_ground_crop (an extension, default 0): train on the image rows that can reach the loss only.  The loss
        # sees the ground branch through rows h_l/2.. of its maps, so the gradient of every other row is exactly zero and the
        # rows above `dead_ground_rows` influence neither the loss nor any gradient (the L2_norm scale cancels in
        # LM_update, forward and backward).  What changes is the 14th element of the train-mode tuple: the returned confidence
        # maps are then only computed from the crop on (valid from row h_l/2, zero above the crop).
        skip = 0
        if (getattr(model.args, 'train_ground_crop', 0) and model.level == 3 and getattr(model.args, 'Optimizer', 'LM') == 'LM'
                and not model.polar):                   # (proj='polar' reads every row: no crop, whatever the flag says)
            skip = dead_ground_rows(grd_img.shape[-2])
        grd_in = grd_img[:, :, skip:, :] if skip else grd_img      # (a view: the extractor takes the window's plane stride)
        grd_feats, grd_confs, grd_inv, cg = vgg_forward_nhwc(model.GrdFeatureNet, grd_in, want_conf=want_conf,
                                                             defer_norm=True, save_for_backward=True)
        _phase('fwd_grd')
        L = model._levels
        ctx.conf0 = grd_confs[0] if (model.level == 2 and grd_confs is not None) else None      # (the head's backward needs its own map)
        sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = L(sat_feats), L(sat_inv), L(grd_feats), L(grd_confs), L(grd_inv)
        trace = model.lm_solve(sat_feats, grd_feats, grd_confs, grd_img.shape[-2:], extra, level_first, init_pose,
                               sat_inv, grd_inv, keep_normal_eq=True, gt_depth=gt_depth)
        _phase('lm_fwd')
        ctx.model, ctx.names, ctx.extra, ctx.level_first, ctx.init_pose = model, names, extra, level_first, init_pose
        ctx.gt_depth = gt_depth                         # (no gradient: kept as it is for the backward's recomputed projection)
        ctx.state = (sat_feats, grd_feats, grd_confs, tuple(grd_img.shape[-2:]), trace.detach(), model.last_normal_eq, sat_inv, grd_inv, cs, cg,
                     model.last_keep)
        out_confs = ()
        if want_conf:
            out_confs = tuple(grd_confs)
            if skip:                                    # full-size maps for the caller, zero above the crop
                out_confs = tuple(torch.nn.functional.pad(c, (0, 0, skip >> (3 - l), 0)) for l, c in enumerate(grd_confs))
            ctx.mark_non_differentiable(*out_confs)     # loss_method 0 does not read them; their LM-weight role is in backward()
        # (no zero tensors for the outputs that got no gradient: autograd would fill three [B,h,w] maps per step just to hand
        #  them to a backward that ignores them)
        ctx.set_materialize_grads(False)
        return (trace,) + out_confs

    @staticmethod
    def backward(ctx, d_trace, *unused):
        model = ctx.model
        _phase('loss')
        sat_feats, grd_feats, grd_confs, grd_hw, trace, neq, sat_inv, grd_inv, cs, cg, keep = take_state(ctx)
        if d_trace is None:         # (only the confidence maps were used downstream: they are non-differentiable outputs)
            d_trace = torch.zeros_like(trace)
        # the ground maps' gradient lives in rows h_l/2.. (all the LM loop reads): the backward skips the rows above its support
        f8 = _bwd_first_row8(model, grd_hw, grd_feats[-1].shape[1])       # (grd_feats[-1]: the H/2 map)
        d_sat, d_grd, d_conf, d_lam = model.lm_backward(sat_feats, grd_feats, grd_confs, grd_hw, trace, neq, d_trace, ctx.extra,
                                                   ctx.level_first, ctx.init_pose, sat_inv, grd_inv, keep, grd_first_row8=f8,
                                                   gt_depth=ctx.gt_depth)
        _phase('lm_bwd')
        if model.level == 2:        # x15 takes no part in the loop: its gradient (and its confidence map's) is zero
            zf = lambda cx: torch.zeros_like(cx['feats'][0], dtype=torch.float32)
            d_sat, d_grd = [zf(cs)] + list(d_sat), [zf(cg)] + list(d_grd)
            if grd_confs is not None and all(c is not None for c in d_conf):
                grd_confs, d_conf = [ctx.conf0] + list(grd_confs), [torch.zeros_like(ctx.conf0)] + list(d_conf)
        a = model.args
        use_w = model.using_weight and all(c is not None for c in d_conf)
        # LM_update renormalises both projected maps (models_kitti.py:982-990), so the loss does not depend on the per-sample
        # scale of either extractor's output: d_feat is orthogonal to feat and the L2_norm backward needs no (x . dy) pass
        # (HLA_VGG_BWD_SCALE_INVARIANT, include/hla.h).  model.bwd_stats = {}: diagnostics, filled with the satellite branch's
        # live / total backward tiles; costs a device sync.  args.wgrad_two_phase: A/B and tests (bit 0
        # HLA_VGG_BWD_WGRAD_TWO_PHASE, bit 1 ..._WGRAD0_UNFUSED).  args.bwd_two_streams = 0 keeps both branches on one stream.
        grads = extractor_grads(model, cs, cg, d_sat, d_grd, grd_confs if use_w else None, d_conf if use_w else None,
                                scale_invariant=getattr(a, 'Optimizer', 'LM') == 'LM', first_row8=f8,
                                dense=not bool(getattr(a, 'bwd_trim', 1)), wgrad_two_phase=int(getattr(a, 'wgrad_two_phase', 0)),
                                stats=getattr(model, 'bwd_stats', None), two_streams=bool(getattr(a, 'bwd_two_streams', 1)))
        if getattr(a, 'train_damping', 0):
            d = model.damping.detach().double()
            sg = torch.sigmoid(d)
            lam = 10.0 ** (-6 + sg * 11.0)
            dlam_dd = lam * np.log(10.0) * 11.0 * sg * (1 - sg)
            if d.dim() == 0:
                n = 2 if a.rotation_range == 0 else 1
                grads['damping'] = (d_lam[:n].sum() * dlam_dd).float()
            else:
                grads['damping'] = (d_lam.view(1, 3) * dlam_dd).float()
            sync = getattr(model, 'grad_sync', None)
            if sync:
                sync.finish(sync.start({'damping': grads['damping']}))
        _phase('vgg_bwd')
        return (None,) * 9 + tuple(grads.get(n) for n in ctx.names)


class _ScoreFn(torch.autograd.Function):
    """``S2GPBase.score_candidates`` under autograd.  forward: the costs [B,K] of every scored level, then their sums [B,K,8]
    (non-differentiable); backward: parameter gradients of both extractors from HIP kernels (level 3 models)."""

    @staticmethod
    def forward(ctx, model, names, sat_map, grd_img, poses, levels, extra, *params):
        sat_feats, sat_inv, grd_feats, grd_confs, grd_inv, cs, cg = extract_saved(model, sat_map, grd_img, bool(model.using_weight))
        hw = tuple(grd_img.shape[-2:])
        res = [model.score_poses(sat_feats, grd_feats, grd_confs, hw, poses, l, extra, sat_inv, grd_inv) for l in levels]
        costs, sums = tuple(r[0] for r in res), tuple(r[1] for r in res)
        ctx.model, ctx.names, ctx.extra, ctx.levels = model, names, extra, levels
        ctx.state = (sat_feats, grd_feats, grd_confs, hw, poses, sums, sat_inv, grd_inv, cs, cg)
        ctx.mark_non_differentiable(*sums)
        ctx.set_materialize_grads(False)
        return costs + sums

    @staticmethod
    def backward(ctx, *d_out):
        model = ctx.model
        sat_feats, grd_feats, grd_confs, hw, poses, sums, sat_inv, grd_inv, cs, cg = take_state(ctx, 'score_candidates call')
        bwd = lambda n, l: model.score_poses_bwd(sat_feats, grd_feats, grd_confs, hw, poses, l, sums[n], d_out[n], ctx.extra,
                                                 sat_inv, grd_inv)
        d_sat, d_grd, d_conf = _pose.score_level_grads(model, bwd, ctx.levels, d_out, sat_feats, grd_feats, grd_confs)
        # the cost renormalises both maps: every d_map is orthogonal to its map (HLA_VGG_BWD_SCALE_INVARIANT, include/hla.h), and
        # the ground maps' gradient lives in the rows the score reads (row0..: the backward skips the rows above its support)
        f8 = 0 if model.polar else _bwd_first_row8(model, hw, grd_feats[-1].shape[1])
        grads = extractor_grads(model, cs, cg, d_sat, d_grd, grd_confs if d_conf else None, d_conf, scale_invariant=True,
                                first_row8=f8, dense=not bool(getattr(model.args, 'bwd_trim', 1)),
                                wgrad_two_phase=int(getattr(model.args, 'wgrad_two_phase', 0)))
        return (None,) * 7 + tuple(grads.get(n) for n in ctx.names)

