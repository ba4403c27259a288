"""``LM_G2SP`` -- the ground->satellite variant of the KITTI model (``models_kitti.py:22-499``).  ``proj='geo'``: the
ground feature map is projected onto the satellite plane with the per-sample camera intrinsics and the LM update
runs on the satellite grid.  ``proj='nn'``: the ground branch is ``VGGUnet_G2S`` (folded maps of the satellite maps' sizes)
and the projection is the in-plane similarity warp of ``inplane_grd_to_map`` (289-332); ``left_camera_k`` is accepted and not
read.  Same module surface as the reference (ctor argument, ``forward(sat_map, grd_img_left, left_camera_k, gt_shift_u,
gt_shift_v, gt_heading, mode, ...)``, state-dict keys).  Under autograd the forward runs
inside one ``torch.autograd.Function`` whose backward is ``hla_g2s_lm_solve_bwd`` + ``hla_vgg_backward`` x 2."""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib, _pose, utils
from ._autograd import extract_saved, extractor_grads, grad_params, take_state
from ._pose import _poses_arg
from ._s2gp import loss_from_trace, raise_like_reference
from .VGG import VGGUnet, VGGUnet_G2S, vgg_forward_nhwc


class LM_G2SP(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.level = args.level
        self.N_iters = args.N_iters
        self.using_weight = args.using_weight
        self.loss_method = args.loss_method
        if args.level not in (3, 4):
            raise NotImplementedError('args.level must be 3 (x15, x18, x21) or 4 (+ x24)')
        self.proj = getattr(args, 'proj', 'geo')
        if self.proj not in ('geo', 'nn'):
            raise NotImplementedError(f"proj={self.proj!r}: 'geo' and 'nn' are built (the reference's LM_G2SP has no other projection; 'polar' is out of scope)")
        if self.proj == 'nn' and args.using_weight:
            # the reference samples the UNFOLDED c0 ([H/8,W/8]) with the folded level-0 grid (models_kitti.py:298): defined, but
            # plainly unintended -- refused rather than reproduced or silently replaced
            raise NotImplementedError('using_weight with proj=nn')
        precision = getattr(args, 'precision', 'fp32')
        self.SatFeatureNet = VGGUnet(self.level, precision=precision)
        self.GrdFeatureNet = (VGGUnet_G2S if self.proj == 'nn' else VGGUnet)(self.level, precision=precision)         # 35-38
        self.damping = nn.Parameter(args.damping * torch.ones(size=(1, 3), dtype=torch.float32))   # models_kitti.py:41
        self.meters_per_pixel = [utils.get_meter_per_pixel() * (2 ** (3 - l)) for l in range(4)]
        self.last_trace = None
        self.last_normal_eq = None
        self.keep_normal_eq = False
        self.last_corr = None        # corr: the correlation surface [B,Ny,Nx] fp32 of every level of the last call (an extension)
        self.last_score_loss = None  # score_loss: costs [B,K+1] and sums [B,K+1,8] per scored level of the last call (entry 0: the true pose)

    def _structs(self, sat_feats, grd_feats, grd_confs, camera_k, sat_inv_norm, grd_inv_norm):
        dev = sat_feats[0].device
        a = self.args
        B, L = sat_feats[0].shape[0], len(sat_feats)
        cfg = _lib.S2GConfig()
        cfg.ford, cfg.n_levels, cfg.n_iters, cfg.level_first = 0, L, self.N_iters, 0
        cfg.using_weight, cfg.use_hessian, cfg.dof = (1 if self.using_weight else 0), 0, 3
        cfg.proj = 1 if self.proj == 'nn' else 0
        cfg.shift_range_lat, cfg.shift_range_lon = float(a.shift_range_lat), float(a.shift_range_lon)
        cfg.rotation_range = float(a.rotation_range)
        lam = self.damping.detach().double().reshape(-1).tolist() if getattr(a, 'train_damping', 0) else [float(a.damping)] * 3
        for i in range(3):
            cfg.damping[i] = lam[i]
        lv = (_lib.S2GLevel * L)()
        for l in range(L):
            s, g = sat_feats[l], grd_feats[l]
            A, Cn = s.shape[1], s.shape[3]
            if not (s.shape[2] == A and g.shape[0] == B and g.shape[3] == Cn and s.is_contiguous() and g.is_contiguous()
                    and s.dtype == torch.float32 and g.dtype == torch.float32):
                raise ValueError(f'level {l}: inconsistent feature maps sat {tuple(s.shape)} / grd {tuple(g.shape)}')
            lv[l].sat_feat, lv[l].grd_feat = s.data_ptr(), g.data_ptr()
            lv[l].grd_conf = grd_confs[l].data_ptr() if (self.using_weight and grd_confs[l] is not None) else 0
            lv[l].sat_inv_norm = sat_inv_norm[l].data_ptr() if sat_inv_norm is not None else 0
            lv[l].grd_inv_norm = grd_inv_norm[l].data_ptr() if grd_inv_norm is not None else 0
            lv[l].A, lv[l].h, lv[l].w, lv[l].C, lv[l].row0, lv[l].grd_row_skip = A, g.shape[1], g.shape[2], Cn, 0, 0
            lv[l].meter_per_pixel = utils.get_meter_per_pixel() * utils.get_process_satmap_sidelength() / A   # 71-72
            lv[l].centre = float(A // 2)
        if self.proj == 'nn':            # the in-plane warp has no camera in it
            return cfg, lv, None
        K = camera_k.to(dev).float().contiguous()
        if tuple(K.shape) != (B, 3, 3):
            raise ValueError(f'left_camera_k must be [B,3,3], got {tuple(K.shape)}')
        return cfg, lv, K

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def lm_solve(self, sat_feats, grd_feats, grd_confs, camera_k, ori_hw, init_pose=None, sat_inv_norm=None,
                 grd_inv_norm=None, keep_normal_eq=None):
        """NHWC fp32 feature lists (raw + [L,B] fp64 inverse norms, or already normalised) -> trace [B,N_iters,L,3]."""
        lib = _lib.load()
        dev = sat_feats[0].device
        B, L = sat_feats[0].shape[0], len(sat_feats)
        cfg, lv, K = self._structs(sat_feats, grd_feats, grd_confs, camera_k, sat_inv_norm, grd_inv_norm)
        trace = torch.empty(B, self.N_iters, L, 3, device=dev, dtype=torch.float32)
        strict = bool(getattr(self.args, 'strict_errors', 0))
        want_neq = strict or (self.keep_normal_eq if keep_normal_eq is None else keep_normal_eq)
        neq = torch.empty(L * self.N_iters, B, 16, device=dev, dtype=torch.float64) if want_neq else None
        nbytes = lib.hla_g2s_workspace_bytes(C.byref(cfg), lv, B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p0 = init_pose.to(dev).float().contiguous() if init_pose is not None else None
        oh, ow = (0, 0) if self.proj == 'nn' else (int(ori_hw[0]), int(ori_hw[1]))      # (the in-plane warp reads neither)
        rc = lib.hla_g2s_lm_solve(C.byref(cfg), lv, _lib.ptr(K), oh, ow, _lib.ptr(p0), _lib.ptr(trace),
                                  _lib.ptr(neq), _lib.ptr(ws), nbytes, B, _lib.stream_ptr())
        _lib.check(rc, 'hla_g2s_lm_solve')
        # the reference's run-time errors (see _s2gp.raise_like_reference).  This direction has no norms among its sums: a
        # sample with no satellite pixel projecting into the ground image has H = 0 exactly
        risky = cfg.use_hessian or min(cfg.damping[i] for i in range(3)) <= 0.0
        if risky or strict:
            raise_like_reference(trace, neq[:, :, 2:8].abs().sum(-1) if strict else None, 0)
        # a detached alias: under autograd `trace` becomes the Function's output (grad_fn -> ctx), and ctx/model must not hold it
        # or every step's ctx (8.5 GB of saved workspaces at B = 32) lives in a reference cycle until the cyclic GC runs
        self.last_trace, self.last_normal_eq = trace.detach(), neq
        return trace

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def lm_backward(self, sat_feats, grd_feats, grd_confs, camera_k, ori_hw, trace, normal_eq, d_trace, init_pose=None,
                    sat_inv_norm=None, grd_inv_norm=None):
        """d(loss)/d(trace) -> (d_sat[l], d_grd[l], d_conf[l] or None, d_lambda[3]); gradients w.r.t. the normalised maps."""
        lib = _lib.load()
        dev = sat_feats[0].device
        B, L = sat_feats[0].shape[0], len(sat_feats)
        cfg, lv, K = self._structs(sat_feats, grd_feats, grd_confs, camera_k, sat_inv_norm, grd_inv_norm)
        d_sat = [torch.zeros_like(f) for f in sat_feats]
        d_grd = [torch.zeros_like(f) for f in grd_feats]
        d_conf = [torch.zeros_like(grd_confs[l]) if (self.using_weight and grd_confs[l] is not None) else None for l in range(L)]
        gr = (_lib.S2GLevelGrad * L)()
        for l in range(L):
            gr[l].d_sat_feat, gr[l].d_grd_feat = d_sat[l].data_ptr(), d_grd[l].data_ptr()
            gr[l].d_grd_conf = d_conf[l].data_ptr() if d_conf[l] is not None else 0
        d_lambda = torch.zeros(3, device=dev, dtype=torch.float64)
        dtr = d_trace.contiguous().float()
        nbytes = lib.hla_g2s_bwd_workspace_bytes(C.byref(cfg), lv, B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p0 = init_pose.to(dev).float().contiguous() if init_pose is not None else None
        oh, ow = (0, 0) if self.proj == 'nn' else (int(ori_hw[0]), int(ori_hw[1]))
        rc = lib.hla_g2s_lm_solve_bwd(C.byref(cfg), lv, gr, _lib.ptr(K), oh, ow, _lib.ptr(p0),
                                      _lib.ptr(trace), _lib.ptr(normal_eq), _lib.ptr(dtr), _lib.ptr(d_lambda), _lib.ptr(ws),
                                      nbytes, B, _lib.stream_ptr())
        _lib.check(rc, 'hla_g2s_lm_solve_bwd')
        return d_sat, d_grd, d_conf, d_lambda

    def _score_structs(self, sat_feats, grd_feats, grd_confs, camera_k, ori_hw, sat_inv_norm, grd_inv_norm):
        """``_pose.score_poses``' structs: (cfg, lv, (camera_k, ori_h, ori_w)), what ``hla_g2s_pose_score[_bwd]`` take."""
        cfg, lv, Kc = self._structs(sat_feats, grd_feats, grd_confs, camera_k, sat_inv_norm, grd_inv_norm)
        oh, ow = (0, 0) if self.proj == 'nn' else (int(ori_hw[0]), int(ori_hw[1]))      # (the in-plane warp reads neither)
        return cfg, lv, (Kc, oh, ow)

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def score_poses(self, sat_feats, grd_feats, grd_confs, camera_k, ori_hw, poses, level, sat_inv_norm=None, grd_inv_norm=None):
        """The matching term of this direction at given poses, on feature maps extracted once (``hla_g2s_pose_score``,
        include/hla.h): low-level like ``lm_solve``, with the same map arguments.  ``poses`` [K,3] (shared by the samples) or
        [B,K,3], (shift_u, shift_v, heading) in normalised units; ``level`` indexes the lists.  Returns (cost [B,K] fp32, sums
        [B,K,8] fp64): over the satellite pixels whose projection is in view sum f^2, sum s^2, sum f s, the same three weighted,
        their number, and sum s^2 over all pixels; cost = sum w (f/||f|| - s/||s||)^2 over the overlap, +inf with nothing in view."""
        structs = lambda: self._score_structs(sat_feats, grd_feats, grd_confs, camera_k, ori_hw, sat_inv_norm, grd_inv_norm)
        return _pose.score_poses('hla_g2s_pose_score', structs, sat_feats, poses, level)

    @_lib.on_device(lambda self, sat_feats, *a, **k: sat_feats[0])
    def score_poses_bwd(self, sat_feats, grd_feats, grd_confs, camera_k, ori_hw, poses, level, sums, d_cost, sat_inv_norm=None,
                        grd_inv_norm=None):
        """Backward of ``score_poses`` (``hla_g2s_pose_score_bwd``, include/hla.h): the same map arguments, ``sums`` [B,K,8] of
        the forward and ``d_cost`` [B,K] -> (d_sat [B,A,A,C], d_grd [B,h,w,C], d_conf [B,h,w] or None) of level ``level``, fp32
        NHWC, with respect to the L2-normalised maps -- what ``vgg_backward_nhwc(..., scale_invariant=True)`` takes.  All three
        are written by the call; poses get no gradient.  d_sat is bitwise reproducible, d_grd and d_conf (fp32 atomics) are not."""
        structs = lambda: self._score_structs(sat_feats, grd_feats, grd_confs, camera_k, ori_hw, sat_inv_norm, grd_inv_norm)
        return _pose.score_poses_bwd('hla_g2s_pose_score_bwd', structs, sat_feats, grd_feats, grd_confs, poses, level, sums, d_cost)

    def _features(self, sat_map, grd_img_left, want_conf):
        """Both extractors of the inference path, normalisation deferred: (sat_feats, sat_inv, grd_feats, grd_confs, grd_inv)."""
        sat_feats, _, sat_inv = vgg_forward_nhwc(self.SatFeatureNet, sat_map, want_conf=False, defer_norm=True)
        grd_feats, grd_confs, grd_inv = vgg_forward_nhwc(self.GrdFeatureNet, grd_img_left, want_conf=want_conf, defer_norm=True)
        return sat_feats, sat_inv, grd_feats, grd_confs, grd_inv

    def _score_checks(self, what, sat_map, grd_img_left):
        if getattr(self.args, 'dropout', 0):
            raise NotImplementedError(f'{what} with args.dropout: a pose is scored on every pixel')
        if self.proj == 'nn' and self.using_weight:
            raise NotImplementedError('using_weight with proj=nn')
        self._check_images(sat_map, grd_img_left)

    @_lib.on_device(lambda self, sat_map, *a, **k: sat_map)
    def score_candidates(self, sat_map, grd_img_left, left_camera_k, poses, levels=None):
        """The matching term at ``poses`` ([K,3] or [B,K,3], normalised units) on the maps of the two images, differentiable with
        respect to both extractors' parameters (not the poses): -> (costs, sums), a list of [B,K] fp32 costs and a list of
        [B,K,8] fp64 sums, one entry per level in ``levels`` (default: every level).  Under autograd it is ONE autograd.Function:
        both extractors with their activations saved, ``hla_g2s_pose_score`` per scored level; its backward runs
        ``hla_g2s_pose_score_bwd`` per scored level and ``hla_vgg_backward`` for both extractors.  ``sums`` carry no gradient.
        Without grad it is the inference extractors plus ``score_poses``."""
        self._score_checks('score_candidates', sat_map, grd_img_left)
        cand = _poses_arg(poses, sat_map.shape[0]).to(sat_map.device).contiguous()
        lvls = _pose.levels_arg(levels, self.level)
        under = grad_params(self)
        if under:
            out = _G2sScoreFn.apply(self, under[0], sat_map, grd_img_left, left_camera_k, cand, lvls, *under[1])
            return list(out[:len(lvls)]), list(out[len(lvls):])
        with torch.no_grad():
            sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = self._features(sat_map, grd_img_left, bool(self.using_weight))
            res = [self.score_poses(sat_feats, grd_feats, grd_confs, left_camera_k, grd_img_left.shape[-2:], cand, l, sat_inv,
                                    grd_inv) for l in lvls]
        return [r[0] for r in res], [r[1] for r in res]

    def score_loss(self, sat_map, grd_img_left, left_camera_k, candidates, gt_shift_u, gt_shift_v, gt_heading, levels=None,
                   min_in_view=0.5):
        """Metric learning on the surface ``forward_search`` ranks with, ``LM_S2GP.score_loss`` in this direction (an extension,
        in the form of the reference's triplet_loss, models_kitti.py:579-595): the pose list of every sample is the true pose
        (gt_shift_u, gt_shift_v, gt_heading: [B] or [B,1], normalised units) followed by ``candidates`` ([K,3] or [B,K,3]); per
        scored level (``levels``, default all)
            loss_l = sum_b sum_k log(1 + exp(10 (cost[b, true] - cost[b, k]))) / (B K)
        over the candidates that keep at least ``min_in_view`` of the sample's best pixel count in view (``eligible_cost``'s rule
        over the K + 1 entries; the others contribute exactly zero), summed over the levels: a scalar that back-propagates into
        both extractors through HIP kernels (``score_candidates``).  ``last_score_loss`` keeps the costs [B,K+1] and sums
        [B,K+1,8] per level."""
        self._score_checks('score_loss', sat_map, grd_img_left)
        poses = _pose.true_pose_first((gt_shift_u, gt_shift_v, gt_heading), candidates, sat_map.shape[0], sat_map.device)
        costs, sums = self.score_candidates(sat_map, grd_img_left, left_camera_k, poses, levels)
        return _pose.score_loss_tail(self, costs, sums, min_in_view)

    @_lib.on_device(lambda self, sat_map, *a, **k: sat_map)
    def forward_search(self, sat_map, grd_img_left, left_camera_k, candidates, top_m=1, score_level=0, min_in_view=0.5):
        """A pose search in front of the LM loop, the composition of ``S2GPBase._search`` in this direction: extract the features
        once, score the ``candidates`` ([K,3] or [B,K,3]; ``pose_grid``) at ``score_level``, run the loop from the ``top_m`` best
        eligible ones (``eligible_cost``), keep the final pose that scores best at the finest level.  No autograd, no host sync,
        no random numbers.  -> (shift_lat[B], shift_lon[B], theta[B]) like ``forward(mode='test')``; ``last_search`` keeps cost,
        sums, start_index [B,top_m], traces [B,top_m,N_iters,L,3], final_cost [B,top_m] and best [B]."""
        self._check_images(sat_map, grd_img_left)
        cand, M = _pose.search_candidates(candidates, top_m, sat_map)
        with torch.no_grad():
            sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = self._features(sat_map, grd_img_left, bool(self.using_weight))
            hw = grd_img_left.shape[-2:]
            score = lambda poses, level: self.score_poses(sat_feats, grd_feats, grd_confs, left_camera_k, hw, poses, level,
                                                          sat_inv, grd_inv)
            solve = lambda p0: self.lm_solve(sat_feats, grd_feats, grd_confs, left_camera_k, hw, p0, sat_inv, grd_inv)
            pose = _pose.search(self, cand, M, score, solve, score_level, len(sat_feats) - 1, min_in_view)
        return pose[:, 1], pose[:, 0], pose[:, 2]

    def corr(self, sat_map, grd_img_left, left_camera_k, gt_shift_u=None, gt_shift_v=None, gt_heading=None, mode='train',
             file_name=None, gt_depth=None):
        """models_kitti.py:501-577, the reference's signature: the dense translation search.  Per level the ground map is projected
        at the zero pose, centre-cropped by the shift ranges, normalised and correlated with the satellite map at every shift
        (``_g2s_corr``; ``hla_g2s_corr``, include/hla.h).  mode='train' -> the triplet loss (579-595) summed over the levels, a
        scalar that back-propagates into both extractors; any other mode -> (pred_u [B], pred_v [B]), the argmin shift of the
        LAST level in metres, computed without autograd.  ``self.last_corr`` keeps corr [B,Ny,Nx] of every level.  The
        correlation reads fp32 maps in every precision mode; gt_heading, file_name and gt_depth are ignored as in the reference;
        proj='nn' raises NotImplementedError."""
        from . import _g2s_corr
        return _g2s_corr.corr(self, sat_map, grd_img_left, left_camera_k, gt_shift_u, gt_shift_v, mode)

    def _check_images(self, sat_map, grd_img_left, gpu=True):
        _lib.image_pair(sat_map, grd_img_left, self.damping, gpu)
        if self.proj == 'nn':
            A, (H, W) = sat_map.shape[-1], grd_img_left.shape[-2:]
            if 2 * H != A or W != 2 * A:
                raise ValueError(f"proj='nn' warps the FOLDED ground maps ([H,W] -> [2H,W/2]) in the satellite maps' plane, so they must "
                                 f'be the satellite maps\' size: grd_img must be [B,3,A/2,2A] = [B,3,{A // 2},{2 * A}] for sat_map '
                                 f'[B,3,{A},{A}], got {tuple(grd_img_left.shape)}')

    @_lib.on_device(lambda self, sat_map, *a, **k: sat_map)
    def forward(self, sat_map, grd_img_left, left_camera_k, gt_shift_u=None, gt_shift_v=None, gt_heading=None,
                mode='train', file_name=None, gt_depth=None, init_pose=None):
        """mode='test' -> (shift_lat[B], shift_lon[B], theta[B]) (models_kitti.py:498-499);
        mode='train' -> the 14-tuple (486-496); under autograd its loss back-propagates through the HIP backward (_G2sFn)."""
        self._check_images(sat_map, grd_img_left, gpu=False)
        want_conf = bool(self.using_weight) or mode == 'train'
        under = grad_params(self)
        if under:
            out = _G2sFn.apply(self, under[0], sat_map, grd_img_left, left_camera_k, want_conf, init_pose, *under[1])
            trace, grd_confs = out[0], (list(out[1:]) if want_conf else [None] * self.level)
        else:
            sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = self._features(sat_map, grd_img_left, want_conf)
            trace = self.lm_solve(sat_feats, grd_feats, grd_confs, left_camera_k, grd_img_left.shape[-2:], init_pose, sat_inv,
                                  grd_inv)
        shift_lons, shift_lats, thetas = trace[..., 0], trace[..., 1], trace[..., 2]        # models_kitti.py:470-472
        if mode == 'train':
            a = self.args
            out = loss_from_trace(self.loss_method, trace, (1, 0, 2), gt_shift_v[:, 0], gt_shift_u[:, 0], gt_heading[:, 0],
                                  a.coe_shift_lat, a.coe_shift_lon, a.coe_heading)
            return (*out, [c.unsqueeze(1) for c in grd_confs])
        return shift_lats[:, -1, -1], shift_lons[:, -1, -1], thetas[:, -1, -1]


class _G2sFn(torch.autograd.Function):
    """forward: trace [B,N,L,3] (+ the three ground confidence maps); backward: parameter gradients from HIP kernels."""

    @staticmethod
    def forward(ctx, model, names, sat_map, grd_img, camera_k, want_conf, init_pose, *params):
        sat_feats, sat_inv, grd_feats, grd_confs, grd_inv, cs, cg = extract_saved(model, sat_map, grd_img, want_conf)
        trace = model.lm_solve(sat_feats, grd_feats, grd_confs, camera_k, grd_img.shape[-2:], init_pose, sat_inv, grd_inv,
                               keep_normal_eq=True)
        ctx.model, ctx.names, ctx.init_pose = model, names, init_pose
        ctx.state = (sat_feats, grd_feats, grd_confs, camera_k, tuple(grd_img.shape[-2:]), trace.detach(), model.last_normal_eq,
                     sat_inv, grd_inv, cs, cg)
        outs = (trace,) + (tuple(grd_confs) if want_conf else ())
        if want_conf:
            ctx.mark_non_differentiable(*grd_confs)
        return outs

    @staticmethod
    def backward(ctx, d_trace, *unused):
        model = ctx.model
        sat_feats, grd_feats, grd_confs, camera_k, ori_hw, trace, neq, sat_inv, grd_inv, cs, cg = take_state(ctx)
        d_sat, d_grd, d_conf, d_lam = model.lm_backward(sat_feats, grd_feats, grd_confs, camera_k, ori_hw, trace, neq, d_trace,
                                                        ctx.init_pose, sat_inv, grd_inv)
        use_w = model.using_weight and all(c is not None for c in d_conf)
        grads = extractor_grads(model, cs, cg, d_sat, d_grd, grd_confs if use_w else None, d_conf if use_w else None)
        if getattr(model.args, 'train_damping', 0):            # lambda is the parameter itself (models_kitti.py:357-358)
            grads['damping'] = d_lam.view(1, 3).float()
            sync = getattr(model, 'grad_sync', None)
            if sync:
                sync.finish(sync.start({'damping': grads['damping']}))
        return (None,) * 7 + tuple(grads.get(n) for n in ctx.names)


class _G2sScoreFn(torch.autograd.Function):
    """``LM_G2SP.score_candidates`` under autograd.  forward: the costs [B,K] of every scored level, then their sums [B,K,8]
    (non-differentiable); backward: parameter gradients of both extractors from HIP kernels."""

    @staticmethod
    def forward(ctx, model, names, sat_map, grd_img, camera_k, poses, levels, *params):
        sat_feats, sat_inv, grd_feats, grd_confs, grd_inv, cs, cg = extract_saved(model, sat_map, grd_img, bool(model.using_weight))
        hw = tuple(grd_img.shape[-2:])
        res = [model.score_poses(sat_feats, grd_feats, grd_confs, camera_k, hw, poses, l, sat_inv, grd_inv) for l in levels]
        costs, sums = tuple(r[0] for r in res), tuple(r[1] for r in res)
        ctx.model, ctx.names, ctx.levels = model, names, levels
        ctx.state = (sat_feats, grd_feats, grd_confs, camera_k, hw, poses, sums, sat_inv, grd_inv, cs, cg)
        ctx.mark_non_differentiable(*sums)
        ctx.set_materialize_grads(False)
        return costs + sums

    @staticmethod
    def backward(ctx, *d_out):
        model = ctx.model
        sat_feats, grd_feats, grd_confs, camera_k, hw, poses, sums, sat_inv, grd_inv, cs, cg = take_state(ctx, 'score_candidates call')
        bwd = lambda n, l: model.score_poses_bwd(sat_feats, grd_feats, grd_confs, camera_k, hw, poses, l, sums[n], d_out[n],
                                                 sat_inv, grd_inv)
        d_sat, d_grd, d_conf = _pose.score_level_grads(model, bwd, ctx.levels, d_out, sat_feats, grd_feats, grd_confs)
        # the cost renormalises both maps: every d_map is orthogonal to its map (HLA_VGG_BWD_SCALE_INVARIANT, include/hla.h)
        grads = extractor_grads(model, cs, cg, d_sat, d_grd, grd_confs if d_conf else None, d_conf, scale_invariant=True)
        return (None,) * 7 + tuple(grads.get(n) for n in ctx.names)
