"""``LM_S2GP_Ford`` -- Ford-AV model with the reference's surface (``models_ford.py:21-1036``) and
``loss_func`` (``models_ford.py:1041-1093``), executed by libhla."""
from __future__ import annotations

import torch

from . import _lib
from ._s2gp import S2GPBase, ford_K_network_input, loss_func, loss_from_trace, pose_grid  # noqa: F401


class LM_S2GP_Ford(S2GPBase):
    ford = True

    def forward(self, sat_map, grd_img_left, satmap_sidelength_meters, R_FL, T_FL,
                gt_shift_u=None, gt_shift_v=None, gt_theta=None, mode='train',
                file_name=None, level_first=0, loop=0, init_pose=None):
        """mode='test' -> (shift_u[B], shift_v[B], theta[B]) (models_ford.py:864-865);
        mode='train' -> 14-tuple (models_ford.py:858-862).  gt_* are [B] (float64 from the dataloader)."""
        want_conf = bool(self.using_weight) or mode == 'train'
        extra = dict(R_FL=R_FL, T_FL=T_FL, side_m=float(satmap_sidelength_meters))
        trace, grd_confs = self.localise(sat_map, grd_img_left, want_conf, extra, level_first, init_pose,
                                          return_confs=(mode == 'train'))
        us, vs, thetas = trace[..., 0], trace[..., 1], trace[..., 2]
        if mode == 'train':
            a = self.args
            coe_heading = 0 if a.rotation_range == 0 else a.coe_heading
            dev = trace.device
            # loss_func(us, vs, thetas, gt_shift_u, gt_shift_v, gt_theta, ...) of models_ford.py:837-839 on the trace's columns
            out = loss_from_trace(self.loss_method, trace, (0, 1, 2), gt_shift_u.to(dev), gt_shift_v.to(dev), gt_theta.to(dev),
                                  a.coe_shift_lat, a.coe_shift_lon, coe_heading)
            return (*out, [c.unsqueeze(1) for c in grd_confs])
        res = (us[:, -1, -1], vs[:, -1, -1], thetas[:, -1, -1])
        if torch.is_grad_enabled():
            res = tuple(r.clone().requires_grad_(True) for r in res)
        return res

    def forward_search(self, sat_map, grd_img_left, satmap_sidelength_meters, R_FL, T_FL, candidates, top_m=1, score_level=0,
                       min_in_view=0.5, level_first=0):
        """``LM_S2GP.forward_search`` on the Ford chain: the candidates are scored on feature maps extracted once, the LM loop runs
        from the ``top_m`` best eligible ones and the final pose that scores best at the finest level is returned as the tuple
        of ``forward(mode='test')``: (shift_u[B], shift_v[B], theta[B]).  ``last_search`` keeps the scores and the traces."""
        extra = dict(R_FL=R_FL, T_FL=T_FL, side_m=float(satmap_sidelength_meters))
        pose = self._search(sat_map, grd_img_left, extra, candidates, top_m, score_level, min_in_view, level_first)
        return pose[:, 0], pose[:, 1], pose[:, 2]

    def score_loss(self, sat_map, grd_img_left, satmap_sidelength_meters, R_FL, T_FL, candidates, gt_shiftu, gt_shiftv, gt_heading,
                   levels=None, min_in_view=0.5):
        """``LM_S2GP.score_loss`` on the Ford chain: the triplet-form loss of the true pose (gt_shiftu, gt_shiftv, gt_heading)
        against ``candidates`` on the score surface of ``forward_search``, summed over the scored levels; a scalar that
        back-propagates into both extractors.  ``last_score_loss`` keeps the costs and sums."""
        extra = dict(R_FL=R_FL, T_FL=T_FL, side_m=float(satmap_sidelength_meters))
        return self._score_loss(sat_map, grd_img_left, extra, candidates, (gt_shiftu, gt_shiftv, gt_heading), levels, min_in_view)

    @_lib.on_device(lambda self, sat_map, *a, **k: sat_map)
    def forward_views(self, sat_map, grd_imgs, satmap_sidelength_meters, R, T, camera_k=None, level_first=0, init_pose=None):
        """Multi-view localisation: ONE LM loop over V ground images per satellite tile -- several calibrated cameras, or earlier
        frames carried forward by odometry -- each with its own rigid transform to the one body pose being solved for.
        sat_map [B,3,A,A]; grd_imgs [B,V,3,H,W], one size for all views; R [B,V,3,3], T [B,V,3] camera v -> body (what
        ``forward`` takes as R_FL, T_FL); camera_k [V,3,3] in the convention of ``ford_K_network_input()`` (given for a 256x1024
        image), default: that matrix for every view.  GrdFeatureNet is shared by all views, so the weights of a single-view
        training apply.  One step is the reference's LM_update on the union of the views' pixels (``lm_solve_views``); V = 1 is
        ``forward(mode='test')``, with the same RNG consumption.  A view outside the satellite map still contributes the norm of
        its ground features.  Returns the tuple of ``forward(mode='test')``: (shift_u[B], shift_v[B], theta[B]).
        Inference only: it runs under no_grad, its outputs carry no gradient, and NO BACKWARD EXISTS (there is no mode='train')."""
        if getattr(self.args, 'dropout', 0):
            raise NotImplementedError('forward_views with args.dropout: the dropout loop is not built for several views')
        if getattr(self.args, 'estimate_depth', 0):
            raise NotImplementedError('forward_views with args.estimate_depth: depth lifting is not built for several views')
        if self.polar and level_first:
            raise NotImplementedError("LM_S2GP_Ford(proj='polar') with level_first=1: the reference's level-first loop reads only "
                                      "the bottom half of the polar maps (it has no proj branch); that combination is not built")
        _lib.require_gpu(sat_map, 'sat_map')
        _lib.require_gpu(grd_imgs, 'grd_imgs')
        if sat_map.dim() != 4 or grd_imgs.dim() != 5 or sat_map.shape[0] != grd_imgs.shape[0] or sat_map.shape[1] != 3 \
                or grd_imgs.shape[2] != 3 or sat_map.shape[2] != sat_map.shape[3] or grd_imgs.shape[1] < 1:
            raise ValueError(f'expected sat_map [B,3,A,A] and grd_imgs [B,V,3,H,W] with one B, got {tuple(sat_map.shape)} '
                             f'and {tuple(grd_imgs.shape)}')
        _lib.same_device(('sat_map', sat_map), ('grd_imgs', grd_imgs), ('parameters', self.damping))
        B, V, _, H, W = grd_imgs.shape
        if V > 8:
            raise ValueError(f'forward_views: at most 8 views, got {V}')
        K = torch.as_tensor(ford_K_network_input() if camera_k is None else camera_k, dtype=torch.float32).cpu()
        K = K.reshape(1, 3, 3).expand(V, 3, 3) if K.numel() == 9 else K
        if tuple(K.shape) != (V, 3, 3):
            raise ValueError(f'camera_k must be [V,3,3] with V = {V}, got {tuple(K.shape)}')
        with torch.no_grad():
            tables = self.view_tables(H, W, K, sat_map.device)
            sat_feats, sat_inv, grd_feats, grd_confs, grd_inv = self._features(sat_map, grd_imgs.reshape(B * V, 3, H, W),
                                                                               bool(self.using_weight), False, pair=False)
            trace = self.lm_solve_views(sat_feats, grd_feats, grd_confs, (H, W), V, R, T, float(satmap_sidelength_meters), tables,
                                        level_first, init_pose, sat_inv, grd_inv)
        self.last_trace = trace
        return trace[:, -1, -1, 0], trace[:, -1, -1, 1], trace[:, -1, -1, 2]
