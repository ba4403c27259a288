"""``LM_S2GP`` -- KITTI satellite->ground localisation model with the reference's surface
(``models_kitti.py:598-1316``): ``LM_S2GP(args)``; ``forward(sat_map, grd_img_left, gt_shiftu, gt_shiftv,
gt_heading, mode, file_name, gt_depth, loop, level_first)``; 49-tensor state dict with identical keys.
The hot path (two VGG U-Nets, projection + Jacobian, N_iters x levels LM steps) runs in libhla (HIP, gfx950).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _orien
from ._g2sp import LM_G2SP  # noqa: F401  (models_kitti.py:22-499)
from ._s2gp import S2GPBase, loss_func, loss_from_trace, pose_grid  # noqa: F401  (loss_func re-exported like the reference module)


class LM_S2GP(S2GPBase):
    ford = False

    def __init__(self, args):
        super().__init__(args)
        # models_kitti.py:642-646: built for four levels whatever args.level is (plain CPU tensors, not buffers: the state dict
        # keeps the reference's 49 keys); device copies and the column windows of orien_corr are cached per device
        self.polar_grids = [self.polar_coordinates(level) for level in range(4)]
        self._polar_cache = {}
        self.last_orien_corr = None      # [(corr [B,S] fp32, degree_per_pixel)] per level of the last orien_corr call (an extension)

    # -- the coarse heading search (models_kitti.py:1494-1624) -------------------------------
    def polar_coordinates(self, level):
        """models_kitti.py:1518-1541: [1, A//2, 8A, 2] sampling coordinates of the polar satellite map, A = 512 / 2^(3-level)."""
        return _orien.polar_coordinates(self.meters_per_pixel[level], level)

    def polar_transform(self, sat_feat, level):
        """models_kitti.py:1494-1516: sat_feat [B,C,A,A] -> its polar resampling [B,C,A//2,8A] (the grid is built for the map's
        own A, as there)."""
        from .jacobian import grid_sample
        B, _, A, _ = sat_feat.shape
        grd_H, grd_W = A // 2, A * 2
        v, u = torch.meshgrid(torch.arange(0, grd_H, dtype=torch.float32), torch.arange(0, 4 * grd_W, dtype=torch.float32), indexing='ij')
        theta = u / grd_W * np.pi * 2
        radius = (1 - v / grd_H) * 40 / self.meters_per_pixel[level]
        us = A / 2 + radius * torch.cos(np.pi / 4 - theta)
        vs = A / 2 - radius * torch.sin(np.pi / 4 - theta)
        grids = torch.stack([us, vs], dim=-1).unsqueeze(dim=0).repeat(B, 1, 1, 1).to(sat_feat.device)
        return grid_sample(sat_feat, grids)[0]

    def _polar_window(self, level, n, W, B, device):
        """[B,H,W+S-1,2]: the columns of polar_grids[level] that the shifts of orien_corr read (``_orien.window_columns``), built
        once per (device, level, n, W, B)."""
        key = (str(device), level, n, W, B)
        if key not in self._polar_cache:
            g = self.polar_grids[level]
            cols = torch.tensor(_orien.window_columns(g.shape[2], W, n), dtype=torch.long)
            self._polar_cache[key] = g[:, :, cols, :].to(device).expand(B, -1, -1, -1).contiguous()
        return self._polar_cache[key]

    def orien_corr(self, sat_map, grd_img_left, gt_shiftu=None, gt_shiftv=None, gt_heading=None, mode='train',
                   file_name=None, gt_depth=None):
        """models_kitti.py:1543-1605, the reference's signature.  mode='train' -> the triplet loss (1607-1624), a scalar that
        back-propagates into both extractors; any other mode -> the argmin heading of the LAST level, [B] in degrees.
        ``self.last_orien_corr`` keeps (corr [B,S], degree_per_pixel) of every level.  sat_map must be 512 x 512 and the ground
        image 256 rows high (the polar grids are built for that, as in the reference); the correlation reads fp32 maps in
        every precision mode."""
        return _orien.orien_corr(self, sat_map, grd_img_left, gt_heading, mode)

    def forward(self, sat_map, grd_img_left, gt_shiftu=None, gt_shiftv=None, gt_heading=None, mode='train',
                file_name=None, gt_depth=None, loop=0, level_first=0, init_pose=None):
        """sat_map [B,3,A,A], grd_img_left [B,3,H,W] fp32 in [0,1] on the GPU.
        mode='test'  -> (shift_lat[B], shift_lon[B], theta[B])   (models_kitti.py:1316)
        mode='train' -> the reference's 14-tuple                 (models_kitti.py:1312-1314)
        ``init_pose`` [B,3] (shift_u, shift_v, heading) is an extension; the reference always starts at 0.
        ``gt_depth`` [B,dH,dW] with ``args.use_gt_depth``: every ground pixel is lifted to its camera ray times the depth
        (nearest-resampled to each level), masked where the depth is -1, instead of onto the flat ground
        (models_kitti.py:741-748); without the flag, or without a map, it is ignored as in the reference."""
        if not getattr(self.args, 'use_gt_depth', 0):
            gt_depth = None
        want_conf = bool(self.using_weight) or mode == 'train'
        trace, grd_confs = self.localise(sat_map, grd_img_left, want_conf, None, level_first, init_pose,
                                          return_confs=(mode == 'train'), gt_depth=gt_depth)
        shift_lons, shift_lats, thetas = trace[..., 0], trace[..., 1], trace[..., 2]   # models_kitti.py:1281-1283
        if mode == 'train':
            a = self.args
            coe_heading = 0 if a.rotation_range == 0 else a.coe_heading
            # loss_func(shift_lats, shift_lons, thetas, gt_shiftv[:, 0], gt_shiftu[:, 0], gt_heading[:, 0], ...) of
            # models_kitti.py:1304-1310, on the trace's columns (lat = 1, lon = 0, theta = 2)
            out = loss_from_trace(self.loss_method, trace, (1, 0, 2), gt_shiftv[:, 0], gt_shiftu[:, 0], gt_heading[:, 0],
                                  a.coe_shift_lat, a.coe_shift_lon, coe_heading)
            return (*out, [c.unsqueeze(1) for c in grd_confs])
        res = (shift_lats[:, -1, -1], shift_lons[:, -1, -1], thetas[:, -1, -1])
        if torch.is_grad_enabled():
            # train_kitti.py:63-64 calls .backward() on the test outputs "to release the graph"
            res = tuple(r.clone().requires_grad_(True) for r in res)
        return res

    def forward_search(self, sat_map, grd_img_left, candidates, top_m=1, score_level=0, min_in_view=0.5, level_first=0,
                       gt_depth=None):
        """A pose search around the LM loop (an extension; the reference starts its loop at the zero pose).  The features are
        extracted once (the mode='test' path); ``candidates`` -- [K,3] shared by the samples or [B,K,3], (shift_u, shift_v,
        heading) in normalised units, e.g. ``pose_grid(5, 5, 5)`` -- are scored at level ``score_level`` with the loop's own
        objective (``score_poses``); the ``top_m`` best of those that keep at least ``min_in_view`` of the sample's best pixel
        count in view start one LM loop each (each draws its own re-initialisation values: ``top_m`` times the RNG consumption
        of ``forward``), and the final pose that scores best at the finest level is returned, as the tuple of
        ``forward(mode='test')``: (shift_lat[B], shift_lon[B], theta[B]).  Always without gradients; no host sync.
        ``last_search`` keeps cost [B,K], sums [B,K,8], start_index [B,M], traces [B,M,N,L,3], final_cost [B,M], best [B]."""
        if gt_depth is not None and getattr(self.args, 'use_gt_depth', 0):
            raise NotImplementedError('forward_search with a depth map: depth-lifted pose scoring is not built')
        pose = self._search(sat_map, grd_img_left, None, candidates, top_m, score_level, min_in_view, level_first)
        return pose[:, 1], pose[:, 0], pose[:, 2]

    def score_loss(self, sat_map, grd_img_left, candidates, gt_shiftu, gt_shiftv, gt_heading, levels=None, min_in_view=0.5,
                   gt_depth=None):
        """Metric learning on the surface ``forward_search`` ranks with (an extension, in the form of the reference's
        triplet_loss, models_kitti.py:579-595 and 1607-1624): the pose list of every sample is the true pose (gt_shiftu,
        gt_shiftv, gt_heading: [B] or [B,1], normalised units) followed by ``candidates`` ([K,3] or [B,K,3], e.g.
        ``pose_grid(5, 5, 5)``); per scored level (``levels``, default all)
            loss_l = sum_b sum_k log(1 + exp(10 (cost[b, true] - cost[b, k]))) / (B K)
        over the candidates that keep at least ``min_in_view`` of the sample's best pixel count in view (``eligible_cost``'s rule
        over the K + 1 entries; the others contribute exactly zero), and the result is the sum over the levels: a scalar that
        back-propagates into both extractors through HIP kernels (``score_candidates``).  Call it next to
        ``forward(mode='train')``.  ``last_score_loss`` keeps the costs [B,K+1] and sums [B,K+1,8] per level."""
        if gt_depth is not None and getattr(self.args, 'use_gt_depth', 0):
            raise NotImplementedError('score_loss with a depth map: depth-lifted pose scoring is not built')
        return self._score_loss(sat_map, grd_img_left, None, candidates, (gt_shiftu, gt_shiftv, gt_heading), levels, min_in_view)
