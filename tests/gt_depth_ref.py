"""fp64-capable restatement of ``args.use_gt_depth`` for ``LM_S2GP`` (models_kitti.py:741-748), built on ``oracle.ref_cpu`` the way
``tests/polar_ref.py`` is: the oracle's model with per-sample points and mask in place of the shared ground-plane table.  With a
depth map every ground pixel is lifted to ``xyz_w * depth`` -- the camera ray K^-1 [u,v,1] of grd_img2cam (673) times the depth map
resampled to the level by ``F.interpolate`` (default mode, nearest) -- and masked where the resampled map is -1; nothing else changes
(rows h/2.., every updater, both loop orders).  The product is formed in fp32, as in the reference (table and depth are fp32
tensors there, also in an fp64 run of the model).  ``tests/test_gt_depth_cpu.py`` pins this restatement, run in fp32, to the REAL
reference's recorded fp32 results (tools/make_golden_gt_depth.py).  Also here: the depth-map generator shared by that script and
the tests."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

DEPTH_HW = (94, 311)        # the fixtures' depth map: no multiple or divisor of any level size


def depth_map(seed, B, dH=DEPTH_HW[0], dW=DEPTH_HW[1]):
    """The synthetic depth map of the fixtures and tests, regenerated from its seed (``highlyaccurate_amd.synthetic.gt_depth``:
    ground-plane depth x (1 + 0.2 U(0,1)), 15 % holes of -1).  [B,dH,dW] fp32 (CPU)."""
    from highlyaccurate_amd import synthetic
    return synthetic.gt_depth(B, dH, dW, seed)


def camera_rays(K_ori, grd_H, grd_W, ori_H, ori_W):
    """``xyz_w`` of grd_img2cam (models_kitti.py:657-673), the third element it returns: [1,h,w,3] fp32."""
    K = torch.tensor(K_ori, dtype=torch.float32).reshape(1, 3, 3).clone()
    Ks = K.clone()
    Ks[:, :1, :] = K[:, :1, :] * grd_W / ori_W
    Ks[:, 1:2, :] = K[:, 1:2, :] * grd_H / ori_H
    Kinv = torch.inverse(Ks)
    v, u = torch.meshgrid(torch.arange(0, grd_H, dtype=torch.float32), torch.arange(0, grd_W, dtype=torch.float32), indexing='ij')
    uv1 = torch.stack([u, v, torch.ones_like(u)], dim=-1).unsqueeze(0)
    return torch.sum(Kinv[:, None, None, :, :] * uv1[:, :, :, None, :], dim=-1)


def lifted_points(rays, gt_depth):
    """models_kitti.py:742-748 for one level: rays [1,h,w,3] fp32, gt_depth [B,dH,dW] -> (xyz [B,h,w,3] fp32, mask [B,h,w] fp32)."""
    H, W = rays.shape[1:3]
    gt_depth = gt_depth.float()
    depth = F.interpolate(gt_depth[:, None, :, :], (H, W))
    xyz = rays * depth.permute(0, 2, 3, 1)
    mask = F.interpolate((gt_depth != -1).float()[:, None, :, :], (H, W), mode='nearest')[:, 0]
    return xyz, mask


class LM_S2GP_Depth(O.LM_S2GP):
    """``oracle.ref_cpu.LM_S2GP`` with the gt_depth branch.  ``self.gt_depth`` is the map of the current call (``forward`` sets it from
    its argument; tests that drive ``_step`` / ``project_map_to_grd`` themselves set it directly)."""

    def __init__(self, args, grd_hw=(256, 1024)):
        super().__init__(args, grd_hw=grd_hw)
        self.rays = [camera_rays(O.KITTI_K, grd_hw[0] / 2 ** (3 - l), grd_hw[1] / 2 ** (3 - l), 256, 1024) for l in range(4)]
        self.gt_depth = None

    def _pose_to_uv(self, pos, A, su, sv, th, extra, require_jac=True):
        if not self.args.use_gt_depth or self.gt_depth is None:
            return super()._pose_to_uv(pos, A, su, sv, th, extra, require_jac)
        if self.args.proj != 'geo':
            raise IndexError('tuple index out of range')        # xyz_grds[level][2] of a grd_img2cam_polar table
        xyz, mask = lifted_points(self.rays[pos], self.gt_depth)
        uv, jac = O.kitti_pose_to_uv(self.args, xyz, su, sv, th, A, require_jac)
        return uv, jac, mask.to(su.dtype)

    def forward(self, sat_map, grd_img_left, gt_shiftu=None, gt_shiftv=None, gt_heading=None, mode='train',
                file_name=None, gt_depth=None, loop=0, level_first=0):
        self.gt_depth = gt_depth
        try:
            return super().forward(sat_map, grd_img_left, gt_shiftu, gt_shiftv, gt_heading, mode, file_name, None, loop, level_first)
        finally:
            self.gt_depth = None


def build(args, seed, dtype=torch.float32, bias_scale=0.0, grd_hw=(256, 1024)):
    """``oracle.ref_cpu.build('kitti', ...)`` for the depth-aware model (same portable synthetic weights)."""
    net = LM_S2GP_Depth(args, grd_hw=grd_hw)
    net.load_state_dict(O.synth_model_state(seed, bias_scale, rotation_range=args.rotation_range))
    return net.to(dtype)


def stacked_trace(on, B):
    """The oracle's (lats, lons, thetas) [B,N,L] -> (u, v, theta) as [B,N*L,3], iteration-major whatever the loop order."""
    lat, lon, th = on.trace
    return torch.stack([lon, lat, th], -1).detach().reshape(B, -1, 3).double().numpy()


def normal_eq(onet, sat, grd, conf, pose, level, using_weight, keep=None):
    """The 14 sums of one step over rows h/2.. of the level map from the restatement's own projection (``onet.gt_depth`` set):
    S, G, H(6), U(3), V(3), what hla_s2g_lm_solve reports in normal_eq slots 0..13.  ``keep`` [(h - h//2)*w] bool: args.dropout."""
    su, sv, th = pose
    dt = su.dtype
    f, _, jac, _, mask = onet.project_map_to_grd(sat[level].to(dt), None, su, sv, th, level, None)
    g = grd[level].to(dt) * mask[:, None]
    w = conf[level].to(dt) * mask[:, None] if using_weight else torch.ones_like(g[:, :1])
    h0 = f.shape[-2] // 2
    f, g, w, jac = f[:, :, h0:], g[:, :, h0:], w[:, :, h0:], jac[:, :, :, h0:]
    B = f.shape[0]
    if keep is not None:
        k = keep.reshape(1, 1, *f.shape[-2:]).to(dt)
        f, g, jac = f * k, g * k, jac * k[None]
    s_, g_, J = f.reshape(B, -1), g.reshape(B, -1), jac.reshape(3, B, -1)
    W = w.expand(-1, f.shape[1], -1, -1).reshape(B, -1)
    out = [(s_ * s_).sum(1), (g_ * g_).sum(1)]
    for p, q in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        out.append((W * J[p] * J[q]).sum(1))
    out += [(W * J[p] * s_).sum(1) for p in range(3)] + [(W * J[p] * g_).sum(1) for p in range(3)]
    return torch.stack(out, 1).numpy()
