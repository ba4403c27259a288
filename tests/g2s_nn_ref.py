"""fp64-capable restatement of ``LM_G2SP(proj='nn')`` (models_kitti.py:22-499 with VGGUnet_G2S, VGG.py:206-345, and
inplane_grd_to_map, models_kitti.py:289-332), built from the pieces of ``oracle.ref_cpu`` (the VGG layers, ``grid_sample``,
``lm_update_g2s``, ``loss_func``).  The reference class mixes hard-coded float32 tensors into its arithmetic and cannot run in
fp64; this one can, and ``tests/test_g2s_nn_cpu.py`` pins it, run in fp32, to the reference's recorded fp32 results."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O


def fold(t):
    """[B,C,H,W] -> [B,C,2H,W/2] by reshape (VGG.py:278-279 and its kin)."""
    B, C, H, W = t.shape
    return t.reshape(B, C, 2 * H, W // 2)


class VGGUnet_G2S(O.VGGUnet):
    """The folded ground extractor: the encoder is VGGUnet's, every decoder input is the fold of an encoder map, conf0 reads the
    unfolded x15 (VGG.py:322)."""

    def raw_maps(self, x):
        r = F.relu
        x2 = self.conv2(r(self.conv0(x)))
        x3 = F.max_pool2d(x2, 2)
        x7 = self.conv7(r(self.conv5(r(x3))))
        x8 = F.max_pool2d(x7, 2)
        x14 = self.conv14(r(self.conv12(r(self.conv10(r(x8))))))
        x15 = F.max_pool2d(x14, 2)
        x2_, x3_, x8_, x15_ = fold(x2), fold(x3), fold(x8), fold(x15)
        up = lambda t, like: F.interpolate(t, like.shape[2:], mode='nearest')
        x18 = self.conv_dec1(torch.cat([up(x15_, x8_), x8_], 1))
        x21 = self.conv_dec2(torch.cat([up(x18, x3_), x3_], 1))
        x24 = self.conv_dec3(torch.cat([up(x21, x2_), x2_], 1))
        return x15, x15_, x18, x21, x24

    def forward(self, x):
        x15, x15_, x18, x21, x24 = self.raw_maps(x)
        confs = [torch.sigmoid(-m(t)) for m, t in
                 ((self.conf0, x15), (self.conf1, x18), (self.conf2, x21), (self.conf3, x24))]
        feats = [O.l2_norm_map(t) for t in (x15_, x18, x21, x24)]
        sel = {-1: [0], -2: [1], -3: [2], 2: [1, 2], 3: [0, 1, 2], 4: [0, 1, 2, 3]}[self.level]
        return [feats[i] for i in sel], [confs[i] for i in sel]


def inplane_pose_to_uv(args, A, shift_u, shift_v, heading):
    """inplane_grd_to_map (models_kitti.py:289-332): uv [B,A,A,2] where every pixel of the A x A satellite map samples the
    (folded) ground map, and d(uv)/d(shift_u, shift_v, heading), each [B,A,A,2].  The mask is all ones."""
    dt = shift_u.dtype
    B = shift_u.shape[0]
    mpp = O.meter_per_pixel() * O.SATMAP_PROCESS_SIDELENGTH / A                         # 291-292
    T = torch.cat([-args.shift_range_lon * shift_u / mpp, args.shift_range_lat * shift_v / mpp], -1)      # [B,2]  295-297
    k = args.rotation_range / 180 * np.pi
    ang = heading * k
    c, s = torch.cos(ang), torch.sin(ang)
    R = torch.cat([c, -s, s, c], -1).view(B, 2, 2)                                      # 302
    i = torch.arange(A)
    vv, uu = torch.meshgrid(i, i, indexing='ij')
    uv2 = torch.stack([uu, vv], -1).to(dt) - A / 2                                      # [A,A,2]  304-307
    uv = torch.einsum('bij,hwj->bhwi', R, uv2) + T[:, None, None, :] + A / 2            # 309-312
    one = torch.ones(B, 1, 1, 1, dtype=dt)
    du = (-args.shift_range_lon / mpp) * torch.tensor([1.0, 0.0], dtype=dt) * one.expand(B, A, A, 1)
    dv = (args.shift_range_lat / mpp) * torch.tensor([0.0, 1.0], dtype=dt) * one.expand(B, A, A, 1)
    dR = k * torch.cat([-s, -c, c, -s], -1).view(B, 2, 2)                               # 321-322
    dth = torch.einsum('bij,hwj->bhwi', dR, uv2)
    return uv, (du, dv, dth)


def lm_step(args, damping, su, sv, th, grd_feat, sat_feat):
    """One level of one iteration (models_kitti.py:455-466 with proj == 'nn', using_weight == 0)."""
    A = sat_feat.shape[-1]
    uv, jac = inplane_pose_to_uv(args, A, su, sv, th)
    f, new_jac = O.grid_sample(grd_feat, uv, torch.stack(jac, 0))
    return O.lm_update_g2s(args, damping, su, sv, th, f, None, sat_feat, new_jac, 0)


def solve(args, damping, sat_feats, grd_feats, n_iters, pose0=None):
    """The pose loop on given (normalised) NCHW maps -> trace [B,n_iters,L,3] = (shift_u, shift_v, heading)."""
    B, dt = sat_feats[0].shape[0], sat_feats[0].dtype
    if pose0 is None:
        su, sv, th = (torch.zeros(B, 1, dtype=dt) for _ in range(3))
    else:
        su, sv, th = (pose0[:, i:i + 1].to(dt) for i in range(3))
    rows = []
    for _ in range(n_iters):
        row = []
        for l in range(len(sat_feats)):
            su, sv, th = lm_step(args, damping, su, sv, th, grd_feats[l], sat_feats[l])
            row.append(torch.cat([su, sv, th], -1))
        rows.append(torch.stack(row, 1))
    return torch.stack(rows, 1)


def normal_sums(args, su, sv, th, grd_feat, sat_feat):
    """The 12 sums of one step as hla_g2s_lm_solve reports them (normal_eq slots 2..13): H(6), J'f (3), J's (3)."""
    A = sat_feat.shape[-1]
    uv, jac = inplane_pose_to_uv(args, A, su, sv, th)
    f, J = O.grid_sample(grd_feat, uv, torch.stack(jac, 0))
    B = f.shape[0]
    Jb = J.flatten(2).permute(1, 2, 0)                  # [B,D,3]
    H = Jb.transpose(1, 2) @ Jb
    jf = (Jb.transpose(1, 2) @ f.reshape(B, -1, 1))[..., 0]
    js = (Jb.transpose(1, 2) @ sat_feat.reshape(B, -1, 1))[..., 0]
    return torch.cat([torch.stack([H[:, 0, 0], H[:, 0, 1], H[:, 0, 2], H[:, 1, 1], H[:, 1, 2], H[:, 2, 2]], -1), jf, js], -1)


class LM_G2SP_NN(torch.nn.Module):
    """LM_G2SP(args) with args.proj == 'nn' and using_weight == 0; same state-dict keys as the reference's."""

    def __init__(self, args):
        super().__init__()
        if args.using_weight:
            raise NotImplementedError('using_weight with proj=nn')
        self.args = args
        self.level = args.level
        self.N_iters = args.N_iters
        self.SatFeatureNet = O.VGGUnet(self.level)
        self.GrdFeatureNet = VGGUnet_G2S(self.level)
        self.damping = torch.nn.Parameter(args.damping * torch.ones(1, 3))
        self.trace = None

    def forward(self, sat_map, grd_img_left, left_camera_k=None, gt_shift_u=None, gt_shift_v=None, gt_heading=None,
                mode='train'):
        sat_feats, _ = self.SatFeatureNet(sat_map)
        grd_feats, grd_confs = self.GrdFeatureNet(grd_img_left)
        tr = solve(self.args, self.damping, sat_feats, grd_feats, self.N_iters)
        self.trace = tr
        shift_lons, shift_lats, thetas = tr[..., 0], tr[..., 1], tr[..., 2]
        if mode == 'train':
            a = self.args
            out = O.loss_func(shift_lats, shift_lons, thetas, gt_shift_v[:, 0], gt_shift_u[:, 0], gt_heading[:, 0],
                              a.coe_shift_lat, a.coe_shift_lon, a.coe_heading)
            return (*out, grd_confs)
        return shift_lats[:, -1, -1], shift_lons[:, -1, -1], thetas[:, -1, -1]
