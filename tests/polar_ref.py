"""fp64-capable restatements of the reference's "polar" family.  (1) ``proj='polar'`` for ``LM_S2GP`` / ``LM_S2GP_Ford`` (models_kitti.py:626-633, 684-698, 1194-1205;
models_ford.py:54-58, 157-171, 738-749), built from the pieces of ``oracle.ref_cpu``: the oracle's models already hand the whole
map to the updater for any ``args.proj`` other than 'geo' (``_S2GPBase._step``), so all that is restated here is the table --
``grd_img2cam_polar`` with its all-ones mask.  ``tests/test_polar_cpu.py`` pins it, run in fp32, to the REAL reference's recorded
fp32 results (tools/make_golden_polar.py).  (2) ``LM_S2GP.orien_corr`` (further down): the reference's function in plain
tensor ops on ``O.grid_sample``, with ``triplet_loss``."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O


def polar_points(grd_H, grd_W):
    """grd_img2cam_polar: a 45-degree fan of 30 m on the plane y = camera height.  fp32 like the reference's table (it stays fp32
    in an fp64 run).  Returns (xyz [1,h,w,3], mask [1,h,w] of ones)."""
    v, u = torch.meshgrid(torch.arange(0, grd_H, dtype=torch.float32), torch.arange(0, grd_W, dtype=torch.float32), indexing='ij')
    theta = u / grd_W * np.pi / 4
    radius = (1 - v / grd_H) * 30
    z = radius * torch.cos(np.pi / 4 - theta)
    x = -radius * torch.sin(np.pi / 4 - theta)
    y = O.CAMERA_HEIGHT * torch.ones_like(z)
    return torch.stack([x, y, z], dim=-1).unsqueeze(0), torch.ones_like(z).unsqueeze(0)


def _polar_tables(net, grd_hw):
    assert net.args.proj == 'polar' and net.level in (3, 4), 'level 2 (Ford) keeps the ground-plane tables'
    net.xyz_grds = [polar_points(grd_hw[0] / 2 ** (3 - l), grd_hw[1] / 2 ** (3 - l)) for l in range(4)]


class LM_S2GP_Polar(O.LM_S2GP):
    def __init__(self, args, grd_hw=(256, 1024)):
        super().__init__(args, grd_hw=grd_hw)
        _polar_tables(self, grd_hw)


class LM_S2GP_Ford_Polar(O.LM_S2GP_Ford):
    def __init__(self, args, grd_hw=(256, 1024)):
        super().__init__(args, grd_hw=grd_hw)
        _polar_tables(self, grd_hw)


def build(kind, args, seed, dtype=torch.float32, bias_scale=0.0, grd_hw=(256, 1024)):
    """``oracle.ref_cpu.build`` for the polar models (same portable synthetic weights)."""
    net = {'kitti': LM_S2GP_Polar, 'ford': LM_S2GP_Ford_Polar}[kind](args, grd_hw=grd_hw)
    net.load_state_dict(O.synth_model_state(seed, bias_scale, rotation_range=(10.0 if kind == 'ford' else args.rotation_range)))
    return net.to(dtype)


def normal_eq(onet, sat, grd, conf, pose, level, using_weight, extra=None, keep=None):
    """The 14 sums of one step over the WHOLE level map, from the oracle's own projection: S, G, H(6), U(3), V(3)
    (what hla_s2g_lm_solve reports in normal_eq slots 0..13).  ``keep`` [h*w] bool: args.dropout's pixel subset of the step (a
    dropped pixel leaves every sum, models_kitti.py:968-974)."""
    su, sv, th = pose
    dt = su.dtype
    f, _, jac, _, mask = onet.project_map_to_grd(sat[level].to(dt), None, su, sv, th, level, extra)
    g = grd[level].to(dt) * mask[:, None]
    w = conf[level].to(dt) * mask[:, None] if using_weight else torch.ones_like(g[:, :1])
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


# ----------------------------------------------------------------------------------------------------------------------
# LM_S2GP.orien_corr (models_kitti.py:1518-1624): the coarse heading search
# ----------------------------------------------------------------------------------------------------------------------
def polar_grid(level):
    """polar_coordinates (models_kitti.py:1518-1541): [1, A//2, 8A, 2] fp32 coordinates into the level's A x A satellite map,
    A = 512 / 2^(3-level); range 40 m at the top row, one turn per 2A columns."""
    mpp = O.meter_per_pixel() * (2 ** (3 - level))
    A = 512 / 2 ** (3 - level)
    H, W = A // 2, A * 2
    v, u = torch.meshgrid(torch.arange(0, H, dtype=torch.float32), torch.arange(0, 4 * W, dtype=torch.float32), indexing='ij')
    theta = u / W * np.pi * 2
    radius = (1 - v / H) * 40 / mpp
    return torch.stack([A / 2 + radius * torch.cos(np.pi / 4 - theta), A / 2 - radius * torch.sin(np.pi / 4 - theta)], -1).unsqueeze(0)


def polar_window(P, W, n):
    """polar_sat1 of models_kitti.py:1582-1585 (the slices clamp like Python's: n = 0 takes the whole map in front)."""
    sat_W = P.shape[-1]
    if sat_W - W < n:
        return torch.cat([P[..., -n:], P, P[..., :n - sat_W + W]], -1)
    return torch.cat([P[..., -n:], P[..., :W + n]], -1)


def orien_corr_level(sat_feat, grd_feat, level, rotation_range):
    """One level of orien_corr (1569-1599) on NCHW maps of any float dtype -> (corr [B,S], degree_per_pixel, n, P1, g).  The grid
    keeps its fp32 VALUES (it is an fp32 table in the reference, also in an fp64 run); the arithmetic is the maps' dtype."""
    B, C, H, W = grd_feat.shape
    g = F.normalize(grd_feat.reshape(B, -1)).reshape(B, -1, H, W)
    P, _ = O.grid_sample(sat_feat, polar_grid(level).to(sat_feat.dtype).repeat(B, 1, 1, 1))
    deg = 90 / W
    n = int(np.ceil(rotation_range / deg))
    P1 = polar_window(P, W, n)
    return corr_from_window(P1, grd_feat), deg, n, P1, g


def corr_from_window(P1, grd_feat, safe_clamp=False):
    """models_kitti.py:1572, 1588-1594 on a given window P1 [B,C,H,W+S-1] -> corr [B,S].  ``safe_clamp``: the same VALUES with the
    clamp max(sqrt(E), 1e-6) written so that autograd sends no gradient through a clamped E (the reference's own graph gives
    0 * inf = NaN for E == 0; the product defines that gradient as zero)."""
    B, C, H, W = grd_feat.shape
    g = F.normalize(grd_feat.reshape(B, -1)).reshape(B, -1, H, W)
    dot = F.conv2d(P1.reshape(1, B * C, H, -1), g, groups=B)[0, :, 0, :]
    E = F.avg_pool2d(P1.pow(2), (H, W), stride=1, divisor_override=1)[:, :, 0, :].sum(1)
    if safe_clamp:
        live = E > 1e-12
        den = torch.where(live, torch.sqrt(torch.where(live, E, torch.ones_like(E))), torch.full_like(E, 1e-6))
    else:
        den = torch.maximum(torch.sqrt(E), torch.ones_like(E) * 1e-6)
    return 2 - 2 * dot / den


def triplet_loss(corr_list, gt_heading, rotation_range):
    """models_kitti.py:1607-1624; corr_list = [(corr [B,S], degree_per_pixel)]."""
    gt = gt_heading * rotation_range
    losses = []
    for corr, deg in corr_list:
        B, S = corr.shape
        idx = ((S - 1) / 2 + torch.round(gt[:, 0].float() / deg)).long()
        pos = corr[range(B), idx]
        losses.append(torch.sum(torch.log(1 + torch.exp((pos[:, None] - corr) * 10))) / (B * (S - 1)))
    return torch.sum(torch.stack(losses, 0))


def orien_corr(net, sat_map, grd_img, gt_heading=None, mode='train'):
    """LM_S2GP.orien_corr on an oracle model (its two extractors) -> (loss or the last level's heading [B], corr_list)."""
    sat_feats, _ = net.SatFeatureNet(sat_map)
    grd_feats, _ = net.GrdFeatureNet(grd_img)
    corr_list = []
    for l in range(len(sat_feats)):
        corr, deg, n, _, _ = orien_corr_level(sat_feats[l], grd_feats[l], l, net.args.rotation_range)
        corr_list.append((corr, deg))
    if mode == 'train':
        return triplet_loss(corr_list, gt_heading, net.args.rotation_range), corr_list
    return (torch.argmin(corr, dim=-1) - n) * deg, corr_list
