"""CPU restatement of ``LM_G2SP.corr`` and its ``triplet_loss`` (models_kitti.py:501-595) in torch, at the dtype of its inputs
(fp64 for the reference, fp32 for the distance that sets the gates), with autograd for the gradients.

Per level: project the ground map at the zero pose (``oracle.ref_cpu.g2s_pose_to_uv`` + ``grid_sample``; the features are not
masked), centre-crop it with torchvision's rule, F.normalize it, correlate it with the satellite map at every shift (grouped
conv2d), divide by the root of the window energy (avg_pool2d with divisor_override=1, channel sum) clamped at 1e-6:
corr = 2 - 2 dot / D.  The loss takes corr at the rounded ground-truth shift as the positive."""
import numpy as np
import torch
import torch.nn.functional as F


def _mpp0():
    from oracle import ref_cpu as O
    return O.meter_per_pixel()


def level_mpp(level):
    """self.meters_per_pixel[level] = utils.get_meter_per_pixel() * 2^(3 - level): fixed per level."""
    return _mpp0() * 2 ** (3 - level)


def crop_plan(A, level, lat, lon):
    """(Hc, Wc, top, left): models_kitti.py:546-548 and torchvision's center_crop (round half to even, Python's round)."""
    mpp = level_mpp(level)
    Hc, Wc = int(A - lat * 2 / mpp), int(A - lon * 2 / mpp)
    if Hc < 1 or Wc < 1:
        raise ValueError('crop below one pixel')
    return Hc, Wc, int(round((A - Hc) / 2.0)), int(round((A - Wc) / 2.0))


def corr_from_crop(s, f, safe_clamp=False):
    """s [B,C,A,A] the (normalised) satellite map, f [B,C,Hc,Wc] the crop before F.normalize -> (corr, dot, E), each [B,Ny,Nx].
    ``safe_clamp``: D = sqrt(max(E, 1e-12)) -- the same VALUES as max(sqrt(E), 1e-6), with a zero instead of an infinite slope of
    the root at E = 0, so autograd gives 'no gradient through a clamped E' instead of NaN."""
    B, C, A, _ = s.shape
    Hc, Wc = f.shape[-2:]
    g = F.normalize(f.reshape(B, -1)).reshape(B, C, Hc, Wc)
    dot = F.conv2d(s.reshape(1, B * C, A, A), g, groups=B)[0]
    E = F.avg_pool2d(s.pow(2), (Hc, Wc), stride=1, divisor_override=1).sum(dim=1)
    if safe_clamp:
        D = torch.sqrt(torch.clamp(E, min=1e-12))
    else:
        D = torch.maximum(torch.sqrt(E), torch.ones_like(E) * 1e-6)
    return 2 - 2 * dot / D, dot, E


def corr_loops(s, f):
    """The same in four nested Python loops (for the smallest shapes only)."""
    B, C, A, _ = s.shape
    Hc, Wc = f.shape[-2:]
    Ny, Nx = A - Hc + 1, A - Wc + 1
    out = torch.zeros(B, Ny, Nx, dtype=s.dtype)
    for b in range(B):
        n = max(float(f[b].pow(2).sum().sqrt()), 1e-12)
        for dy in range(Ny):
            for dx in range(Nx):
                d = e = 0.0
                for y in range(Hc):
                    for x in range(Wc):
                        sv = s[b, :, y + dy, x + dx]
                        d += float((f[b, :, y, x] / n * sv).sum())
                        e += float((sv * sv).sum())
                out[b, dy, dx] = 2 - 2 * d / max(e ** 0.5, 1e-6)
    return out


def _wrap(i, n):
    """A Python index: [-n, n) wraps, anything else is out of range (None)."""
    i = int(i)
    if not -n <= i < n:
        return None
    return i + n if i < 0 else i


def gt_index(gt_u, gt_v, lat, lon, mpp, Ny, Nx):
    """models_kitti.py:587-588 in fp32: -> [(h, w) or None per sample]."""
    gu, gv = gt_u.float().reshape(-1), gt_v.float().reshape(-1)
    w = torch.round(Nx / 2 + gu * lon / mpp)
    h = torch.round(Ny / 2 - gv * lat / mpp)
    out = []
    for hh, ww in zip(h.tolist(), w.tolist()):
        hi, wi = _wrap(hh, Ny), _wrap(ww, Nx)
        out.append(None if hi is None or wi is None else (hi, wi))
    return out


def triplet_level(corr, gt_u, gt_v, lat, lon, mpp):
    """models_kitti.py:584-592 for one level; NaN where the reference's index raises."""
    B, Ny, Nx = corr.shape
    idx = gt_index(gt_u, gt_v, lat, lon, mpp, Ny, Nx)
    if any(i is None for i in idx):
        return torch.full((), float('nan'), dtype=corr.dtype)
    pos = torch.stack([corr[b, h, w] for b, (h, w) in enumerate(idx)])
    return torch.sum(torch.log(1 + torch.exp((pos.reshape(-1, 1, 1) - corr) * 10))) / (B * (Ny * Nx - 1))


def triplet_loss(corrs, gt_u, gt_v, lat, lon):
    return torch.stack([triplet_level(c, gt_u, gt_v, lat, lon, level_mpp(l)) for l, c in enumerate(corrs)]).sum()


def predict(corr, mpp):
    B, Ny, Nx = corr.shape
    idx = torch.argmin(corr.reshape(B, -1), dim=1)
    return (idx % Nx - Nx / 2) * mpp, -(idx // Nx - Ny / 2) * mpp, idx


def project_crop(args, grd_feat, K, A, level, ori_hw):
    """grd_feat [B,C,h,w] -> the centre crop [B,C,Hc,Wc] of its zero-pose projection onto the A x A plane, and the crop plan."""
    from oracle import ref_cpu as O
    B = grd_feat.shape[0]
    dt = grd_feat.dtype
    z = torch.zeros(B, 1, dtype=dt)
    h, w = grd_feat.shape[-2:]
    uv, _, _ = O.g2s_pose_to_uv(args, A, z, z, z, K, h, w, ori_hw[0], ori_hw[1], require_jac=False)
    proj = O.grid_sample(grd_feat, uv)[0]
    Hc, Wc, top, left = plan = crop_plan(A, level, args.shift_range_lat, args.shift_range_lon)
    return proj[:, :, top:top + Hc, left:left + Wc], plan, uv[:, top:top + Hc, left:left + Wc]


def compose(args, sat_feats, grd_feats, K, ori_hw, safe_clamp=True):
    """Every level: -> [corr [B,Ny,Nx]] at the dtype of the maps (normalised NCHW lists of the oracle's extractors)."""
    out = []
    for l, (s, g) in enumerate(zip(sat_feats, grd_feats)):
        crop, _, _ = project_crop(args, g, K, s.shape[-1], l, ori_hw)
        out.append(corr_from_crop(s, crop, safe_clamp)[0])
    return out


# ---- direct sums at single entries, for shapes where the dense reference is not affordable (all fp64 numpy, NHWC) ----
def dot_at(s, g, dy, dx):
    """s [A,A,C], g [Hc,Wc,C] (already normalised) -> (dot, E) at shift (dy, dx)."""
    Hc, Wc, _ = g.shape
    win = s[dy:dy + Hc, dx:dx + Wc]
    return float((win * g).sum()), float((win * win).sum())


def d_g_at(s, ddot, y, x, c):
    """d_g[y,x,c] = sum_{dy,dx} ddot[dy,dx] s[y+dy,x+dx,c]."""
    Ny, Nx = ddot.shape
    return float((ddot * s[y:y + Ny, x:x + Nx, c]).sum())


def d_sat_conv_at(g, ddot, r, x, c):
    """sum_{dy,dx} ddot[dy,dx] g[r-dy,x-dx,c] with g zero outside."""
    Ny, Nx = ddot.shape
    Hc, Wc, _ = g.shape
    t = 0.0
    for dy in range(max(0, r - Hc + 1), min(Ny - 1, r) + 1):
        lo, hi = max(0, x - Wc + 1), min(Nx - 1, x)
        if lo <= hi:
            dxs = np.arange(lo, hi + 1)
            t += float((ddot[dy, dxs] * g[r - dy, x - dxs, c]).sum())
    return t
