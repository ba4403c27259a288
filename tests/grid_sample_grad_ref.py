"""Shared by tests/test_grid_sample_grad_{cpu,gpu}.py and tools/make_golden_grid_sample_grad.py: the cases of the
``jacobian.grid_sample`` gradient tests (inputs from ``numpy.random.RandomState``), the yardstick (autograd through
``oracle.ref_cpu.grid_sample`` on the CPU, in fp64 and in fp32) and the gate.  Not a test module."""
import functools

import numpy as np
import torch

from oracle import ref_cpu as O

#        N,  C, IH, IW,  H,  W, M (None: jac=None)
CASES = {'S1': (2, 5, 7, 9, 6, 11, 3),         # scalar channel path, odd sizes, per-sample strides
         'S2': (2, 64, 18, 18, 9, 20, 3),      # 64-lane path, pixel count not a multiple of the tile
         'S3': (1, 256, 6, 5, 3, 7, 4),        # four channels per lane, M != 3
         'S4': (3, 16, 10, 12, 5, 13, 1),      # four pixels per wave, last wave partial
         'S5': (2, 1, 33, 17, 16, 70, None),   # C = 1, no Jacobian
         'S6': (1, 64, 6, 8, 16, 16, 3)}       # every sample inside one texel cell: 256 colliding adds per texel
SEEDS = {k: 100 + i for i, k in enumerate(CASES)}
FLOOR = 2.4e-7          # 2 ulp (2 * 2^-23) of the largest element


def planted(IH, IW):
    return np.array([[IW - 1, 2.5], [3, IH - 1], [0, 0], [2, 3], [IW - 1.5, IH - 1.25]], np.float32)


def make_case(name):
    """fp32 numpy arrays: img [N,C,IH,IW], uv [N,H,W,2], jac [M,N,H,W,2] or None, and the cotangents g_out [N,C,H,W],
    g_jac [M,N,C,H,W] or None."""
    N, C, IH, IW, H, W, M = CASES[name]
    rs = np.random.RandomState(SEEDS[name])
    img = rs.standard_normal((N, C, IH, IW)).astype(np.float32)
    if name == 'S6':
        uv = np.stack([rs.uniform(3, 4, (N, H, W)), rs.uniform(2, 3, (N, H, W))], -1).astype(np.float32)
    else:
        uv = np.stack([rs.uniform(-1.5, IW + 0.5, (N, H, W)), rs.uniform(-1.5, IH + 0.5, (N, H, W))], -1).astype(np.float32)
        uv[0].reshape(-1, 2)[:5] = planted(IH, IW)
    jac = rs.standard_normal((M, N, H, W, 2)).astype(np.float32) if M else None
    g_out = rs.standard_normal((N, C, H, W)).astype(np.float32)
    g_jac = rs.standard_normal((M, N, C, H, W)).astype(np.float32) if M else None
    return img, uv, jac, g_out, g_jac


def T(a, dtype=None, device=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dtype, device=device)


def linear_loss(g_out, g_jac, use=('out', 'jac_out')):
    def loss(out, jout):
        parts = []
        if 'out' in use:
            parts.append((out * g_out.to(out)).sum())
        if 'jac_out' in use and jout is not None:
            parts.append((jout * g_jac.to(jout)).sum())
        return sum(parts)
    return loss


def grads(fn, img, uv, jac, loss, need=(True, True, True)):
    """Gradients of loss(*fn(img, uv, jac)) with respect to the inputs flagged in ``need`` (None for the others)."""
    leaves = [t.detach().requires_grad_(n) if t is not None else None for t, n in zip((img, uv, jac), need)]
    loss(*fn(*leaves)).backward()
    return [None if t is None else t.grad for t in leaves]


def oracle_grads(name, dtype, use=('out', 'jac_out')):
    img, uv, jac, g_out, g_jac = (T(a, dtype) for a in make_case(name))
    return grads(O.grid_sample, img, uv, jac, linear_loss(g_out, g_jac, use))


@functools.lru_cache(maxsize=None)
def oracle_pair(name, use=('out', 'jac_out')):
    """(fp64, fp32) oracle gradients of a case, computed once and shared (treat as read-only)."""
    return oracle_grads(name, torch.float64, use), oracle_grads(name, torch.float32, use)


def ratio(got, ref64, ref32):
    """|got - ref64| / max(4 |ref32 - ref64|, FLOOR max|ref64|) in max-norm: the gate is ratio <= 1.  Also returns the error in
    units of the oracle's own fp32 gap."""
    ref64 = ref64.double().cpu()
    err = (got.detach().double().cpu() - ref64).abs().max().item()
    gap = (ref32.double().cpu() - ref64).abs().max().item()
    bound = max(4 * gap, FLOOR * ref64.abs().max().item())
    return err / bound if bound > 0 else (0.0 if err == 0 else float('inf')), err / gap if gap > 0 else float('nan')


def check(tag, got, ref64, ref32):
    names = ('d_image', 'd_optical', 'd_jac')
    worst = 0.0
    for n, g, r64, r32 in zip(names, got, ref64, ref32):
        if r64 is None:
            assert g is None, f'{tag} {n}: expected None'
            continue
        assert g is not None, f'{tag} {n}: gradient missing'
        assert g.shape == r64.shape, (tag, n, g.shape, r64.shape)
        r, x = ratio(g, r64, r32)
        print(f'{tag} {n}: {x:.2f} x the oracle fp32 gap, {r:.3f} of the gate')
        worst = max(worst, r)
    assert worst <= 1.0, f'{tag}: {worst:.3f} of the gate'


def gn_loss(fn, ghat, cvec):
    """One damped Gauss-Newton step on the operator's outputs, per sample: s = out/|out|, J = jac_out/|out|, r = s - ghat,
    delta = -(J^T J + 0.1 I)^-1 J^T r; loss = sum delta . c."""
    def loss(out, jout):
        N, M = out.shape[0], jout.shape[0]
        s = out.reshape(N, -1)
        nrm = s.norm(dim=1, keepdim=True)
        J = jout.permute(1, 0, 2, 3, 4).reshape(N, M, -1).transpose(1, 2) / nrm[:, :, None]       # [N,P,M]
        r = s / nrm - ghat.to(s)
        A = J.transpose(1, 2) @ J + 0.1 * torch.eye(M, dtype=s.dtype, device=s.device)
        delta = -torch.linalg.solve(A, (J.transpose(1, 2) @ r[:, :, None]))[:, :, 0]
        return (delta * cvec.to(s)).sum()
    return loss


def gt_depth_projection(fn, sat, pose, rays, depth, w_out, w_jac, A, rot_range=10.0, shift=1.0, mpp=1.0):
    """The ``use_gt_depth`` branch of the ground-to-satellite projection (models_kitti.py:741-748 with 719-737, 754-765):
    camera rays scaled by a depth map, rotated by the heading and shifted, mapped to satellite pixels, with the analytic
    Jacobian of the coordinates with respect to (shift_u, shift_v, heading); then the operator.  Returns a scalar loss."""
    su, sv, th = pose[:, 0:1] * shift, pose[:, 1:2] * shift, pose[:, 2:3] * (rot_range / 180 * np.pi)
    B = pose.shape[0]
    cos, sin, zero, one = torch.cos(th), torch.sin(th), torch.zeros_like(th), torch.ones_like(th)
    R = torch.cat([cos, zero, -sin, zero, one, zero, sin, zero, cos], -1).view(B, 3, 3)
    dR = (rot_range / 180 * np.pi) * torch.cat([-sin, zero, -cos, zero, zero, zero, cos, zero, -sin], -1).view(B, 3, 3)
    T0 = torch.cat([sv, 1.65 * one, -su], -1)
    xyz_grd = rays[None] * depth[..., None]                                                      # [B,H,W,3]
    xyz = (R[:, None, None] * xyz_grd[:, :, :, None, :]).sum(-1) - (R * T0[:, None, :]).sum(-1)[:, None, None, :]
    uv = torch.stack([xyz[..., 2], xyz[..., 0]], -1) / mpp + A / 2
    e_u = torch.tensor([0., 0., -1.], dtype=pose.dtype, device=pose.device) * shift
    e_v = torch.tensor([1., 0., 0.], dtype=pose.dtype, device=pose.device) * shift
    d_u = -(R * e_u).sum(-1)[:, None, None, :].expand_as(xyz)
    d_v = -(R * e_v).sum(-1)[:, None, None, :].expand_as(xyz)
    d_t = (dR[:, None, None] * xyz_grd[:, :, :, None, :]).sum(-1) - (dR * T0[:, None, :]).sum(-1)[:, None, None, :]
    jac = torch.stack([torch.stack([d[..., 2], d[..., 0]], -1) / mpp for d in (d_u, d_v, d_t)], 0)      # [3,B,H,W,2]
    out, jout = fn(sat, uv, jac)
    return (out * w_out.to(out)).sum() + (jout * w_jac.to(out)).sum()
