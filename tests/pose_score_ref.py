"""fp64-capable reference of ``hla_s2g_pose_score`` (include/hla.h): the LM objective at K candidate poses per sample, on one
level with free geometry.  Built on ``lm_kernel_ref.level_uv`` (the oracle's projections) and ``lm_kernel_ref._operands`` (the
oracle's sampling and masks); runs in the dtype of its inputs, so the same code on fp32 inputs is the "ref32" that sizes gates.

``O.grid_sample`` asserts when no pixel of its batch is in view (jacobian.py:172), so every hypothesis is evaluated in a batch
that also holds the samples at ``guard_pose`` (in view by construction of the caller's level); the guard rows are dropped."""
import numpy as np
import torch

import lm_kernel_ref as R

N_SUMS = 6        # sum s^2, sum g^2, sum s g, sum w s^2, sum w g^2, sum w s g


def _twice(geom, lv):
    """geom and level with every sample twice (the second copy is evaluated at the guard pose)."""
    from types import SimpleNamespace
    g = SimpleNamespace(**vars(geom))
    if geom.ford:
        g.R_FL, g.T_FL = torch.cat([geom.R_FL, geom.R_FL]), torch.cat([geom.T_FL, geom.T_FL])
    o = SimpleNamespace(**vars(lv))
    o.sat, o.grd, o.conf = torch.cat([lv.sat, lv.sat]), torch.cat([lv.grd, lv.grd]), torch.cat([lv.conf, lv.conf])
    return g, o


def cost_from_sums(sums):
    """The kernel's closing formula on [..., >= 6] sums, in their dtype."""
    ns = torch.clamp(torch.sqrt(sums[..., 0]), min=1e-6)
    ng = torch.clamp(torch.sqrt(sums[..., 1]), min=1e-6)
    return sums[..., 3] / (ns * ns) + sums[..., 4] / (ng * ng) - 2 * sums[..., 5] / (ns * ng)


def score(geom, lv, poses, using_weight, guard_pose=(0.0, 0.0, 0.0)):
    """geom / lv as in lm_kernel_ref (maps in dtype dt); poses [B,K,3] (any float dtype, used in dt).
    -> sums [B,K,6] dt, mags [B,K,6] fp64 (sums of the absolute values of the terms), counts [B,K,2] int64 (ground mask AND in
    view, ground mask; rows row0.. only), cost [B,K] dt by the kernel's formula, direct [B,K] dt = sum w (s/ns - g/ng)^2."""
    dt = lv.sat.dtype
    B, K = poses.shape[:2]
    g2, lv2 = _twice(geom, lv)
    guard = torch.tensor([guard_pose], dtype=dt).expand(B, 3)
    out = [[] for _ in range(4)]
    for k in range(K):
        pose = R.pose_cols(torch.cat([poses[:, k].to(dt), guard]), dt)
        uv, jac, mask = R.level_uv(g2, lv2, pose)
        f, g, gc, _ = R._operands(lv2.sat, lv2.grd, lv2.conf if using_weight else None, uv, jac, mask, lv.row0, None)
        f, g, gc, uv = f[:B], g[:B], gc[:B], uv[:B, lv.row0:]
        s_, g_ = f.reshape(B, -1), g.reshape(B, -1)
        W = gc.expand(-1, f.shape[1], -1, -1).reshape(B, -1)      # conf x mask, or the mask
        terms = [s_ * s_, g_ * g_, s_ * g_, W * s_ * s_, W * g_ * g_, W * s_ * g_]
        sums = torch.stack([t.sum(1) for t in terms], 1)
        out[0].append(sums)
        out[1].append(torch.stack([t.abs().double().sum(1) for t in terms], 1))
        u, v = uv[..., 0], uv[..., 1]
        m = mask.expand(B, -1, -1)[:, lv.row0:] > 0
        inb = (u >= 0) & (u <= lv.A - 1) & (v >= 0) & (v <= lv.A - 1)
        out[2].append(torch.stack([(inb & m).reshape(B, -1).sum(1), m.reshape(B, -1).sum(1)], 1))
        ns = torch.clamp(torch.sqrt(sums[:, 0]), min=1e-6)[:, None]
        ng = torch.clamp(torch.sqrt(sums[:, 1]), min=1e-6)[:, None]
        out[3].append((W * (s_ / ns - g_ / ng) ** 2).sum(1))
    sums, mags, counts, direct = [torch.stack(o, 1) for o in out]
    return sums, mags, counts, cost_from_sums(sums), direct


def hypotheses(B, K, seed, out_of_view=None, lim=0.3):
    """[B,K,3] fp32 random poses in [-lim, lim]; hypothesis 0 is the zero pose, hypothesis ``out_of_view`` (if given) is
    lm_kernel_ref.OUT_OF_VIEW_POSE for every sample."""
    p = np.random.RandomState(seed).uniform(-lim, lim, size=(B, K, 3)).astype(np.float32)
    p[:, 0] = 0
    if out_of_view is not None:
        p[:, out_of_view] = R.OUT_OF_VIEW_POSE
    return torch.from_numpy(p)


# (ford, shape, C, A, B, using_weight) of the cases tests/test_pose_score_gpu.py runs in fp32 that are not in its C x dtype x weight grid
GPU_CASES = [(1, 'ragged', 64, 16, 3, 0), (0, 'ragged', 64, 13, 3, 1), (1, 'ragged', 64, 13, 3, 0), (1, 'ragged', 64, 16, 3, 1),
             (0, 'sub_tile', 256, 16, 1, 1), (0, 'skip', 128, 16, 2, 1), (0, 'mid', 64, 16, 2, 0), (1, 'mid', 16, 16, 2, 1),
             (0, 'many', 16, 16, 2, 0), (0, 'ragged', 64, 16, 9, 1)]
K_CASE = 7                # hypotheses of those cases; hypothesis 3 is out of view
OUT_K = 3


# hypotheses of the planted-minimum cases: at least 0.25 x 6 m = 3 satellite pixels apart in shift, so that no wrong one samples
# the texels the true one (hypothesis 2) does; hypothesis 3 is out of view
PLANTED_POSES = [(0.0, 0.0, 0.0), (0.25, 0.0, 0.0), (-0.125, 0.25, 0.1), R.OUT_OF_VIEW_POSE, (0.0, -0.25, 0.0), (0.25, 0.25, -0.2),
                 (-0.25, -0.25, 0.2)]


def planted_poses(B):
    return torch.tensor(PLANTED_POSES, dtype=torch.float32)[None].repeat(B, 1, 1)


def planted_level(ford, shape, C, A, B, seed, k_true, poses):
    """A level whose ground map IS the satellite map sampled (fp64) at hypothesis ``k_true``'s pose, masked like the kernel's s:
    that hypothesis' cost is 0 up to rounding.  -> (geom, level with fp32 maps)."""
    geom, lv = R.make_geom(ford, B), R.make_level(ford, shape, C, A, B, seed)
    l64, g64 = R.cast_level(lv, torch.float64), R.cast_geom(geom, torch.float64)
    g2, lv2 = _twice(g64, l64)
    pose = R.pose_cols(torch.cat([poses[:, k_true].double(), torch.zeros(B, 3, dtype=torch.float64)]), torch.float64)
    uv, jac, mask = R.level_uv(g2, lv2, pose)
    f, _, _, _ = R._operands(lv2.sat, lv2.grd, None, uv, jac, mask, 0, None)
    lv.grd = f[:B].float().contiguous()
    lv.grd[:, :, :lv.skip] = 0
    return geom, lv
