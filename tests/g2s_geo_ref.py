"""fp64 reference of ONE step of the ground -> satellite LM loop (``LM_G2SP``, proj == 'geo') with free geometry: per-sample
intrinsics with skew entries, an ``ori_hw`` the map sizes do not divide, any (A, C, h, w) -- built from
``oracle.ref_cpu.g2s_pose_to_uv``, ``grid_sample`` and ``lm_update_g2s`` (none of them restated) -- and the input cases of
tests/test_g2s_kernels_vs_fp64.py.  tests/test_g2s_geo_ref_cpu.py pins the reference to ``lm_update_g2s`` and asserts, on the
reference alone, every property a case exists for; the GPU module imports the same builders, so both see the same inputs."""
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ref_cpu as O

F64, F32 = torch.float64, torch.float32
ORI_HW = (251, 1003)                 # divides none of the ground-map sizes below
MAPS = ((12, 40), (20, 36), (9, 25))
NEAR = 2.0 ** -9                     # "at a border": within this many pixels of it
GUARD = 1e-6                         # no pixel closer than this to a texel line or a border (see pixel_classes)
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
DPARAM = [[0.4, 0.7, 0.55]]          # lambda of every case (the value test_g2s_lm_backward_small_vs_oracle_autograd uses)


def pick_tile(npix):
    """lm_pick_tile (csrc/lm_common.h), restated."""
    return 256 if npix >= 16384 else (128 if npix >= 4096 else 64)


def tiles(A):
    """-> (pixels per tile, tiles per sample, pixels in the last tile)."""
    tp = pick_tile(A * A)
    nt = (A * A + tp - 1) // tp
    return tp, nt, A * A - (nt - 1) * tp


def make_args(ranges=(20.0, 20.0, 10.0), **kw):
    """(shift_range_lat, shift_range_lon, rotation_range); lambda is always the damping parameter handed to ``step``."""
    return O.default_args(shift_range_lat=ranges[0], shift_range_lon=ranges[1], rotation_range=ranges[2], train_damping=1, **kw)


def cols(pose, dt=F64):
    return tuple(pose[:, i:i + 1].to(dt) for i in range(3))


def project(args, pose, grd, conf, A, K, ori_hw, using_weight):
    """project_grd_to_map (models_kitti.py:163-303): -> projected features [B,C,A,A], projected confidence or None, Jacobian
    [3,B,C,A,A].  ``pose`` = (su, sv, th), each [B,1]; ``K`` [B,3,3] in the ORIGINAL image's pixels."""
    h, w = grd.shape[-2:]
    uv, jac, _ = O.g2s_pose_to_uv(args, A, *pose, K, h, w, *ori_hw)
    f, J = O.grid_sample(grd, uv, torch.stack(jac, 0))
    c = O.grid_sample(conf, uv)[0] if using_weight else None
    return f, c, J


def sums_of(f, c, J, sat):
    """Projected features f [B,C,A,A], weight c [B,1,A,A] or None, Jacobian J [3,B,C,A,A], satellite map -> (sums [B,12], T [B,12]):
    H(6), J'W f (3), J'W s (3) and, for each, the sum of the absolute values of its terms."""
    B = f.shape[0]
    Jb = J.flatten(2)                                               # [3,B,D]
    JW = Jb * c.expand_as(f).reshape(1, B, -1) if c is not None else Jb
    fs = (f.reshape(B, -1), sat.reshape(B, -1))
    terms = [JW[i] * Jb[j] for i, j in PAIRS] + [JW[i] * t for t in fs for i in range(3)]
    return torch.stack([t.sum(1) for t in terms], 1), torch.stack([t.abs().sum(1) for t in terms], 1)


def normal_sums(args, su, sv, th, grd, conf, sat, K, ori_hw, using_weight):
    """The 12 sums in the order hla_g2s_lm_solve writes them to normal_eq[2..13] -- H(6), J'W f (3), J'W s (3) -- and T_k, the
    sum of the absolute values of each sum's terms.  -> (sums [B,12], mags [B,12]) in the maps' dtype."""
    f, c, J = project(args, (su, sv, th), grd, conf, sat.shape[-1], K, ori_hw, using_weight)
    return sums_of(f, c, J, sat)


def delta_from_sums(sums, lam):
    """delta = -(H + lam I)^-1 (J'W f - J'W s) from the 12 sums (models_kitti.py:357-372)."""
    B = sums.shape[0]
    H = sums.new_zeros(B, 3, 3)
    for k, (i, j) in enumerate(PAIRS):
        H[:, i, j] = H[:, j, i] = sums[:, k]
    g = (sums[:, 6:9] - sums[:, 9:12]).unsqueeze(-1)
    return -(torch.inverse(H + lam.to(sums.dtype) * torch.eye(3, dtype=sums.dtype)) @ g)[..., 0]


def step(args, lam, pose, grd, conf, sat, K, ori_hw, using_weight):
    """One level of one iteration: (su, sv, th) -> (su, sv, th).  ``lam`` [1,3]."""
    f, c, J = project(args, pose, grd, conf, sat.shape[-1], K, ori_hw, using_weight)
    return O.lm_update_g2s(args, lam, *pose, f, c, sat, J, using_weight)


def solve(args, lam, sat, grd, conf, K, ori_hw, n_iters, using_weight, pose0=None):
    """The pose loop on given NCHW maps -> trace [B,n_iters,L,3] = (shift_u, shift_v, heading).  With requires_grad leaves
    (maps, lam) this is the autograd-able loop of the gradient tests."""
    B, dt = sat[0].shape[0], sat[0].dtype
    pose = cols(torch.zeros(B, 3) if pose0 is None else pose0, dt)
    rows = []
    for _ in range(n_iters):
        row = []
        for l in range(len(sat)):
            pose = step(args, lam, pose, grd[l], conf[l], sat[l], K, ori_hw, using_weight)
            row.append(torch.cat(pose, -1))
        rows.append(torch.stack(row, 1))
    return torch.stack(rows, 1)


def pixel_classes(args, su, sv, th, K, A, hw, ori_hw):
    """Where the A x A satellite pixels land in an (h, w) ground map, per sample (fp64):
      inb      pixels in bounds;   behind  ... of them with z <= 1e-6 (sampled, Jacobian forced to zero);
      edge     ... in a first or last cell of a row or column (x0 in {0, w-2}, y0 in {0, h-2}; where x1 / y1 would clamp);
      last     ... in the last tile of the sample (pixels (nt-1) TP and up; ``tiles``);
      near     [8] counts within NEAR of u = 0, u = w-1, v = 0, v = h-1, (inside, outside) each, the other coordinate in range;
      min_dist how far the closest pixel is from changing its cell or its in-bounds decision: for a pixel in bounds the distance
               of u and v to the nearest texel line (the borders are texel lines), for a pixel out of bounds its largest border
               violation.  u == 0 or v == 0 EXACTLY (q0 == 0 / q1 == 0: the quotient is exact on both sides) is not counted."""
    h, w = hw
    uv, _, mask = O.g2s_pose_to_uv(args, A, su.double(), sv.double(), th.double(), K, h, w, *ori_hw, require_jac=False)
    B = uv.shape[0]
    u, v = uv[..., 0].reshape(B, -1), uv[..., 1].reshape(B, -1)
    front = mask.reshape(B, -1)
    inu, inv = (u >= 0) & (u <= w - 1), (v >= 0) & (v <= h - 1)
    inb = inu & inv
    x0, y0 = torch.floor(u), torch.floor(v)
    edge = inb & ((x0 <= 0) | (x0 >= w - 2) | (y0 <= 0) | (y0 >= h - 2))
    inf = torch.full_like(u, float('inf'))
    du = torch.where(u == 0, inf, (u - torch.round(u)).abs())
    dv = torch.where(v == 0, inf, (v - torch.round(v)).abs())
    viol = torch.stack([-u, u - (w - 1), -v, v - (h - 1)], 0).max(0)[0]
    dist = torch.where(inb, torch.minimum(du, dv), viol)
    near = []
    for x, lim, other in ((u, 0.0, inv), (u, w - 1.0, inv), (v, 0.0, inu), (v, h - 1.0, inu)):
        sgn = 1.0 if lim == 0.0 else -1.0                        # inside is x > 0 at the near border, x < lim at the far one
        d = (x - lim) * sgn
        near += [((d > 0) & (d <= NEAR) & other).sum(1), ((d < 0) & (d >= -NEAR) & other).sum(1)]
    tp, nt, _ = tiles(A)
    return SimpleNamespace(inb=inb.sum(1), behind=(inb & ~front).sum(1), edge=edge.sum(1), last=inb[:, (nt - 1) * tp:].sum(1), near=torch.stack(near, 1),
                           min_dist=dist.min(1)[0], npix=A * A)


# ----------------------------------------------------------------------------------------------------------------------
# intrinsics
# ----------------------------------------------------------------------------------------------------------------------
def ordinary_K(rs, B):
    """Per-sample intrinsics in the original image's pixels: every entry its own, skew entries and a perturbed third row.
    Sample 0 has a short focal length: its view is wide enough to hold the far corner of the satellite map, i.e. the pixels of the
    ragged last tile (with fx of 450 and more that tile would be all out of view and would contribute zeros)."""
    oh, ow = ORI_HW
    K = np.zeros((B, 3, 3))
    fx = rs.uniform(450, 650, B)
    fx[0] = rs.uniform(200, 300)
    K[:, 0] = np.stack([fx, rs.uniform(-15, 15, B), rs.uniform(0.42, 0.58, B) * ow], 1)
    K[:, 1] = np.stack([rs.uniform(-8, 8, B), rs.uniform(380, 560, B), rs.uniform(0.35, 0.5, B) * oh], 1)
    K[:, 2] = np.stack([rs.uniform(-0.03, 0.03, B), rs.uniform(-0.03, 0.03, B), rs.uniform(0.95, 1.05, B)], 1)
    return torch.from_numpy(K.astype(np.float32))


def _plain_K(rs):
    """One sample, zero skew K01 and the plain third row: at pose 0 a satellite pixel (v_c, u_c) has z = mpp u_c and
    u = fx' v_c / u_c + cx',  v = (K10' mpp v_c + 1.65 fy') / (mpp u_c) + cy'   (' = scaled to the ground map)."""
    K = ordinary_K(rs, 1)[0]
    K[0, 1] = 0.0
    K[2] = torch.tensor([0.0, 0.0, 1.0])
    return K


def border_K(rs, A, hw):
    """Eight samples, one per border side: u = 0, u = w-1, v = 0, v = h-1, each just inside and just outside (2^-10 px).
    u: the centre row (v_c = 0) projects to u = cx' for every pixel in front of the camera, so cx puts that whole row at the
    border.  v: cy solved for the one pixel (v_c, u_c) = (2, 4)."""
    h, w = hw
    oh, ow = ORI_HW
    eps = 2.0 ** -10
    mpp = O.meter_per_pixel() * O.SATMAP_PROCESS_SIDELENGTH / A
    Ks = []
    for side in range(8):
        K = _plain_K(rs)
        lim, off = ((0.0, eps), (0.0, -eps), (w - 1.0, -eps), (w - 1.0, eps), (0.0, eps), (0.0, -eps), (h - 1.0, -eps), (h - 1.0, eps))[side]
        if side < 4:
            K[0, 2] = (lim + off) * ow / w
        else:
            vc, uc = 2.0, 4.0
            rest = (float(K[1, 0]) * h / oh * mpp * vc + 1.65 * float(K[1, 1]) * h / oh) / (mpp * uc)
            K[1, 2] = (lim + off - rest) * oh / h
        Ks.append(K)
    return torch.stack(Ks)


def behind_K(rs):
    """K = [[fx, 0, 0], [K10, fy, 0], [0, 0, 1]] with a tiny fy, for shift_range_lat = 0: the camera stands on the centre pixel
    (X = 0, Z = -lon su from it), so for su >= 0 that pixel has z <= 1e-6 at any heading, q0 = 0 exactly (u = 0) and
    v = 1.65e6 fy' = 0.3792 h (4.55 of 12 rows, 7.58 of 20): in bounds and behind the camera.  Unlike a rotation centre it does
    depend on the pose (d z / d su = -lon), so a backward that forgot ``front`` would send its 1e12-scaled terms into d/d su."""
    K = _plain_K(rs)
    K[0, 2] = K[1, 2] = 0.0
    K[1, 0] = 100.0
    K[1, 1] = 0.4137 * ORI_HW[0] / 1.65e6 * (1 - 1.0 / 12)
    return K


def out_of_view_K(rs):
    K = _plain_K(rs)
    K[0, 2] = -1.0e5
    return K


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def _maps(rs, B, levels):
    T = lambda a: torch.from_numpy(a.astype(np.float32))
    sat = [T(rs.standard_normal((B, C, A, A)) * 0.02) for A, C, _ in levels]
    grd = [T(rs.standard_normal((B, C, h, w)) * 0.02) for _, C, (h, w) in levels]
    conf = [T(rs.uniform(0.27, 0.5, size=(B, 1, h, w))) for _, _, (h, w) in levels]
    return sat, grd, conf


def _case(name, levels, B, K, N, p0=None, ranges=(20.0, 20.0, 10.0), **extra):
    rs = np.random.RandomState(_seed('maps', name))
    sat, grd, conf = _maps(rs, B, levels)
    assert tuple(K.shape) == (B, 3, 3) and K.dtype == F32
    return SimpleNamespace(name=name, levels=levels, B=B, K=K, N=N, p0=p0, ranges=ranges, ori_hw=ORI_HW, sat=sat, grd=grd, conf=conf,
                           ordinary=list(range(B)), **extra)


def _rand_pose(rs, B, scale=0.2):
    return torch.from_numpy(rs.uniform(-scale, scale, size=(B, 3)).astype(np.float32))


SHAPES = [(7, 256, MAPS[2]), (7, 128, MAPS[0]), (7, 64, MAPS[1]),
          (18, 256, MAPS[0]), (18, 128, MAPS[1]), (18, 64, MAPS[2]),
          (70, 256, MAPS[1]), (70, 128, MAPS[2]), (70, 64, MAPS[0]),
          (130, 256, MAPS[2]), (130, 128, MAPS[0]), (130, 64, MAPS[1])]
_CASES = {}


def shape_case(A, Cn):
    """One level, one step, B = 2, a random starting pose."""
    hw = [s[2] for s in SHAPES if s[:2] == (A, Cn)][0]
    rs = np.random.RandomState(_seed('shape', A, Cn))
    return _case(f'shape A{A} C{Cn}', [(A, Cn, hw)], 2, ordinary_K(rs, 2), 1, _rand_pose(rs, 2))


def border_case():
    """B = 8, pose 0: sample i sits at border side i (border_K)."""
    rs = np.random.RandomState(_seed('border'))
    A, hw = 18, MAPS[0]
    c = _case('border', [(A, 64, hw)], 8, border_K(rs, A, hw), 1, None)
    c.ordinary = []
    return c


def octet_case(B):
    """B = 8 / 9 (the XCD-affine block map; idle blocks at 9), two small levels (ragged, under one tile), two iterations, a random
    pose0; the B = 8 case is the first eight samples of the B = 9 one."""
    rs = np.random.RandomState(_seed('octet'))
    K, p0 = ordinary_K(rs, 9), _rand_pose(rs, 9)
    c = _case('octet', [(18, 64, MAPS[0]), (7, 256, MAPS[2])], 9, K, 2, p0)
    return take(c, list(range(B)), f'octet B{B}')


def out_case():
    """B = 3, sample 1 has nothing in view at any level (cx far outside); two levels x two iterations, pose0 None."""
    rs = np.random.RandomState(_seed('out'))
    K = ordinary_K(rs, 3)
    K[1] = out_of_view_K(rs)
    c = _case('out', [(18, 128, MAPS[1]), (70, 64, MAPS[0])], 3, K, 2, None, out=1)
    c.ordinary = [0, 2]
    return c


def behind_case():
    """B = 2, shift_range_lat = 0, sample 1 = behind_K starting at su = +0.15: its centre pixel is in bounds and behind the camera
    at every step of both levels."""
    rs = np.random.RandomState(_seed('behind'))
    K = ordinary_K(rs, 2)
    K[1] = behind_K(rs)
    p0 = _rand_pose(rs, 2)
    p0[1] = torch.tensor([0.15, -0.07, 0.12])
    c = _case('behind', [(18, 128, MAPS[0]), (70, 64, MAPS[1])], 2, K, 2, p0, ranges=(0.0, 20.0, 10.0), behind=1)
    c.ordinary = [0]
    return c


def deep_case():
    """Two iterations x (a ragged level, the 67-tile level with a 4-pixel last tile), B = 2, pose0 None."""
    rs = np.random.RandomState(_seed('deep', 1))        # (16900 pixels x 4 steps: a draw whose pixels all keep GUARD, asserted on the CPU)
    return _case('deep', [(18, 256, MAPS[2]), (130, 64, MAPS[1])], 2, ordinary_K(rs, 2), 2, None)


def mid_case():
    """Two iterations x (fewer pixels than a tile, 128-pixel tiles with a 36-pixel last one), B = 3, random pose0."""
    rs = np.random.RandomState(_seed('mid'))
    return _case('mid', [(7, 256, MAPS[2]), (70, 128, MAPS[0])], 3, ordinary_K(rs, 3), 2, _rand_pose(rs, 3))


def deferred_case():
    """Raw maps = the normalised maps / inv, inv per sample and level in 0.5 .. 3 (exact in fp32); the kernel gets raw + inv."""
    rs = np.random.RandomState(_seed('deferred'))
    c = _case('deferred', [(18, 128, MAPS[0]), (7, 64, MAPS[2])], 3, ordinary_K(rs, 3), 2, _rand_pose(rs, 3))
    q = lambda: torch.from_numpy(np.round(rs.uniform(0.5, 3.0, size=(2, 3)) * 64) / 64)          # [L,B] fp64, multiples of 1/64
    c.sat_inv, c.grd_inv = q(), q()
    return c


CASES = dict(border=border_case, out=out_case, behind=behind_case, deep=deep_case, mid=mid_case, deferred=deferred_case,
             octet8=lambda: octet_case(8), octet9=lambda: octet_case(9))


def get(name, *a):
    """A case, made once per session and never modified."""
    key = (name,) + a
    if key not in _CASES:
        _CASES[key] = shape_case(*a) if name == 'shape' else CASES[name]()
    return _CASES[key]


def take(c, idx, name=None):
    """The case restricted to samples ``idx`` (in that order)."""
    d = dict(vars(c))
    d.update(name=name or f'{c.name}{idx}', B=len(idx), K=c.K[idx].contiguous(), p0=None if c.p0 is None else c.p0[idx].contiguous(),
             sat=[t[idx].contiguous() for t in c.sat], grd=[t[idx].contiguous() for t in c.grd], conf=[t[idx].contiguous() for t in c.conf],
             ordinary=[i for i, b in enumerate(idx) if b in c.ordinary])
    for k in ('sat_inv', 'grd_inv'):
        if k in d:
            d[k] = d[k][:, idx].contiguous()
    for k in ('out', 'behind'):
        if k in d:
            d[k] = idx.index(d[k]) if d[k] in idx else None
    return SimpleNamespace(**d)


def raw_maps(c):
    """(sat, grd) fp32 NCHW lists as the kernel reads them: the case's maps, or with deferred norms maps / inv."""
    if not hasattr(c, 'sat_inv'):
        return c.sat, c.grd
    raw = lambda ts, inv: [(t.double() / inv[l].view(-1, 1, 1, 1)).float() for l, t in enumerate(ts)]
    return raw(c.sat, c.sat_inv), raw(c.grd, c.grd_inv)


def cast(c, dt, requires_grad=False):
    """-> (sat, grd, conf) lists in ``dt`` as the reference reads them (with deferred norms: the fp32 raw maps x inv, formed in
    fp64), fresh leaves when ``requires_grad``."""
    sat, grd = raw_maps(c)
    if hasattr(c, 'sat_inv'):
        sat = [t.double() * c.sat_inv[l].view(-1, 1, 1, 1) for l, t in enumerate(sat)]
        grd = [t.double() * c.grd_inv[l].view(-1, 1, 1, 1) for l, t in enumerate(grd)]
    f = lambda ts: [t.to(dt).clone().requires_grad_(requires_grad) for t in ts]
    return f(sat), f(grd), f(c.conf)


def lam_of(dt=F64):
    return torch.tensor(DPARAM, dtype=F32).to(dt)


def start_pose(c):
    return torch.zeros(c.B, 3) if c.p0 is None else c.p0


def reference_trace(c, using_weight, dt=F64):
    sat, grd, conf = cast(c, dt)
    with torch.no_grad():
        return solve(make_args(c.ranges), lam_of(dt), sat, grd, conf, c.K, c.ori_hw, c.N, using_weight, c.p0)


def reference_grads(c, using_weight, coef, dt=F64):
    """Autograd through the loop, loss = sum(coef * trace) -> (sat, grd, conf leaves with .grad, lam leaf, trace)."""
    sat, grd, conf = cast(c, dt, requires_grad=True)
    lam = lam_of(dt).requires_grad_(True)
    tr = solve(make_args(c.ranges), lam, sat, grd, conf, c.K, c.ori_hw, c.N, using_weight, c.p0)
    (coef.to(dt) * tr).sum().backward()
    return sat, grd, conf, lam, tr.detach()


def coef_of(c):
    return torch.from_numpy(np.random.RandomState(_seed('coef', c.name)).standard_normal((c.B, c.N, len(c.levels), 3)))
