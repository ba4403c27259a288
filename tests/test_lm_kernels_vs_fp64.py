"""The LM pose-loop kernels (csrc/lm_solve.hip: lm_accum, lm_solve, lm_inview_kernel; csrc/lm_backward.hip: lm_bwd_accum,
lm_bwd_solve; csrc/lm_common.h: lm_pixel, lm_point, lm_block_map) against the free-geometry fp64 reference of
tests/lm_kernel_ref.py, through the C ABI (hla_s2g_lm_solve / hla_s2g_lm_solve_bwd) with hand-made levels: pixels exactly on,
just inside and just outside every border of the satellite map, in clamped far-corner cells and on texels; fewer pixels than a
tile, ragged last tiles, stored rows offset by grd_row_skip, more than 64 tiles per sample (the two-pass closing reduction),
and B = 8 / 9 (the XCD-affine block map with idle blocks); fp32, fp16 and bf16 maps; both projection chains.

Gates (none of them measured on the kernels):
  sums       |hip - ref64| <= 2e-6 * T_k, T_k = the reference's fp64 sum of the absolute values of sum k's terms
  pose       |hip - ref64| <= max(1e-6, 2 |ref32 - ref64|) componentwise, one step from the pose the kernel itself started from
  gradients  max|hip - ref64| / max|ref64| < 2e-4 per tensor (fp64 autograd through the reference's steps)
  exact      in-view counts, sums of a sample without a pixel in view, its unchanged pose, batch independence, repeats
Measured errors: EXPERIMENTS.md, "LM kernels against fp64 at tile and map borders"."""
import ctypes as C

import numpy as np
import pytest
import torch

import lm_kernel_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
TOL_SUM, TOL_POSE, TOL_GRAD = 2e-6, 1e-6, 2e-4
SENTINEL = 7.0
DPARAM = [[0.55, 0.6, 0.5]]              # damping parameter of the backward cases: lambda = 10^(-6 + 11 sigmoid(.)) ~ 1 .. 3


def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _lambda(dparam=DPARAM):
    return (10.0 ** (-6 + torch.sigmoid(torch.tensor(dparam, dtype=F64)) * 11.0)).reshape(-1).tolist()


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI with free geometry
# ----------------------------------------------------------------------------------------------------------------------
class _Call:
    """Structs of one hla_s2g_lm_solve / _bwd call and the device tensors they point to."""

    def __init__(self, geom, levels, N=1, level_first=0, using_weight=0, use_hessian=0, dof=3, damping=(1.0, 1.0, 1.0), keep=None,
                 inv_norm=None, reach_mode=0, reach_flag=None, reach_col0=None):
        """reach_mode / reach_flag (int32 [B] on the device) / reach_col0 (per level): the fields of the same name of hla_s2g_config."""
        from highlyaccurate_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        d = self.dev = _dev()
        self.L, self.N, self.B = len(levels), N, levels[0].sat.shape[0]
        self.levels = levels
        cfg = self.cfg = _lib.S2GConfig()
        cfg.ford, cfg.n_levels, cfg.n_iters, cfg.level_first = int(geom.ford), self.L, N, int(level_first)
        cfg.using_weight, cfg.use_hessian, cfg.dof = int(using_weight), int(use_hessian), dof
        cfg.shift_range_lat, cfg.shift_range_lon, cfg.rotation_range = geom.ranges
        for i in range(3):
            cfg.damping[i] = damping[i]
        cfg.optimizer, cfg.count_in_view, cfg.proj = 0, 1, 0
        self.keep = keep.to(d).contiguous() if keep is not None else None
        if self.keep is not None:
            cfg.keep, cfg.keep_stride = self.keep.data_ptr(), self.keep.shape[1]
        self.lv = (_lib.S2GLevel * self.L)()
        self.t, self.inv = [], []
        codes = {torch.float32: _lib.HLA_F32, torch.bfloat16: _lib.HLA_BF16, torch.float16: _lib.HLA_F16}
        for l, v in enumerate(levels):
            sat = v.sat.permute(0, 2, 3, 1).contiguous().to(d)
            grd = v.grd[:, :, v.skip:].permute(0, 2, 3, 1).contiguous().to(d)
            conf = v.conf[:, 0, v.skip:].contiguous().to(d)
            tab = v.table.contiguous().to(d)
            assert sat.dtype == grd.dtype == v.dtype and tuple(tab.shape) == (v.h, v.w, 3) and tab.dtype == torch.float32
            assert tuple(sat.shape) == (self.B, v.A, v.A, v.C) and tuple(grd.shape) == (self.B, v.h - v.skip, v.w, v.C)
            assert tuple(conf.shape) == (self.B, v.h - v.skip, v.w) and 0 <= v.skip <= v.row0 < v.h
            self.t.append((sat, grd, conf, tab))
            s = self.lv[l]
            s.sat_feat, s.grd_feat, s.xyz, s.feat_dtype = sat.data_ptr(), grd.data_ptr(), tab.data_ptr(), codes[v.dtype]
            s.grd_conf = conf.data_ptr() if using_weight else 0
            s.A, s.h, s.w, s.C, s.row0, s.grd_row_skip = v.A, v.h, v.w, v.C, v.row0, v.skip
            s.meter_per_pixel, s.centre = v.mpp, v.centre
            if inv_norm is not None:
                iv = [torch.tensor(x, dtype=F64, device=d) for x in inv_norm[l]]
                self.inv.append(iv)
                s.sat_inv_norm, s.grd_inv_norm = iv[0].data_ptr(), iv[1].data_ptr()
        self.R_FL = geom.R_FL.float().contiguous().to(d) if geom.ford else None
        self.T_FL = geom.T_FL.float().contiguous().to(d) if geom.ford else None
        self.reach_flag = reach_flag
        cfg.reach_mode = int(reach_mode)
        cfg.reach_flag = reach_flag.data_ptr() if reach_flag is not None else None
        for l, c0 in enumerate(reach_col0 or ()):
            cfg.reach_col0[l] = int(c0)

    def forward(self, p0, rand_uv, out=None):
        """-> trace [B,N,L,3] fp32, normal_eq [steps,B,16] fp64 (CPU tensors).  out = (trace, normal_eq, workspace) device tensors
        to run on (a second call of the reach protocol); NaN-filled fresh ones otherwise.  They are kept in self.trace / .neq / .ws
        from before the call on, so that a call that fails validation can be shown to have left them alone."""
        d, lib, _lib = self.dev, self.lib, self._lib
        steps = self.L * self.N
        self.p0 = p0.float().contiguous().to(d)
        ruv = rand_uv.float().contiguous().to(d)
        assert tuple(self.p0.shape) == (self.B, 3) and tuple(ruv.shape) == (steps, 2, self.B)
        nbytes = lib.hla_s2g_workspace_bytes(C.byref(self.cfg), self.lv, self.B)
        if out is None:
            trace = torch.full((self.B, self.N, self.L, 3), float('nan'), device=d, dtype=F32)
            neq = torch.full((steps, self.B, 16), float('nan'), device=d, dtype=F64)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
        else:
            trace, neq, ws = out
            assert trace.shape == (self.B, self.N, self.L, 3) and neq.shape == (steps, self.B, 16) and ws.numel() == nbytes
        self.trace, self.neq, self.ws = trace, neq, ws
        rc = lib.hla_s2g_lm_solve(C.byref(self.cfg), self.lv, _lib.ptr(self.R_FL), _lib.ptr(self.T_FL), _lib.ptr(self.p0), _lib.ptr(ruv),
                                  _lib.ptr(trace), _lib.ptr(neq), _lib.ptr(ws), nbytes, self.B, _lib.stream_ptr())
        _lib.check(rc, 'hla_s2g_lm_solve')
        torch.cuda.synchronize()
        return trace.cpu(), neq.cpu()

    def backward(self, d_trace, overwrite=1, deterministic=0):
        """After ``forward``.  -> d_sat[l] [B,C,A,A], d_grd[l] [B,C,hs,w] (stored rows), d_conf[l] [B,hs,w], d_damping [4] (CPU, fp64).
        The ground-gradient rows above row0 are handed over holding SENTINEL; the rows the loop owns hold SENTINEL too when it
        overwrites them on its first visit, zeros when it adds."""
        d, lib, _lib = self.dev, self.lib, self._lib
        self.cfg.grd_grad_overwrite, self.cfg.deterministic = int(overwrite), int(deterministic)
        gr = (_lib.S2GLevelGrad * self.L)()
        bufs = []
        for l, v in enumerate(self.levels):
            sat, grd, conf, _ = self.t[l]
            d_sat = torch.full_like(sat, SENTINEL) if deterministic else torch.zeros_like(sat)
            d_grd = torch.full_like(grd, SENTINEL)
            if not overwrite:
                d_grd[:, v.row0 - v.skip:] = 0
            d_conf = torch.zeros_like(conf)
            gr[l].d_sat_feat, gr[l].d_grd_feat = d_sat.data_ptr(), d_grd.data_ptr()
            gr[l].d_grd_conf = d_conf.data_ptr() if self.cfg.using_weight else 0
            bufs.append((d_sat, d_grd, d_conf))
        dtr = d_trace.float().contiguous().to(d)
        d_lam = torch.full((4,), float('nan'), device=d, dtype=F64)
        nbytes = lib.hla_s2g_bwd_workspace_bytes(C.byref(self.cfg), self.lv, self.B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
        rc = lib.hla_s2g_lm_solve_bwd(C.byref(self.cfg), self.lv, gr, _lib.ptr(self.R_FL), _lib.ptr(self.T_FL), _lib.ptr(self.p0),
                                      _lib.ptr(self.trace), _lib.ptr(self.neq), _lib.ptr(dtr), _lib.ptr(d_lam), _lib.ptr(ws), nbytes,
                                      self.B, _lib.stream_ptr())
        _lib.check(rc, 'hla_s2g_lm_solve_bwd')
        torch.cuda.synchronize()
        self.cfg.deterministic = 0
        return ([b[0].permute(0, 3, 1, 2).cpu().double() for b in bufs], [b[1].permute(0, 3, 1, 2).cpu().double() for b in bufs],
                [b[2].cpu().double() for b in bufs], d_lam.cpu())


# ----------------------------------------------------------------------------------------------------------------------
# gates
# ----------------------------------------------------------------------------------------------------------------------
def _gate_sums(tag, got, sums, mags):
    """got [B,14] (normal_eq[..., :14]) against the reference's sums [B,14] on the scale of their absolute terms."""
    got, sums, mags = np.asarray(got, np.float64), sums.detach().double().numpy(), mags.detach().double().numpy()
    assert np.isfinite(got).all(), (tag, got)
    err = np.abs(got - sums)
    ratio = (err / np.where(mags > 0, mags, 1.0)).max()
    print(f'LMK sums {tag}: worst |hip - ref64| / T_k = {ratio:.2e} (limit {TOL_SUM:.0e})')
    assert (err <= TOL_SUM * mags).all(), (tag, (err / np.where(mags > 0, mags, 1.0)).max(0))
    return ratio


def _gate_pose(tag, got, p64, p32):
    got = np.asarray(got, np.float64)
    p64, p32 = [torch.cat(p, 1).detach().double().numpy() for p in (p64, p32)]
    allow = np.maximum(TOL_POSE, 2 * np.abs(p32 - p64))
    err = np.abs(got - p64)
    print(f'LMK pose {tag}: max |hip - ref64| = {err.max():.2e}, ref32 gap {np.abs(p32 - p64).max():.2e}, worst ratio {(err / allow).max():.2f}')
    assert np.isfinite(got).all() and (err <= allow).all(), (tag, err, allow)


def _gate_grad(tag, got, ref):
    got, ref = np.asarray(got, np.float64), ref.detach().double().numpy()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    scale = np.abs(ref).max()
    assert scale > 0 and np.isfinite(got).all(), tag
    e = np.abs(got - ref).max() / scale
    print(f'LMK grad {tag}: max|hip - ref64| / max|ref64| = {e:.2e} (limit {TOL_GRAD:.0e})')
    assert e < TOL_GRAD, (tag, e)


_LEVELS = {}


def _border_level(ford, shape, Cn, A, B, dtype=torch.float32):
    """(geom, level) of a pose-0 case, made once per session and never modified."""
    key = (ford, shape, Cn, A, B, dtype)
    if key not in _LEVELS:
        _LEVELS[key] = (R.make_geom(ford, B), R.make_level(ford, shape, Cn, A, B, R.case_seed(ford, shape, Cn, A, B), dtype=dtype))
    return _LEVELS[key]


def _zero_pose(B):
    return torch.zeros(B, 3), torch.zeros(1, 2, B)


# ----------------------------------------------------------------------------------------------------------------------
# forward at pose 0: the border classes
# ----------------------------------------------------------------------------------------------------------------------
def _forward_pose0(ford, shape, Cn, A, B, dtype, using_weight, inv_norm=None, level=None):
    """level: (geom, lv) to run on (None: the border level of the case)."""
    geom, lv = level if level is not None else _border_level(ford, shape, Cn, A, B, dtype)
    ref_lv = R.cast_level(lv, F64)
    run_lv = lv
    if inv_norm is not None:        # deferred norms: the kernel reads raw maps and rescales its sums; the reference reads raw * inv
        run_lv = R.cast_level(lv, F32)
        for k, iv in zip(('sat', 'grd'), inv_norm):
            raw = (getattr(lv, k) / torch.tensor(iv, dtype=F32).view(-1, 1, 1, 1)).contiguous()
            setattr(run_lv, k, raw)
            setattr(ref_lv, k, raw.double() * torch.tensor(iv, dtype=F64).view(-1, 1, 1, 1))
    call = _Call(geom, [run_lv], using_weight=using_weight, inv_norm=[inv_norm] if inv_norm is not None else None)
    trace, neq = call.forward(*_zero_pose(B))
    pose = R.pose_cols(torch.zeros(B, 3), F64)
    sums, mags, count = R.level_sums(R.cast_geom(geom, F64), ref_lv, pose, using_weight)
    tag = f"pose0 {'ford' if ford else 'kitti'} {shape} C{Cn} A{A} B{B} {str(dtype)[6:]} w{using_weight}" + (' deferred' if inv_norm else '')
    _gate_sums(tag, neq[0, :, :14], sums, mags)
    assert np.array_equal(neq[0, :, 14].numpy(), count.double().numpy()), (tag, neq[0, :, 14], count)
    assert int(count.min()) >= 0.25 * lv.h * lv.w
    return call, trace, neq


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['fp32', 'fp16', 'bf16'])
@pytest.mark.parametrize('Cn', [16, 64, 128, 256])
def test_forward_border_classes_every_width_and_map_type(Cn, dtype, using_weight):
    _forward_pose0(0, 'ragged', Cn, 16, 3, dtype, using_weight)


@pytest.mark.parametrize('ford,A', [(1, 16), (0, 13), (1, 13)])
@pytest.mark.parametrize('using_weight', [0, 1])
def test_forward_border_classes_ford_and_odd_map(ford, A, using_weight):
    """The Ford chain reaches u = 0 and v = 0; A = 13 has a half-integer centre (KITTI) / an integer one (Ford)."""
    _forward_pose0(ford, 'ragged', 64, A, 3, torch.float32, using_weight)


@pytest.mark.parametrize('shape,Cn,B,using_weight', [('sub_tile', 256, 1, 0), ('skip', 128, 2, 1), ('mid', 64, 2, 1), ('many', 16, 2, 0),
                                                     ('octet', 64, 8, 1), ('octet', 64, 9, 1)])
def test_forward_border_classes_tile_shapes(shape, Cn, B, using_weight):
    _forward_pose0(0, shape, Cn, 16, B, torch.float32, using_weight)


def test_forward_border_classes_16bit_many_tiles():
    """fp16 maps through the two-pass closing reduction (65 tiles)."""
    _forward_pose0(0, 'many', 16, 16, 2, torch.float16, 0)


def test_forward_deferred_norms():
    _forward_pose0(0, 'ragged', 64, 16, 3, torch.float32, 1, inv_norm=([0.5, 1.7, 3.1], [2.3, 0.4, 1.0]))


@pytest.mark.parametrize('kw', [dict(use_hessian=1, damping=0.5), dict(dof=2), dict(dof=1)])
def test_forward_one_step_solver_variants(kw):
    """use_hessian and the 2-DoF / 1-DoF solves on a ragged level from a random pose: sums and the one-step pose."""
    kw = dict(kw)
    dof, damping = kw.pop('dof', 3), kw.pop('damping', 1.0)
    geom, lv = _border_level(0, 'ragged', 64, 16, 3)
    geom = R.SimpleNamespace(**vars(geom))
    lat, lon, rot = R.RANGES
    geom.ranges = (lat, lon, 0.0) if dof == 2 else ((0.0, 0.0, rot) if dof == 1 else R.RANGES)
    p0 = torch.from_numpy(np.random.RandomState(31).uniform(-0.3, 0.3, size=(3, 3)).astype(np.float32))
    ruv = torch.from_numpy(np.random.RandomState(32).uniform(-1, 1, size=(1, 2, 3)).astype(np.float32))
    call = _Call(geom, [lv], using_weight=1, dof=dof, damping=(damping,) * 3, **kw)
    trace, neq = call.forward(p0, ruv)
    args = R.update_args(geom.ranges, damping=damping, **kw)
    new = {}
    for dt in (F64, F32):
        pose = R.pose_cols(p0, dt)
        new[dt] = R.level_step(args, R.cast_geom(geom, dt), R.cast_level(lv, dt), pose, 1, tuple(ruv[0, i][:, None].to(dt) for i in range(2)))
    sums, mags, count = R.level_sums(R.cast_geom(geom, F64), R.cast_level(lv, F64), R.pose_cols(p0, F64), 1)
    tag = f'variant dof{dof} {kw}'
    _gate_sums(tag, neq[0, :, :14], sums, mags)
    assert np.array_equal(neq[0, :, 14].numpy(), count.double().numpy())
    _gate_pose(tag, trace[:, 0, 0], new[F64], new[F32])


# ----------------------------------------------------------------------------------------------------------------------
# forward, random poses, two levels x two iterations, teacher-forced
# ----------------------------------------------------------------------------------------------------------------------
def _two_level_forward(geom, levels, p0, rand_uv, level_first, using_weight, keep):
    call = _Call(geom, levels, N=2, level_first=level_first, using_weight=using_weight, keep=keep)
    trace, neq = call.forward(p0, rand_uv)
    return call, trace, neq


@pytest.mark.parametrize('ford,level_first,use_keep,using_weight', R.RANDOM_CASES)
def test_forward_random_poses_two_levels_teacher_forced(ford, level_first, use_keep, using_weight):
    seed = R.case_seed('random', ford, level_first)
    geom, levels, p0, rand_uv, keep = R.make_two_level_case(ford, seed)
    keep = keep if use_keep else None
    B, out = 3, 1
    _, trace, neq = _two_level_forward(geom, levels, p0, rand_uv, level_first, using_weight, keep)
    args = R.update_args()
    casts = {dt: (R.cast_geom(geom, dt), [R.cast_level(lv, dt) for lv in levels]) for dt in (F64, F32)}
    tag0 = f"random {'ford' if ford else 'kitti'} lf{level_first} keep{use_keep} w{using_weight}"
    prev = p0
    for k, (i, l) in enumerate(R.step_order(2, 2, level_first)):
        lv = levels[l]
        kp = keep[k, :(lv.h - lv.row0) * lv.w].bool() if use_keep else None
        new = {}
        for dt in (F64, F32):
            g, lvs = casts[dt]
            new[dt] = R.level_step(args, g, lvs[l], R.pose_cols(prev, dt), using_weight, tuple(rand_uv[k, j][:, None].to(dt) for j in range(2)),
                                   keep=kp)
        g, lvs = casts[F64]
        sums, mags, count = R.level_sums(g, lvs[l], R.pose_cols(prev, F64), using_weight, kp)
        _gate_sums(f'{tag0} step {k}', neq[k, :, :14], sums, mags)
        assert np.array_equal(neq[k, :, 14].numpy(), count.double().numpy()), (k, neq[k, :, 14], count)
        _gate_pose(f'{tag0} step {k}', trace[:, i, l], new[F64], new[F32])
        # the sample without a pixel in view: exact zeros, and the step leaves its pose bit for bit
        assert int(count[out]) == 0
        assert not bool(neq[k, out, [0] + list(range(2, 11))].any()), neq[k, out]
        assert torch.equal(trace[out, i, l], p0[out])
        prev = trace[:, i, l]
    # its batch mates are what they are without it, bit for bit
    g2, l2, p2, r2 = R.drop_sample(geom, levels, p0, rand_uv, out)
    _, trace2, neq2 = _two_level_forward(g2, l2, p2, r2, level_first, using_weight, keep)
    sel = [b for b in range(B) if b != out]
    assert torch.equal(trace2, trace[sel]) and torch.equal(neq2[:, :, :15], neq[:, sel, :15])


# ----------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------
def _reference_grads(geom, levels, p0, rand_uv, N, level_first, using_weight, coef, keep=None, use_keep=False, dt=F64):
    """fp64 autograd through the reference's steps from pose0, loss = sum(coef * trace).  -> leaves (with .grad), dparam.
    dt = torch.float32: the reference's own fp32 run (tests/test_cell_runs_cpu.py)."""
    g = R.cast_geom(geom, dt)
    lvs = [R.cast_level(lv, dt, requires_grad=True) for lv in levels]
    dparam = torch.tensor(DPARAM, dtype=dt, requires_grad=True)
    args = R.update_args(train_damping=1)
    pose = R.pose_cols(p0, dt)
    loss = 0
    for k, (i, l) in enumerate(R.step_order(len(levels), N, level_first)):
        lv = lvs[l]
        kp = keep[k, :(lv.h - lv.row0) * lv.w].bool() if use_keep else None
        pose = R.level_step(args, g, lv, pose, using_weight, tuple(rand_uv[k, j][:, None].to(dt) for j in range(2)), dparam, kp)
        loss = loss + (coef[:, i, l].to(dt) * torch.cat(pose, 1)).sum()
    loss.backward()
    return lvs, dparam


def _gate_all_grads(tag, levels, lvs, dparam, using_weight, d_sat, d_grd, d_conf, d_lam):
    for l, (v, r) in enumerate(zip(levels, lvs)):
        _gate_grad(f'{tag} L{l} d_sat', d_sat[l], r.sat.grad)
        _gate_grad(f'{tag} L{l} d_grd', d_grd[l][:, :, v.row0 - v.skip:], r.grd.grad[:, :, v.row0:])
        assert not bool(r.grd.grad[:, :, :v.row0].any())
        # rows above row0 are the caller's: untouched
        assert bool((d_grd[l][:, :, :v.row0 - v.skip] == SENTINEL).all()), (tag, l)
        if using_weight:
            _gate_grad(f'{tag} L{l} d_conf', d_conf[l], r.conf.grad[:, 0, v.skip:])
    sg = torch.sigmoid(dparam.detach())
    lam = 10.0 ** (-6 + sg * 11.0)
    got = d_lam[:3].view(1, 3) * lam * np.log(10.0) * 11.0 * sg * (1 - sg)
    _gate_grad(f'{tag} d_damping', got, dparam.grad)


def _backward_pose0(ford, shape, Cn, A, B, using_weight, deterministic=0, pose=None, level=None):
    """One level, one step, backward against fp64 autograd.  pose: the start pose of every sample (None: pose 0); level: (geom, lv)
    to run on (None: the border level of the case)."""
    geom, lv = level if level is not None else _border_level(ford, shape, Cn, A, B)
    p0, ruv = _zero_pose(B)
    if pose is not None:
        p0 = torch.tensor([pose], dtype=F32).repeat(B, 1)
    call = _Call(geom, [lv], using_weight=using_weight, damping=_lambda())
    call.forward(p0, ruv)
    coef = torch.from_numpy(np.random.RandomState(R.case_seed('coef', shape, Cn, B)).standard_normal((B, 1, 1, 3)))
    lvs, dparam = _reference_grads(geom, [lv], p0, ruv, 1, 0, using_weight, coef)
    tag = f"bwd pose{0 if pose is None else pose} {'ford' if ford else 'kitti'} {shape} C{Cn} A{A} B{B} w{using_weight}" + \
          (' det' if deterministic else '') + (' given level' if level is not None else '')
    out = call.backward(coef, overwrite=1, deterministic=deterministic)
    _gate_all_grads(tag, [lv], lvs, dparam, using_weight, *out)
    return call, coef, out


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('Cn', [16, 64, 128, 256])
def test_backward_border_classes_every_width(Cn, using_weight):
    call, coef, out = _backward_pose0(0, 'ragged', Cn, 16, 3, using_weight)
    # zero-filled ground-gradient rows that every visit adds to: the same bits as the overwriting first visit
    acc = call.backward(coef, overwrite=0)
    assert torch.equal(acc[1][0], out[1][0]) and torch.equal(acc[2][0], out[2][0])


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('ford,A', [(1, 16), (0, 13), (1, 13)])
def test_backward_border_classes_ford_and_odd_map(ford, A, using_weight):
    _backward_pose0(ford, 'ragged', 64, A, 3, using_weight)


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('shape,Cn,B', [('sub_tile', 256, 1), ('skip', 128, 2), ('mid', 64, 2), ('many', 16, 2), ('octet', 64, 8), ('octet', 64, 9)])
def test_backward_border_classes_tile_shapes(shape, Cn, B, using_weight):
    _backward_pose0(0, shape, Cn, 16, B, using_weight)


def test_backward_many_tiles_two_iterations():
    """130 backward tiles per sample AND a later step to close: the two-pass reduction of the coefficient adjoints in the closing
    solve (one level x one iteration has nothing to close, so it never reads them)."""
    B = 2
    geom, lv = _border_level(0, 'many', 16, 16, B)
    p0, ruv = torch.zeros(B, 3), torch.zeros(2, 2, B)
    call = _Call(geom, [lv], N=2, using_weight=1, damping=_lambda())
    call.forward(p0, ruv)
    coef = torch.from_numpy(np.random.RandomState(41).standard_normal((B, 2, 1, 3)))
    lvs, dparam = _reference_grads(geom, [lv], p0, ruv, 2, 0, 1, coef)
    _gate_all_grads('bwd many two iterations', [lv], lvs, dparam, 1, *call.backward(coef))


@pytest.mark.parametrize('shape,B', [('ragged', 3), ('octet', 9)])
def test_backward_deterministic_mode(shape, B):
    """cfg.deterministic: within the gradient gate of the reference, no range overflow reported, two calls bitwise equal."""
    call, coef, out = _backward_pose0(0, shape, 64, 16, B, 1, deterministic=1)
    assert float(out[3][3]) == 0.0
    again = call.backward(coef, overwrite=1, deterministic=1)
    for a, b in zip(out[:3], again[:3]):
        assert torch.equal(a[0], b[0])
    assert torch.equal(out[3], again[3]) and bool(out[0][0].any())


@pytest.mark.parametrize('ford,level_first,use_keep,using_weight', R.RANDOM_CASES)
def test_backward_random_poses_two_levels(ford, level_first, use_keep, using_weight):
    seed = R.case_seed('random', ford, level_first)
    geom, levels, p0, rand_uv, keep = R.make_two_level_case(ford, seed)
    B, out_b = 3, 1
    call = _Call(geom, levels, N=2, level_first=level_first, using_weight=using_weight, keep=keep if use_keep else None, damping=_lambda())
    call.forward(p0, rand_uv)
    coef = torch.from_numpy(np.random.RandomState(seed + 3).standard_normal((B, 2, 2, 3)))
    lvs, dparam = _reference_grads(geom, levels, p0, rand_uv, 2, level_first, using_weight, coef, keep, bool(use_keep))
    tag = f"bwd random {'ford' if ford else 'kitti'} lf{level_first} keep{use_keep} w{using_weight}"
    out = call.backward(coef, overwrite=1)
    _gate_all_grads(tag, levels, lvs, dparam, using_weight, *out)
    acc = call.backward(coef, overwrite=0)
    for l in range(2):
        assert torch.equal(acc[1][l], out[1][l]), l
        # the sample that never had a pixel in view sends nothing to its satellite map
        assert not bool(out[0][l][out_b].any()) and not bool(lvs[l].sat.grad[out_b].any())
