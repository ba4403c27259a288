"""The multi-view LM loop (csrc/lm_views.hip: lmv_accum, lmv_close) against the fp64 reference of tests/lm_views_ref.py -- one
``LM_update`` on the union of the views' pixels -- through the C ABI (hla_s2g_lm_solve_views) with hand-made levels of
tests/lm_kernel_ref.py: a border table per view, FORD_R and dyadic variations of FORD_T per view.

Gates: those of tests/test_lm_kernels_vs_fp64.py, none of them measured on the kernels:
  sums   (view_sums and normal_eq)  |hip - ref64| <= 2e-6 * T_k, T_k = the reference's fp64 sum of the absolute values of sum k's terms
  pose   |hip - ref64| <= max(1e-6, 2 |ref32 - ref64|) componentwise, one step from the pose the kernel itself started from;
         multi-step traces step by step, each reference step restarted from the kernel's previous pose
  exact  batch independence, repeats, a masked-out view against the call without it, the pose of a sample no view sees
Measured errors: EXPERIMENTS.md, "Multi-view LM loop"."""
import ctypes as C

import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import lm_views_ref as VR
import test_lm_kernels_vs_fp64 as K

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


class _ViewsCall:
    """Structs of one hla_s2g_lm_solve_views call and the device tensors they point to."""

    def __init__(self, geom, levels, N=1, level_first=0, using_weight=0, use_hessian=0, damping=(1.0, 1.0, 1.0), optimizer=0,
                 inv_norm=None):
        from highlyaccurate_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        d = self.dev = K._dev()
        self.L, self.N, self.B, self.V = len(levels), N, levels[0].sat.shape[0], levels[0].V
        cfg = self.cfg = _lib.S2GConfig()
        cfg.ford, cfg.n_levels, cfg.n_iters, cfg.level_first = 1, self.L, N, int(level_first)
        cfg.using_weight, cfg.use_hessian, cfg.dof = int(using_weight), int(use_hessian), 3
        cfg.shift_range_lat, cfg.shift_range_lon, cfg.rotation_range = geom.ranges
        for i in range(3):
            cfg.damping[i] = damping[i]
        cfg.optimizer = optimizer
        self.lv = (_lib.S2GLevel * self.L)()
        self.t, self.inv = [], []
        codes = {torch.float32: _lib.HLA_F32, torch.bfloat16: _lib.HLA_BF16, torch.float16: _lib.HLA_F16}
        J = self.B * self.V
        for l, v in enumerate(levels):
            sat = v.sat.permute(0, 2, 3, 1).contiguous().to(d)
            grd = v.grd[:, :, v.skip:].permute(0, 2, 3, 1).contiguous().to(d)
            conf = v.conf[:, 0, v.skip:].contiguous().to(d)
            tab = v.table.contiguous().to(d)
            assert tuple(tab.shape) == (self.V, v.h, v.w, 3) and tab.dtype == torch.float32
            assert tuple(sat.shape) == (self.B, v.A, v.A, v.C) and tuple(grd.shape) == (J, v.h - v.skip, v.w, v.C)
            assert tuple(conf.shape) == (J, v.h - v.skip, v.w) and 0 <= v.skip <= v.row0 < v.h
            self.t.append((sat, grd, conf, tab))
            s = self.lv[l]
            s.sat_feat, s.grd_feat, s.xyz, s.feat_dtype = sat.data_ptr(), grd.data_ptr(), tab.data_ptr(), codes[v.dtype]
            s.grd_conf = conf.data_ptr() if using_weight else 0
            s.A, s.h, s.w, s.C, s.row0, s.grd_row_skip = v.A, v.h, v.w, v.C, v.row0, v.skip
            s.meter_per_pixel, s.centre = v.mpp, v.centre
            if inv_norm is not None:
                iv = [torch.tensor(x, dtype=F64, device=d) for x in inv_norm[l]]
                assert iv[0].numel() == self.B and iv[1].numel() == J
                self.inv.append(iv)
                s.sat_inv_norm, s.grd_inv_norm = iv[0].data_ptr(), iv[1].data_ptr()
        self.R_FL = geom.R_FL.float().contiguous().to(d)
        self.T_FL = geom.T_FL.float().contiguous().to(d)
        assert tuple(self.R_FL.shape) == (self.B, self.V, 3, 3) and tuple(self.T_FL.shape) == (self.B, self.V, 3)

    def workspace_bytes(self, V=None):
        return self.lib.hla_s2g_views_workspace_bytes(C.byref(self.cfg), self.lv, self.B, self.V if V is None else V)

    def forward(self, p0, rand_uv, V=None, short_ws=0, expect_error=False):
        """-> trace [B,N,L,3] fp32, normal_eq [steps,B,16], view_sums [steps,B,V,16] fp64 (CPU).  expect_error: the call must
        return an error status; -> (status, outputs) with the outputs still holding their NaN fill if nothing was launched."""
        d, lib, _lib = self.dev, self.lib, self._lib
        steps = self.L * self.N
        p0d = p0.float().contiguous().to(d) if p0 is not None else None
        ruv = rand_uv.float().contiguous().to(d)
        assert tuple(ruv.shape) == (steps, 2, self.B)
        Vc = self.V if V is None else V
        nbytes = self.workspace_bytes()
        trace = torch.full((self.B, self.N, self.L, 3), float('nan'), device=d, dtype=F32)
        neq = torch.full((steps, self.B, 16), float('nan'), device=d, dtype=F64)
        vs = torch.full((steps, self.B, self.V, 16), float('nan'), device=d, dtype=F64)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=d)
        rc = lib.hla_s2g_lm_solve_views(C.byref(self.cfg), self.lv, Vc, _lib.ptr(self.R_FL), _lib.ptr(self.T_FL), _lib.ptr(p0d),
                                        _lib.ptr(ruv), _lib.ptr(trace), _lib.ptr(neq), _lib.ptr(vs), _lib.ptr(ws),
                                        nbytes - short_ws, self.B, _lib.stream_ptr())
        torch.cuda.synchronize()
        if expect_error:
            return rc, (trace.cpu(), neq.cpu(), vs.cpu())
        _lib.check(rc, 'hla_s2g_lm_solve_views')
        return trace.cpu(), neq.cpu(), vs.cpu()


_CASES = {}


def _case(shape, Cn, B, V, dtype=torch.float32):
    """(geom, level) of a one-level case, made once per session and never modified."""
    key = (shape, Cn, B, V, dtype)
    if key not in _CASES:
        _CASES[key] = (VR.make_views_geom(B, V), VR.make_views_level(shape, Cn, 16, B, V, R.case_seed('views', shape, Cn, B, V), dtype=dtype))
    return _CASES[key]


def _draws(lv_or_B, steps=1, seed=5):
    B = lv_or_B if isinstance(lv_or_B, int) else lv_or_B.sat.shape[0]
    return VR.random_pose(B, seed), VR.random_draws(steps, B, seed + 1)


def _ruv(rand_uv, k, dt):
    return tuple(rand_uv[k, j][:, None].to(dt) for j in range(2))


def _check_step(tag, geom, lv, prev, using_weight, ruv_k, got_pose, got_neq, got_vs, args=None, gn=False, ref_lv=None):
    """One step from ``prev`` [B,3]: every view's sums, the total and the pose after the step against the references."""
    args = args or R.update_args()
    ref_lv = ref_lv or lv
    g64, l64 = VR.cast_views_geom(geom, F64), R.cast_level(ref_lv, F64)
    p64 = R.pose_cols(prev, F64)
    worst = 0.0
    for v in range(lv.V):
        sums, mags = VR.one_view_sums(g64, l64, p64, v, using_weight)
        assert not bool(got_vs[:, v, 14:].any())
        worst = max(worst, K._gate_sums(f'{tag} view {v}', got_vs[:, v, :14], sums, mags))
    sums, mags = VR.views_sums(g64, l64, p64, using_weight)
    assert not bool(got_neq[:, 14:].any())
    worst = max(worst, K._gate_sums(f'{tag} total', got_neq[:, :14], sums, mags))
    new = {}
    for dt in (F64, F32):
        new[dt] = VR.views_step(args, VR.cast_views_geom(geom, dt), R.cast_level(ref_lv, dt), R.pose_cols(prev, dt), using_weight,
                                tuple(r.to(dt) for r in ruv_k), gauss_newton=gn)
    K._gate_pose(tag, got_pose, new[F64], new[F32])
    return worst


def _one_step(shape, Cn, B, V, dtype, using_weight, pose0=False, **kw):
    geom, lv = _case(shape, Cn, B, V, dtype)
    p0, ruv = _draws(lv)
    if pose0:
        p0 = torch.zeros(B, 3)
    call = _ViewsCall(geom, [lv], using_weight=using_weight, **kw)
    trace, neq, vs = call.forward(p0, ruv)
    tag = f"views {shape} C{Cn} B{B} V{V} {str(dtype)[6:]} w{using_weight}{' pose0' if pose0 else ''}"
    _check_step(tag, geom, lv, p0, using_weight, _ruv(ruv, 0, F32), trace[:, 0, 0], neq[0], vs[0])
    return call, trace, neq, vs


@pytest.mark.parametrize('shape,Cn,B,V,using_weight', [
    ('sub_tile', 256, 1, 2, 0), ('ragged', 64, 2, 3, 1), ('ragged', 256, 2, 1, 1), ('skip', 128, 2, 2, 1), ('mid', 64, 1, 3, 0),
    ('many', 16, 1, 2, 1)])
def test_one_step_tile_shapes_fp32(shape, Cn, B, V, using_weight):
    """sub_tile: fewer pixels than a tile; ragged: a 3-px last tile; skip: stored rows offset by grd_row_skip; mid: 256-px tiles;
    many: 65 tiles per view, the closing reduction's second pass over the lane stride."""
    _one_step(shape, Cn, B, V, torch.float32, using_weight)


@pytest.mark.parametrize('V', [1, 2, 3])
def test_border_classes_at_pose_zero(V):
    """Pose 0: view 0's pixels sit exactly on, just inside and just outside every border of the satellite map."""
    _one_step('ragged', 64, 2, V, torch.float32, 1, pose0=True)


@pytest.mark.parametrize('dtype,Cn,V', [(torch.float16, 128, 2), (torch.bfloat16, 64, 3)], ids=['fp16', 'bf16'])
def test_one_step_16bit_maps(dtype, Cn, V):
    _one_step('ragged', Cn, 2, V, dtype, 1)


@pytest.mark.parametrize('B,V', [(3, 3), (8, 2)])
def test_block_map_with_idle_blocks(B, V):
    """B * V = 9: the XCD-affine block map with seven idle blocks per tile; B * V = 16: two whole octets."""
    _one_step('octet', 64, B, V, torch.float32, 1)


@pytest.mark.parametrize('kw', [dict(use_hessian=1, damping=0.5), dict(gn=1), dict(using_weight=0)], ids=['use_hessian', 'gn', 'unweighted'])
def test_one_step_solver_variants(kw):
    kw = dict(kw)
    gn, damping, w = kw.pop('gn', 0), kw.pop('damping', 1.0), kw.pop('using_weight', 1)
    geom, lv = _case('ragged', 64, 2, 3)
    p0, ruv = _draws(lv, seed=31)
    call = _ViewsCall(geom, [lv], using_weight=w, damping=(damping,) * 3, optimizer=3 if gn else 0, **kw)
    trace, neq, vs = call.forward(p0, ruv)
    args = R.update_args(damping=damping, **kw)
    _check_step(f'views variant gn{gn} {kw}', geom, lv, p0, w, _ruv(ruv, 0, F32), trace[:, 0, 0], neq[0], vs[0], args=args, gn=bool(gn))


def test_deferred_norms_differ_per_view():
    """The kernel reads raw maps and rescales every view's sums with that view's ground norm; the reference reads raw * inv."""
    B, V = 2, 2
    geom, lv = _case('ragged', 64, B, V)
    inv = ([0.5, 1.7], [2.3, 0.4, 1.0, 3.1])
    run_lv, ref_lv = R.cast_level(lv, F32), R.cast_level(lv, F64)
    for k, iv in zip(('sat', 'grd'), inv):
        raw = (getattr(lv, k) / torch.tensor(iv, dtype=F32).view(-1, 1, 1, 1)).contiguous()
        setattr(run_lv, k, raw)
        setattr(ref_lv, k, raw.double() * torch.tensor(iv, dtype=F64).view(-1, 1, 1, 1))
    p0, ruv = _draws(lv)
    trace, neq, vs = _ViewsCall(geom, [run_lv], using_weight=1, inv_norm=[inv]).forward(p0, ruv)
    _check_step('views deferred norms', geom, lv, p0, 1, _ruv(ruv, 0, F32), trace[:, 0, 0], neq[0], vs[0], ref_lv=ref_lv)


def _two_level_case(seed, B=3, V=2, out_sample=1):
    levels = [VR.make_views_level(s, Cn, A, B, V, seed + 10 * l, mpp) for l, (s, Cn, A, mpp) in enumerate(R.TWO_LEVELS)]
    p0 = VR.random_pose(B, seed + 77)
    p0[out_sample] = torch.tensor(R.OUT_OF_VIEW_POSE)
    return VR.make_views_geom(B, V), levels, p0, VR.random_draws(4, B, seed + 78)


@pytest.mark.parametrize('level_first,using_weight', [(0, 1), (1, 0)])
def test_two_levels_both_loop_orders_teacher_forced(level_first, using_weight):
    """2 levels x 2 iterations (tile counts 3 and 17: the coarser level leaves part_ld > nt), every step checked from the pose the
    kernel left; sample 1 starts where no view sees the map: zero Jacobian sums and its pose kept bit for bit."""
    B, out = 3, 1
    geom, levels, p0, rand_uv = _two_level_case(R.case_seed('views2', level_first))
    trace, neq, vs = _ViewsCall(geom, levels, N=2, level_first=level_first, using_weight=using_weight).forward(p0, rand_uv)
    prev = p0
    for k, (i, l) in enumerate(R.step_order(2, 2, level_first)):
        _check_step(f'views two levels lf{level_first} step {k}', geom, levels[l], prev, using_weight, _ruv(rand_uv, k, F32),
                    trace[:, i, l], neq[k], vs[k])
        assert not bool(neq[k, out, [0] + list(range(2, 11))].any()), neq[k, out]
        assert not bool(vs[k, out][:, [0] + list(range(2, 11))].any())
        assert float(neq[k, out, 1]) > 0                      # (out of the map, the views still contribute their ||g||^2)
        assert torch.equal(trace[out, i, l], p0[out])
        prev = trace[:, i, l]


def test_batch_independence_and_repeats():
    B, V = 3, 2
    geom, lv = _case('ragged', 64, B, V)
    p0, ruv = VR.random_pose(B, 9), VR.random_draws(2, B, 10)
    call = _ViewsCall(geom, [lv], N=2, using_weight=1)
    out = call.forward(p0, ruv)
    again = call.forward(p0, ruv)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    for b in range(B):
        g1, l1 = VR.select_samples(geom, lv, [b])
        alone = _ViewsCall(g1, [l1], N=2, using_weight=1).forward(p0[b:b + 1], ruv[:, :, b:b + 1].contiguous())
        assert torch.equal(alone[0][0], out[0][b]) and torch.equal(alone[1][:, 0], out[1][:, b]) and torch.equal(alone[2][:, 0], out[2][:, b]), b


def test_masked_out_view_is_absent_bit_for_bit():
    B, V = 2, 3
    geom, lv = _case('ragged', 64, B, V)
    lm = R.SimpleNamespace(**vars(lv))
    lm.table = lv.table.clone()
    lm.table[1] = VR.masked_table(lv.table[1])
    p0, ruv = VR.random_pose(B, 13), VR.random_draws(2, B, 14)
    trace, neq, vs = _ViewsCall(geom, [lm], N=2, using_weight=1).forward(p0, ruv)
    gw, lw = VR.select_views(geom, lv, [0, 2])
    trace2, neq2, vs2 = _ViewsCall(gw, [lw], N=2, using_weight=1).forward(p0, ruv)
    assert not bool(vs[:, :, 1].any())
    assert torch.equal(trace, trace2) and torch.equal(neq, neq2) and torch.equal(vs[:, :, [0, 2]], vs2)


def test_duplicated_view_and_single_view_against_the_single_view_loop():
    B = 2
    geom, lv = _case('ragged', 64, B, 3)
    p0, ruv = _draws(lv, seed=21)
    g1, l1 = VR.select_views(geom, lv, [0])
    one = _ViewsCall(g1, [l1], using_weight=1).forward(p0, ruv)
    g2, l2 = VR.select_views(geom, lv, [0, 0])
    two = _ViewsCall(g2, [l2], using_weight=1).forward(p0, ruv)
    d = float((two[0] - one[0]).abs().max())
    print(f'LMV duplicated view against V = 1: max |pose difference| = {d:.2e}')
    assert d <= 1e-6
    assert torch.equal(two[2][:, :, 0], two[2][:, :, 1]) and torch.equal(two[2][:, :, 0], one[2][:, :, 0])
    # V = 1 against hla_s2g_lm_solve on the same inputs
    single = R.SimpleNamespace(**vars(l1))
    single.table = l1.table[0]
    gs = R.SimpleNamespace(ford=1, ranges=geom.ranges, R_FL=g1.R_FL[:, 0], T_FL=g1.T_FL[:, 0])
    call = K._Call(gs, [single], using_weight=1)
    call.cfg.count_in_view = 0
    trace_s, neq_s = call.forward(p0, ruv)
    d = float((trace_s - one[0]).abs().max())
    print(f'LMV V = 1 against hla_s2g_lm_solve: max |pose difference| = {d:.2e}')
    assert d <= 1e-6
    assert np.allclose(neq_s[0, :, :14].numpy(), one[1][0, :, :14].numpy(), rtol=1e-12, atol=0)


def _refusal(name):
    geom, lv = _case('ragged', 64, 2, 2)
    call = _ViewsCall(geom, [lv], using_weight=1)
    kw = {}
    keep = None
    if name == 'kitti':
        call.cfg.ford = 0
    elif name == 'keep':
        keep = torch.ones(1, (lv.h - lv.row0) * lv.w, dtype=torch.uint8, device=call.dev)
        call.cfg.keep, call.cfg.keep_stride = keep.data_ptr(), keep.shape[1]
    elif name == 'depth':
        call.lv[0].depth = call.t[0][3].data_ptr()
    elif name == 'ray':
        call.lv[0].ray = call.t[0][3].data_ptr()
    elif name == 'reach_mode':
        flag = torch.zeros(2, dtype=torch.int32, device=call.dev)
        keep = flag
        call.cfg.reach_mode, call.cfg.reach_flag = 1, flag.data_ptr()
    elif name == 'count_in_view':
        call.cfg.count_in_view = 1
    elif name in ('sgd', 'adam'):
        call.cfg.optimizer = 1 if name == 'sgd' else 2
    elif name == 'proj':
        call.cfg.proj = 1
    elif name == 'V0':
        kw['V'] = 0
    elif name == 'V9':
        kw['V'] = 9
    elif name == 'workspace':
        kw['short_ws'] = 1
    return call, kw, keep


@pytest.mark.parametrize('name', ['kitti', 'keep', 'depth', 'ray', 'reach_mode', 'count_in_view', 'sgd', 'adam', 'proj', 'V0', 'V9', 'workspace'])
def test_refusals_return_an_error_and_launch_nothing(name):
    call, kw, keep = _refusal(name)
    p0, ruv = _draws(2)
    rc, (trace, neq, vs) = call.forward(p0, ruv, expect_error=True, **kw)
    assert rc != 0 and call.lib.hla_last_error().decode(), name
    assert bool(torch.isnan(trace).all() and torch.isnan(neq).all() and torch.isnan(vs).all()), name
    if name in ('V0', 'V9'):
        assert call.workspace_bytes(V=kw['V']) == 0
    del keep
