#!/usr/bin/env python3
"""Time ``hla_s2g_lm_solve_views`` (one LM loop over V views) against V separate ``hla_s2g_lm_solve`` calls on the same maps, at
the Ford benchmark's LM shapes (256x1024 ground images, a 512^2 satellite tile: levels of 256 / 128 / 64 channels, 10 iterations
= 30 steps), through the C ABI on seeded maps.  Whole calls from device events, the two alternating in every repeat after a
warm-up of both; the per-kernel times of the views loop from ``hla_prof`` records in a run of their own.  Medians and the spread.
The V single-view loops do not compute the views loop's result (V poses, not one): the comparison prices the feature.

Usage:  python tools/lm_views_bench.py [--batch 8] [--views 4] [--reps 20] [--warmup 3] [--dtype fp16] [--iters 10]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from highlyaccurate_amd import _lib                                            # noqa: E402
from highlyaccurate_amd._s2gp import ford_K_network_input, ground_plane_table  # noqa: E402

GRD_HW, SAT_A, SIDE_M = (256, 1024), 512, 112.64
LEVELS = ((256, 8), (128, 4), (64, 2))                       # channels, down-sampling of the level's maps
RANGES = (20.0, 20.0, 10.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_config(n_iters):
    cfg = _lib.S2GConfig()
    cfg.ford, cfg.n_levels, cfg.n_iters, cfg.dof = 1, len(LEVELS), n_iters, 3
    cfg.shift_range_lat, cfg.shift_range_lon, cfg.rotation_range = RANGES
    for i in range(3):
        cfg.damping[i] = 0.1
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--dtype', default='fp16', choices=['fp32', 'fp16'])
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    dev = torch.device('cuda:0')
    lib = _lib.load()
    B, V = args.batch, args.views
    J = B * V
    dt, code = (torch.float16, _lib.HLA_F16) if args.dtype == 'fp16' else (torch.float32, _lib.HLA_F32)
    g = torch.Generator(device='cpu').manual_seed(7)
    K = ford_K_network_input()
    keep = []
    lv_views = (_lib.S2GLevel * len(LEVELS))()
    lv_single = [(_lib.S2GLevel * len(LEVELS))() for _ in range(V)]
    for l, (Cn, down) in enumerate(LEVELS):
        h, w, A = GRD_HW[0] // down, GRD_HW[1] // down, SAT_A // down
        sat = (torch.randn(B, A, A, Cn, generator=g) / np.sqrt(Cn * A * A)).to(dt).to(dev)
        # [V,B,...] in memory: view v's maps are one contiguous batch of B for the single-view calls ...
        grd_vb = (torch.randn(V, B, h, w, Cn, generator=g) / np.sqrt(Cn * h * w / 2)).to(dt).to(dev)
        # ... and [B,V,...] (index b * V + v) for the views call: the same values
        grd_bv = grd_vb.transpose(0, 1).contiguous()
        table = ground_plane_table(K, h, w, 256, 1024).to(dev)
        tables = table[None].expand(V, -1, -1, -1).contiguous()
        keep += [sat, grd_vb, grd_bv, table, tables]
        for s, grd, tab in [(lv_views[l], grd_bv, tables)] + [(lv_single[v][l], grd_vb[v], table) for v in range(V)]:
            s.sat_feat, s.grd_feat, s.xyz, s.feat_dtype = sat.data_ptr(), grd.data_ptr(), tab.data_ptr(), code
            s.A, s.h, s.w, s.C, s.row0, s.grd_row_skip = A, h, w, Cn, h // 2, 0
            s.meter_per_pixel, s.centre = SIDE_M / A, float(A // 2)
    rs = np.random.RandomState(9)
    P = np.array([[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]])
    Rm = np.stack([np.array([[np.cos(a), -np.sin(a), 0.], [np.sin(a), np.cos(a), 0.], [0., 0., 1.]]) @ P
                   for a in rs.uniform(-0.3, 0.3, size=J)]).reshape(B, V, 3, 3)
    Tm = np.array([1.7, 0.3, -1.2]) + rs.uniform(-0.5, 0.5, size=(B, V, 3))
    R_bv, T_bv = torch.from_numpy(Rm).float().to(dev), torch.from_numpy(Tm).float().to(dev)
    R_vb, T_vb = R_bv.transpose(0, 1).contiguous(), T_bv.transpose(0, 1).contiguous()
    cfg = make_config(args.iters)
    steps = len(LEVELS) * args.iters
    rand_uv = (torch.rand(steps, 2, B, generator=g) * 2 - 1).to(dev)
    trace = torch.empty(B, args.iters, len(LEVELS), 3, device=dev)
    traces = torch.empty(V, B, args.iters, len(LEVELS), 3, device=dev)
    nv = lib.hla_s2g_views_workspace_bytes(C.byref(cfg), lv_views, B, V)
    n1 = lib.hla_s2g_workspace_bytes(C.byref(cfg), lv_single[0], B)
    ws_v, ws_1 = torch.empty(nv, dtype=torch.uint8, device=dev), torch.empty(n1, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()

    def views():
        _lib.check(lib.hla_s2g_lm_solve_views(C.byref(cfg), lv_views, V, _lib.ptr(R_bv), _lib.ptr(T_bv), None, _lib.ptr(rand_uv),
                                              _lib.ptr(trace), None, None, _lib.ptr(ws_v), nv, B, st), 'hla_s2g_lm_solve_views')

    def singles():
        for v in range(V):
            _lib.check(lib.hla_s2g_lm_solve(C.byref(cfg), lv_single[v], _lib.ptr(R_vb[v]), _lib.ptr(T_vb[v]), None, _lib.ptr(rand_uv),
                                            _lib.ptr(traces[v]), None, _lib.ptr(ws_1), n1, B, st), 'hla_s2g_lm_solve')

    for _ in range(args.warmup):
        views()
        singles()
    torch.cuda.synchronize()
    t_v, t_s = [], []
    for _ in range(args.reps):                               # alternating: both see the same clocks and neighbours
        t_v.append(timed(views))
        t_s.append(timed(singles))
    _lib.prof_enable(True)                                   # a run of its own: the event pairs serialise the launches
    views()
    rec = _lib.prof_fetch()
    _lib.prof_enable(False)
    med, q = statistics.median, lambda x: [round(v, 3) for v in (min(x), max(x))]
    finite = bool(torch.isfinite(trace).all() and torch.isfinite(traces).all())
    out = dict(B=B, V=V, dtype=args.dtype, steps=steps, reps=args.reps, views_call_ms=round(med(t_v), 3), views_min_max_ms=q(t_v),
               single_calls_ms=round(med(t_s), 3), single_min_max_ms=q(t_s), ratio=round(med(t_v) / med(t_s), 3),
               lmv_accum_ms=round(sum(r[1] for r in rec if r[0] == 'lmv_accum'), 3),
               lmv_close_ms=round(sum(r[1] for r in rec if r[0] == 'lmv_close'), 3), launches=len(rec), finite=finite)
    print(json.dumps({'lm_views_bench': out}))


if __name__ == '__main__':
    main()
