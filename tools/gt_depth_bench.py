#!/usr/bin/env python3
"""Time the fused LM loop with and without a depth map (``args.use_gt_depth``) at B = 32 and KITTI shapes: the 15-step forward
(``lm_solve``) and its backward (``lm_backward``), on random feature pyramids, (a) flat ground, (b) with a 375 x 1242 depth map per
sample.  For scale, (c) the same projection composed of torch ops around ``jacobian.grid_sample``
(tests/grid_sample_grad_ref.gt_depth_projection) for ONE step at the finest level, forward and forward + backward: that form
materialises the [3,B,C,h,w] Jacobian which the fused loop exists to avoid; its size is reported.  Device events, warm-up, median
of repeats; the variants alternate inside each repeat.  Prints a table and one JSON line.

Usage:  python tools/gt_depth_bench.py [--reps 10] [--warmup 3] [--batch 32]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from highlyaccurate_amd import synthetic, utils                 # noqa: E402
from highlyaccurate_amd.jacobian import grid_sample             # noqa: E402
from highlyaccurate_amd.models_kitti import LM_S2GP             # noqa: E402
from tests.grid_sample_grad_ref import gt_depth_projection      # noqa: E402

GRD_HW, SAT_A, CS = (256, 1024), 512, (256, 128, 64)
DEPTH_HW = (375, 1242)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    d = torch.device('cuda:0')
    B = a.batch
    g = torch.Generator(device=d)
    g.manual_seed(1)
    sat = [torch.randn(B, SAT_A >> (3 - l), SAT_A >> (3 - l), c, device=d, generator=g) for l, c in enumerate(CS)]
    grd = [torch.randn(B, GRD_HW[0] >> (3 - l), GRD_HW[1] >> (3 - l), c, device=d, generator=g) for l, c in enumerate(CS)]
    depth = synthetic.gt_depth(B, *DEPTH_HW, 7, d)
    net = LM_S2GP(synthetic.reference_args(use_gt_depth=1)).to(d)
    d_trace = torch.randn(B, net.N_iters, 3, 3, device=d, generator=g)
    state = {}

    def fwd(dep):
        torch.manual_seed(0)
        state[dep is None] = (net.lm_solve(sat, grd, [None] * 3, GRD_HW, None, 0, keep_normal_eq=True, gt_depth=dep), net.last_normal_eq)

    def bwd(dep):
        tr, neq = state[dep is None]
        net.lm_backward(sat, grd, [None] * 3, GRD_HW, tr, neq, d_trace, None, 0, gt_depth=dep)

    # (c) one step of the composed form at the finest level
    l = 2
    A, h, w, Cn = sat[l].shape[1], grd[l].shape[1], grd[l].shape[2], CS[l]
    rays = net.ray_tables(*GRD_HW, d)[l]
    ri, ci = net.depth_indices(h, w, *DEPTH_HW, d)
    dl = depth[:, ri.long()][:, :, ci.long()]
    sat_nchw = sat[l].permute(0, 3, 1, 2).detach().requires_grad_(True)        # channels-last storage, as the operator likes it
    pose = torch.zeros(B, 3, device=d, requires_grad=True)
    w_out, w_jac = torch.ones(1, device=d), torch.ones(3, 1, 1, 1, 1, device=d)
    mpp = utils.get_meter_per_pixel() * utils.get_process_satmap_sidelength() / A
    jac_bytes = 3 * B * Cn * h * w * 4

    def composed(backward):
        with torch.set_grad_enabled(backward):
            loss = gt_depth_projection(grid_sample, sat_nchw, pose, rays, dl, w_out, w_jac, A, shift=20.0, mpp=mpp)
        if backward:
            loss.backward()
            sat_nchw.grad = pose.grad = None

    legs = {'fwd_plain': lambda: fwd(None), 'fwd_depth': lambda: fwd(depth), 'bwd_plain': lambda: bwd(None), 'bwd_depth': lambda: bwd(depth),
            'composed_step_fwd': lambda: composed(False), 'composed_step_fwd_bwd': lambda: composed(True)}
    for f in legs.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, f in legs.items():
            ts[k].append(timed(f))
    med = {k: round(statistics.median(v), 4) for k, v in ts.items()}
    spread = {k: [round(min(v), 4), round(max(v), 4)] for k, v in ts.items()}
    moved = float((state[False][0] - state[True][0]).abs().max())
    print(f'B = {B}, KITTI shapes, 15 LM steps; depth map {DEPTH_HW[0]} x {DEPTH_HW[1]}; median ms over {a.reps} repeats [min, max]')
    for k in legs:
        print(f'  {k:<24} {med[k]:>9.3f}  {spread[k]}')
    print(f'  composed form, one step at the finest level (C = {Cn}, {h} x {w}): materialises a [3,{B},{Cn},{h},{w}] fp32 Jacobian = '
          f'{jac_bytes / 2 ** 20:.0f} MiB (x 15 steps over three levels in the reference); the fused loop forms none')
    print(f'  |trace with depth - trace without| = {moved:.3e}')
    print(json.dumps({'gt_depth_bench': dict(B=B, reps=a.reps, median_ms=med, min_max_ms=spread, composed_jacobian_bytes=jac_bytes,
                                             depth_hw=DEPTH_HW, trace_moved=moved)}))


if __name__ == '__main__':
    main()
