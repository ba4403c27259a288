#!/usr/bin/env python3
"""Time the correlation stage of ``LM_S2GP.orien_corr`` behind the extractors -- window sampling, ``hla_orien_corr``, the triplet
loss -- and its backward down to d(sat map) / d(ground map), at the three KITTI levels (B = 32, rotation_range = 10), against
the same computation written in torch ops on the same GPU (the reference's way: the whole 4W-wide polar map sampled by
``oracle.ref_cpu.grid_sample``, ``cat``, grouped ``conv2d``, ``avg_pool2d``, autograd).  Device events, warm-up, median of
repeats; the two implementations alternate inside each repeat.  Prints one table row per level and a JSON line at the end.

Usage:  python tools/orien_corr_bench.py [--batch 32] [--reps 10] [--warmup 3] [--inner 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from highlyaccurate_amd import _orien                 # noqa: E402
from oracle import ref_cpu as O                       # noqa: E402
from tests import polar_ref as R                      # noqa: E402

LEVELS = [(0, 256, 64, 32, 128), (1, 128, 128, 64, 256), (2, 64, 256, 128, 512)]       # level, C, A, H, W
ROTATION_RANGE = 10.0


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--inner', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    dev = torch.device('cuda:0')
    B = args.batch
    rows = []
    print(f'{"lvl":>3} {"C":>4} {"HxW":>9} {"S":>4} | {"fwd hip":>8} {"fwd torch":>9} {"ratio":>6} | {"f+b hip":>8} {"f+b torch":>9} {"ratio":>6} | '
          f'{"corr TFLOP/s":>12}')
    for level, C, A, H, W in LEVELS:
        rs = np.random.RandomState(C)
        sat = torch.from_numpy(rs.standard_normal((B, A, A, C)).astype(np.float32)).to(dev)
        grd = torch.from_numpy(rs.standard_normal((B, H, W, C)).astype(np.float32)).to(dev)
        sat, grd = sat / sat.reshape(B, -1).norm(dim=1).view(B, 1, 1, 1), grd / grd.reshape(B, -1).norm(dim=1).view(B, 1, 1, 1)
        gh = torch.from_numpy(rs.uniform(-1, 1, B).astype(np.float32)).to(dev)
        deg, n = _orien.shifts(ROTATION_RANGE, W)
        full = _orien.polar_coordinates(O.meter_per_pixel() * 2 ** (3 - level), level)
        cols = torch.tensor(_orien.window_columns(full.shape[2], W, n))
        grid = full[:, :, cols, :].expand(B, -1, -1, -1).contiguous().to(dev)
        S = 2 * n + 1
        one = torch.ones(1, device=dev)
        loss = torch.empty(1, device=dev)

        def hip_fwd():
            P1 = _orien.sample_window(sat, grid)
            corr, saved = _orien.corr_forward(P1, grd, None, None)
            _orien.triplet_loss(corr, gh, ROTATION_RANGE, deg, loss, False)
            return P1, corr, saved

        def hip_fb():
            P1, corr, saved = hip_fwd()
            d_corr = _orien.triplet_loss_bwd(corr, gh, ROTATION_RANGE, deg, one)
            d_P1, d_grd = _orien.corr_backward(P1, grd, None, None, saved, d_corr)
            return _orien.sample_window_bwd(sat, grid, d_P1), d_grd

        sat_t = sat.permute(0, 3, 1, 2).detach().requires_grad_(True)           # NCHW-shaped, channels-last in memory
        grd_t = grd.permute(0, 3, 1, 2).detach().requires_grad_(True)
        full_d = full.to(dev).repeat(B, 1, 1, 1)
        gt = gh.view(B, 1)

        def torch_loss():
            g = torch.nn.functional.normalize(grd_t.reshape(B, -1)).reshape(B, C, H, W)      # (corr_from_window normalises again: a no-op)
            P, _ = O.grid_sample(sat_t, full_d)
            return R.triplet_loss([(R.corr_from_window(R.polar_window(P, W, n), g), deg)], gt, ROTATION_RANGE)

        def torch_fwd():
            with torch.no_grad():
                torch_loss()

        def torch_fb():
            torch_loss().backward()
            sat_t.grad = grd_t.grad = None
        legs = {'fwd_hip': hip_fwd, 'fwd_torch': torch_fwd, 'fb_hip': hip_fb, 'fb_torch': torch_fb}
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        ts = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, f in legs.items():          # alternate the implementations inside a repeat
                ts[k].append(timed(f, args.inner))
        corr_only = statistics.median(timed(lambda: _orien.corr_forward(hip_fwd()[0], grd, None, None), args.inner) for _ in range(args.reps))
        med = {k: statistics.median(v) for k, v in ts.items()}
        flop = 2.0 * B * H * W * S * C
        row = dict(level=level, B=B, C=C, H=H, W=W, S=S, **{k: round(v, 4) for k, v in med.items()},
                   fwd_ratio=round(med['fwd_torch'] / med['fwd_hip'], 2), fb_ratio=round(med['fb_torch'] / med['fb_hip'], 2),
                   corr_gflop=round(flop / 1e9, 2), fwd_stage_tflops=round(flop / (med['fwd_hip'] * 1e-3) / 1e12, 2),
                   fwd_plus_corr_ms=round(corr_only, 4))
        rows.append(row)
        print(f'{level:>3} {C:>4} {H:>4}x{W:<4} {S:>4} | {med["fwd_hip"]:>8.3f} {med["fwd_torch"]:>9.3f} {row["fwd_ratio"]:>5.1f}x | '
              f'{med["fb_hip"]:>8.3f} {med["fb_torch"]:>9.3f} {row["fb_ratio"]:>5.1f}x | {row["fwd_stage_tflops"]:>12.2f}', flush=True)
    print('times in ms (median); ratio = torch ops / HIP; TFLOP/s = 2 B H W S C of the contraction over the whole forward stage (sampling included)')
    print(json.dumps({'orien_corr_bench': rows}))


if __name__ == '__main__':
    main()
