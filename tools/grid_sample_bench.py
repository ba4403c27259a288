#!/usr/bin/env python3
"""Time ``jacobian.grid_sample`` forward and forward + backward on the GPU against the same call made of plain torch ops
(``oracle.ref_cpu.grid_sample`` run on the GPU: the reference's way).  Device events, warm-up, median of repeats; the two
implementations alternate inside each repeat.  Prints one table row per (shape, wanted gradients) and a JSON line at the end.

The atomic rate is 4 taps x C x 4 B x samples in view / time of the backward alone (forward + backward minus forward); the
chip-wide figure it is set beside, about 1.3 TB/s of added bytes, is the programming guide's, not one measured on this kernel.

Usage:  python tools/grid_sample_bench.py [--reps 20] [--warmup 5] [--inner 10]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from highlyaccurate_amd.jacobian import grid_sample   # noqa: E402
from oracle import ref_cpu as O                       # noqa: E402

SHAPES = [(256, 64, 32, 128), (128, 128, 64, 256), (64, 256, 128, 512)]       # C, IH = IW, H, W
N, M = 4, 3
GUIDE_ATOMIC_TBS = 1.3


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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    dev = torch.device('cuda:0')
    rows = []
    print(f'{"C":>4} {"IHxIW":>9} {"HxW":>9} {"grads":>6} | {"fwd hip":>8} {"fwd torch":>9} {"ratio":>6} | {"f+b hip":>8} {"f+b torch":>9} '
          f'{"ratio":>6} | {"bwd ms":>7} {"atomic TB/s":>11}')
    for C, S, H, W in SHAPES:
        rs = np.random.RandomState(C)
        img = torch.from_numpy(rs.standard_normal((N, S, S, C)).astype(np.float32)).to(dev).permute(0, 3, 1, 2)   # channels-last
        uv = torch.from_numpy(rs.uniform(-0.1 * S, 1.1 * S, (N, H, W, 2)).astype(np.float32)).to(dev)
        jac = torch.from_numpy(rs.standard_normal((M, N, H, W, 2)).astype(np.float32)).to(dev)
        g_out = torch.randn(N, C, H, W, device=dev)
        g_jac = torch.randn(M, N, C, H, W, device=dev)
        in_view = int(((uv[..., 0] >= 0) & (uv[..., 0] <= S - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= S - 1)).sum())
        for label, need in (('image', (True, False, False)), ('all', (True, True, True))):
            leaves = [t.detach().requires_grad_(n) for t, n in zip((img, uv, jac), need)]

            def fwd(fn):
                with torch.no_grad():
                    fn(*leaves)

            def fwd_bwd(fn):
                out, jout = fn(*leaves)
                torch.autograd.backward([out, jout], [g_out, g_jac])
                for t in leaves:
                    t.grad = None
            legs = {'fwd_hip': lambda: fwd(grid_sample), 'fwd_torch': lambda: fwd(O.grid_sample),
                    'fb_hip': lambda: fwd_bwd(grid_sample), 'fb_torch': lambda: fwd_bwd(O.grid_sample)}
            for f in legs.values():
                for _ in range(args.warmup):
                    f()
            torch.cuda.synchronize()
            ts = {k: [] for k in legs}
            for _ in range(args.reps):
                for k, f in legs.items():          # alternate the implementations inside a repeat
                    ts[k].append(timed(f, args.inner))
            med = {k: statistics.median(v) for k, v in ts.items()}
            bwd = med['fb_hip'] - med['fwd_hip']
            tbs = 4 * C * 4 * in_view / (bwd * 1e-3) / 1e12 if bwd > 0 else float('nan')
            row = dict(C=C, IH=S, IW=S, H=H, W=W, grads=label, in_view=in_view, **{k: round(v, 4) for k, v in med.items()},
                       fwd_ratio=round(med['fwd_torch'] / med['fwd_hip'], 2), fb_ratio=round(med['fb_torch'] / med['fb_hip'], 2),
                       bwd_ms=round(bwd, 4), atomic_TBs=round(tbs, 3), guide_atomic_TBs=GUIDE_ATOMIC_TBS)
            rows.append(row)
            print(f'{C:>4} {S:>4}x{S:<4} {H:>4}x{W:<4} {label:>6} | {med["fwd_hip"]:>8.3f} {med["fwd_torch"]:>9.3f} {row["fwd_ratio"]:>5.1f}x | '
                  f'{med["fb_hip"]:>8.3f} {med["fb_torch"]:>9.3f} {row["fb_ratio"]:>5.1f}x | {bwd:>7.3f} {tbs:>11.3f}', flush=True)
    print('times in ms (median); ratio = torch ops / HIP; atomic TB/s beside the guide\'s chip-wide %.1f TB/s (not measured here)' % GUIDE_ATOMIC_TBS)
    print(json.dumps({'grid_sample_bench': rows}))


if __name__ == '__main__':
    main()
