#!/usr/bin/env python3
"""Time ``hla_g2s_corr`` and ``hla_g2s_corr_bwd`` (the correlation stage of ``LM_G2SP.corr`` behind the extractors and the sampler)
at the three KITTI levels: the contraction kernels from ``hla_prof`` records (the forward MFMA kernel, the two backward gathers),
the whole calls from device events, and -- where it runs -- ``F.conv2d(groups=B)`` on the same operands beside the forward, as
context.  Median of repeats after warm-up.  Prints one table row per level and a JSON line at the end.

Usage:  python tools/g2s_corr_bench.py [--batch 32] [--reps 5] [--warmup 2] [--levels 0,1,2] [--torch-levels 0,1]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from highlyaccurate_amd import _g2s_corr as G, _lib    # noqa: E402

LEVELS = {0: (256, 64, 38), 1: (128, 128, 76), 2: (64, 256, 153)}       # level: C, A, crop (ranges 20 m / 20 m)
PEAK_TFLOPS = 157.3                                                      # fp32 matrix peak of the MI355X


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--levels', default='0,1,2')
    ap.add_argument('--torch-levels', default='0,1')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    dev = torch.device('cuda:0')
    B = args.batch
    rows = []
    for level in (int(x) for x in args.levels.split(',')):
        C, A, crop = LEVELS[level]
        N = A - crop + 1
        rs = np.random.RandomState(C)
        sat = torch.from_numpy(rs.standard_normal((B, A, A, C)).astype(np.float32)).to(dev)
        g2s = torch.from_numpy(rs.standard_normal((B, crop, crop, C)).astype(np.float32)).to(dev)
        sat = sat / sat.reshape(B, -1).norm(dim=1).view(B, 1, 1, 1)
        d_corr = torch.from_numpy(rs.standard_normal((B, N, N)).astype(np.float32)).to(dev)
        d_corr -= d_corr.mean(dim=(1, 2), keepdim=True)
        fwd = lambda: G.corr_forward(sat, g2s, None, None)
        for _ in range(args.warmup):
            corr, saved = fwd()
            G.corr_backward(sat, g2s, None, None, saved, d_corr)
        torch.cuda.synchronize()
        t_f, t_b, k_f, k_b, fl = [], [], [], [], 0.0
        for _ in range(args.reps):
            _lib.prof_enable(True)
            ms, (corr, saved) = timed(fwd)
            rec = _lib.prof_fetch()
            t_f.append(ms)
            k_f.append(sum(r[1] for r in rec if r[0] == 'g2s_corr_dot'))
            fl = sum(r[2] for r in rec if r[0] == 'g2s_corr_dot')
            ms, _ = timed(lambda: G.corr_backward(sat, g2s, None, None, saved, d_corr))
            rec = _lib.prof_fetch()
            _lib.prof_enable(False)
            t_b.append(ms)
            k_b.append(sum(r[1] for r in rec if r[0] == 'g2s_corr_bwd'))
        med = statistics.median
        algo = 2.0 * B * crop * crop * C * N * N
        row = dict(level=level, B=B, C=C, A=A, crop=crop, shifts=N, fwd_call_ms=round(med(t_f), 3), fwd_kernel_ms=round(med(k_f), 3),
                   bwd_call_ms=round(med(t_b), 3), bwd_kernel_ms=round(med(k_b), 3), algorithmic_gflop=round(algo / 1e9, 2),
                   executed_gflop=round(fl / 1e9, 2), fwd_tflops_executed=round(fl / (med(k_f) * 1e-3) / 1e12, 2),
                   fwd_tflops_algorithmic=round(algo / (med(k_f) * 1e-3) / 1e12, 2),
                   fwd_share_of_peak=round(fl / (med(k_f) * 1e-3) / 1e12 / PEAK_TFLOPS, 3), padding_share=round(1 - algo / fl, 3),
                   bwd_tflops_algorithmic=round(2 * algo / (med(k_b) * 1e-3) / 1e12, 2))
        if str(level) in args.torch_levels.split(','):
            try:
                s_t = sat.permute(0, 3, 1, 2).reshape(1, B * C, A, A)
                g_t = g2s.permute(0, 3, 1, 2)
                conv = lambda: torch.nn.functional.conv2d(s_t, g_t, groups=B)
                for _ in range(args.warmup):
                    conv()
                torch.cuda.synchronize()
                row['torch_conv2d_ms'] = round(med([timed(conv)[0] for _ in range(args.reps)]), 3)
            except Exception as e:                      # the grouped conv with a crop-sized kernel may not run at all
                row['torch_conv2d_ms'] = f'failed: {type(e).__name__}'
        rows.append(row)
        print(row, flush=True)
    print(json.dumps({'g2s_corr_bench': rows}))


if __name__ == '__main__':
    main()
