#!/usr/bin/env python3
"""Time the pose search: (a) ``hla_s2g_pose_score`` at the KITTI level-0 and level-2 shapes (B = 32, K = 27 and 125, fp32 and fp16
maps) against the composition the package offered before it -- ``jacobian.grid_sample`` on K-times-expanded coordinates plus
torch reductions for the same unweighted sums (the coordinates are made on the host outside the timed region, which favours the baseline) --
and (b) ``LM_S2GP.forward_search(pose_grid(5, 5, 5), top_m=1)`` against ``forward(mode='test')`` in bf16, with the scoring and the
finest-level rescoring timed on their own.  Device events, warm-up, median of repeats, the legs alternating inside a repeat.
Prints table rows and one JSON line.

Usage:  python tools/pose_score_bench.py [--batch 32] [--reps 10] [--warmup 3] [--inner 3] [--skip-model]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from highlyaccurate_amd.jacobian import grid_sample           # noqa: E402
from highlyaccurate_amd.models_kitti import LM_S2GP, pose_grid  # noqa: E402
from highlyaccurate_amd import utils                            # noqa: E402
from oracle import ref_cpu as O                                 # noqa: E402
import lm_kernel_ref as R                                       # noqa: E402

GRD_HW, SAT_A, CS = (256, 1024), 512, (256, 128, 64)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def median_ms(legs, reps, warmup, inner):
    for f in legs.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            ts[k].append(timed(f, inner))
    return {k: statistics.median(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--skip-model', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    dev = torch.device('cuda:0')
    B = a.batch
    args = O.default_args(N_iters=5)
    net = LM_S2GP(args).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    sat = [torch.randn(B, SAT_A >> (3 - l), SAT_A >> (3 - l), CS[l], device=dev, generator=g) for l in range(3)]
    grd = [torch.randn(B, GRD_HW[0] >> (3 - l), GRD_HW[1] >> (3 - l), CS[l], device=dev, generator=g) for l in range(3)]
    tables = net.xyz_tables(GRD_HW[0], GRD_HW[1], dev)
    ranges = (args.shift_range_lat, args.shift_range_lon, args.rotation_range)
    rows = []
    print(f'{"lvl":>3} {"C":>4} {"K":>4} {"maps":>5} | {"fused":>8} {"composed":>9} {"ratio":>6}')
    for level in (0, 2):
        A, C, (h, w) = sat[level].shape[1], CS[level], grd[level].shape[1:3]
        row0 = h // 2
        mpp = utils.get_meter_per_pixel() * utils.get_process_satmap_sidelength() / A
        for K in (27, 125):
            poses = pose_grid(3, 3, 3) if K == 27 else pose_grid(5, 5, 5)
            pd, tab = poses, tables[level].cpu()
            # coordinates of the K poses stacked along the rows: [B, K * (h - row0), w, 2] (made once, not timed)
            uv = []
            for k in range(K):
                p = tuple(pd[k:k + 1, i:i + 1].expand(B, 1) for i in range(3))
                u, _, mask = R.pose_to_uv_kitti(tab, *p, A, mpp, A / 2.0, ranges)
                uv.append(u[:, row0:])
            uv = torch.cat(uv, 1).contiguous().to(dev)
            m = (tables[level][row0:, :, 2] > 0).float()[None, :, :, None]
            for dt in (torch.float32, torch.float16):
                s_l = [t.to(dt) for t in sat]
                g_l = [t.to(dt) for t in grd]
                img = s_l[level].permute(0, 3, 1, 2)                # NCHW view of the NHWC map

                def fused():
                    return net.score_poses(s_l, g_l, [None] * 3, GRD_HW, poses, level)

                def composed():
                    f, _ = grid_sample(img, uv)                     # [B,C,K*h',w], NHWC in memory
                    f = f.permute(0, 2, 3, 1).reshape(B, K, h - row0, w, C) * m[:, None]
                    gm = g_l[level][:, row0:].float() * m
                    inb = ((uv[..., 0] >= 0) & (uv[..., 0] <= A - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= A - 1)).reshape(B, K, -1)
                    return ((f * f).sum((2, 3, 4)), (gm * gm).sum((1, 2, 3)), (f * gm[:, None]).sum((2, 3, 4)),
                            (inb & (m.reshape(1, 1, -1) > 0)).sum(2))

                med = median_ms({'fused': fused, 'composed': composed}, a.reps, a.warmup, a.inner)
                row = dict(level=level, B=B, C=C, K=K, maps=str(dt)[6:], fused_ms=round(med['fused'], 4),
                           composed_ms=round(med['composed'], 4), ratio=round(med['composed'] / med['fused'], 2))
                rows.append(row)
                print(f'{level:>3} {C:>4} {K:>4} {row["maps"]:>5} | {med["fused"]:>8.3f} {med["composed"]:>9.3f} {row["ratio"]:>5.1f}x', flush=True)
                del s_l, g_l, img
            del uv
    out = {'pose_score_bench': rows}
    if not a.skip_model:
        net = LM_S2GP(O.default_args(N_iters=5, precision='bf16')).to(dev).eval()
        sat_img = torch.rand(B, 3, SAT_A, SAT_A, device=dev, generator=g)
        grd_img = torch.rand(B, 3, *GRD_HW, device=dev, generator=g)
        cands = pose_grid(5, 5, 5)
        with torch.no_grad():
            sf, si, gf, gc, gi = net._features(sat_img, grd_img, False, False)
            net.forward_search(sat_img, grd_img, cands)
            finals = net.last_search['traces'][:, :, -1, -1, :].contiguous()
            legs = {'forward': lambda: net(sat_img, grd_img, mode='test'),
                    'forward_search': lambda: net.forward_search(sat_img, grd_img, cands, top_m=1),
                    'score_125_level0': lambda: net.score_poses(sf, gf, gc, GRD_HW, cands, 0, None, si, gi),
                    'rescore_1_level2': lambda: net.score_poses(sf, gf, gc, GRD_HW, finals, 2, None, si, gi)}
            med = median_ms(legs, a.reps, a.warmup, a.inner)
        out['forward_search_bench'] = dict(B=B, precision='bf16', K=125, top_m=1, **{k: round(v, 4) for k, v in med.items()},
                                           added_ms=round(med['forward_search'] - med['forward'], 4))
        print('forward_search vs forward (ms): ' + ', '.join(f'{k} {v:.3f}' for k, v in med.items()))
    print('times in ms (median); ratio = composed / fused')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
