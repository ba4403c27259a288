#!/usr/bin/env python3
"""Time LM_G2SP's pose search: (a) ``hla_g2s_pose_score`` at the KITTI level-0 and level-2 shapes (B = 32, K = 27 and 125, 'geo'
and 'nn') against the composition the package offered before it -- ``jacobian.grid_sample`` on K-times-expanded coordinates plus
torch reductions for the same unweighted sums (the coordinates are made on the host outside the timed region, which favours the
baseline) -- with the time of ONE accumulate launch of the LM loop at that level (g2s_accum / g2s_ip_accum, from the library's own
launch timers) times K as a second yardstick, and (b) ``LM_G2SP.forward_search(pose_grid(5, 5, 5), top_m=1)`` against
``forward(mode='test')``.  Device events, warm-up, median of repeats, the legs alternating inside a repeat.
Prints table rows and one JSON line.

Usage:  python tools/g2s_pose_score_bench.py [--batch 32] [--reps 10] [--warmup 3] [--inner 3] [--skip-model]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from highlyaccurate_amd import _lib                              # noqa: E402
from highlyaccurate_amd.jacobian import grid_sample              # noqa: E402
from highlyaccurate_amd.models_kitti import LM_G2SP, pose_grid   # noqa: E402
from oracle import ref_cpu as O                                  # noqa: E402
import g2s_nn_ref as NN                                          # noqa: E402

GRD_HW, SAT_A, CS = (256, 1024), 512, (256, 128, 64)
KITTI_K = [[582.9802 * 1024 / 1242, 0.0, 496.2420 * 1024 / 1242], [0.0, 482.7076 * 256 / 375, 125.0034 * 256 / 375], [0.0, 0.0, 1.0]]


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


def accum_launch_ms(net1, s, g, cam, reps):
    """Median time of the accumulate launch of a one-level, one-iteration LM loop on these maps (the library's launch timers)."""
    net1.lm_solve([s], [g], [None], cam, GRD_HW)
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    for _ in range(reps):
        net1.lm_solve([s], [g], [None], cam, GRD_HW)
    recs = _lib.prof_fetch()
    _lib.prof_enable(False)
    return statistics.median([ms for name, ms, _, _ in recs if name.startswith('lm_accum')])


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
    g = torch.Generator(device=dev).manual_seed(1)
    cam = torch.tensor(KITTI_K, dtype=torch.float32)[None].repeat(B, 1, 1)
    rows = []
    print(f'{"proj":>4} {"lvl":>3} {"C":>4} {"K":>4} | {"fused":>8} {"composed":>9} {"ratio":>6} | {"K x accum":>9}')
    for proj in ('geo', 'nn'):
        args = O.default_args(N_iters=5, proj=proj)
        net = LM_G2SP(args).to(dev).eval()
        net1 = LM_G2SP(O.default_args(N_iters=1, proj=proj)).to(dev).eval()
        sat = [torch.randn(B, SAT_A >> (3 - l), SAT_A >> (3 - l), CS[l], device=dev, generator=g) for l in range(3)]
        ghw = [((GRD_HW[0] >> (3 - l), GRD_HW[1] >> (3 - l)) if proj == 'geo' else (SAT_A >> (3 - l),) * 2) for l in range(3)]
        grd = [torch.randn(B, ghw[l][0], ghw[l][1], CS[l], device=dev, generator=g) for l in range(3)]
        for level in (0, 2):
            A, C, (h, w) = sat[level].shape[1], CS[level], ghw[level]
            img = grd[level].permute(0, 3, 1, 2)                    # NCHW view of the NHWC map
            fix = sat[level]
            acc = accum_launch_ms(net1, sat[level], grd[level], cam.to(dev), a.reps)
            for K in (27, 125):
                poses = pose_grid(3, 3, 3) if K == 27 else pose_grid(5, 5, 5)
                # coordinates of the K poses stacked along the rows: [B, K * A, A, 2] (made once, not timed; every sample has
                # the same intrinsics here, so one sample's coordinates are repeated)
                uv = []
                for k in range(K):
                    p = tuple(poses[k:k + 1, i:i + 1] for i in range(3))
                    if proj == 'geo':
                        u, _, _ = O.g2s_pose_to_uv(args, A, *p, cam[:1], h, w, *GRD_HW, require_jac=False)
                    else:
                        u, _ = NN.inplane_pose_to_uv(args, A, *p)
                    uv.append(u)
                uv = torch.cat(uv, 1).to(dev).expand(B, -1, -1, -1).contiguous()

                def fused():
                    return net.score_poses(sat, grd, [None] * 3, cam, GRD_HW, poses, level)

                def composed():
                    f, _ = grid_sample(img, uv)                     # [B,C,K*A,A], NHWC in memory
                    f = f.permute(0, 2, 3, 1).reshape(B, K, A, A, C)
                    inb = ((uv[..., 0] >= 0) & (uv[..., 0] <= w - 1) & (uv[..., 1] >= 0) & (uv[..., 1] <= h - 1)).reshape(B, K, A, A)
                    s2 = (fix * fix).sum(3)
                    return ((f * f).sum((2, 3, 4)), (s2[:, None] * inb).sum((2, 3)), (f * fix[:, None]).sum((2, 3, 4)), inb.sum((2, 3)))

                try:
                    med = median_ms({'fused': fused, 'composed': composed}, a.reps, a.warmup, a.inner)
                except torch.cuda.OutOfMemoryError:     # the composition holds B x K x A x A x C floats several times over
                    torch.cuda.empty_cache()
                    med = dict(median_ms({'fused': fused}, a.reps, a.warmup, a.inner), composed=float('nan'))
                row = dict(proj=proj, level=level, B=B, C=C, K=K, fused_ms=round(med['fused'], 4), composed_ms=round(med['composed'], 4),
                           ratio=round(med['composed'] / med['fused'], 2), accum_launch_ms=round(acc, 4), k_accum_ms=round(K * acc, 4))
                rows.append(row)
                print(f'{proj:>4} {level:>3} {C:>4} {K:>4} | {med["fused"]:>8.3f} {med["composed"]:>9.3f} {row["ratio"]:>5.1f}x | {K * acc:>9.3f}',
                      flush=True)
                del uv
        del sat, grd
    out = {'g2s_pose_score_bench': rows}
    if not a.skip_model:
        out['forward_search_bench'] = []
        cands = pose_grid(5, 5, 5)
        for proj in ('geo', 'nn'):
            net = LM_G2SP(O.default_args(N_iters=5, proj=proj)).to(dev).eval()
            sat_img = torch.rand(B, 3, SAT_A, SAT_A, device=dev, generator=g)
            grd_img = torch.rand(B, 3, *GRD_HW, device=dev, generator=g)
            camd = cam.to(dev)
            with torch.no_grad():
                legs = {'forward': lambda: net(sat_img, grd_img, camd, mode='test'),
                        'forward_search': lambda: net.forward_search(sat_img, grd_img, camd, cands, top_m=1)}
                med = median_ms(legs, a.reps, a.warmup, a.inner)
            out['forward_search_bench'].append(dict(proj=proj, B=B, precision='fp32', K=125, top_m=1,
                                                    **{k: round(v, 4) for k, v in med.items()},
                                                    added_ms=round(med['forward_search'] - med['forward'], 4)))
            print(f'{proj}: forward_search vs forward (ms): ' + ', '.join(f'{k} {v:.3f}' for k, v in med.items()))
    print('times in ms (median); ratio = composed / fused; K x accum = K launches of the LM loop\'s accumulate kernel at that level')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
