#!/usr/bin/env python3
"""Time ``LM_G2SP.score_loss`` at KITTI shapes (B = 32, grd 256 x 1024, sat 512 x 512, ``pose_grid(5, 5, 5)`` as candidates: 126
poses per sample and level, three levels) for proj='geo' without and with weights and for proj='nn': (a) forward + backward,
(b) the same call without the backward (forward under autograd: activations saved), (c) ``forward(mode='train')`` + backward on the
same box for scale; and the share of the score backward kernel (``gpsb_accum``, profiled as "lm_bwd_accum") per level in (a).
Device events, warm-up, median of repeats, the legs alternating inside a repeat.  Prints table rows and one JSON line.

Usage:  python tools/g2s_score_loss_bench.py [--batch 32] [--reps 7] [--warmup 3] [--precision fp16x3]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from highlyaccurate_amd import _lib                                # noqa: E402
from highlyaccurate_amd.models_kitti import LM_G2SP, pose_grid     # noqa: E402
from oracle import ref_cpu as O                                    # noqa: E402

GRD_HW, SAT_A = (256, 1024), 512
KITTI_K = [[582.9802 * 1024 / 1242, 0.0, 496.2420 * 1024 / 1242], [0.0, 482.7076 * 256 / 375, 125.0034 * 256 / 375], [0.0, 0.0, 1.0]]
MODELS = (('geo', 'geo', 0), ('geo weighted', 'geo', 1), ('nn', 'nn', 0))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precision', default='fp16x3')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    dev = torch.device('cuda:0')
    B = a.batch
    sat, grd, gu, gv, gh = [t.to(dev) for t in O.synth_images(3, B, grd_hw=GRD_HW, sat_a=SAT_A)]
    cam = torch.tensor(KITTI_K, dtype=torch.float32)[None].repeat(B, 1, 1).to(dev)
    cands = pose_grid(5, 5, 5)
    rows = []
    for name, proj, uw in MODELS:
        args = O.default_args(N_iters=5, proj=proj, using_weight=uw)
        args.precision = a.precision
        torch.manual_seed(1)
        net = LM_G2SP(args).to(dev).train()

        def zero():
            for p in net.parameters():
                p.grad = None

        def score_fb():
            zero()
            net.score_loss(sat, grd, cam, cands, gu, gv, gh).backward()

        def score_f():
            net.score_loss(sat, grd, cam, cands, gu, gv, gh)

        def train_fb():
            zero()
            net(sat, grd, cam, gu, gv, gh, mode='train')[0].backward()

        legs = {'score_loss_fwd_bwd': score_fb, 'score_loss_fwd': score_f, 'train_fwd_bwd': train_fb}
        for f in legs.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        ts = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                ts[k].append(timed(f))
        med = {k: statistics.median(v) for k, v in ts.items()}
        # one profiled iteration: the score backward's accumulate launches, in level order
        _lib.prof_enable(True)
        _lib.prof_fetch()
        score_fb()
        rec = _lib.prof_fetch()
        _lib.prof_enable(False)
        acc = [ms for kname, ms, _, _ in rec if kname == 'lm_bwd_accum']
        row = dict(model=name, precision=a.precision, B=B, K=int(cands.shape[0]) + 1, **{k: round(v, 3) for k, v in med.items()},
                   gpsb_accum_ms=[round(x, 3) for x in acc],
                   gpsb_share=[round(x / med['score_loss_fwd_bwd'], 4) for x in acc])
        rows.append(row)
        print(f"{name:>12}: score_loss fwd+bwd {med['score_loss_fwd_bwd']:.2f} ms, fwd only {med['score_loss_fwd']:.2f} ms, "
              f"train fwd+bwd {med['train_fwd_bwd']:.2f} ms; gpsb_accum per level {row['gpsb_accum_ms']} ms = {row['gpsb_share']} of fwd+bwd",
              flush=True)
        del net
        torch.cuda.empty_cache()
    print(json.dumps({'g2s_score_loss_bench': rows}))


if __name__ == '__main__':
    main()
