#!/usr/bin/env python3
"""Generate the fixture of ``args.use_gt_depth`` for ``LM_S2GP`` by running the REAL reference on the CPU (build container only,
like tools/make_golden_polar.py, whose helpers in oracle/make_golden.py this script imports):

  tests/golden/e2e_kitti_gt_depth.npz   full KITTI shape (256 x 1024, A = 512), B = 1, seeds 1 and 2, with a 94 x 311 depth map per
                                        seed that is regenerated from its seed (tests/gt_depth_ref.depth_map(seed + 200, B)) and
                                        not stored: the reference's 15-step fp32 trace in both loop orders (``trace32_<seed>``,
                                        ``trace32_lf_<seed>``; [B,N*L,3] iteration-major, i.e. the layout of the model's
                                        [B,N,L,3] trace), its final pose and train-mode tuple, the same from the fp64 restatement
                                        (tests/gt_depth_ref.py), which measures the reference's own fp32 rounding, and the
                                        reference's flat-ground trace of the same inputs (``plain32_<seed>``); for seed 1, with
                                        train_damping = 1, the train tuple and gradient samples ([sum|g|, sum g^2, 64 samples]
                                        per key of oracle.make_golden.GRAD_KEYS) from the reference's autograd (fp32) and the
                                        restatement's (fp64); and, per level, sampled entries and the sum of the reference's
                                        ray table xyz_grds[l][2]

A seed is ill-conditioned if |trace_fp32 - restatement_fp64| exceeds 1e-3: the script stops there and the seed has to be replaced.

Usage:  python tools/make_golden_gt_depth.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import make_golden as MG  # noqa: E402
from oracle import ref_cpu as O       # noqa: E402
from tests import gt_depth_ref as R   # noqa: E402

GOLD = MG.GOLD
TABLE_SALT = 51
DEPTH_SEED = 200          # depth map of fixture seed s: R.depth_map(s + DEPTH_SEED, B)


def stat(g):
    g = g.double().reshape(-1)
    return np.concatenate([[g.abs().sum().item(), (g * g).sum().item()], g[MG.sample_idx(g.numel(), 77)].numpy()])


def tuple9(res):
    return np.stack([np.atleast_1d(r.detach().double().numpy()) if r.dim() else np.full(3, float(r.detach())) for r in res[:9]])


def ref_trace(mk, args, seed, B, depth, level_first):
    """The reference's mode='test' run with LM_update logged -> (trace [B,N*L,3] iteration-major, final [B,3])."""
    net = MG.ref_model(mk, 'LM_S2GP', args, seed, torch.float32)
    sat, grd, *_ = O.synth_images(seed + 100, B)
    log, orig = [], net.LM_update

    def wrap(*a, **k):
        r = orig(*a, **k)
        log.append(torch.stack([x.detach()[:, 0] for x in r[:3]], -1))
        return r
    net.LM_update = wrap
    torch.manual_seed(seed)
    with torch.no_grad():
        res = net(sat, grd, mode='test', gt_depth=depth, level_first=level_first)
    N, L = args.N_iters, args.level
    t = torch.stack(log, 1).double()                       # execution order
    if level_first:
        t = t.reshape(B, L, N, 3).permute(0, 2, 1, 3).reshape(B, N * L, 3)
    return t.numpy(), torch.stack([r.detach() for r in res], -1).double().numpy()


def gen(mk, seeds=(1, 2), B=1):
    args = O.default_args(use_gt_depth=1)
    out = {'seeds': np.array(seeds), 'B': np.array(B), 'depth_hw': np.array(R.DEPTH_HW), 'depth_seed': np.array(DEPTH_SEED)}
    net = MG.ref_model(mk, 'LM_S2GP', args, seeds[0], torch.float32)
    for l in range(4):
        t = net.xyz_grds[l][2].detach().reshape(-1)
        out[f'ray_shape_l{l}'] = np.array(net.xyz_grds[l][2].shape[1:])
        out[f'ray_samples_l{l}'] = t[MG.sample_idx(t.numel(), TABLE_SALT + l)].numpy()
        out[f'ray_sum_l{l}'] = np.array(t.double().sum().item())
    for seed in seeds:
        depth = R.depth_map(seed + DEPTH_SEED, B)
        sat, grd, gu, gv, gh = O.synth_images(seed + 100, B)
        out[f'plain32_{seed}'], _ = ref_trace(mk, args, seed, B, None, 0)
        same, _ = ref_trace(mk, O.default_args(use_gt_depth=0), seed, B, depth, 0)
        assert np.array_equal(same, out[f'plain32_{seed}']), 'use_gt_depth=0 with a depth map is not the plain run'
        for lf, tag in ((0, ''), (1, '_lf')):
            t32, f32 = ref_trace(mk, args, seed, B, depth, lf)
            out[f'trace32{tag}_{seed}'], out[f'final32{tag}_{seed}'] = t32, f32
            on = R.build(args, seed, torch.float64)
            torch.manual_seed(seed)
            with torch.no_grad():
                on(sat.double(), grd.double(), mode='test', gt_depth=depth, level_first=lf)
            out[f'otrace64{tag}_{seed}'] = R.stacked_trace(on, B)
            gap = np.abs(t32 - out[f'otrace64{tag}_{seed}']).max()
            moved = np.abs(t32 - out[f'plain32_{seed}']).max()
            print(f'kitti gt_depth seed {seed} level_first {lf}: final {f32.tolist()} |fp32 - restatement fp64| {gap:.2e} '
                  f'|depth - flat ground| {moved:.2e}', flush=True)
            assert gap < 1e-3, 'ill-conditioned seed: replace it (see the module docstring)'
        net = MG.ref_model(mk, 'LM_S2GP', args, seed, torch.float32)
        torch.manual_seed(seed)
        with torch.no_grad():
            res = net(sat, grd, gu, gv, gh, mode='train', gt_depth=depth)
        assert len(res) == 14
        out[f'tuple32_{seed}'] = tuple9(res)
        on = R.build(args, seed, torch.float64)
        torch.manual_seed(seed)
        with torch.no_grad():
            ro = on(sat.double(), grd.double(), gu.double(), gv.double(), gh.double(), mode='train', gt_depth=depth)
        out[f'otuple64_{seed}'] = tuple9(ro)
    seed = seeds[0]
    depth = R.depth_map(seed + DEPTH_SEED, B)
    atd = O.default_args(use_gt_depth=1, train_damping=1)
    sat, grd, gu, gv, gh = O.synth_images(seed + 100, B)
    net = MG.ref_model(mk, 'LM_S2GP', atd, seed, torch.float32)
    torch.manual_seed(seed)
    res = net(sat, grd, gu, gv, gh, mode='train', gt_depth=depth)
    res[0].backward()
    sdp = dict(net.named_parameters())
    out['tuple32_td'] = tuple9(res)
    for k in MG.GRAD_KEYS:
        out[f'grad32_{k}'] = stat(sdp[k].grad)
    out['nograd_32'] = np.array([k for k, p in sdp.items() if p.grad is None])
    on = R.build(atd, seed, torch.float64)
    torch.manual_seed(seed)
    ro = on(sat.double(), grd.double(), gu.double(), gv.double(), gh.double(), mode='train', gt_depth=depth)
    ro[0].backward()
    sdo = dict(on.named_parameters())
    out['otuple64_td'] = tuple9(ro)
    for k in MG.GRAD_KEYS:
        out[f'ograd64_{k}'] = stat(sdo[k].grad)
    print(f'kitti gt_depth train_damping=1 seed {seed}: loss {float(res[0].detach()):.4f} (restatement fp64 {float(ro[0].detach()):.4f})', flush=True)
    np.savez_compressed(os.path.join(GOLD, 'e2e_kitti_gt_depth.npz'), **out)


if __name__ == '__main__':
    mk, mf, jac, VGG = MG.import_reference()
    gen(mk)
