#!/usr/bin/env python3
"""Generate tests/golden/grid_sample_grad.npz by running the REAL reference's ``jacobian.grid_sample`` under autograd on the
CPU (build container only, like oracle/make_golden.py, whose torchvision shim this script imports).  Arrays only.

Cases S1 and S2 of tests/grid_sample_grad_ref.py (inputs regenerated on both sides from ``numpy.random.RandomState(seed)``;
loss = sum(out * g_out) + sum(jac_out * g_jac)).  Per case <k>:

  <k>_seed, <k>_shape (N, C, IH, IW, H, W, M), <k>_planted [5,2]   the coordinates planted in batch 0
  <k>_g_out, <k>_g_jac                    the two cotangents -- S1 whole; S2 as (sum, sum of squares, first 64 elements): they
                                          are part of the seeded stream, and whole they would be 370 KB
  <k>_d_optical{32,64}, <k>_d_jac{32,64}  the reference's gradients in fp32 and in fp64, whole
  <k>_d_image{32,64}                      S1 whole; S2 (41 472 elements, 500 KB in both precisions) at the 2048 flat indices
                                          <k>_d_image_idx, plus <k>_d_image_stat{32,64} = (sum |g|, sum g^2) over the whole tensor

Usage:  python tools/make_golden_grid_sample_grad.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import make_golden as MG          # noqa: E402
from tests import grid_sample_grad_ref as R   # noqa: E402

N_IDX = 2048


def brief(a):
    a = a.astype(np.float64).reshape(-1)
    return np.concatenate([[a.sum(), (a * a).sum()], a[:64]])


def stat(g):
    g = g.double().reshape(-1)
    return np.array([g.abs().sum().item(), (g * g).sum().item()])


def main():
    jac_mod = MG.import_reference()[2]
    out = {}
    for k in ('S1', 'S2'):
        img, uv, jac, g_out, g_jac = R.make_case(k)
        N, C, IH, IW, H, W, M = R.CASES[k]
        whole = k == 'S1'
        out[f'{k}_seed'], out[f'{k}_shape'], out[f'{k}_planted'] = np.array(R.SEEDS[k]), np.array(R.CASES[k]), R.planted(IH, IW)
        out[f'{k}_g_out'], out[f'{k}_g_jac'] = (g_out, g_jac) if whole else (brief(g_out), brief(g_jac))
        idx = None if whole else np.sort(np.random.RandomState(R.SEEDS[k] + 1000).choice(img.size, N_IDX, replace=False))
        if idx is not None:
            out[f'{k}_d_image_idx'] = idx
        for bits, dt in ((32, torch.float32), (64, torch.float64)):
            ts = [R.T(a, dt) for a in (img, uv, jac, g_out, g_jac)]
            d_img, d_uv, d_jac = R.grads(jac_mod.grid_sample, ts[0], ts[1], ts[2], R.linear_loss(ts[3], ts[4]))
            out[f'{k}_d_optical{bits}'], out[f'{k}_d_jac{bits}'] = d_uv.numpy(), d_jac.numpy()
            if whole:
                out[f'{k}_d_image{bits}'] = d_img.numpy()
            else:
                out[f'{k}_d_image{bits}'] = d_img.numpy().reshape(-1)[idx]
                out[f'{k}_d_image_stat{bits}'] = stat(d_img)
        gap = {n: np.abs(out[f'{k}_{n}32'].astype(np.float64) - out[f'{k}_{n}64']).max() for n in ('d_image', 'd_optical', 'd_jac')}
        print(k, 'reference |fp32 - fp64|:', {n: f'{v:.2e}' for n, v in gap.items()}, flush=True)
    path = os.path.join(MG.GOLD, 'grid_sample_grad.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
