#!/usr/bin/env python3
"""Generate the fixtures of ``LM_G2SP(proj='nn')`` by running the REAL reference on the CPU (build container only, like
oracle/make_golden.py, whose torchvision shim and helpers this script imports):

  tests/golden/vgg_g2s_small.npz     VGGUnet_G2S(4) on a 2 x 3 x 16 x 48 image, non-zero biases: fp32 and fp64 maps and confidences.
                                     (Not kat_small.npz's 32 x 64: with both precisions of all four maps that file would be 2.1 MB,
                                     over the 1 MiB limit for a committed file; 16 x 48 is 0.8 MB.  W = 48 is a multiple of 16,
                                     as the fold needs; the folded maps are 4x3 / 8x6 / 16x12 / 32x24, all partial conv tiles,
                                     and two samples exercise the per-sample strides.)
  tests/golden/e2e_kitti_g2s_nn.npz  full KITTI shape (256 x 1024, A = 512), seeds 1 and 2 as e2e_kitti_g2s.npz: the 15-step
                                     fp32 trace, final pose, train-mode tuple, confidence shapes; for seed 1 gradient samples
                                     ([sum|g|, sum g^2, 64 samples] per key, train_damping = 1) from the reference's autograd, and
                                     the same quantities from the fp64 restatement (tests/g2s_nn_ref.py) -- the reference class
                                     cannot run in fp64 -- which measure the reference's own fp32 rounding
  tests/golden/state_dict_manifest_g2s_nn.json   key -> shape of LM_G2SP(proj='nn').state_dict(), in order

Neither seed is ill-conditioned: |trace_fp32 - restatement_fp64| stays below 1e-3 (printed below), so none was replaced.

Usage:  python tools/make_golden_g2s_nn.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import make_golden as MG  # noqa: E402
from oracle import ref_cpu as O       # noqa: E402
from tests import g2s_nn_ref as R     # noqa: E402

GOLD = MG.GOLD
GRAD_KEYS = MG.GRAD_KEYS + ['GrdFeatureNet.conv_dec2.3.weight', 'damping']


def stat(g):
    g = g.double().reshape(-1)
    return np.concatenate([[g.abs().sum().item(), (g * g).sum().item()], g[MG.sample_idx(g.numel(), 77)].numpy()])


def tuple9(res):
    return np.stack([np.atleast_1d(r.detach().double().numpy()) if r.dim() else np.full(3, float(r.detach())) for r in res[:9]])


def gen_vgg(VGG):
    rs = np.random.RandomState(23)
    sd = O.synth_vgg_state(rs, bias_scale=0.05)
    net = VGG.VGGUnet_G2S(4)
    net.load_state_dict(sd)
    x = torch.from_numpy(rs.random_sample((2, 3, 16, 48)).astype(np.float32))
    out = {'seed': np.array(23), 'x_shape': np.array(x.shape)}
    with torch.no_grad():
        f32, c32 = net(x)
        f64, c64 = net.double()(x.double())
    for l in range(4):
        out[f'vgg_feat32_l{l}'], out[f'vgg_feat64_l{l}'] = f32[l].numpy(), f64[l].numpy()
        out[f'vgg_conf32_l{l}'], out[f'vgg_conf64_l{l}'] = c32[l].numpy(), c64[l].numpy()
    np.savez_compressed(os.path.join(GOLD, 'vgg_g2s_small.npz'), **out)
    print('vgg_g2s_small.npz:', [tuple(f.shape) for f in f64], [tuple(c.shape) for c in c64], flush=True)


def gen_e2e(mk, seeds=(1, 2), B=1):
    torch.Tensor.cuda = lambda self, *a, **k: self          # models_kitti.py:304 calls .cuda() on an index tensor
    args = O.default_args(proj='nn')
    out = {'seeds': np.array(seeds), 'B': np.array(B)}
    for seed in seeds:
        net = mk.LM_G2SP(args)
        torch.autograd.set_detect_anomaly(False)
        sd = O.synth_model_state(seed)
        sd['damping'] = args.damping * torch.ones(1, 3)
        net.load_state_dict(sd)
        if seed == seeds[0]:
            man = [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
            with open(os.path.join(GOLD, 'state_dict_manifest_g2s_nn.json'), 'w') as f:
                json.dump({'LM_G2SP_nn': {'class': 'LM_G2SP', 'args': {'proj': 'nn'}, 'n_tensors': len(man), 'state_dict': man}}, f)
        sat, grd, gu, gv, gh = O.synth_images(seed + 100, B)
        K = torch.tensor([O.KITTI_K], dtype=torch.float32).repeat(B, 1, 1)
        log = []
        orig = net.LM_update

        def wrap(*a, **k):
            r = orig(*a, **k)
            log.append(torch.stack([x.detach()[:, 0] for x in r], -1))
            return r
        net.LM_update = wrap
        with torch.no_grad():
            res = net(sat, grd, K, mode='test')
        out[f'trace32_{seed}'] = torch.stack(log, 1).double().numpy()          # [B, steps, 3] = (u, v, heading)
        out[f'final32_{seed}'] = torch.stack([r.detach() for r in res], -1).double().numpy()
        res = net(sat, grd, K, gu, gv, gh, mode='train')
        assert len(res) == 14
        out[f'tuple32_{seed}'] = tuple9(res)
        out[f'conf_shapes_{seed}'] = np.array([c.shape for c in res[13]])
        # the fp64 column: the restatement
        on = R.LM_G2SP_NN(O.default_args(proj='nn', train_damping=1))
        on.load_state_dict(sd)
        on = on.double()
        ro = on(sat.double(), grd.double(), K, gu.double(), gv.double(), gh.double(), mode='train')
        out[f'otrace64_{seed}'] = on.trace.detach().reshape(B, -1, 3).numpy()
        out[f'otuple64_{seed}'] = tuple9(ro)
        gap = np.abs(out[f'trace32_{seed}'] - out[f'otrace64_{seed}']).max()
        if seed == seeds[0]:          # gradient samples from the reference's own autograd (fp32), train_damping = 1
            net.args.train_damping = 1
            net.zero_grad()
            res = net(sat, grd, K, gu, gv, gh, mode='train')
            res[0].backward()
            sdp = dict(net.named_parameters())
            for k in GRAD_KEYS:
                out[f'grad32_{k}'] = stat(sdp[k].grad)
            out['nograd_32'] = np.array([k for k, p in sdp.items() if p.grad is None])
            net.args.train_damping = 0
            ro[0].backward()
            sdo = dict(on.named_parameters())
            for k in GRAD_KEYS:
                out[f'ograd64_{k}'] = stat(sdo[k].grad)
        print(f'g2s nn seed {seed}: final {out[f"final32_{seed}"].tolist()} first step {out[f"trace32_{seed}"][0, 0].tolist()} '
              f'loss {float(res[0]):.2f} |fp32 - restatement fp64| {gap:.2e}', flush=True)
        assert gap < 1e-3, 'ill-conditioned seed: replace it (see the module docstring)'
    np.savez_compressed(os.path.join(GOLD, 'e2e_kitti_g2s_nn.npz'), **out)


if __name__ == '__main__':
    mk, mf, jac, VGG = MG.import_reference()
    gen_vgg(VGG)
    gen_e2e(mk)
