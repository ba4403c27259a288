"""O.VGGUnet's forward with its ReLU and 2x2 max-pool decisions made explicit, for references that take the GPU's side of
knife-edges.

TEST INFRASTRUCTURE ONLY.  ``forward`` computes what ``O.VGGUnet.forward`` computes (``oracle/ref_cpu.py``), in the
dtype of the module, with every ReLU written as ``z * mask`` and every max-pool as a gather at an argmax index (2 * row + col
inside the window, first maximum in row-major order, like ``F.max_pool2d``).  Left to itself it takes its own decisions and
its autograd equals the oracle's; given ``dec`` it takes those instead.  A decision whose margin (|z|, or the gap between a
window's two largest values) lies below the forward error of the kernels is a knife-edge: the kernels may take either side,
and the backward routes the gradient accordingly.  The decision points, in forward order, with the map that holds the
kernels' side of them (``vgg_plan``, ``highlyaccurate_amd/csrc/vgg_layers.h``):

  relu: a0 (conv0), x3, a5, x8, a10, a12, x15r, d1a, x18r, d2a, x21r, and at level 4 x2r, d3a, x24r
  pool: x3 (idx3), x8 (idx8), x15 (idx15)
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

RELUS = ['a0', 'x3', 'a5', 'x8', 'a10', 'a12', 'x15r', 'd1a', 'x18r', 'd2a', 'x21r']
RELUS4 = ['x2r', 'd3a', 'x24r']
POOLS = ['x3', 'x8', 'x15']


def windows(t):
    """[B, C, H, W] -> [B, C, H/2, W/2, 4], the last index 2 * row + col of the 2x2 window."""
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def forward(net: O.VGGUnet, x: torch.Tensor, dec: dict = None, record: dict = None):
    """(feats, confs) of ``net`` (an ``O.VGGUnet``) on ``x``.  ``dec``: {('relu', name): bool mask, ('pool', name): int64
    index} to take; the rest is decided here.  ``record`` (a dict) receives, per decision point, the decision taken and its
    margin relative to the sample's largest |value| of that map."""
    dec = dec or {}

    def relu(name, z):
        m = dec.get(('relu', name))
        if m is None:
            m = z > 0
        if record is not None:
            s = z.detach().abs().amax((1, 2, 3), keepdim=True).clamp_min(1e-300)
            record[('relu', name)] = (m, z.detach().abs() / s)
        return z * m.to(z.dtype)

    def pool(name, t):
        w = windows(t)
        i = dec.get(('pool', name))
        if i is None:
            i = w.detach().argmax(-1)
        if record is not None:
            top = w.detach().topk(2, -1).values
            s = t.detach().abs().amax((1, 2, 3), keepdim=True).unsqueeze(-1).clamp_min(1e-300)[..., 0]
            record[('pool', name)] = (i, (top[..., 0] - top[..., 1]) / s)
        return torch.gather(w, -1, i.unsqueeze(-1)).squeeze(-1)

    up = lambda t, like: F.interpolate(t, like.shape[2:], mode='nearest')
    a0 = relu('a0', net.conv0(x))
    x2 = net.conv2(a0)
    x3 = relu('x3', pool('x3', x2))
    a5 = relu('a5', net.conv5(x3))
    x8 = relu('x8', pool('x8', net.conv7(a5)))
    a10 = relu('a10', net.conv10(x8))
    a12 = relu('a12', net.conv12(a10))
    x15 = pool('x15', net.conv14(a12))
    x15r = relu('x15r', x15)
    d1a = relu('d1a', net.conv_dec1[1](torch.cat([up(x15r, x8), x8], 1)))
    x18 = net.conv_dec1[3](d1a)
    x18r = relu('x18r', x18)
    d2a = relu('d2a', net.conv_dec2[1](torch.cat([up(x18r, x3), x3], 1)))
    x21 = net.conv_dec2[3](d2a)
    x21r = relu('x21r', x21)
    raws, acts = [x15, x18, x21], [x15r, x18r, x21r]
    if net.level == 4:
        x2r = relu('x2r', x2)
        d3a = relu('d3a', net.conv_dec3[1](torch.cat([up(x21r, x2r), x2r], 1)))
        x24 = net.conv_dec3[3](d3a)
        raws.append(x24)
        acts.append(relu('x24r', x24))
    heads = (net.conf0, net.conf1, net.conf2, net.conf3)
    confs = [torch.sigmoid(-torch.sigmoid(heads[l][1](a))) for l, a in enumerate(acts)]
    return [O.l2_norm_map(t) for t in raws], confs
