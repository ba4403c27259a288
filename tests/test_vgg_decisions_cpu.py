"""CPU checks of ``vgg_decisions``: the explicit-decision VGGUnet forward behind the GPU backward references."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
import vgg_decisions as D


def _setup(level):
    rs = np.random.RandomState(17)
    sd = O.synth_vgg_state(rs, bias_scale=0.05)
    x = torch.from_numpy(rs.random_sample((2, 3, 16, 48)))
    net = O.VGGUnet(level)
    net.load_state_dict(sd)
    return net.double(), x, rs


def _grads(net, feats, confs, ups):
    net.zero_grad()
    sum((u * t).sum() for u, t in zip(ups, feats + confs)).backward()
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('level', [3, 4])
def test_own_decisions_are_the_oracle(level):
    """Left to itself (and given its own recorded decisions back) the forward and its autograd are the oracle's."""
    net, x, rs = _setup(level)
    f, c = net(x)
    ups = [torch.from_numpy(rs.standard_normal(tuple(t.shape))) for t in f + c]
    ref = _grads(net, f, c, ups)
    rec = {}
    f1, c1 = D.forward(net, x, record=rec)
    assert len(rec) == len(D.RELUS) + len(D.POOLS) + (len(D.RELUS4) if level == 4 else 0)
    for a, b in zip(f1 + c1, f + c):
        assert (a - b).abs().max() <= 1e-15 * b.abs().max()
    for dec in (None, {k: m for k, (m, _) in rec.items()}):
        f2, c2 = D.forward(net, x, dec)
        g = _grads(net, f2, c2, ups)
        assert set(g) == set(ref)
        for k in ref:
            assert (g[k] - ref[k]).abs().max() <= 1e-12 * ref[k].abs().max(), k


def test_a_taken_decision_moves_the_gradient():
    """Flipping one ReLU decision (the smallest |z| at conv10's output) or one pool argmax (the closest window of conv7's)
    moves the gradients below it (conv10 / conv7, and conv0) and leaves those above it (conv12 / conv10): a flip at a knife-edge changes the forward
    values by at most its margin (1e-6 of the map here), the gradient routing entirely."""
    net, x, rs = _setup(3)
    rec = {}
    f, c = D.forward(net, x, record=rec)
    ups = [torch.from_numpy(rs.standard_normal(tuple(t.shape))) for t in f + c]
    base = _grads(net, f, c, ups)
    for key, below, above in ((('relu', 'a10'), 'conv10.weight', 'conv12.weight'), (('pool', 'x8'), 'conv7.weight', 'conv10.weight')):
        dec = {k: m.clone() for k, (m, _) in rec.items()}
        m, margin = rec[key]
        if key[0] == 'pool':        # (a window whose maximum survives the ReLU behind the pool)
            margin = margin + (~rec['relu', 'x8'][0]).double()
        i = np.unravel_index(int(torch.argmin(margin)), m.shape)
        dec[key][i] = (not bool(m[i])) if key[0] == 'relu' else (int(m[i]) + 1) % 4
        f2, c2 = D.forward(net, x, dec)
        g = _grads(net, f2, c2, ups)
        moved = {k for k in base if (g[k] - base[k]).norm() > 1e-4 * base[k].norm()}
        assert below in moved and 'conv0.weight' in moved, (key, moved)
        assert above not in moved and 'conv_dec1.3.weight' not in moved, (key, moved)
