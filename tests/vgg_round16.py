"""Rounding-aware CPU restatement of the library's bf16 / fp16 VGGUnet forward.

TEST INFRASTRUCTURE ONLY.  ``oracle/ref_cpu.py`` restates the reference; this file restates *our* 16-bit forward: the
same arithmetic as ``O.VGGUnet`` (``oracle/ref_cpu.py``, ``raw_maps`` / ``forward``), with every value rounded to the
16-bit type T (round to nearest even) exactly where the kernels store or feed one.  Rounding points (file:line relative
to ``highlyaccurate_amd/csrc``):

  * packed weights: every conv weight is rounded to T (``conv_kernels.h:1676``, ``out[e] = (T)v``)
  * the fp32 input image: converted to T inside ``conv02_kernel`` (``conv_kernels.h:1476``)
  * conv0's bias: a T hi + lo pair in k slots 27 / 28 against an input of 1.0 (``conv_kernels.h:1665-1666``, ``:1458-1459``)
  * relu(conv0): staged in LDS as T for conv2 (``conv_kernels.h:1506``); pixels outside the image are 0 (conv2's zero pad)
  * stored post-ReLU / pooled activations: rounded to T (``store4``, ``conv_kernels.h:166-173``, by the epilogues):
    x3, a5, x8, a10, a12, x15r, d1a, x18r, d2a, x21r, and at level 4 x2r, d3a, x24r (``vgg.hip`` layer walk)
  * accumulators start at the fp32 bias (``conv_kernels.h:1176-1184``); products of T operands are exact in fp32
  * raw feature maps and their sum of squares come from the fp32 accumulators; ``feat16`` maps are fp16 in both modes,
    saturated at +-65504, and the sum of squares and the ReLU'd activation are taken from that fp16 value
    (``conv_kernels.h:566-573``)
  * confidence heads read the stored T activations (``vgg.hip`` conf launches) with fp32 accumulation; their fp32 weights
    enter the MFMA as a T hi + lo pair, hi = T(w), lo = T(w - hi) (``conf_kernel``, ``conv_kernels.h:1808-1809``)

``accum``: ``torch.float64`` accumulates exactly (up to fp64), ``torch.float32`` runs torch's float32 convolutions on the
same rounded operands.  Their difference is the noise floor of rounding flips -- elements within accumulation error of a
rounding midpoint -- that a GPU comparison with the fp64 emulation has to allow.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def _hi_lo(w, dtype):
    """An fp32 value as the kernels carry it in a T hi + lo pair (differences formed in fp32, exact), summed in fp64."""
    if dtype is None:
        return w
    wf = w.float()
    hi = wf.to(dtype).float()
    return hi.double() + (wf - hi).to(dtype).double()


def _conv(x, sd, name, rnd, acc, bias=None):
    w = rnd(sd[name + '.weight'].to(acc))
    if bias is None and (name + '.bias') in sd:
        bias = sd[name + '.bias'].to(acc)
    return F.conv2d(x, w, bias, padding=1)


def forward(sd: dict, x: torch.Tensor, level: int = 3, dtype: torch.dtype = None, accum: torch.dtype = torch.float64,
            feat16: bool = False):
    """The 16-bit forward of VGGUnet(level) on the NCHW image ``x``, with parameters from the state dict ``sd``.

    ``dtype`` None turns every rounding off (then this is ``O.VGGUnet`` computed in ``accum``).  Returns
    ``(feats, confs, raws)``: the L2-normalised maps and confidence maps of ``O.VGGUnet.forward`` (levels 3 / 4: all
    three / four of them) and the raw maps x15, x18, x21 (, x24), all in ``accum``."""
    assert level in (3, 4)
    acc = accum

    def rnd(t):
        return t if dtype is None else t.to(dtype).to(acc)

    def act(t):             # a stored post-ReLU activation
        return rnd(F.relu(t))

    pool = lambda t: F.max_pool2d(t, 2)
    up = lambda t, like: F.interpolate(t, like.shape[2:], mode='nearest')
    h16 = (lambda t: t) if not feat16 else (lambda t: t.clamp(-65504.0, 65504.0).to(torch.float16).to(acc))
    sd = {k: v.detach().to(torch.float64) for k, v in sd.items()}
    x = rnd(x.to(acc))
    a0 = act(_conv(x, sd, 'conv0', rnd, acc, bias=_hi_lo(sd['conv0.bias'], dtype).to(acc)))
    x2 = _conv(a0, sd, 'conv2', rnd, acc)
    x3 = act(pool(x2))
    a5 = act(_conv(x3, sd, 'conv5', rnd, acc))
    x8 = act(pool(_conv(a5, sd, 'conv7', rnd, acc)))
    a10 = act(_conv(x8, sd, 'conv10', rnd, acc))
    a12 = act(_conv(a10, sd, 'conv12', rnd, acc))
    x15 = h16(pool(_conv(a12, sd, 'conv14', rnd, acc)))
    x15r = act(x15)
    d1a = act(_conv(torch.cat([up(x15r, x8), x8], 1), sd, 'conv_dec1.1', rnd, acc))
    x18 = h16(_conv(d1a, sd, 'conv_dec1.3', rnd, acc))
    x18r = act(x18)
    d2a = act(_conv(torch.cat([up(x18r, x3), x3], 1), sd, 'conv_dec2.1', rnd, acc))
    x21 = h16(_conv(d2a, sd, 'conv_dec2.3', rnd, acc))
    x21r = act(x21)
    raws, acts = [x15, x18, x21], [x15r, x18r, x21r]
    if level == 4:
        x2r = act(x2)
        d3a = act(_conv(torch.cat([up(x21r, x2r), x2r], 1), sd, 'conv_dec3.1', rnd, acc))
        x24 = _conv(d3a, sd, 'conv_dec3.3', rnd, acc)
        raws.append(x24)
        acts.append(act(x24))
    # heads: sigmoid(-sigmoid(conv(relu(map)))) on the stored activations (O.VGGUnet.forward), weights as hi + lo
    confs = [torch.sigmoid(-torch.sigmoid(F.conv2d(a, _hi_lo(sd[f'conf{l}.1.weight'], dtype).to(acc), padding=1)))
             for l, a in enumerate(acts)]
    feats = [O.l2_norm_map(t) for t in raws]
    return feats, confs, raws


# Gate of a GPU map against the emulation.  One rounding flip changes the next layer's sums by more than fp32 error and so flips
# more of ITS elements: past a few layers and a few thousand elements the flips saturate and the fp32-vs-fp64 noise becomes a
# sizeable fraction of the rounding error itself.  Per map, by the CPU's noise / rounding ratio:
#   flip-free (< 1e-2): gate = k x noise, at least the fp32-arithmetic floor; the rounding must be >= 10 x the gate
#   partial (1e-2 .. 0.1): the same gate, no teeth requirement
#   saturated (>= 0.1): the same gate, at least half the rounding error -- a second flip realisation may exceed the CPU's
NOISE_L2, NOISE_MAX = 2.0, 4.0
ABS_L2, ABS_MAX = 1e-6, 2e-6
SAT_RATIO, FREE_RATIO, SAT_FLOOR = 0.1, 1e-2, 0.5


def gate(e64, e32, exact):
    """{'l2', 'max': the gates of relL2 / max-rel against ``e64``; 'regime'; 'rnd_l2', 'rnd_max': the rounding the emulation
    models (against ``exact``); 'noise_l2', 'noise_max': ``e32`` against ``e64``}."""
    g = dict(rnd_l2=rel_l2(e64, exact), rnd_max=max_rel(e64, exact), noise_l2=rel_l2(e32, e64), noise_max=max_rel(e32, e64))
    ratio = g['noise_l2'] / max(g['rnd_l2'], 1e-300)
    g['regime'] = 'saturated' if ratio >= SAT_RATIO else ('partial' if ratio >= FREE_RATIO else 'flip-free')
    g['l2'] = max(NOISE_L2 * g['noise_l2'], ABS_L2)
    g['max'] = max(NOISE_MAX * g['noise_max'], ABS_MAX)
    if g['regime'] == 'saturated':
        g['l2'] = max(g['l2'], SAT_FLOOR * g['rnd_l2'])
        g['max'] = max(g['max'], SAT_FLOOR * g['rnd_max'])
    return g


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def max_rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
