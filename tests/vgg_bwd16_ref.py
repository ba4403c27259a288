"""Per-launch CPU restatement of the library's bf16 / fp16 VGGUnet backward, and the checker that compares a run with it.

TEST INFRASTRUCTURE ONLY.  ``vgg_round16.py`` restates the 16-bit *forward*; this file restates every launch of
``vgg_backward_t<T>`` (``highlyaccurate_amd/csrc/vgg_backward.hip``) for T = bf16 / fp16 in torch on the CPU.  ``walk`` goes
through the launches in the kernels' order.  Teacher-forced (``forced`` = the gradient maps a run left in its workspace),
every launch is restated as a function of the operands THAT launch read; free-running (``forced`` = None, ``backward``), each
launch reads what the restatement itself produced.  All maps here are NCHW fp64 tensors holding T-representable values.

Every product in these kernels is exact in fp32 (two 16-bit operands); the inexact steps are the fp32 accumulation and the
named roundings.  Rounding points (file:line relative to ``highlyaccurate_amd/csrc``):

  * transposed packed weights: every weight rounded to T, ``out[e] = (T)v`` (``conv_kernels.h:1676``, packed by
    ``vgg_pack_all_T``, ``vgg_backward.hip:557-566``); the weight gradients read the stored T activations
  * L2-norm backward, ``l2bwd_apply_kernel`` (``vgg_backward.hip:188-196``): ``c1 = (float)inv``, one-pass form
    ``out = T(c1 * dy)`` -- ONE fp32 product, reproduced exactly here; two-pass form ``out = T(c1 * dy - c3 * x)`` with
    ``c3 = (float)(inv^3 * dot)``, ``dot`` from fp32 partial sums of 256 products (``l2bwd_dot_kernel``, ``:101-109``):
    fp32 arithmetic that may be contracted, so it gets an error band (``l2_backward``)
  * confidence heads: ``conf_dz_kernel`` (``:233-240``) forms dz in fp32 (``logf``), ``conf_bwd_kernel`` (``:272-278``) reads
    the stored T gradient, adds ``act > 0 ? sum_t w[t] * dz : 0`` with the head's fp32 weights in fp32 and stores ``T(.)``
  * data gradients: the fp32 accumulator (summed over the 2x2 block first with ``pool_sum``, ``conv_kernels.h:589-591``) is
    rounded to T when staged, ``RowStager<T>::put`` -> ``store4`` (``conv_kernels.h:359-360``, ``:199-206``); the flush
    (``:425-430``) then forms ``f = (float)e; f = mask > 0 ? f : 0; f += add`` (inside the add window only) and stores
    ``(T)f``: the second rounding.  fp32 ``s + add`` of two T values is one IEEE addition and is reproduced exactly
  * ``unpool_add_kernel`` (level 4, ``vgg_backward.hip:224``): ``T((idx == pos ? g : 0) + skip)``, one fp32 addition, exact here
  * weight / bias gradients: fp32 sums of exact T x T products (``wgrad_kernels.h``); the bias gradient multiplies the
    gradient tile with a ones fragment (``frag_ones``, ``conv_kernels.h:194-197``)
  * conv0's weight gradient, BOTH routes, multiplies T values: the stored-map route (``wgrad0_kernel``,
    ``wgrad_kernels.h:842``, ``:867``) reads conv2's data gradient as the stored T map and converts the fp32 image to T in the
    B fragment; the fused route (``conv_epilogue_wg0``, ``conv_kernels.h:816``, ``:828``, ``:872``) stages the fp32 accumulator
    through ``RowStager<T>::put`` -- the same T rounding the stored map gets -- masks it, and converts the image to T likewise.
    Neither route ever multiplies the fp32 accumulator itself.  The two therefore sum the SAME exact products and differ in
    the order of fp32 sums only: per 8 x 32 tile, two row halves, 1024 slabs and a gather (fused) against k-split partials
    over 4 x 32 tiles (stored map).  conv0's gradient contracts a sign-changing gradient with a positive image over every
    pixel, so it cancels heavily: |dW| is 1e-2 .. 1e-3 of S = sum |g||x|, and an order-only difference of a few 1e-6 of S is
    the ``CONV0_TOL = 2e-3`` of a tensor's norm that ``test_backward_16bit_wgrad_groupings_agree`` allows between the routes.

``accum``: ``torch.float64`` sums exactly (up to fp64); ``torch.float32`` runs torch's float32 convolutions on the same
operands -- the noise model of fp32 accumulation (as ``vgg_round16.forward``).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

W_ORDER = ['conv0', 'conv2', 'conv5', 'conv7', 'conv10', 'conv12', 'conv14', 'conv_dec1.1', 'conv_dec1.3', 'conv_dec2.1',
           'conv_dec2.3', 'conv_dec3.1', 'conv_dec3.3']
# (cin, cout) as the kernels run them: conv_dec3.* zero-padded to 64 channels (vgg_layers.h:7-12)
LAYERS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (384, 128), (128, 128), (192, 64),
          (64, 64), (128, 64), (64, 64)]
WG_TH = 4
EPS24 = 2.0 ** -24
MAX_EXCUSABLE = 0.05
NOISE_K, NOISE_FLOOR = 4.0, 2.0 ** -22

# forward workspace maps: name -> (resolution divisor, stored channels)
FWD_MAPS = {'x3': (2, 64), 'a5': (2, 128), 'x8': (4, 128), 'a10': (4, 256), 'a12': (4, 256), 'x15r': (8, 256), 'd1a': (4, 128),
            'x18r': (4, 128), 'd2a': (2, 64), 'x21r': (2, 64), 'x2r': (1, 64), 'd3a': (1, 64), 'x24r': (1, 64), 'a0': (1, 64)}
FWD_IDX = {'idx3': (2, 64), 'idx8': (4, 128), 'idx15': (8, 256)}
BWD_MAPS = {'g_x21': (2, 64), 'g_d2a': (2, 64), 'g_x18': (4, 128), 'l2_18': (4, 128), 'g_d1a': (4, 128), 'g_x15': (8, 256),
            'l2_15': (8, 256), 'g_a12': (4, 256), 'g_a10': (4, 256), 'g_x8': (4, 128), 'g_x8p': (4, 128), 'g_a5': (2, 128),
            'g_x3': (2, 64), 'g_x3p': (2, 64), 'g_a0': (1, 64)}
BWD_MAPS4 = {'g_x24': (1, 64), 'g_d3a': (1, 64), 'g_x2p': (1, 64), 'g_c2': (1, 64), 'l2_21': (2, 64)}


# ---------------------------------------------------------------------------------------------------------------------
# workspace layouts (2-byte elements)
# ---------------------------------------------------------------------------------------------------------------------
class _Taker:
    def __init__(self):
        self.p, self.o = {}, 0

    def take(self, name, nbytes):
        self.p[name] = self.o
        self.o += -(-nbytes // 256) * 256


def fwd_plan(B, H, W, level4, es=2):
    """``vgg_plan`` (vgg_layers.h:47-86) of a training forward: {name: byte offset}, total."""
    t, P = _Taker(), B * H * W
    for name in ('x3', 'a5', 'x8', 'a10', 'a12', 'x15r', 'd1a', 'x18r', 'd2a', 'x21r'):
        div, C = FWD_MAPS[name]
        t.take(name, P // (div * div) * C * es)
    tiles = lambda h, w: ((h + 7) // 8) * ((w + 31) // 32)
    for i, n in enumerate((tiles(H // 4, W // 4) * 2, tiles(H // 4, W // 4), tiles(H // 2, W // 2), tiles(H, W))):
        t.take(f'ss{i}', B * n * 8)
    t.take('inv', 4 * B * 8)
    t.take('amax', 16 * B * 4)
    if level4:
        for name in ('x2r', 'd3a', 'x24r'):
            t.take(name, P * 64 * es)
    t.take('a0', P * 64 * es)
    for name, (div, C) in FWD_IDX.items():
        t.take(name, P // (div * div) * C)
    return t.p, t.o


def _ksplit(cout, cin, ntile, resident=512):
    ks = max(resident // max((cout // 64) * (cin // 64), 1), 1)
    return min(ks, ntile)


def _dyn_total(H, W):
    """``dyn_layout(H, W).total`` (vgg_backward.hip:331-353), in ints."""
    o = 0

    def take(n):
        nonlocal o
        o += (n + 3) & ~3
    for h in (H // 8, H // 4, H // 2):
        take(2 * h)
    for d in (2, 2, 2, 4, 4, 4, 8, 4, 4, 4, 2, 2, 1):
        take(2 * ((H // d + 7) // 8))
    for d in (2, 2, 2, 4, 4, 4, 4, 4, 4, 2, 2, 1):
        take(4)
        take(((H // d + 7) // 8) * ((W // d + 31) // 32))
    for d in (2, 2, 4, 4, 4, 4, 4, 2, 2, 1, 1):
        take(4)
        take(((H // d + WG_TH - 1) // WG_TH) * ((W // d + 31) // 32))
    take(4)
    return o


def bwd_plan(B, H, W, level4, es=2):
    """``bwd_plan`` (vgg_backward.hip:500-535): {name: byte offset}, total.  Every gradient map has its own slot; only
    ``part`` / ``bpart`` are reused, and with the fused conv0 gradient the ``g_a0`` slot holds partials instead of a map."""
    t, P = _Taker(), B * H * W
    for name in ('g_x21', 'g_d2a', 'g_x18', 'l2_18', 'g_d1a', 'g_x15', 'l2_15', 'g_a12', 'g_a10', 'g_x8', 'g_x8p', 'g_a5',
                 'g_x3', 'g_x3p', 'g_a0'):
        div, C = BWD_MAPS[name]
        t.take(name, P // (div * div) * C * es)
    t.take('dot', B * 64 * 8)
    maxpart = 1024 * 2 * 64 * 32 * 4
    hs = (1, 1, 2, 2, 4, 4, 4, 4, 4, 2, 2)
    for l in range(1, 13 if level4 else 11):
        div = hs[l] if l < 11 else 1
        h, w = H // div, W // div
        ntile = B * ((h + WG_TH - 1) // WG_TH) * ((w + 31) // 32)
        cin, cout = LAYERS[l]
        maxpart = max(maxpart, _ksplit(cout, cin, ntile) * cout * cin * 9 * 4)
    t.take('part', maxpart)
    t.take('bpart', 2048 * 256 * 4)
    t.take('dz', (P if level4 else P // 4) * 4)
    t.take('dyn', _dyn_total(H, W) * 4)
    t.take('gamax', 24 * B * 4)
    if level4:
        for name in ('g_x24', 'g_d3a', 'g_x2p', 'g_c2'):
            t.take(name, P * 64 * es)
        t.take('l2_21', P // 4 * 64 * es)
    return t.p, t.o


def _view16(ws, off, B, h, w, C, dtype):
    """(values NCHW fp64, raw int16 NCHW) of the NHWC 16-bit map at byte offset ``off`` of the uint8 workspace ``ws``."""
    raw = ws[off:off + B * h * w * C * 2].view(torch.int16).view(B, h, w, C).permute(0, 3, 1, 2)
    return raw.contiguous().view(dtype).double(), raw


def read_forward(ws, B, H, W, level, dtype, names=None):
    """The saved forward workspace (a CPU uint8 tensor): 16-bit activations as NCHW fp64 and the argmax bytes as NCHW long."""
    p, total = fwd_plan(B, H, W, level == 4)
    assert ws.numel() == total, ('forward workspace layout', ws.numel(), total)
    fw = {}
    for name, (div, C) in FWD_MAPS.items():
        if (name in ('x2r', 'd3a', 'x24r') and level != 4) or (names is not None and name not in names):
            continue
        fw[name] = _view16(ws, p[name], B, H // div, W // div, C, dtype)[0]
    for name, (div, C) in FWD_IDX.items():
        if names is not None and name not in names:
            continue
        h, w = H // div, W // div
        fw[name] = ws[p[name]:p[name] + B * h * w * C].view(B, h, w, C).permute(0, 3, 1, 2).long()
    return fw


def read_backward(ws, B, H, W, level, dtype, names=None):
    """The backward workspace after a call: ({map: NCHW fp64}, {map: raw int16}).  Unwritten elements of a 0xFF-filled
    workspace read as NaN / raw -1."""
    p, total = bwd_plan(B, H, W, level == 4)
    assert ws.numel() >= total, ('backward workspace layout', ws.numel(), total)
    maps, raws = {}, {}
    for name, (div, C) in list(BWD_MAPS.items()) + (list(BWD_MAPS4.items()) if level == 4 else []):
        if names is not None and name not in names:
            continue
        maps[name], raws[name] = _view16(ws, p[name], B, H // div, W // div, C, dtype)
    return maps, raws


# ---------------------------------------------------------------------------------------------------------------------
# rounding
# ---------------------------------------------------------------------------------------------------------------------
def _t(v, dtype):
    return v if dtype is None else v.to(dtype).to(v.dtype)


def _neighbour(s, up, dtype):
    """The T value next to the T value ``s`` (held in fp64), above it where ``up`` else below."""
    bits = s.to(dtype).view(torch.int16).to(torch.int32)
    neg, mag = bits < 0, bits & 0x7FFF
    away = up ^ neg
    nmag = torch.where(mag == 0, torch.ones_like(mag), torch.where(away, mag + 1, mag - 1))
    nneg = torch.where(mag == 0, ~up, neg)
    return (nmag - 32768 * nneg.to(torch.int32)).to(torch.int16).view(dtype).double()


def round_interval(acc, band, dtype):
    """(a, lo, hi): a = T(acc) and the T values a sum within ``band`` of ``acc`` can round to, lo = T(acc - band) ..
    hi = T(acc + band) (rounding is monotone).  lo != hi exactly where ``acc`` lies within ``band`` of a rounding midpoint."""
    return _t(acc, dtype), _t(acc - band, dtype), _t(acc + band, dtype)


def _add32(s, add, dtype):
    """``(T)((float)s + (float)add)``: the flush's fp32 addition of two T values and its rounding, both exact IEEE steps."""
    return (s.float() + add.float()).to(dtype).double()


def excuse_band(acc32, acc64, S, K):
    """The distance from a rounding midpoint inside which an fp32-accumulated sum may round the other way, and rho.
    The closed-form bound of fp32 accumulation in any order, 2 K 2^-24 S (K products, S = the sum of their magnitudes, the
    factor 2 for the MFMA's undocumented internal rounding), is the OUTER limit -- but it is a worst case that no sum comes
    near: measured on the CPU it puts 17 .. 70 % of every map within reach of a midpoint (K S / |acc| is 1e4 .. 2e5, against
    the 2^13 that separate an fp16 ulp from an fp32 ulp), and a check that excuses half of a map proves nothing.  The band
    used is the noise model's, with the constant of ``vgg_round16.gate``: NOISE_K = 4 x rho x S, rho = the LARGEST
    |acc32 - acc64| / S over the map of the CPU's own fp32 accumulation of the same operands (measured 0.3 .. 2 x 2^-24,
    whatever K: the deviation of a sum relative to S is largest where a few products dominate, and then it is a few half
    ulps of them), never more than the closed form.  An rms-based band fails: |error| / S has no Gaussian tail (elements
    differ in how many products matter), one element in 1e5 lies beyond 16 rms.  The band comes from the reference alone."""
    outer = 2 * K * EPS24 * S
    nz = S > 0
    rho = float(((acc32 - acc64).abs()[nz] / S[nz]).max()) if nz.any() else 0.0
    return torch.minimum(outer, NOISE_K * rho * S), rho


def stage(acc, band, mask, add, dtype):
    """RowStager<T>::put + flush: s = T(acc); s = mask ? s : 0; out = T(s + add).  ``mask`` bool or None, ``add`` (zero outside
    the add window) or None.  Returns dict(out, lo, hi, exc): [lo, hi] = what the launch can store when its accumulator is
    within ``band`` of ``acc`` (every step is monotone in s), exc = lo != hi: the first rounding is near a midpoint."""
    if dtype is None:
        out = acc if mask is None else torch.where(mask, acc, torch.zeros_like(acc))
        out = out if add is None else out + add
        return dict(out=out, lo=out, hi=out, exc=torch.zeros_like(out, dtype=torch.bool))
    v = list(round_interval(acc, band, dtype))
    if mask is not None:
        v = [torch.where(mask, t, torch.zeros_like(t)) for t in v]
    exc = v[1] != v[2]
    if add is not None:
        v = [_add32(t, add, dtype) for t in v]
    return dict(out=v[0], lo=v[1], hi=v[2], exc=exc)


# ---------------------------------------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------------------------------------
def _zero_above(t, row):
    """Rows above ``row`` read as zero (src_row_lo / add_row_lo / row_begin: never written, never read)."""
    if row > 0:
        t = t.clone()
        t[:, :, :row] = 0
    return t


def unpool(g, idx):
    """Virtual unpool (conv_kernels.h:1012, wgrad_kernels.h:190-214): g at half resolution goes to position idx = 2*row+col
    of its 2x2 window."""
    B, C, h, w = g.shape
    pos = (2 * (torch.arange(2 * h) & 1)).view(1, 1, -1, 1) + (torch.arange(2 * w) & 1).view(1, 1, 1, -1)
    up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return torch.where(up(idx) == pos, up(g), torch.zeros((), dtype=g.dtype))


def l2_backward(x, dy, inv, dtype, accum=torch.float64, scale_invariant=False, row0=0):
    """L2-norm backward of one raw map.  x, dy: NCHW (fp32 values), inv [B] fp64.  Rows above ``row0`` are not written (NaN).
    One-pass form: T(fl32(c1 * dy)), reproduced exactly.  Two-pass form: acc = c1 * dy - c3 * x with the band
    2 * (3 eps (|c1 dy| + |c3 x|) + |x| inv^3 * 32 eps * sqrt(sum (x dy)^2)): three fp32 roundings (or a contraction) of the
    two terms and c3's own rounding (a closed-form bound), and the dot product's fp32 partial sums: each thread adds 256
    products in fp32 before it goes to fp64 (vgg_backward.hip:104-109), a random walk of 256 roundings with standard deviation
    about 0.4 sqrt(256) eps sqrt(sum p^2) = 6.4 eps sqrt(sum p^2) over all threads; 32 = five of those.  (The closed-form
    256 eps sum|p| is 700 times wider and excuses 14 % of an fp16 map.)"""
    B = x.shape[0]
    al = inv.double().view(B, 1, 1, 1)
    if dtype is None:
        c1 = al
        dot = (x.double() * dy.double()).sum((1, 2, 3), keepdim=True)
        acc = c1 * dy.double() if scale_invariant else c1 * dy.double() - al ** 3 * dot * x.double()
        r = dict(out=acc, lo=acc, hi=acc, exc=torch.zeros_like(acc, dtype=torch.bool))
    elif scale_invariant:
        acc = (al.float() * dy.float()).double()
        r = stage(acc, torch.zeros_like(acc), None, None, dtype)
    else:
        xd, dd = x.double(), dy.double()
        if accum == torch.float32:
            dot = (x.float() * dy.float()).sum((1, 2, 3), keepdim=True).double()
        else:
            dot = (xd * dd).sum((1, 2, 3), keepdim=True)
        sdot = ((xd * dd) ** 2).sum((1, 2, 3), keepdim=True).sqrt()
        c1, c3 = al.float().double(), (al ** 3 * dot).float().double()
        if accum == torch.float32:
            acc = (c1.float() * dy.float() - c3.float() * x.float()).double()
        else:
            acc = c1 * dd - c3 * xd
        band = 2 * (3 * EPS24 * ((c1 * dd).abs() + (c3 * xd).abs()) + xd.abs() * al ** 3 * 32 * EPS24 * sdot)
        r = stage(acc, band, None, None, dtype)
    r['row_begin'] = row0
    if row0 > 0:
        for k in ('out', 'lo', 'hi'):
            r[k] = r[k].clone()
            r[k][:, :, :row0] = float('nan')
    return r


def conf_backward(conf, d_conf, act, w, g_in, dtype, accum=torch.float64):
    """conf_dz_kernel + conf_bwd_kernel<T> of one head.  conf, d_conf [B,h,w] (fp32 values), act = the stored relu(map) NCHW,
    w [1,C,3,3] the head's fp32 weight, g_in = dict(out, alt, exc) of the raw-map gradient it adds into (in place on the GPU).
    Returns (dict(out, lo, hi, exc) of the updated map, dw, (S_dw, E_dw)).
    z = g + (act > 0 ? d : 0) with d = sum_t w_t dz_t in fp32 from an fp32 dz.  Its band is per element and in closed form:
    sum_t |w_t| e_t + 9 eps sum_t |w_t dz_t| + eps |z|, with e = eps |d_conf| c (1 - c) (4 |1 - 2 s| + 6 s (1 - s)) the error
    of dz: s = log((1 - c) / c) carries at most 4 eps of absolute error (the subtraction, the division and logf at 2 ulp of a
    value below 1; the CPU's own fp32 evaluation is off by 1.9 eps at most), the five-factor product six relative roundings;
    then nine fp32 multiply-adds and the fp32 addition to g.  The formula is ill-conditioned where the head saturates
    (s -> 1: dz is 1e-3 off in relative terms at s = 0.9999, on the GPU as here), so the band is large where d dominates z:
    the upstream gradient of the confidence maps has to be of the size of the feature maps', not 30 times it, for the
    excusable share to stay small (``case_inputs``).  A map-wide noise figure is useless here: its maximum is set by the few
    saturated pixels."""
    c, dc = conf.double().unsqueeze(1), d_conf.double().unsqueeze(1)
    wd = w.double()
    s = torch.log((1 - c) / c)
    dz64 = -dc * c * (1 - c) * s * (1 - s)
    c32, dc32 = c.float(), dc.float()
    s32 = torch.log((1 - c32) / c32)
    dz32 = -dc32 * c32 * (1 - c32) * s32 * (1 - s32)
    d64 = F.conv_transpose2d(dz64, wd, padding=1)
    f32 = accum == torch.float32 and dtype is not None
    dz = dz32.double() if f32 else dz64
    on = act > 0
    dw = conv2d_weight(act.to(accum), w.shape, dz.to(accum), padding=1).double()
    e = EPS24 * dc.abs() * c * (1 - c) * (4 * (1 - 2 * s).abs() + 6 * s * (1 - s))
    # S of the head's weight gradient, and E: what the error of dz alone can move it by (outside the fp32 summation)
    s_dw = (conv2d_weight(act.abs(), w.shape, dz64.abs(), padding=1), conv2d_weight(act.abs(), w.shape, e, padding=1))
    if dtype is None:
        out = g_in['out'] + torch.where(on, d64, torch.zeros_like(d64))
        return dict(out=out, lo=out, hi=out, exc=torch.zeros_like(out, dtype=torch.bool), row_begin=0), dw, s_dw
    d32 = F.conv_transpose2d(dz32, wd.float(), padding=1).double()
    derr = F.conv_transpose2d(e, wd.abs(), padding=1) + 9 * EPS24 * F.conv_transpose2d(dz64.abs(), wd.abs(), padding=1)
    dd = torch.where(on, d32 if f32 else d64, torch.zeros_like(d64))
    add = lambda g: (g.float() + dd.float()).double() if f32 else g + dd
    z = add(g_in['out'])
    band = torch.where(on, derr + EPS24 * z.abs(), torch.zeros_like(z))
    out = _t(z, dtype)
    lo, hi = _t(add(g_in['lo']) - band, dtype), _t(add(g_in['hi']) + band, dtype)
    return dict(out=out, lo=lo, hi=hi, exc=lo != hi, row_begin=g_in.get('row_begin', 0), inplace=True), dw, s_dw


def dgrad(g, wT, mask, add, dtype, accum=torch.float64, idx=None, pool_sum=False, row_begin=0, src_row_lo=0, add_row_lo=0):
    """One data-gradient launch.  g: the T gradient map it reads (half resolution with ``idx``), wT [Cout_l, n, 3, 3]: the
    layer's T weights restricted to the launch's input channels, mask: the stored activation (> 0 passes) at output
    resolution, add: the fan-in map or None.  row_begin / src_row_lo in the launch's full-resolution rows, add_row_lo in
    output rows (ConvArgs).  Returns dict(out, lo, hi, exc, S, K, row_begin[output rows], ...)."""
    if idx is not None:
        g = unpool(g, idx)
    g = _zero_above(g, src_row_lo)
    cv = lambda t, ww, dt: F.conv_transpose2d(t.to(dt), ww.to(dt), padding=1).double()
    acc64 = cv(g, wT, torch.float64)
    acc32 = cv(g, wT, torch.float32) if (dtype is not None or accum == torch.float32) else acc64
    S = cv(g.abs(), wT.abs(), torch.float64)
    K = 9 * wT.shape[0]
    if pool_sum:
        a32 = acc32.float()             # (t + u) + the neighbouring lane's (t + u), conv_kernels.h:589-591
        v = a32[:, :, 0::2] + a32[:, :, 1::2]
        acc32 = (v[:, :, :, 0::2] + v[:, :, :, 1::2]).double()
        acc64 = 4 * F.avg_pool2d(acc64, 2)
        S, K, rb = 4 * F.avg_pool2d(S, 2), 4 * K, row_begin // 2
    else:
        rb = row_begin
    acc = acc32 if accum == torch.float32 else acc64
    band, rho = excuse_band(acc32, acc64, S, K)
    m = None if mask is None else mask > 0
    if add is not None:
        add = _zero_above(add, add_row_lo)
    r = stage(acc, band, m, add, dtype)
    r.update(S=S, K=K, row_begin=rb, acc=acc, band=band, mask=m, add=add, rho=rho)
    if rb > 0:
        for k in ('out', 'lo', 'hi'):
            r[k] = r[k].clone()
            r[k][:, :, :rb] = float('nan')
    return r


def unpool_add(g, idx, skip, dtype):
    """unpool_add_kernel (level 4): T((idx == pos ? g : 0) + skip), one fp32 addition."""
    u = unpool(g, idx)
    out = u + skip if dtype is None else _add32(u, skip, dtype)
    return dict(out=out, lo=out, hi=out, exc=torch.zeros_like(out, dtype=torch.bool), row_begin=0)


def wgrad(x1, x2, up1, g, idx, accum=torch.float64, row_begin=0, want_S=True, bias=True):
    """One weight-gradient launch: the input is cat(up(x1) if up1 else x1, x2), the gradient ``g`` is expanded with ``idx``
    (g_unpool) when given; pixel rows above ``row_begin`` carry no gradient and are skipped.
    Returns dict(dw, db, S, Sb): S = sum over pixels of |g| |x| per weight, Sb = sum |g| per output channel."""
    if idx is not None:
        g = unpool(g, idx)
    g = _zero_above(g, row_begin)
    if up1:
        x1 = x1.repeat_interleave(2, 2).repeat_interleave(2, 3)
    x = x1 if x2 is None else torch.cat([x1, x2], 1)
    shape = (g.shape[1], x.shape[1], 3, 3)
    r = dict(dw=conv2d_weight(x.to(accum), shape, g.to(accum), padding=1).double())
    if bias:
        r['db'] = g.to(accum).sum((0, 2, 3)).double()
    if want_S:
        r['S'] = conv2d_weight(x.abs(), shape, g.abs(), padding=1)
        r['Sb'] = g.abs().sum((0, 2, 3))
    return r


def _n_rows(first_row8, with_conf, scale_invariant, level4):
    """The n_* / rb_* first rows of ``vgg_backward_t`` (vgg_backward.hip:644-663)."""
    f = 0 if (level4 or not scale_invariant) else first_row8
    wc = 1 if with_conf else 0
    ev = lambda v: 0 if v < 0 else v & ~1
    nn = lambda v: max(v, 0)
    n = {}
    n['x21'] = 4 * f - wc if f else 0
    n['d2a'] = nn(n['x21'] - 1)
    n['rb_up18'] = ev(n['d2a'] - 1)
    n['x18'] = n['rb_up18'] // 2
    n['x3p'] = nn(n['d2a'] - 1)
    n['d1a'] = nn(n['x18'] - 1)
    n['rb_up15'] = ev(n['d1a'] - 1)
    n['x15'] = n['rb_up15'] // 2
    n['x8p'] = nn(n['d1a'] - 1)
    n['a12'] = nn(2 * n['x15'] - 1)
    n['a10'] = nn(n['a12'] - 1)
    n['x8'] = nn(n['a10'] - 1)
    n['a5'] = nn(2 * n['x8'] - 1)
    n['x3'] = nn(n['a5'] - 1)
    n['a0'] = nn(2 * n['x3'] - 1)
    return n


def round_weights(sd, level, dtype):
    """({layer index: [cout, cin, 3, 3] fp64 weight rounded to T as pack_weights_multi_kernel<T> rounds it}, [the heads' fp32
    weights]); conv_dec3.* and conf3 zero-padded to 64 channels.  dtype None: the parameters as they are, in fp64."""
    cast = (lambda w: w.detach().double()) if dtype is None else (lambda w: w.detach().float())

    def padded(w, co, ci):
        wp = torch.zeros(co, ci, 3, 3, dtype=w.dtype)
        wp[:w.shape[0], :w.shape[1]] = w
        return wp
    wt, heads = {}, []
    for l, name in enumerate(W_ORDER[:13 if level == 4 else 11]):
        w = cast(sd[name + '.weight'])
        if l >= 11:
            w = padded(w, LAYERS[l][1], LAYERS[l][0])
        wt[l] = (w if dtype is None else w.to(dtype)).double()
    for l in range(4 if level == 4 else 3):
        w = cast(sd[f'conf{l}.1.weight'])
        heads.append((padded(w, 1, 64) if l == 3 else w).double())
    return wt, heads


def walk(sd, x, fw, raws, inv, d_feats, confs, d_confs, level, dtype, accum=torch.float64, forced=None, scale_invariant=False,
         first_row8=0, unfused0=True, only=None, want_S=True, dgrads=True, dynamic=False):
    """Every launch of ``vgg_backward_t<T>`` (dense walk) in the kernels' order.
    sd: state dict; x: NCHW image; fw: forward maps (``read_forward`` / ``forward_saved``); raws / d_feats: NCHW lists (level 4:
    64 channels for map 3); inv [L, B]; confs / d_confs: [B,h,w] lists or None.
    forced: {map: NCHW fp64} -- the gradient maps each launch READS are taken from here (teacher forcing; NaN = unwritten)
    instead of from this walk's own outputs.  dgrads=False (needs ``forced``): skip the data-gradient restatements, e.g. for
    the fp32 noise figures of the weight gradients.  dynamic: the data-dependent trimming left parts of the maps unwritten
    that are exactly zero; the launches read them as zero (``check_map(dynamic=True)`` holds the maps to that).  only: restrict the weight-gradient launches to these layer indices and skip the
    data-gradient restatements (needs ``forced``).
    Returns (maps, wg): maps[name] = dict(out, lo, hi, exc, S, K, row_begin) per stored map, wg[layer] = dict(dw, db, S, Sb);
    wg['conf', l] = dict(dw, S, E)."""
    level4 = level == 4
    NL = 4 if level4 else 3
    with_conf = confs is not None and d_confs is not None
    n = _n_rows(first_row8, with_conf, scale_invariant, level4)
    wt, heads = round_weights(sd, level, dtype)
    maps, wg = {}, {}
    if forced is not None and dynamic:
        forced = {k: torch.nan_to_num(v, nan=0.0) for k, v in forced.items()}
    rd = (lambda name: forced[name]) if forced is not None else (lambda name: maps[name]['out'])
    img = _t(x.double(), dtype)

    def dg(l, c0, nch, src, idx, out, mask, add, pool, rb=0, slo=0, alo=0):
        if only is not None or not (dgrads or (out == 'g_a0' and not unfused0)):
            return
        maps[out] = dgrad(rd(src), wt[l][:, c0:c0 + nch], fw[mask], None if add is None else rd(add), dtype, accum,
                          idx=None if idx is None else fw[idx], pool_sum=pool, row_begin=rb, src_row_lo=slo, add_row_lo=alo)

    def wgd(l, x1, x2, up1, g, idx, rb=0):
        if only is not None and l not in only:
            return
        wg[l] = wgrad(fw[x1], None if x2 is None else fw[x2], up1, rd(g), None if idx is None else fw[idx], accum, rb, want_S,
                      bias=l < 7)

    if only is None:
        l2names = ['l2_15', 'l2_18', 'l2_21' if level4 else 'g_x21', 'g_x24']
        acts = ['x15r', 'x18r', 'x21r', 'x24r']
        row0 = [n['x15'], n['x18'], n['x21'], 0]
        for l in range(NL):
            r = l2_backward(raws[l], d_feats[l], inv[l], dtype, accum, scale_invariant, row0[l] if scale_invariant else 0)
            if with_conf:
                r, dw, s_dw = conf_backward(confs[l], d_confs[l], fw[acts[l]], heads[l], r, dtype, accum)
                wg['conf', l] = dict(dw=dw, S=s_dw[0], E=s_dw[1])
            maps[l2names[l]] = r
    if level4:
        dg(12, 0, 64, 'g_x24', None, 'g_d3a', 'd3a', None, False)
        wgd(12, 'd3a', None, 0, 'g_x24', None)
        dg(11, 0, 64, 'g_d3a', None, 'g_x21', 'x21r', 'l2_21', True)
        dg(11, 64, 64, 'g_d3a', None, 'g_x2p', 'x2r', None, False)
        wgd(11, 'x21r', 'x2r', 1, 'g_d3a', None)
    dg(10, 0, 64, 'g_x21', None, 'g_d2a', 'd2a', None, False, n['d2a'], n['x21'])
    wgd(10, 'd2a', None, 0, 'g_x21', None, n['x21'])
    dg(9, 0, 128, 'g_d2a', None, 'g_x18', 'x18r', 'l2_18', True, n['rb_up18'], n['d2a'])
    dg(9, 128, 64, 'g_d2a', None, 'g_x3p', 'x3', None, False, n['x3p'], n['d2a'])
    wgd(9, 'x18r', 'x3', 1, 'g_d2a', None, n['d2a'])
    dg(8, 0, 128, 'g_x18', None, 'g_d1a', 'd1a', None, False, n['d1a'], n['x18'])
    wgd(8, 'd1a', None, 0, 'g_x18', None, n['x18'])
    dg(7, 0, 256, 'g_d1a', None, 'g_x15', 'x15r', 'l2_15', True, n['rb_up15'], n['d1a'])
    dg(7, 256, 128, 'g_d1a', None, 'g_x8p', 'x8', None, False, n['x8p'], n['d1a'])
    wgd(7, 'x15r', 'x8', 1, 'g_d1a', None, n['d1a'])
    dg(6, 0, 256, 'g_x15', 'idx15', 'g_a12', 'a12', None, False, n['a12'], 2 * n['x15'])
    wgd(6, 'a12', None, 0, 'g_x15', 'idx15', 2 * n['x15'])
    dg(5, 0, 256, 'g_a12', None, 'g_a10', 'a10', None, False, n['a10'], n['a12'])
    wgd(5, 'a10', None, 0, 'g_a12', None, n['a12'])
    dg(4, 0, 128, 'g_a10', None, 'g_x8', 'x8', 'g_x8p', False, n['x8'], n['a10'], n['x8p'])
    wgd(4, 'x8', None, 0, 'g_a10', None, n['a10'])
    dg(3, 0, 128, 'g_x8', 'idx8', 'g_a5', 'a5', None, False, n['a5'], 2 * n['x8'])
    wgd(3, 'a5', None, 0, 'g_x8', 'idx8', 2 * n['x8'])
    dg(2, 0, 64, 'g_a5', None, 'g_x3', 'x3', 'g_x3p', False, n['x3'], n['a5'], n['x3p'])
    wgd(2, 'x3', None, 0, 'g_a5', None, n['a5'])
    if level4:
        if only is None and dgrads:
            maps['g_c2'] = unpool_add(rd('g_x3'), fw['idx3'], rd('g_x2p'), dtype)
        dg(1, 0, 64, 'g_c2', None, 'g_a0', 'a0', None, False)
        wgd(1, 'a0', None, 0, 'g_c2', None)
    else:
        dg(1, 0, 64, 'g_x3', 'idx3', 'g_a0', 'a0', None, False, n['a0'], 2 * n['x3'])
        wgd(1, 'a0', None, 0, 'g_x3', 'idx3', 2 * n['x3'])
    if only is None or 0 in only:
        # conv0's weight gradient: both routes multiply T(conv2's data gradient) with T(image) (module docstring).  The stored-map
        # route reads g_a0 from memory (teacher-forced when the map exists); the fused route never stores it, so there the
        # restatement's own g_a0 stands in (an excusable element of it moves dW0 by one T-ulp of one product)
        g0 = forced['g_a0'] if (forced is not None and unfused0) else maps['g_a0']['out']
        g0 = _zero_above(g0, n['a0'])
        r = dict(dw=conv2d_weight(img.to(accum), (64, 3, 3, 3), g0.to(accum), padding=1).double(),
                 db=g0.to(accum).sum((0, 2, 3)).double())
        if want_S:
            r['S'] = conv2d_weight(img.abs(), (64, 3, 3, 3), g0.abs(), padding=1)
            r['Sb'] = g0.abs().sum((0, 2, 3))
        wg[0] = r
    return maps, wg


def grads_of(wg, sd, level):
    """{parameter name: gradient} from ``walk``'s weight-gradient records, in the parameters' own shapes."""
    out = {}
    for l, r in wg.items():
        if isinstance(l, tuple):
            name = f'conf{l[1]}.1.weight'
            out[name] = r['dw'][:, :sd[name].shape[1]]
            continue
        name = W_ORDER[l]
        co, ci = sd[name + '.weight'].shape[:2]
        out[name + '.weight'] = r['dw'][:co, :ci]
        if 'db' in r:
            out[name + '.bias'] = r['db']
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a forward that keeps what the backward reads (the CPU stand-in's operands; the GPU tests read the real workspace)
# ---------------------------------------------------------------------------------------------------------------------
def _pool_idx(t):
    """2x2 max-pool and the kernels' argmax byte 2*row+col: the upper row wins ties inside a column, then the left column wins
    (conv_kernels.h:684-689)."""
    a, b, c, d = t[:, :, 0::2, 0::2], t[:, :, 0::2, 1::2], t[:, :, 1::2, 0::2], t[:, :, 1::2, 1::2]
    rl, rr = (c > a).long(), (d > b).long()
    ml, mr = torch.maximum(a, c), torch.maximum(b, d)
    idx = torch.where(mr > ml, 2 * rr + 1, 2 * rl)
    return torch.maximum(ml, mr), idx


def forward_saved(sd, x, level=3, dtype=None, accum=torch.float64):
    """``vgg_round16.forward`` with everything a training forward saves: (fw, raws, confs, inv) -- fw = the stored activations
    and argmax bytes by workspace name, raws = the raw maps (level 4: x24 zero-padded to 64 channels), confs [B,h,w], inv [L,B]."""
    import vgg_round16 as R16
    acc = accum
    rnd = lambda t: t if dtype is None else t.to(dtype).to(acc)
    act = lambda t: rnd(F.relu(t))
    up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    sdd = {k: v.detach().to(torch.float64) for k, v in sd.items()}
    cv = lambda t, name, bias=None: R16._conv(t, sdd, name, rnd, acc, bias=bias)
    fw = {}
    xi = rnd(x.to(acc))
    fw['a0'] = act(cv(xi, 'conv0', R16._hi_lo(sdd['conv0.bias'], dtype).to(acc)))
    x2 = cv(fw['a0'], 'conv2')
    p, fw['idx3'] = _pool_idx(x2)
    fw['x3'] = act(p)
    fw['a5'] = act(cv(fw['x3'], 'conv5'))
    p, fw['idx8'] = _pool_idx(cv(fw['a5'], 'conv7'))
    fw['x8'] = act(p)
    fw['a10'] = act(cv(fw['x8'], 'conv10'))
    fw['a12'] = act(cv(fw['a10'], 'conv12'))
    x15, fw['idx15'] = _pool_idx(cv(fw['a12'], 'conv14'))
    fw['x15r'] = act(x15)
    fw['d1a'] = act(cv(torch.cat([up(fw['x15r']), fw['x8']], 1), 'conv_dec1.1'))
    x18 = cv(fw['d1a'], 'conv_dec1.3')
    fw['x18r'] = act(x18)
    fw['d2a'] = act(cv(torch.cat([up(fw['x18r']), fw['x3']], 1), 'conv_dec2.1'))
    x21 = cv(fw['d2a'], 'conv_dec2.3')
    fw['x21r'] = act(x21)
    raws, acts = [x15, x18, x21], ['x15r', 'x18r', 'x21r']
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], 64 - t.shape[1], *t.shape[2:], dtype=t.dtype)], 1)
    if level == 4:
        fw['x2r'] = act(x2)
        fw['d3a'] = pad(act(cv(torch.cat([up(fw['x21r']), fw['x2r']], 1), 'conv_dec3.1')))
        x24 = pad(F.conv2d(fw['d3a'][:, :32], rnd(sdd['conv_dec3.3.weight'].to(acc)), padding=1))
        fw['x24r'] = act(x24)
        raws.append(x24)
        acts.append('x24r')
    confs = []
    for l, a in enumerate(acts):
        w = R16._hi_lo(sdd[f'conf{l}.1.weight'], dtype).to(acc)
        confs.append(torch.sigmoid(-torch.sigmoid(F.conv2d(fw[a][:, :w.shape[1]], w, padding=1)))[:, 0])
    if dtype is not None:       # what the GPU hands over: fp32 raw maps and confidence maps
        raws, confs = [t.float() for t in raws], [c.float() for c in confs]
    B = x.shape[0]
    inv = torch.stack([1.0 / t.double().reshape(B, -1).norm(dim=1).clamp_min(1e-12) for t in raws])
    fw = {k: (v if v.dtype == torch.long else v.double()) for k, v in fw.items()}
    return fw, raws, confs, inv


def backward(sd, x, d_feats, d_confs=None, level=3, dtype=None, accum=torch.float64, saved=None, **kw):
    """Free-running backward from the upstream gradients to all parameter gradients: ``forward_saved`` (or the given ``saved``
    = (fw, raws, confs, inv), e.g. a GPU run's) and then ``walk`` on its own outputs.  dtype None: every rounding off.
    Returns (grads, maps, wg)."""
    fw, raws, confs, inv = saved if saved is not None else forward_saved(sd, x, level, dtype, accum)
    maps, wg = walk(sd, x, fw, raws, inv, d_feats, confs if d_confs is not None else None, d_confs, level, dtype, accum, **kw)
    return grads_of(wg, sd, level), maps, wg


def maps_of(maps):
    """{name: stored values} of a walk: what a run with these roundings leaves in its workspace (NaN = unwritten)."""
    return {k: r['out'] for k, r in maps.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def check_map(tag, name, got, rec, dtype, raw=None, out=print, dynamic=False):
    """A stored T map against its restatement.  Exact equality wherever no rounding is near a midpoint; where the first
    rounding is excusable (``rec['exc']``, from the reference alone) the element must lie in [lo, hi], the values the launch
    stores when its accumulator is anywhere within the band -- second rounding included, which is stricter than "within one
    T-ulp of the reference per excused rounding" wherever the band is below an ulp (all but elements cancelled to nearly zero);
    the excusable share must stay <= 5 %; no NaN / Inf in the written region; rows above row_begin still unwritten (NaN, and
    raw 0xFFFF when ``raw`` is given).  dynamic (data-dependent trimming): an element may also be left unwritten where the
    reference is exactly zero -- outside the support -- and nowhere else.  Returns the list of failures (empty = pass)."""
    fails = []
    rb = rec.get('row_begin', 0)
    assert got.shape == rec['out'].shape, (tag, name, got.shape, rec['out'].shape)
    if rb > 0:
        # (a map the confidence heads add into in place is read and stored back above its first row too: NaN stays NaN)
        if not torch.isnan(got[:, :, :rb]).all() or (raw is not None and not rec.get('inplace') and not (raw[:, :, :rb] == -1).all()):
            fails.append(f'{name}: rows above {rb} were written')
    g, r, lo, hi, e = (t[:, :, rb:] for t in (got, rec['out'], rec['lo'], rec['hi'], rec['exc']))
    skipped = torch.isnan(g) & (lo == 0) & (hi == 0) if dynamic else torch.zeros_like(e)
    if not (torch.isfinite(g) | skipped).all():
        fails.append(f'{name}: {int((~(torch.isfinite(g) | skipped)).sum())} non-finite element(s) in the written region')
    ok = ((g >= lo) & (g <= hi)) | skipped
    share = float(e.double().mean()) if e.numel() else 0.0
    nbad = int((~ok).sum())
    out(f'{tag} {name}: {g.numel()} elements, excusable share {share:.4%}, off the nominal value {int((ok & (g != r)).sum())}, '
        f'mismatches {nbad}' + (f", rho {rec['rho'] / EPS24:.2f} x 2^-24" if 'rho' in rec else '')
        + (f', unwritten {float(skipped.double().mean()):.1%}' if dynamic else ''))
    if share > MAX_EXCUSABLE:
        fails.append(f'{name}: excusable share {share:.3%} > {MAX_EXCUSABLE:.0%}: the case proves too little')
    if nbad:
        i = torch.nonzero(~ok)[:4]
        fails.append(f'{name}: {nbad} element(s) differ where no rounding is near a midpoint, first at {i.tolist()}: got '
                     f'{[float(g[tuple(j)]) for j in i]}, want {[float(r[tuple(j)]) for j in i]}')
    return fails


def check_sum(tag, name, got, ref64, ref32, S, out=print, extra=None):
    """An fp32 sum (dW / db) against its fp64 restatement: max |gpu - ref64| / S against k = 4 x the same measure of the CPU's
    fp32-accumulating restatement on the same operands, floor 2^-22.  ``extra`` (the confidence heads): the part of
    |gpu - ref64| that the closed-form error of an fp32 operand explains (``conf_backward``: dz, ill-conditioned where the head
    saturates -- one pixel of a 4 x 4 map moved conf2's gradient by 9e-6 S on the GPU against 8e-7 S on the CPU) is taken off
    both figures first.  Returns (failures, gpu figure, cpu figure)."""
    nz = S > 0
    fails = []
    if not torch.isfinite(got).all():
        return [f'{name}: non-finite'], float('inf'), 0.0
    if (got[~nz] != 0).any():
        fails.append(f'{name}: non-zero where no product contributes')
    ex = torch.zeros_like(S) if extra is None else extra

    def m(a):
        return float((((a - ref64).abs() - ex).clamp_min(0)[nz] / S[nz]).max()) if nz.any() else 0.0
    mg, mc = m(got), m(ref32)
    gate = max(NOISE_K * mc, NOISE_FLOOR)
    out(f'{tag} {name}: max|gpu-ref64|/S {mg:.3e}, cpu fp32 {mc:.3e}, gate {gate:.3e}')
    if mg > gate:
        fails.append(f'{name}: max|gpu-ref64|/S {mg:.3e} > gate {gate:.3e} (cpu fp32 {mc:.3e})')
    return fails, mg, mc


def check_run(tag, got_maps, got_grads, rec64, wg64, wg32, sd, level, dtype, raws=None, skip_maps=(), out=print, dynamic=False):
    """Every per-launch check of one run: the stored maps against ``rec64`` and every gradient against ``wg64`` / ``wg32``.
    Returns (failures, table) -- table rows (name, gpu figure, cpu figure) of the fp32 outputs."""
    fails, table = [], []
    for name, rec in rec64.items():
        if name in skip_maps:
            continue
        fails += check_map(tag, name, got_maps[name], rec, dtype, None if raws is None else raws.get(name), out, dynamic)
    g64, g32 = grads_of(wg64, sd, level), grads_of(wg32, sd, level)
    S, E = {}, {}
    for l, r in wg64.items():
        if isinstance(l, tuple):
            name = f'conf{l[1]}.1.weight'
            S[name], E[name] = r['S'][:, :sd[name].shape[1]], r['E'][:, :sd[name].shape[1]]
            continue
        co, ci = sd[W_ORDER[l] + '.weight'].shape[:2]
        S[W_ORDER[l] + '.weight'] = r['S'][:co, :ci]
        if 'db' in r:
            S[W_ORDER[l] + '.bias'] = r['Sb']
    for name in sorted(g64):
        f, mg, mc = check_sum(tag, name, got_grads[name].double(), g64[name], g32[name], S[name], out, E.get(name))
        fails += f
        table.append((name, mg, mc))
    return fails, table


# ---------------------------------------------------------------------------------------------------------------------
# the cases' inputs (the shapes and seeds of test_vgg_kernels_vs_fp64.py)
# ---------------------------------------------------------------------------------------------------------------------
CASES = {'tiny': (1, 8, 8, (3, 4)), 'odd_pooled': (3, 40, 72, (3, 4)), 'tall': (2, 264, 40, (3,)), 'wide': (1, 16, 296, (4,)),
         'odd_batch': (5, 88, 104, (3,))}
MANY_TILES = (4, 264, 296)


def case_inputs(shape, level, conf_scale=0.1):
    """(sd, x, ups, cups, pad): synthetic parameters and image, the upstream gradients of the normalised maps (NCHW) and of the
    confidence maps ([B,1,h,w], x ``conf_scale``: a tenth of the feature maps', see ``conf_backward``), and at level 4 the noise that fills x24's 48 padded gradient channels (NHWC)."""
    import numpy as np
    from oracle import ref_cpu as O
    B, H, W = shape
    rs = np.random.RandomState(7919 * H + 31 * W + 3 * B + level)
    sd = O.synth_vgg_state(rs, bias_scale=0.05)
    x = torch.from_numpy(rs.random_sample((B, 3, H, W)).astype(np.float32))
    shapes = [(B, c, H >> (3 - l), W >> (3 - l)) for l, c in enumerate((256, 128, 64, 16)[:level])]
    ups = [torch.from_numpy(rs.standard_normal(s)) for s in shapes]
    cups = [torch.from_numpy(rs.standard_normal((s[0], 1, s[2], s[3]))) * conf_scale for s in shapes]
    pad = torch.from_numpy(rs.standard_normal((B, H, W, 48)).astype(np.float32)) if level == 4 else None
    return sd, x, ups, cups, pad


def upstream(ups, cups, pad, dtype):
    """(d_feats NCHW, d_confs [B,h,w]) as the backward receives them: fp32 values (fp64 with ``dtype`` None), x24's padded."""
    cast = (lambda t: t.double()) if dtype is None else (lambda t: t.float().double())
    d_feats = [cast(u) for u in ups]
    if pad is not None:
        d_feats[3] = torch.cat([d_feats[3], cast(pad).permute(0, 3, 1, 2)], 1)
    return d_feats, [cast(c[:, 0]) for c in cups]
