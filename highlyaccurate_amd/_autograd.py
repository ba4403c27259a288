"""What the autograd Functions of both directions share: ``_LocaliseFn`` / ``_ScoreFn`` (_s2gp.py), ``_G2sFn`` / ``_G2sScoreFn``
(_g2sp.py) and ``_G2sCorrFn`` (_g2s_corr.py).  Each of them extracts both pyramids with their activations saved, runs its own
kernels, and in ``backward`` turns the per-level map gradients into parameter gradients with ``extractor_grads``."""
from __future__ import annotations

import torch

from .VGG import vgg_backward_nhwc, vgg_forward_nhwc

_SIDE_STREAMS = {}


def _side_stream(device) -> 'torch.cuda.Stream':
    """One extra stream per device, kept OUTSIDE the modules (a Stream inside a module's __dict__ would break pickling / deepcopy)."""
    idx = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    st = _SIDE_STREAMS.get(idx)
    if st is None:
        st = _SIDE_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return st


def grad_params(model):
    """(names, params) of the model when this call is under autograd (its Function takes ``*params``), else None."""
    if not (torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())):
        return None
    named = list(model.named_parameters())
    return [n for n, _ in named], [p for _, p in named]


def extract_saved(model, sat_map, grd_img, want_conf):
    """Both extractors with their activations saved, normalisation deferred:
    (sat_feats, sat_inv, grd_feats, grd_confs, grd_inv, cs, cg); cs / cg are the contexts ``extractor_grads`` takes."""
    sat_feats, _, sat_inv, cs = vgg_forward_nhwc(model.SatFeatureNet, sat_map, want_conf=False, defer_norm=True,
                                                 save_for_backward=True)
    grd_feats, grd_confs, grd_inv, cg = vgg_forward_nhwc(model.GrdFeatureNet, grd_img, want_conf=want_conf, defer_norm=True,
                                                         save_for_backward=True)
    return sat_feats, sat_inv, grd_feats, grd_confs, grd_inv, cs, cg


def take_state(ctx, what='forward'):
    """``ctx.state`` of a Function's forward, released here: the saved workspaces (GBs at B = 32) then go when this backward
    returns, not when the loss tensor dies.  retain_graph is not supported by the HIP backward: a second backward raises."""
    if ctx.state is None:
        raise RuntimeError(f'backward through the same {what} twice: the saved activations are released after the first '
                           'backward; retain_graph is not supported by the HIP backward')
    state, ctx.state = ctx.state, None
    return state


def extractor_grads(model, cs, cg, d_sat, d_grd, grd_confs=None, d_conf=None, *, scale_invariant=False, first_row8=0, dense=False,
                    wgrad_two_phase=0, stats=None, two_streams=False):
    """The tail of every backward: ``hla_vgg_backward`` of the satellite branch (context ``cs``, map gradients ``d_sat``), then of
    the ground branch (``cg``, ``d_grd``, and its confidence maps with their gradients when the heads took part) ->
    {parameter name of the model: gradient}.
    ``scale_invariant`` / ``dense`` / ``wgrad_two_phase``: ``vgg_backward_nhwc``'s, for both branches; ``first_row8``: the ground
    branch's; ``stats``: the satellite branch's.
    ``model.grad_sync`` (parallel.GradSync, optional): the satellite branch's bucket is started before the ground branch's
    backward, so its all-reduce is in flight under those kernels; both are finished here.
    ``two_streams``: without a ``grad_sync``, the satellite branch runs on a side stream next to the ground branch's."""
    sync = getattr(model, 'grad_sync', None)
    # The two extractors' backward passes are independent.  After the data-dependent trimming the satellite branch's launches are
    # sparse (0.42 of the tiles: many of them fill the chip for a round or two only), so next to the ground branch's they cost
    # 24.78 -> 24.43 ms per training step (same-box A/B, four alternating pairs, the faster one every time; the same split of the
    # two FORWARD passes, both dense, measured 2 % slower).  Not with a gradient all-reduce installed: there the satellite bucket
    # is already in flight under the ground branch's backward.
    # Memory: the satellite branch's backward workspace and gradient buffer then come from the side stream's pool of the caching
    # allocator, so the freed block cannot be reused for the ground branch's workspace on the main stream: peak training memory
    # is one backward workspace higher (GB-class at B = 32 in fp32) for that 1.4 %.
    two = two_streams and sync is None
    kw = dict(scale_invariant=scale_invariant, flat=True, dense=dense, wgrad_two_phase=wgrad_two_phase)
    if two:
        cur = torch.cuda.current_stream()
        side = _side_stream(d_sat[0].device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            g_sat, flat_sat = vgg_backward_nhwc(model.SatFeatureNet, cs, d_sat, stats=stats, **kw)
        for t in d_sat:
            t.record_stream(side)
    else:
        g_sat, flat_sat = vgg_backward_nhwc(model.SatFeatureNet, cs, d_sat, stats=stats, **kw)
    grads = {'SatFeatureNet.' + k: v for k, v in g_sat.items()}
    h_sat = sync.start(grads, flat_sat) if sync else None
    g_grd, flat_grd = vgg_backward_nhwc(model.GrdFeatureNet, cg, d_grd, grd_confs, d_conf, first_row8=first_row8, **kw)
    g_grd = {'GrdFeatureNet.' + k: v for k, v in g_grd.items()}
    h_grd = sync.start(g_grd, flat_grd) if sync else None
    if two:
        cur.wait_stream(side)
        for t in [flat_sat] + list(g_sat.values()):       # allocated on the side stream, consumed (optimizer) on this one
            t.record_stream(cur)
    if sync:
        sync.finish(h_sat)
        sync.finish(h_grd)
    grads.update(g_grd)
    return grads
