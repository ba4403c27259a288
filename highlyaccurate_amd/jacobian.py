"""``grid_sample(image, optical, jac=None)`` with the reference's signature (jacobian.py:138-205),
executed by libhla's ``hla_grid_sample``.  Inputs/outputs are NCHW-shaped like the reference's;
internally the image is read channels-last.  Differentiable in all three inputs, as the reference's
chain of torch ops is: the backward is ``hla_grid_sample_bwd`` (first order only; ``d_image`` is
summed with atomics and is not bitwise reproducible from run to run)."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _forward(image, optical, jac):
    """The HIP forward on fp32 NHWC copies.  Returns (out [N,H,W,C], jac_out [M,N,H,W,C] or None, img, opt, jin): the last
    three are what the kernel read (and what the backward reads again)."""
    _lib.require_gpu(image, 'grid_sample image')
    lib = _lib.load()
    N, Cc, IH, IW = image.shape
    _, H, W, _ = optical.shape
    img = image.float().permute(0, 2, 3, 1).contiguous()       # NHWC (no copy if already channels-last)
    opt = optical.float().contiguous()
    out = torch.empty(N, H, W, Cc, device=image.device, dtype=torch.float32)
    M = 0
    jin = jout = None
    if jac is not None:
        M = jac.shape[0]
        jin = jac.float().contiguous()
        jout = torch.empty(M, N, H, W, Cc, device=image.device, dtype=torch.float32)
    if not bool(((opt[..., 0] >= 0) & (opt[..., 0] <= IW - 1) & (opt[..., 1] >= 0) & (opt[..., 1] <= IH - 1)).any()):
        raise AssertionError('grid_sample: no sample falls inside the image')   # jacobian.py:172
    rc = lib.hla_grid_sample(_lib.ptr(img), _lib.ptr(opt), _lib.ptr(jin), _lib.ptr(out), _lib.ptr(jout),
                             N, Cc, IH, IW, H, W, M, _lib.stream_ptr())
    _lib.check(rc, 'hla_grid_sample')
    return out, jout, img, opt, jin


class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, optical, jac):
        out, jout, img, opt, jin = _forward(image, optical, jac)
        ctx.set_materialize_grads(False)            # an unused output costs nothing in the backward
        ctx.save_for_backward(img, opt, jin)
        ctx.meta = [(t.dtype, t.shape) if t is not None else None for t in (image, optical, jac)]
        return out.permute(0, 3, 1, 2), (jout.permute(0, 1, 4, 2, 3) if jout is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_jout):
        img, opt, jin = ctx.saved_tensors
        want_img, want_opt, want_jac = ctx.needs_input_grad
        want_jac = want_jac and g_jout is not None         # jac reaches jac_out only
        if (g_out is None and g_jout is None) or not (want_img or want_opt or want_jac):
            return None, None, None
        N, IH, IW, Cc = img.shape
        _, H, W, _ = opt.shape
        M = jin.shape[0] if jin is not None else 0
        with torch.cuda.device(img.device):
            go = g_out.float().permute(0, 2, 3, 1).contiguous() if g_out is not None else None
            gj = g_jout.float().permute(0, 1, 3, 4, 2).contiguous() if g_jout is not None else None
            d_img = torch.zeros_like(img) if want_img else None                 # accumulated into
            d_opt = torch.empty_like(opt) if want_opt else None
            d_jac = torch.empty_like(jin) if want_jac else None
            rc = _lib.load().hla_grid_sample_bwd(_lib.ptr(img), _lib.ptr(opt), _lib.ptr(jin), _lib.ptr(go), _lib.ptr(gj),
                                                 _lib.ptr(d_img), _lib.ptr(d_opt), _lib.ptr(d_jac),
                                                 N, Cc, IH, IW, H, W, M, _lib.stream_ptr())
            _lib.check(rc, 'hla_grid_sample_bwd')
        res = []
        for g, meta in zip((d_img.permute(0, 3, 1, 2) if want_img else None, d_opt, d_jac), ctx.meta):
            res.append(g.to(meta[0]).reshape(meta[1]) if g is not None else None)
        return tuple(res)


@_lib.on_device(lambda image, *a, **k: image)
def grid_sample(image: torch.Tensor, optical: torch.Tensor, jac: torch.Tensor | None = None):
    """image [N,C,IH,IW]; optical [N,H,W,2] pixel coordinates (x, y); jac [M,N,H,W,2] or None.
    Returns (out [N,C,H,W], jac_out [M,N,C,H,W] or None).  Out-of-bounds samples (and samples exactly on
    the last row/column) are 0, as in the reference.  With grad mode on and an input that requires grad the
    call is recorded for autograd; gradients come back in each input's dtype and shape."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (image, optical, jac)):
        return _GridSample.apply(image, optical, jac)
    out, jout, *_ = _forward(image, optical, jac)
    return out.permute(0, 3, 1, 2), (jout.permute(0, 1, 4, 2, 3) if jout is not None else None)
