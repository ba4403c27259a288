"""``LM_S2GP.score_loss`` under an installed ``grad_sync``: its backward ends in the tail all HIP backwards share
(``_autograd.extractor_grads``), so the gradients of both extractors go through the all-reduce like those of
``forward(mode='train')``.  Modelled on ``test_grad_sync_over_rccl_leaves_one_rank_gradients_unchanged`` (tests/test_gpu_parity.py)
at the shapes of tests/test_score_loss_gpu.py: one process, a one-rank RCCL group, ``GradSync(force=True)``.

Before the five Functions shared that tail, ``_ScoreFn.backward`` never looked at ``model.grad_sync``: this test then fails on
``collectives == 0`` (under data-parallel training the loss kept per-rank gradients, without an error)."""
import socket

import pytest
import torch

from test_score_loss_gpu import _candidates, _dev, _inputs, _loss, _net

pytestmark = pytest.mark.gpu


def test_score_loss_gradients_go_through_an_installed_grad_sync():
    """The all-reduce of one rank is the identity (RCCL averages inside the collective: divided by 1), so every parameter
    gradient must equal the run without a process group -- to 1e-5 in relative L2, that test's own bound, for its reason: the
    satellite map gradient is summed with fp32 atomics, whose order differs from run to run -- and the grad-less parameters
    (no weights: the confidence heads, conv_dec3, damping) stay grad-less."""
    import torch.distributed as dist
    from highlyaccurate_amd.parallel import GradSync
    dev = _dev()
    net = _net(0)
    sat, grd, gt, extra = _inputs(0)
    cands = _candidates()

    def grads():
        net.zero_grad(set_to_none=True)
        _loss(net, 0, sat, grd, extra, cands, gt).backward()
        torch.cuda.synchronize()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}

    base = grads()
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1, device_id=dev)
    try:
        net.grad_sync = GradSync(force=True)
        got = grads()
        collectives = net.grad_sync.collectives
    finally:
        net.grad_sync = None
        dist.destroy_process_group()
    print(f'SCORE_LOSS grad_sync: {collectives} collectives')
    assert collectives >= 2
    assert sum(g is not None for g in base.values()) >= 36
    for n, g in base.items():
        assert (g is None) == (got[n] is None), n
        if g is not None:
            rel = float((g - got[n]).double().norm() / g.double().norm().clamp_min(1e-30))
            print(f'  {n}: rel-l2 {rel:.2e}')
            assert rel < 1e-5, (n, rel)
