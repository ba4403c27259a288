"""``jacobian.grid_sample`` under autograd on the GPU (``hla_grid_sample_bwd``) against fp64 autograd through
``oracle.ref_cpu.grid_sample`` on the CPU, fed the same fp32 inputs and the same random cotangents.

Gate, per gradient tensor, in max-norm:  |hip - ref64| <= max(4 |ref32 - ref64|, 2.4e-7 max|ref64|),  ref32 = the same oracle in
fp32 on the CPU: an fp32 evaluation that sums in another order is expected at about 1x the oracle's own fp32 gap, 4x leaves room
for fused-multiply-add contraction and the 256-term channel sums, and the floor is 2 ulp of the largest element.  Every test
prints its ratios; the worst ones measured on an MI355X are in EXPERIMENTS.md."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import grid_sample_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def hip_fn(*a):
    from highlyaccurate_amd.jacobian import grid_sample
    return grid_sample(*a)


def hip_grads(name, need=(True, True, True), use=('out', 'jac_out'), dtype=torch.float32):
    img, uv, jac, g_out, g_jac = (R.T(a, dtype, DEV) for a in R.make_case(name))
    return R.grads(hip_fn, img, uv, jac, R.linear_loss(g_out, g_jac, use), need)


@pytest.mark.parametrize('case', list(R.CASES))
def test_all_gradients(case):
    r64, r32 = R.oracle_pair(case)
    R.check(case, hip_grads(case), r64, r32)


@pytest.mark.parametrize('case', ['S1', 'S3', 'S4'])
@pytest.mark.parametrize('need', [(True, False, False), (False, True, False), (False, False, True)], ids=['image', 'optical', 'jac'])
def test_one_input_requires_grad(case, need):
    r64, r32 = R.oracle_pair(case)
    got = hip_grads(case, need)
    for g, n in zip(got, need):
        assert (g is not None) == n
    keep = lambda rs: [r if n else None for r, n in zip(rs, need)]
    R.check(f'{case} only {need}', got, keep(r64), keep(r32))


@pytest.mark.parametrize('case', ['S1', 'S2', 'S4'])
@pytest.mark.parametrize('use', [('out',), ('jac_out',)], ids=['out', 'jac_out'])
def test_one_output_used(case, use):
    r64, r32 = R.oracle_pair(case, use)
    got = hip_grads(case, use=use)
    if use == ('out',):                     # jac does not reach out: autograd never visits it
        assert got[2] is None and r64[2] is None
    R.check(f'{case} loss on {use[0]}', got, r64, r32)


def test_no_jacobian_returns_none():
    img, uv, *_ = (R.T(a, torch.float32, DEV) for a in R.make_case('S5'))
    out, jout = hip_fn(img.requires_grad_(True), uv)
    assert jout is None and out.grad_fn is not None and out.shape == (2, 1, 16, 70)


def test_d_image_is_exactly_zero_where_no_sample_lands():
    N, C, IH, IW, H, W, M = 2, 16, 9, 11, 6, 7, 2
    rs = np.random.RandomState(7)
    img = rs.standard_normal((N, C, IH, IW)).astype(np.float32)
    uv = np.stack([rs.uniform(1.2, 5.8, (N, H, W)), rs.uniform(2.1, 6.9, (N, H, W))], -1).astype(np.float32)
    uv[0, 0, :3] = [[-0.5, 3.0], [IW - 0.5, 3.0], [4.0, IH - 0.75]]          # out of view: must add nothing
    uv[1] = np.stack([rs.uniform(-9, -0.01, (H, W)), rs.uniform(IH - 0.99, IH + 5, (H, W))], -1)   # sample 1 all out of view
    jac = rs.standard_normal((M, N, H, W, 2)).astype(np.float32)
    ti, tu, tj = (R.T(a, torch.float32, DEV).requires_grad_(True) for a in (img, uv, jac))
    out, jout = hip_fn(ti, tu, tj)
    (out.sum() + jout.sum()).backward()
    touched = np.zeros((N, IH, IW), bool)
    for (x, y) in uv[0].reshape(-1, 2):
        if 0 <= x <= IW - 1 and 0 <= y <= IH - 1:
            x0, y0 = int(np.floor(x)), int(np.floor(y))
            touched[0, y0:min(y0 + 1, IH - 1) + 1, x0:min(x0 + 1, IW - 1) + 1] = True
    g = ti.grad.cpu().numpy()
    assert touched[0].any() and not touched[0].all() and not touched[1].any()
    assert (g.transpose(0, 2, 3, 1)[~touched] == 0).all()
    assert (g[1] == 0).all() and np.abs(g[0]).max() > 0
    assert (tu.grad[1] == 0).all() and (tj.grad[:, 1] == 0).all()


def test_fp64_noncontiguous_inputs():
    case = 'S1'
    r64, r32 = R.oracle_pair(case)
    img, uv, jac, g_out, g_jac = (R.T(a, torch.float64, DEV) for a in R.make_case(case))
    img_nc = img.transpose(2, 3).contiguous().transpose(2, 3)                        # NCHW, W-major in memory
    uv_nc = torch.stack([uv, uv], -1)[..., 0]                                        # last stride 2
    jac_nc = jac.permute(1, 0, 2, 3, 4).contiguous().permute(1, 0, 2, 3, 4)
    assert not (img_nc.is_contiguous() or uv_nc.is_contiguous() or jac_nc.is_contiguous())
    got = R.grads(hip_fn, img_nc, uv_nc, jac_nc, R.linear_loss(g_out, g_jac))
    for g, ref in zip(got, r64):
        assert g.dtype == torch.float64 and g.shape == ref.shape
    R.check('S1 fp64 non-contiguous', got, r64, r32)


def test_no_grad_path_is_the_plain_forward():
    from highlyaccurate_amd import _lib
    img, uv, jac, *_ = (R.T(a, torch.float32, DEV) for a in R.make_case('S4'))
    N, C, IH, IW, H, W, M = R.CASES['S4']
    nhwc = img.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(N, H, W, C, device=DEV)
    jout = torch.empty(M, N, H, W, C, device=DEV)
    _lib.check(_lib.load().hla_grid_sample(_lib.ptr(nhwc), _lib.ptr(uv), _lib.ptr(jac), _lib.ptr(out), _lib.ptr(jout),
                                           N, C, IH, IW, H, W, M, _lib.stream_ptr()), 'hla_grid_sample')
    want = out.permute(0, 3, 1, 2), jout.permute(0, 1, 4, 2, 3)
    a = hip_fn(img, uv, jac)                                                         # nothing requires grad
    with torch.no_grad():
        b = hip_fn(img.clone().requires_grad_(True), uv, jac)
    c = hip_fn(img.clone().requires_grad_(True), uv, jac)                            # recorded: same values
    for got in (a, b, c):
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    assert all(t.grad_fn is None and not t.requires_grad for t in a + b)
    assert all(t.grad_fn is not None for t in c)


def test_gauss_newton_step_around_the_operator():
    case = 'S2'
    N, C, IH, IW, H, W, M = R.CASES[case]
    img, uv, jac, *_ = R.make_case(case)
    rs = np.random.RandomState(11)
    ghat = rs.standard_normal((N, C * H * W))
    ghat = torch.from_numpy(ghat / np.linalg.norm(ghat, axis=1, keepdims=True))
    cvec = torch.from_numpy(rs.standard_normal((N, M)))
    need = (True, True, False)

    def run(fn, dtype, dev):
        return R.grads(fn, R.T(img, dtype, dev), R.T(uv, dtype, dev), R.T(jac, dtype, dev),
                       R.gn_loss(fn, ghat.to(dev), cvec.to(dev)), need)
    r64, r32 = run(O.grid_sample, torch.float64, 'cpu'), run(O.grid_sample, torch.float32, 'cpu')
    R.check('S2 Gauss-Newton step', run(hip_fn, torch.float32, DEV), r64, r32)


def test_c_boundary_argument_errors():
    from highlyaccurate_amd import _lib
    lib = _lib.load()
    N, C, IH, IW, H, W, M = 1, 4, 5, 6, 2, 3, 2
    img = torch.zeros(N, IH, IW, C, device=DEV)
    uv = torch.full((N, H, W, 2), 1.5, device=DEV)
    jac = torch.zeros(M, N, H, W, 2, device=DEV)
    g_jac = torch.zeros(M, N, H, W, C, device=DEV)
    d_img = torch.zeros_like(img)
    d_jac = torch.zeros_like(jac)
    nul, st = ctypes.c_void_p(0), _lib.stream_ptr()
    p = _lib.ptr
    rc = lib.hla_grid_sample_bwd(p(img), p(uv), nul, nul, p(g_jac), p(d_img), nul, nul, N, C, IH, IW, H, W, M, st)
    assert rc != 0 and 'd_jac_out' in lib.hla_last_error().decode()
    rc = lib.hla_grid_sample_bwd(p(img), p(uv), nul, nul, nul, p(d_img), nul, p(d_jac), N, C, IH, IW, H, W, M, st)
    assert rc != 0 and 'd_jac' in lib.hla_last_error().decode()
    rc = lib.hla_grid_sample_bwd(p(img), p(uv), p(jac), nul, p(g_jac), p(d_img), nul, nul, N, C, IH, IW, H, W, 0, st)
    assert rc != 0 and 'M' in lib.hla_last_error().decode()
    assert lib.hla_grid_sample_bwd(p(img), p(uv), p(jac), nul, p(g_jac), nul, nul, nul, N, C, IH, IW, H, W, M, st) == 0
    assert lib.hla_grid_sample_bwd(p(img), p(uv), p(jac), nul, nul, p(d_img), nul, nul, N, C, IH, IW, H, W, M, st) == 0
    torch.cuda.synchronize()
    assert (d_img == 0).all()


def test_gt_depth_projection_composed_around_the_operator():
    """The intended use: the reference's ``use_gt_depth`` projection written in torch ops around the operator, trained through
    to the satellite map and to the pose."""
    B, C, A, H, W = 2, 5, 9, 6, 11
    rs = np.random.RandomState(5)
    sat = rs.standard_normal((B, C, A, A)).astype(np.float32)
    rays = np.stack([rs.uniform(-1, 1, (H, W)), np.ones((H, W)), rs.uniform(-1, 1, (H, W))], -1).astype(np.float32)
    depth = rs.uniform(1, 4, (B, H, W)).astype(np.float32)
    pose = rs.uniform(-0.5, 0.5, (B, 3)).astype(np.float32)
    w_out = torch.from_numpy(rs.standard_normal((B, C, H, W)))
    w_jac = torch.from_numpy(rs.standard_normal((3, B, C, H, W)))

    def run(fn, dtype, dev):
        s = R.T(sat, dtype, dev).requires_grad_(True)
        p = R.T(pose, dtype, dev).requires_grad_(True)
        R.gt_depth_projection(fn, s, p, R.T(rays, dtype, dev), R.T(depth, dtype, dev), w_out.to(dev), w_jac.to(dev), A).backward()
        return [s.grad, p.grad, None]
    r64, r32 = run(O.grid_sample, torch.float64, 'cpu'), run(O.grid_sample, torch.float32, 'cpu')
    got = run(hip_fn, torch.float32, DEV)
    for n, g, a, b in zip(('d_sat', 'd_pose'), got, r64, r32):
        r, x = R.ratio(g, a, b)
        print(f'gt-depth projection {n}: {x:.2f} x the oracle fp32 gap, {r:.3f} of the gate')
        assert r <= 1.0
