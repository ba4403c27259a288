"""CPU-only checks for the backward of ``jacobian.grid_sample``: the C entry is declared, exported and bound, and the yardstick of
the GPU tests (autograd through ``oracle.ref_cpu.grid_sample``) reproduces the gradients the REAL reference's autograd gave
(tests/golden/grid_sample_grad.npz, written by tools/make_golden_grid_sample_grad.py).

Measured: fp64 oracle against fp64 reference 4e-16 relative at most; fp32 oracle against fp64 reference between 0.64 and 1.00
times the reference's own fp32-versus-fp64 difference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from tests import grid_sample_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_exported_and_bound():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hla.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+hla_grid_sample_bwd\s*\(', text)
    from highlyaccurate_amd import build as B
    from highlyaccurate_amd import _lib
    raw = ctypes.CDLL(B.build())
    assert hasattr(raw, 'hla_grid_sample_bwd')
    fn = _lib.load().hla_grid_sample_bwd
    assert fn.argtypes is not None and len(fn.argtypes) == 16 and fn.restype is ctypes.c_int
    assert int(re.search(r'#define HLA_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION


@pytest.fixture(scope='module')
def gold():
    return load_golden('grid_sample_grad.npz')


@pytest.mark.parametrize('case', ['S1', 'S2'])
def test_fixture_describes_the_case(gold, case):
    img, uv, jac, g_out, g_jac = R.make_case(case)
    N, C, IH, IW, H, W, M = R.CASES[case]
    assert int(gold[f'{case}_seed']) == R.SEEDS[case] and tuple(gold[f'{case}_shape']) == R.CASES[case]
    np.testing.assert_array_equal(gold[f'{case}_planted'], R.planted(IH, IW))
    np.testing.assert_array_equal(uv[0].reshape(-1, 2)[:5], gold[f'{case}_planted'])
    for name, a in (('g_out', g_out), ('g_jac', g_jac)):
        have = gold[f'{case}_{name}']
        if have.shape == a.shape:
            np.testing.assert_array_equal(have, a)
        else:                                           # (sum, sum of squares, first 64 elements) of the seeded stream
            f = a.astype(np.float64).reshape(-1)
            np.testing.assert_array_equal(have, np.concatenate([[f.sum(), (f * f).sum()], f[:64]]))


def _pick(gold, case, name, g):
    """The oracle's gradient in the form the fixture stores it."""
    g = g.detach().double().numpy()
    key = f'{case}_d_image_idx'
    if name == 'd_image' and key in gold.files:
        return g.reshape(-1)[gold[key]]
    return g


@pytest.mark.parametrize('case', ['S1', 'S2'])
def test_oracle_autograd_reproduces_the_reference(gold, case):
    r64, r32 = R.oracle_pair(case)
    for name, g64, g32 in zip(('d_image', 'd_optical', 'd_jac'), r64, r32):
        want64, want32 = gold[f'{case}_{name}64'], gold[f'{case}_{name}32'].astype(np.float64)
        scale = np.abs(want64).max()
        e64 = np.abs(_pick(gold, case, name, g64) - want64).max() / scale
        gap = np.abs(want32 - want64).max()                       # the reference's own fp32 rounding
        e32 = np.abs(_pick(gold, case, name, g32) - want64).max()
        print(f'{case} {name}: fp64 {e64:.1e} relative; fp32 {e32 / gap:.2f} x the reference fp32 gap {gap:.1e}')
        assert e64 <= 1e-12, (case, name, e64)
        assert e32 <= 4 * gap, (case, name, e32, gap)
        key = f'{case}_d_image_stat64'
        if name == 'd_image' and key in gold.files:               # the whole tensor, through two sums
            f = g64.detach().double().reshape(-1)
            np.testing.assert_allclose([f.abs().sum().item(), (f * f).sum().item()], gold[key], rtol=1e-12)
