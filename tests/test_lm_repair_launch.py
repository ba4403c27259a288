"""The single-launch repair loop (csrc/lm_solve.hip: lm_repair_loop) behind hla_s2g_config.reach_mode = 2, through the C ABI with
hand-made levels.

The reference is the multi-launch loop itself: the same call with reach_mode = 0 on the same whole maps.  A flagged sample's
``trace`` and ``normal_eq`` rows must be the same BITS (there is no tolerance to choose), an unflagged sample's rows must still hold
the sentinel they were pre-filled with.  count_in_view is off in both calls (with it the gated call keeps the multi-launch loop,
whose counting launches read every step's coefficients from the workspace); no confidence weights, one map type per pyramid: what
lm_repair_loop is built for.  There are no fp32 cases: hla_s2g_lm_solve keeps the gated multi-launch loop for fp32 maps, so they would
compare that loop with itself.  (An fp32 instantiation was built and held to these checks on the MI355X: normal_eq off by up to
2.98e-07 / 5.36e-07 absolute on SMALL's two flagged samples, 1.07e-06 / 3.22e-06 / 1.07e-06 on LARGE's three, about 1e-7 relative,
and other traces in the re-initialisation case.  The diverging instructions are named in EXPERIMENTS.md, "Repair loop as one
launch".)

Shapes: the smallest that reach each way the kernel can go wrong.  SMALL has the three channel counts on 108 / 432 / 1728 pixels
(128-pixel tiles: 1 tile -- three of the four 256-thread groups idle --, 4 tiles with a 48-pixel last one, 14 tiles -- not a
multiple of 4 -- with a 64-pixel last one; the last level with a grd_row_skip).  LARGE has 4323 pixels (256-pixel tiles: 17, the
last one 227) and 16705 pixels (512-pixel tiles: 33, the last one 321)."""
import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import test_lm_kernels_vs_fp64 as K

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = 7.0
#          (h, w, row0, grd_row_skip), C, A, metres per pixel
SMALL = (((12, 18, 6, 0), 256, 16, 0.5), ((24, 36, 12, 0), 128, 13, 0.75), ((48, 72, 24, 3), 64, 16, 0.5))
LARGE = (((40, 131, 7, 0), 128, 16, 0.5), ((129, 257, 64, 0), 64, 13, 0.75))
# the re-initialisation case: SMALL's shapes on maps 16 times as coarse, so that a pose at the edge of the +-2.5 band (a shift of
# 2.499 x 6 m = 1.9 px here) still has its pixels in view, and a small damping, so that a step is long enough to leave the band
COARSE = tuple((s, C, A, mpp * 16) for s, C, A, mpp in SMALL)
REINIT_DAMPING = (1e-3, 1e-3, 1e-3)
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def tiles(pyramid):
    """(tile size, tiles, pixels of the last tile) per level: lm_pick_tile_fwd of csrc/lm_solve.hip."""
    out = []
    for (h, w, row0, _), _, _, _ in pyramid:
        npix = (h - row0) * w
        tp = 512 if npix >= 16384 else 256 if npix >= 4096 else 128
        nt = -(-npix // tp)
        out.append((tp, nt, npix - (nt - 1) * tp))
    return out


def make_case(pyramid, B, dtype, N, seed, edge_poses=False, use_keep=False):
    """-> (geom, levels, pose0 [B,3], rand_uv [steps,2,B], keep [steps, max npix] uint8 or None), KITTI chain."""
    levels = [R.make_level(0, s, C, A, B, seed + 10 * l, mpp, dtype) for l, (s, C, A, mpp) in enumerate(pyramid)]
    rs = np.random.RandomState(seed + 77)
    p0 = rs.uniform(-0.3, 0.3, size=(B, 3)).astype(np.float32)
    if edge_poses:      # shift_u / shift_v alternately at either edge of the band the re-initialisation rule keeps
        p0[:, 0] = [2.499 * (-1) ** b for b in range(B)]
        p0[:, 1] = [2.499 * (-1) ** (b // 2) for b in range(B)]
    steps = len(pyramid) * N
    rand_uv = rs.uniform(-1, 1, size=(steps, 2, B)).astype(np.float32)
    npix = max((lv.h - lv.row0) * lv.w for lv in levels)
    keep = torch.from_numpy((rs.uniform(size=(steps, npix)) < 0.5).astype(np.uint8)) if use_keep else None
    return R.make_geom(0, B), levels, torch.from_numpy(p0), torch.from_numpy(rand_uv), keep


def reinit_fired(trace, rand_uv, L, N, level_first, samples):
    """[(sample, step, component)] where the pose a step left IS that step's draw: the re-initialisation rule fired there (a draw
    is a uniform fp32 in (-1, 1); an LM step landing on those very bits does not happen)."""
    hits = []
    for k, (i, l) in enumerate(R.step_order(L, N, level_first)):
        for b in samples:
            for j in range(2):
                if float(trace[b, i, l, j]) == float(rand_uv[k, j, b]):
                    hits.append((b, k, j))
    return hits


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _check(case, flags, N=2, level_first=0, damping=(1.0, 1.0, 1.0)):
    """Both calls on one set of device tensors.  -> the reach_mode = 0 trace."""
    geom, levels, p0, rand_uv, keep = case
    B, L = p0.shape[0], len(levels)
    assert len(flags) == B
    d = K._dev()
    flag = torch.tensor(flags, dtype=torch.int32, device=d)
    call = K._Call(geom, levels, N=N, level_first=level_first, keep=keep, damping=damping, reach_mode=0, reach_flag=flag)
    call.cfg.count_in_view = 0
    tr0, nq0 = call.forward(p0, rand_uv)
    assert bool(torch.isfinite(tr0).all()) and bool(torch.isfinite(nq0).all())
    call.cfg.reach_mode = 2
    trace = torch.full((B, N, L, 3), SENTINEL, device=d, dtype=F32)
    neq = torch.full((L * N, B, 16), SENTINEL, device=d, dtype=F64)
    ws = torch.zeros(call.lib.hla_s2g_workspace_bytes(K.C.byref(call.cfg), call.lv, B), dtype=torch.uint8, device=d)
    tr2, nq2 = call.forward(p0, rand_uv, out=(trace, neq, ws))
    assert flag.cpu().tolist() == list(flags)                               # the gated call leaves the flags alone
    on = [b for b in range(B) if flags[b]]
    off = [b for b in range(B) if not flags[b]]
    assert _bits(tr2[on], tr0[on]), (tr2[on], tr0[on])
    assert _bits(nq2[:, on], nq0[:, on]), (nq2[:, on] - nq0[:, on]).abs().amax((0, 2))
    assert bool((tr2[off] == SENTINEL).all()) and bool((nq2[:, off] == SENTINEL).all())
    return tr0


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_small_pyramid_two_of_five_flagged(dtype):
    assert tiles(SMALL) == [(128, 1, 108), (128, 4, 48), (128, 14, 64)]
    _check(make_case(SMALL, 5, DTYPES[dtype], 2, R.case_seed('repair', 'small', dtype)), (1, 0, 1, 0, 0))


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_large_pyramid_all_three_flagged(dtype):
    assert tiles(LARGE) == [(256, 17, 227), (512, 33, 321)]
    _check(make_case(LARGE, 3, DTYPES[dtype], 1, R.case_seed('repair', 'large', dtype)), (1, 1, 1), N=1)


@pytest.mark.parametrize('level_first', [0, 1])
def test_one_flagged_sample(level_first):
    _check(make_case(SMALL, 1, torch.bfloat16, 2, R.case_seed('repair', 'one', level_first)), (1,), level_first=level_first)


def test_dropout_keep_masks():
    _check(make_case(SMALL, 5, torch.bfloat16, 2, R.case_seed('repair', 'keep'), use_keep=True), (1, 0, 1, 0, 0))


REINIT_FLAGS = (1, 1, 0, 1, 1, 1)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_reinitialisation_rule_fires(dtype):
    """Start poses at the edge of the band, on the map types lm_repair_loop serves: the draw of the step (rand_uv of step k, row
    stride B), the rule itself and the pose it leaves for the next step all run in the new kernel.  That the rule fires for a
    flagged sample is read off the reach_mode = 0 trace; a case in which it does not proves nothing and fails."""
    B = len(REINIT_FLAGS)
    case = make_case(COARSE, B, DTYPES[dtype], 2, R.case_seed('repair', 'reinit', dtype), edge_poses=True)
    tr0 = _check(case, REINIT_FLAGS, damping=REINIT_DAMPING)
    hits = reinit_fired(tr0, case[3], len(COARSE), 2, 0, [b for b in range(B) if REINIT_FLAGS[b]])
    print(f'LMREP {dtype} re-initialised (sample, step, component): {hits}')
    assert hits, 'no flagged sample was re-initialised: the case proves nothing'
