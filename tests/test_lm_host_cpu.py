"""CPU-only pins of what the LM entry points decide on the host before their first HIP call: the workspace size of every size
function, and the return code and message of a too-small workspace and of one argument error per launch function.  The library
loads without a device; no compute call is made, and the pointers in the structs are arbitrary non-zero integers that nothing
dereferences (every call here returns before the first HIP call).  The expected numbers are literals recorded from the library
before the host code of these entry points moved into csrc/lm_host.h: a layout that drifts -- a region added to a launcher and
not to its size function, a tile pick that changes -- shows here without a GPU."""
import ctypes as C

import pytest

from highlyaccurate_amd import _lib

OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3
PTR = 0x1000      # never dereferenced

# (A, h, w, C, row0)
BASE3 = [(64, 32, 128, 256, 16), (128, 64, 256, 128, 32), (256, 128, 512, 64, 64)]
FOUR = BASE3 + [(512, 256, 1024, 16, 128)]
# one level whose pixel count sits exactly on a tile-pick threshold (4096, 16384) or just below it.  S2G counts (h - row0) * w
# ground pixels: 32 * 128, 63 * 65, 64 * 256, 129 * 127; G2S counts A * A satellite pixels: 64^2, 63^2, 128^2, 127^2.
S2G_EDGE = {4096: (64, 48, 128, 128, 16), 4095: (64, 79, 65, 128, 16), 16384: (128, 96, 256, 64, 32), 16383: (128, 161, 127, 64, 32)}
G2S_EDGE = {4096: (64, 32, 128, 128, 0), 3969: (63, 32, 128, 128, 0), 16384: (128, 64, 256, 64, 0), 16129: (127, 64, 256, 64, 0)}


def _levels(spec, dtype=_lib.HLA_F32):
    arr = (_lib.S2GLevel * len(spec))()
    for l, (A, h, w, ch, row0) in enumerate(spec):
        v = arr[l]
        v.sat_feat = v.grd_feat = v.grd_conf = v.xyz = PTR
        v.A, v.h, v.w, v.C, v.row0, v.grd_row_skip = A, h, w, ch, row0, 0
        v.meter_per_pixel, v.centre, v.feat_dtype = 0.2 * (l + 1), A / 2.0, dtype
    return arr


def _cfg(n_levels, **kw):
    c = _lib.S2GConfig()
    c.n_levels, c.n_iters, c.dof = n_levels, 5, 3
    c.shift_range_lat = c.shift_range_lon = 20.0
    c.rotation_range = 10.0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _size(fn, spec, B, K=None, **kw):
    lib = _lib.load()
    args = [C.byref(_cfg(len(spec), **kw)), _levels(spec), B] + ([K] if K is not None else [])
    return getattr(lib, fn)(*args)


# ---- workspace sizes: (size function, levels, B[, K], config fields) -> bytes
S2G_SETS = {'base3': BASE3, 'four': FOUR, **{f'edge{n}': [v] for n, v in S2G_EDGE.items()}}
G2S_SETS = {'base3': BASE3, **{f'edge{n}': [v] for n, v in G2S_EDGE.items()}}

LOOP_BYTES = {
    # hla_s2g_workspace_bytes: the same for level_first 0 and 1
    ('s2g', 'base3'): (9472, 68352, 272384), ('s2g', 'four'): (34048, 265472, 1059840),
    ('s2g', 'edge4096'): (3328, 18688, 73216), ('s2g', 'edge4095'): (5376, 35072, 138752),
    ('s2g', 'edge16384'): (5376, 35072, 138752), ('s2g', 'edge16383'): (9472, 67840, 269824),
    # hla_s2g_bwd_workspace_bytes, deterministic = 0
    ('s2g_bwd', 'base3'): (18176, 134912, 538368), ('s2g_bwd', 'four'): (67328, 528384, 2111744),
    ('s2g_bwd', 'edge4096'): (3840, 19968, 78336), ('s2g_bwd', 'edge4095'): (5888, 36352, 143872),
    ('s2g_bwd', 'edge16384'): (9984, 69120, 274944), ('s2g_bwd', 'edge16383'): (9984, 69120, 274944),
    # hla_s2g_bwd_workspace_bytes, deterministic = 1: + the fixed-point accumulators of every level
    ('s2g_det', 'base3'): (58738432, 469896960, 1879586560), ('s2g_det', 'four'): (92342016, 738725888, 2954901760),
    ('s2g_det', 'edge4096'): (4198144, 33574400, 134296064), ('s2g_det', 'edge4095'): (4200192, 33590784, 134361600),
    ('s2g_det', 'edge16384'): (8398592, 67177984, 268710400), ('s2g_det', 'edge16383'): (8398592, 67177984, 268710400),
    # hla_g2s_workspace_bytes / hla_g2s_bwd_workspace_bytes ('four': proj = 1, the projection that has 16 channels)
    ('g2s', 'base3'): (33280, 263936, 1055232), ('g2s', 'four'): (131584, 1050368, 4200960),
    ('g2s', 'edge4096'): (4608, 34560, 137728), ('g2s', 'edge3969'): (8704, 66304, 264704),
    ('g2s', 'edge16384'): (8704, 67328, 268800), ('g2s', 'edge16129'): (16896, 131840, 526848),
    ('g2s_bwd', 'base3'): (49920, 396032, 1583872), ('g2s_bwd', 'four'): (197376, 1575680, 6302464),
    ('g2s_bwd', 'edge4096'): (6912, 51968, 207616), ('g2s_bwd', 'edge3969'): (13056, 99584, 398080),
    ('g2s_bwd', 'edge16384'): (13056, 101120, 404224), ('g2s_bwd', 'edge16129'): (25344, 197888, 791296),
}
LOOP_FN = {'s2g': ('hla_s2g_workspace_bytes', {}), 's2g_bwd': ('hla_s2g_bwd_workspace_bytes', {}),
           's2g_det': ('hla_s2g_bwd_workspace_bytes', {'deterministic': 1}), 'g2s': ('hla_g2s_workspace_bytes', {}),
           'g2s_bwd': ('hla_g2s_bwd_workspace_bytes', {})}
BATCHES = (1, 8, 32)


@pytest.mark.parametrize('which,name', sorted(LOOP_BYTES))
def test_loop_workspace_bytes(which, name):
    fn, kw = LOOP_FN[which]
    g2s = which.startswith('g2s')
    spec = FOUR if name == 'four' else (G2S_SETS if g2s else S2G_SETS)[name]
    if g2s and name == 'four':
        kw = dict(kw, proj=1)
    for level_first in ((0,) if g2s else (0, 1)):
        got = tuple(_size(fn, spec, B, level_first=level_first, **kw) for B in BATCHES)
        assert got == LOOP_BYTES[which, name], (fn, name, level_first, got)


# pose scores: one level, K hypotheses.  (level, K) -> bytes at B = 1, 8, 32
S2G_SCORE_BYTES = {
    ('base3.0', 5): (20480, 163840, 655360), ('base3.1', 5): (40960, 327680, 1310720), ('base3.2', 33): (540672, 4325376, 17301504),
    ('four.3', 5): (81920, 655360, 2621440), ('edge4095', 33): (135168, 1081344, 4325376),
}
G2S_SCORE_BYTES = {
    ('base3.0', 5): (40960, 327680, 1310720), ('base3.1', 5): (81920, 655360, 2621440), ('base3.2', 33): (1081344, 8650752, 34603008),
    ('four.3', 5): (163840, 1310720, 5242880), ('edge3969', 33): (132096, 1056000, 4224000),
}


def _score_level(name):
    if name.startswith('edge'):
        return name
    s, l = name.split('.')
    return {'base3': BASE3, 'four': FOUR}[s][int(l)]


@pytest.mark.parametrize('name,K', sorted(S2G_SCORE_BYTES))
def test_s2g_pose_score_workspace_bytes(name, K):
    v = _score_level(name)
    spec = S2G_SETS[v] if isinstance(v, str) else [v]
    got = tuple(_size('hla_s2g_pose_score_workspace_bytes', spec, B, K) for B in BATCHES)
    assert got == S2G_SCORE_BYTES[name, K], got


@pytest.mark.parametrize('name,K', sorted(G2S_SCORE_BYTES))
def test_g2s_pose_score_workspace_bytes(name, K):
    v = _score_level(name)
    spec = G2S_SETS[v] if isinstance(v, str) else [v]
    proj = 1 if spec[0][3] == 16 else 0
    got = tuple(_size('hla_g2s_pose_score_workspace_bytes', spec, B, K, proj=proj) for B in BATCHES)
    assert got == G2S_SCORE_BYTES[name, K], got


# ---- error returns of the six launch functions, config of the table above at B = 4
def _grads(n):
    g = (_lib.S2GLevelGrad * n)()
    for l in range(n):
        g[l].d_sat_feat = g[l].d_grd_feat = g[l].d_grd_conf = PTR
    return g


def _launch(fn, ws_bytes, spec=BASE3, dtype=_lib.HLA_F32, B=4, K=5, **kw):
    """Call launch function `fn` with a workspace of ws_bytes; -> (return code, hla_last_error())."""
    lib = _lib.load()
    cfg, lv = C.byref(_cfg(len(spec), **kw)), _levels(spec, dtype)
    p = C.c_void_p(PTR)
    rc = {
        'hla_s2g_lm_solve': lambda: lib.hla_s2g_lm_solve(cfg, lv, None, None, None, p, p, None, p, ws_bytes, B, None),
        'hla_s2g_lm_solve_bwd': lambda: lib.hla_s2g_lm_solve_bwd(cfg, lv, _grads(len(spec)), None, None, None, p, p, p, p, p, ws_bytes, B, None),
        'hla_g2s_lm_solve': lambda: lib.hla_g2s_lm_solve(cfg, lv, p, 256, 1024, None, p, None, p, ws_bytes, B, None),
        'hla_g2s_lm_solve_bwd': lambda: lib.hla_g2s_lm_solve_bwd(cfg, lv, _grads(len(spec)), p, 256, 1024, None, p, p, p, p, p, ws_bytes, B, None),
        'hla_s2g_pose_score': lambda: lib.hla_s2g_pose_score(cfg, lv, None, None, p, K, p, p, p, ws_bytes, B, None),
        'hla_g2s_pose_score': lambda: lib.hla_g2s_pose_score(cfg, lv, p, 256, 1024, p, K, p, p, p, ws_bytes, B, None),
    }[fn]()
    return rc, lib.hla_last_error().decode()


# need: what the size function returns for this call (BASE3, B = 4; the pose scores: level 0, K = 5)
NEED = {'hla_s2g_lm_solve': 34304, 'hla_s2g_lm_solve_bwd': 67840, 'hla_g2s_lm_solve': 132096, 'hla_g2s_lm_solve_bwd': 198144,
        'hla_s2g_pose_score': 81920, 'hla_g2s_pose_score': 163840}


@pytest.mark.parametrize('fn', sorted(NEED))
def test_workspace_one_byte_short(fn):
    spec = BASE3[:1] if 'pose_score' in fn else BASE3
    rc, msg = _launch(fn, NEED[fn] - 1, spec)
    assert (rc, msg) == (ERR_WORKSPACE, f'{fn}: workspace {NEED[fn] - 1} < {NEED[fn]}')


def test_workspace_far_too_small_message():
    assert _launch('hla_s2g_lm_solve', 16) == (ERR_WORKSPACE, 'hla_s2g_lm_solve: workspace 16 < 34304')


ARG_ERRORS = {
    'hla_s2g_lm_solve': (dict(dof=7), 'hla_s2g_lm_solve: dof must be 1..3'),
    'hla_s2g_lm_solve_bwd': (dict(dtype=_lib.HLA_BF16), 'hla_s2g_lm_solve_bwd: level 0: the backward needs fp32 feature maps'),
    'hla_g2s_lm_solve': (dict(level_first=1), 'hla_g2s_lm_solve: LM_G2SP is KITTI-only, 3-DoF, iteration-first, identity damping '
                                             '(models_kitti.py:333-379)'),
    'hla_g2s_lm_solve_bwd': (dict(level_first=1), 'hla_g2s_lm_solve_bwd: bad configuration'),
    'hla_s2g_pose_score': (dict(K=0), 'hla_s2g_pose_score: need B > 0 and K >= 1'),
    'hla_g2s_pose_score': (dict(ford=1), 'hla_g2s_pose_score: LM_G2SP is KITTI-only (models_kitti.py:22-499)'),
}


@pytest.mark.parametrize('fn', sorted(ARG_ERRORS))
def test_argument_error(fn):
    kw, text = ARG_ERRORS[fn]
    spec = BASE3[:1] if 'pose_score' in fn else BASE3
    assert _launch(fn, 1 << 40, spec, **kw) == (ERR_ARG, text)
