"""The reach flag of the satellite -> ground LM loop (hla_s2g_config.reach_mode; csrc/lm_common.h: lm_pixel's `u < col0`,
csrc/lm_solve.hip: reach_clear, the masked and the dropped pixels' tap redirect, the gated second call) at kernel level, through
the C ABI with hand-made levels, against the fp64 rule ``lm_kernel_ref.reach_flags``.

Inputs (tests/lm_kernel_ref.py; their conditions are asserted on the references alone in tests/test_lm_reach_ref_cpu.py):
  one level    KITTI chain, A = 16, first valid column col0 = 10 (the ground mask z > 0 is u > 8, so a pixel can take part left of
               the column only when the column lies right of the centre).  A clean table's smallest u is EXACTLY col0; samples
               differ by pose only, and the dyadic poses shift_u = -+2^-14 move every u by exactly -+3 * 2^-12 px: the sample at
               pose 0 must not be flagged, its mate at -2^-14 must, the one at +2^-14 must not.  A case adds one crossing pixel at
               col0 - 2^-12, col0 - 1 or col0 - 1 + 2^-12: the first pixel read, the last of a 3-pixel last tile, one in the last
               of 65 tiles, one in a stored row above row0 (not read), a dropped one, one with zero confidence.
  two levels   A / col0 = 16 / 10 and 13 / 8, 2 iterations, both loop orders, poses that move: one sample crosses only at level 1
               and only in iteration 2, one only under col0[0], one always, one never; every pixel stays >= 50 x the pose gate's
               reach away from its column, so the flags of the fp64 trajectory are the kernel's.
NaN strip: the same calls on maps whose columns < col0 are NaN.  Masked, out-of-view and dropped pixels must then read at column
col0: an unflagged sample's trace, sums and count are finite and bit-equal to a reach_mode = 0 call on the whole map, which is
itself gated against fp64 with the sum and pose gates of tests/test_lm_kernels_vs_fp64.py (TOL_SUM, TOL_POSE) -- the only
tolerances here; everything else is asserted bit for bit.
Flags are handed over holding 7: the init launch has to clear them.
Measured figures and the mutants these tests catch: EXPERIMENTS.md, "Column trim and reach flag at their borders"."""
import numpy as np
import pytest
import torch

import lm_kernel_ref as R
import test_lm_kernels_vs_fp64 as K

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
COL0, A = R.REACH_COL0, R.REACH_A
FLAG_FILL = 7
SENTINEL = 7.0


def _bits(a, b):
    """Bitwise (NaN-safe) equality."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _flag_buffer(B, fill=FLAG_FILL):
    return torch.full((B,), fill, dtype=torch.int32, device=K._dev())


def _run(geom, levels, p0, rand_uv, mode, col0=None, **kw):
    """One hla_s2g_lm_solve call.  -> (call, trace, normal_eq, flags as a list or None)."""
    B = p0.shape[0]
    flag = _flag_buffer(B) if mode else None
    call = K._Call(geom, levels, reach_mode=mode, reach_flag=flag, reach_col0=col0, **kw)
    trace, neq = call.forward(p0, rand_uv)
    return call, trace, neq, (None if flag is None else flag.cpu().tolist())


def _same_rows(tag, got, ref, rows):
    """Samples ``rows`` of (trace, normal_eq): finite where the loop writes, and the same bits."""
    (tr, nq), (tr0, nq0) = got, ref
    assert rows, tag
    assert bool(torch.isfinite(tr[rows]).all()) and bool(torch.isfinite(nq[:, rows, :15]).all()), (tag, tr[rows], nq[:, rows])
    assert _bits(tr[rows], tr0[rows]) and _bits(nq[:, rows], nq0[:, rows]), (tag, tr[rows], tr0[rows])


def _check_one_level(name, Cn=64, dtype=F32, using_weight=0, col0=COL0, p0=None):
    geom, lv, case_p0, keep, _ = R.reach_case(name, Cn, dtype)
    p0 = case_p0 if p0 is None else p0
    B = p0.shape[0]
    ruv = torch.zeros(1, 2, B)
    kp = None if keep is None else keep[0].bool()
    tag = f'reach {name} C{Cn} {str(dtype)[6:]} w{using_weight} col0 {col0}'
    expect = R.reach_flags(geom, [lv], [(0, R.pose_cols(p0, F64))], [col0], keep).tolist()
    kw = dict(using_weight=using_weight, keep=keep)
    # reach_mode 0 on the whole map, against fp64: what an unflagged sample has to reproduce bit for bit
    _, tr0, nq0, _ = _run(geom, [lv], p0, ruv, 0, **kw)
    sums, mags, count = R.level_sums(geom, R.cast_level(lv, F64), R.pose_cols(p0, F64), using_weight, kp)
    K._gate_sums(tag, nq0[0, :, :14], sums, mags)
    assert np.array_equal(nq0[0, :, 14].numpy(), count.double().numpy()), (tag, nq0[0, :, 14], count)
    new = {dt: R.level_step(R.update_args(), geom, R.cast_level(lv, dt), R.pose_cols(p0, dt), using_weight,
                            (torch.zeros(B, 1, dtype=dt), torch.zeros(B, 1, dtype=dt)), keep=kp) for dt in (F64, F32)}
    K._gate_pose(tag, tr0[:, 0, 0], new[F64], new[F32])
    # detection on the whole map: the flags, and no bit of any sample's result moves
    _, tr1, nq1, f1 = _run(geom, [lv], p0, ruv, 1, [col0], **kw)
    assert f1 == expect, (tag, f1, expect)
    assert _bits(tr1, tr0) and _bits(nq1, nq0), tag
    # detection on the NaN strip
    _, tr2, nq2, f2 = _run(geom, [R.nan_strip(lv, col0)], p0, ruv, 1, [col0], **kw)
    assert f2 == expect, (tag, f2, expect)
    un = [b for b in range(B) if not expect[b]]
    if un:
        _same_rows(tag, (tr2, nq2), (tr0, nq0), un)
    print(f'LMR flags {tag}: {f2}')
    return expect


@pytest.mark.parametrize('using_weight', [0, 1])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['fp32', 'fp16', 'bf16'])
@pytest.mark.parametrize('Cn', [16, 64, 128, 256])
def test_flag_on_the_column_every_instantiation(Cn, dtype, using_weight):
    """u = col0 exactly (pose 0), col0 - 3 * 2^-12 (shift_u = -2^-14), col0 + 3 * 2^-12 (+2^-14), and shift_v = 0.25, which brings
    the pixels left of the column that lay outside the map in v into it."""
    assert _check_one_level('clean', Cn, dtype, using_weight) == [0, 1, 0, 1]


@pytest.mark.parametrize('name,Cn,using_weight,expect', [
    ('first', 64, 0, [1, 0, 1]), ('last', 256, 1, [1, 1, 1]), ('many_last', 16, 0, [1, 1]), ('not_read', 128, 1, [0, 0]),
    ('dropped', 64, 1, [0, 0, 1]), ('conf0', 64, 1, [1, 0, 1])])
def test_flag_of_one_crossing_pixel(name, Cn, using_weight, expect):
    """Where the one pixel left of the column sits (first read, last of the ragged last tile, last of 65 tiles, above row0) and
    what it is (dropped: no flag; zero confidence: its taps are read all the same, so it flags)."""
    assert _check_one_level(name, Cn, F32, using_weight) == expect


def test_flag_of_one_crossing_pixel_16bit_many_tiles():
    assert _check_one_level('many_last', 16, torch.float16, 0) == [1, 1]


def test_flag_with_idle_blocks():
    """B = 9 (the XCD-affine block map, seven idle blocks per tile): the crossing sample is the ninth."""
    assert _check_one_level('idle_blocks', 64, F32, 1) == [0] * 8 + [1]


def test_flag_across_two_stream_groups():
    """B = 17: the loop runs samples [0, 16) and [16, 17) on two streams; samples 0, 15 and 16 cross, the others do not."""
    assert _check_one_level('two_groups', 64, F32, 0) == [1] + [0] * 14 + [1, 1]


@pytest.mark.parametrize('col0,expect', [(A - 1, [1, 1, 0, 1]), (0, [0, 0, 0, 0])])
def test_flag_at_the_edges_of_the_legal_columns(col0, expect):
    """reach_col0 = A - 1 is legal: every pixel that takes part with u < A - 1 flags (the sample with nothing in view does not, and
    on a map that is NaN but for its last column its sums are exact zeros); col0 = 0 can flag nothing and clears the flags."""
    p0 = torch.tensor([R.REACH_POSES[0], R.REACH_POSES[1], R.OUT_OF_VIEW_POSE, R.REACH_POSES[2]], dtype=F32)
    assert _check_one_level('clean', 64, F32, 1, col0=col0, p0=p0) == expect


# ----------------------------------------------------------------------------------------------------------------------
# moving poses, two levels x two iterations
# ----------------------------------------------------------------------------------------------------------------------
def _two_level_whole(level_first):
    """The reach_mode = 0 run on whole maps, teacher-forced against fp64 like test_forward_random_poses_two_levels_teacher_forced."""
    geom, levels, p0, rand_uv, keep = R.reach2_case(level_first)
    kw = dict(N=2, level_first=level_first, using_weight=1, keep=keep)
    _, tr0, nq0, _ = _run(geom, levels, p0, rand_uv, 0, **kw)
    args = R.update_args()
    casts = {dt: [R.cast_level(lv, dt) for lv in levels] for dt in (F64, F32)}
    prev = p0
    for k, (i, l) in enumerate(R.step_order(2, 2, level_first)):
        lv = levels[l]
        kp = keep[k, :(lv.h - lv.row0) * lv.w].bool() if keep is not None else None
        new = {dt: R.level_step(args, geom, casts[dt][l], R.pose_cols(prev, dt), 1, tuple(rand_uv[k, j][:, None].to(dt) for j in range(2)),
                                keep=kp) for dt in (F64, F32)}
        sums, mags, count = R.level_sums(geom, casts[F64][l], R.pose_cols(prev, F64), 1, kp)
        K._gate_sums(f'reach2 lf{level_first} step {k}', nq0[k, :, :14], sums, mags)
        assert np.array_equal(nq0[k, :, 14].numpy(), count.double().numpy()), (k, nq0[k, :, 14], count)
        K._gate_pose(f'reach2 lf{level_first} step {k}', tr0[:, i, l], new[F64], new[F32])
        prev = tr0[:, i, l]
    return (geom, levels, p0, rand_uv, keep), kw, (tr0, nq0)


@pytest.mark.parametrize('level_first', [0, 1])
def test_flag_of_moving_poses_two_levels(level_first):
    """The expected flags come from the fp64 reference's own trajectory (sample 3 crosses in the last step only, at level 1;
    sample 1 only under col0[0]; sample 0 reads left of col0[0] = 10 at level 1 all the time, where the column is 8)."""
    (geom, levels, p0, rand_uv, keep), kw, whole = _two_level_whole(level_first)
    steps, _ = R.trajectory(geom, levels, p0, rand_uv, 2, level_first, 1, keep, F64)
    expect = R.reach_flags(geom, levels, steps, R.REACH2_COL0, keep).tolist()
    assert expect == [0, 1, 1, 1]
    _, tr1, nq1, f1 = _run(geom, levels, p0, rand_uv, 1, R.REACH2_COL0, **kw)
    print(f'LMR flags reach2 lf{level_first}: whole maps {f1}')
    assert f1 == expect and _bits(tr1, whole[0]) and _bits(nq1, whole[1])
    strips = [R.nan_strip(lv, c) for lv, c in zip(levels, R.REACH2_COL0)]
    _, tr2, nq2, f2 = _run(geom, strips, p0, rand_uv, 1, R.REACH2_COL0, **kw)
    print(f'LMR flags reach2 lf{level_first}: NaN strips {f2}')
    assert f2 == expect
    _same_rows(f'reach2 lf{level_first}', (tr2, nq2), whole, [0])


# ----------------------------------------------------------------------------------------------------------------------
# the whole protocol: detect on NaN strips, complete the flagged samples' maps, run again gated
# ----------------------------------------------------------------------------------------------------------------------
def _protocol(case, col0, kw, whole, expect):
    geom, levels, p0, rand_uv = case
    B = p0.shape[0]
    flag = _flag_buffer(B)
    strips = [R.nan_strip(lv, c) for lv, c in zip(levels, col0)]
    call = K._Call(geom, strips, reach_mode=1, reach_flag=flag, reach_col0=col0, **kw)
    tr1, nq1 = call.forward(p0, rand_uv)
    f1 = flag.cpu()
    assert f1.tolist() == expect, (f1, expect)
    # the host stands in for the extractor's fix-up pass: the whole maps for the flagged samples, in place
    hit = torch.tensor([b for b in range(B) if expect[b]], device=K._dev())
    for l, lv in enumerate(levels):
        call.t[l][0][hit] = lv.sat.permute(0, 2, 3, 1).contiguous().to(K._dev())[hit]
    call.cfg.reach_mode = 2
    tr2, nq2 = call.forward(p0, rand_uv, out=(call.trace, call.neq, call.ws))
    assert _bits(flag.cpu(), f1)                                                    # the gated call leaves the flags alone
    un = [b for b in range(B) if not expect[b]]
    assert _bits(tr2[un], tr1[un]) and _bits(nq2[:, un], nq1[:, un])               # ... and the unflagged samples' rows
    assert bool(torch.isfinite(tr2).all()) and bool(torch.isfinite(nq2).all())
    assert _bits(tr2, whole[0]) and _bits(nq2, whole[1])                            # every sample: one call on whole maps
    return call


def _one_level_protocol(name):
    geom, lv, p0, keep, _ = R.reach_case(name, 64)
    B = p0.shape[0]
    rand_uv = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, size=(1, 2, B)).astype(np.float32))
    kw = dict(using_weight=1)
    expect = R.reach_flags(geom, [lv], [(0, R.pose_cols(p0, F64))], [COL0]).tolist()
    _, tr0, nq0, _ = _run(geom, [lv], p0, rand_uv, 0, **kw)
    return _protocol((geom, [lv], p0, rand_uv), [COL0], kw, (tr0, nq0), expect), (geom, lv, p0, rand_uv)


def test_protocol_one_level_bitwise():
    _one_level_protocol('clean')


def test_protocol_b17_gated_call_without_stream_split():
    """The gated call runs on the caller's stream alone whatever B is; detection at B = 17 ran on two."""
    _one_level_protocol('two_groups')


@pytest.mark.parametrize('level_first', [0, 1])
def test_protocol_two_levels_moving_poses_bitwise(level_first):
    (geom, levels, p0, rand_uv, keep), kw, whole = _two_level_whole(level_first)
    _protocol((geom, levels, p0, rand_uv), R.REACH2_COL0, kw, whole, [0, 1, 1, 1])


def test_gated_call_with_no_flag_set_writes_nothing():
    geom, lv, p0, _, _ = R.reach_case('clean', 64)
    B = p0.shape[0]
    d = K._dev()
    flag = _flag_buffer(B, 0)
    call = K._Call(geom, [lv], using_weight=1, reach_mode=2, reach_flag=flag)
    trace = torch.full((B, 1, 1, 3), SENTINEL, device=d, dtype=F32)
    neq = torch.full((1, B, 16), SENTINEL, device=d, dtype=F64)
    nbytes = call.lib.hla_s2g_workspace_bytes(K.C.byref(call.cfg), call.lv, B)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=d)
    tr, nq = call.forward(p0, torch.zeros(1, 2, B), out=(trace, neq, ws))
    assert bool((tr == SENTINEL).all()) and bool((nq == SENTINEL).all()) and flag.cpu().tolist() == [0] * B


# ----------------------------------------------------------------------------------------------------------------------
# validation: an error code with a message, nothing launched
# ----------------------------------------------------------------------------------------------------------------------
def _refused(call, p0, match):
    from highlyaccurate_amd._lib import HlaError
    B = p0.shape[0]
    with pytest.raises(HlaError, match=match):
        call.forward(p0, torch.zeros(call.L * call.N, 2, B))
    torch.cuda.synchronize()
    assert bool(torch.isnan(call.trace).all()) and bool(torch.isnan(call.neq).all())      # the NaN fill: nothing ran


def test_validation_of_the_reach_fields():
    geom, lv, p0, _, _ = R.reach_case('clean', 64)
    B = p0.shape[0]
    flag = _flag_buffer(B)
    _refused(K._Call(geom, [lv], reach_mode=1, reach_flag=None, reach_col0=[COL0]), p0, 'reach_mode')
    _refused(K._Call(geom, [lv], reach_mode=2, reach_flag=None), p0, 'reach_mode')
    _refused(K._Call(geom, [lv], reach_mode=3, reach_flag=flag, reach_col0=[COL0]), p0, 'reach_mode')
    _refused(K._Call(geom, [lv], reach_mode=1, reach_flag=flag, reach_col0=[A]), p0, 'reach_col0')
    _refused(K._Call(geom, [lv], reach_mode=1, reach_flag=flag, reach_col0=[-1]), p0, 'reach_col0')
    assert flag.cpu().tolist() == [FLAG_FILL] * B
    # second level's column out of range
    g2, levels, p2, rand_uv, _ = R.reach2_case(0)
    call = K._Call(g2, levels, N=2, reach_mode=1, reach_flag=_flag_buffer(p2.shape[0]), reach_col0=[R.REACH2_COL0[0], levels[1].A])
    _refused(call, p2, r'reach_col0\[1\]')


@pytest.mark.parametrize('mode', [1, 2])
def test_validation_backward_takes_no_reach_mode(mode):
    from highlyaccurate_amd._lib import HlaError
    geom, lv, p0, _, _ = R.reach_case('clean', 64)
    B = p0.shape[0]
    call = K._Call(geom, [lv], using_weight=1, damping=K._lambda())
    call.forward(p0, torch.zeros(1, 2, B))
    flag = _flag_buffer(B)
    call.cfg.reach_mode, call.cfg.reach_flag, call.cfg.reach_col0[0] = mode, flag.data_ptr(), COL0
    with pytest.raises(HlaError, match='reach_mode'):
        call.backward(torch.ones(B, 1, 1, 3))
    assert flag.cpu().tolist() == [FLAG_FILL] * B


def test_validation_ground_to_satellite_takes_no_reach_mode(monkeypatch):
    """hla_g2s_lm_solve, hla_g2s_lm_solve_bwd and hla_g2s_pose_score read the same config struct: reach_mode must be 0 there."""
    from highlyaccurate_amd._lib import HlaError
    import g2s_geo_ref as GR
    import test_g2s_kernels_vs_fp64 as G
    c = GR.get('shape', 7, 64)
    run = G._Run(c, 0)
    trace, _ = run.forward()
    flag = _flag_buffer(c.B)
    structs = run.net._structs

    def with_reach(*a, **k):
        cfg, lv, Kc = structs(*a, **k)
        cfg.reach_mode, cfg.reach_flag = 1, flag.data_ptr()
        return cfg, lv, Kc
    monkeypatch.setattr(run.net, '_structs', with_reach)
    before = run.trace.clone()
    with pytest.raises(HlaError, match='reach_mode'):
        run.net.lm_solve(*run.feats, run.K, run.hw, init_pose=c.p0, keep_normal_eq=True, **run.inv)
    with pytest.raises(HlaError, match='reach_mode'):
        run.backward(GR.coef_of(c))
    with pytest.raises(HlaError, match='reach_mode'):
        run.net.score_poses(*run.feats, run.K, run.hw, torch.zeros(1, 3), 0, **run.inv)
    torch.cuda.synchronize()
    assert flag.cpu().tolist() == [FLAG_FILL] * c.B and _bits(run.trace, before)
