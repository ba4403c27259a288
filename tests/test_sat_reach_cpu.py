"""args.sat_reach_crop on the host: which satellite-map columns the LM loop can read while the pose stays inside its configured
range (``_s2gp.sat_reach``), and how far left every extractor layer therefore has to reach (``_s2gp.reach_walk``,
``first_col32_of_reach``, ``VGG.promised_cols``).  No GPU.

* The reach against a brute-force fp64 scan through ``oracle.ref_cpu.kitti_pose_to_uv`` (the reference's own projection): the same
  smallest column per level, c = 1 for KITTI 512 / 256 x 1024, c = 2 for 1024 / 512 x 2048, c = 0 once the range reaches column 0.
* The walk against the CPU oracle's VGGUnet on a 64 x 256 image: the columns ``promised_cols(1)`` promises depend on no image
  column left of 128 - 2 (conv2 at column 128 reads conv0 at 127, conv0 reads the image at 126), and do depend on column 126.
"""
import itertools

import numpy as np
import torch

from oracle import ref_cpu as O
from highlyaccurate_amd import _s2gp
from highlyaccurate_amd.VGG import promised_cols
from highlyaccurate_amd.models_kitti import LM_S2GP
import sat_reach_cases as SC


def _brute_force_reach(A, grd_hw, lat, lon, rot, n=5):
    """floor(min u) per level over the lattice, through the reference's projection in fp64."""
    args = O.default_args(shift_range_lat=lat, shift_range_lon=lon, rotation_range=rot)
    axis = np.linspace(-1.0, 1.0, n)
    poses = torch.tensor(list(itertools.product(axis, axis, axis)), dtype=torch.float64)
    out = []
    for l in range(3):
        h, w, a = grd_hw[0] >> (3 - l), grd_hw[1] >> (3 - l), A >> (3 - l)
        xyz, mask = O.ground_points(_s2gp.KITTI_K, h, w, 256, 1024)
        xyz, mask = xyz[:, h // 2:], mask[0, h // 2:].bool()
        best = float(a)
        for k0 in range(0, poses.shape[0], 25):
            p = poses[k0:k0 + 25]
            uv, _ = O.kitti_pose_to_uv(args, xyz, p[:, 0:1], p[:, 1:2], p[:, 2:3], a, require_jac=False)
            u, v = uv[..., 0], uv[..., 1]
            ok = (u >= 0) & (u <= a - 1) & (v >= 0) & (v <= a - 1) & mask[None]
            if ok.any():
                best = min(best, float(torch.floor(u[ok].min())))
        out.append(int(best))
    return out


def _model_reach(A, grd_hw, **kw):
    net = LM_S2GP(O.default_args(**kw))
    tables = net.xyz_tables(grd_hw[0], grd_hw[1], 'cpu')[:3]
    mpp = [O.meter_per_pixel() * 512 / (A >> (3 - l)) for l in range(3)]
    a = net.args
    cols = _s2gp.sat_reach(tables, [A >> (3 - l) for l in range(3)], mpp, a.shift_range_lat, a.shift_range_lon, a.rotation_range)
    return cols, net.sat_first_col32(A, *grd_hw)


def test_reach_matches_brute_force_kitti_default():
    cols, c = _model_reach(512, (256, 1024))
    assert cols == _brute_force_reach(512, (256, 1024), 20.0, 20.0, 10.0)
    assert cols == [20, 41, 81]          # floor of 20.6 / 41.1 / 81.9
    assert c == 1
    assert all(p <= q for p, q in zip(promised_cols(c), cols))


def test_reach_at_twice_the_size():
    cols, c = _model_reach(1024, (512, 2048))
    assert cols == _brute_force_reach(1024, (512, 2048), 20.0, 20.0, 10.0)
    assert c == _s2gp.first_col32_of_reach(cols, 1024) == 2
    assert all(p <= q for p, q in zip(promised_cols(c), cols))


def test_wide_range_reaches_column_zero():
    cols, c = _model_reach(512, (256, 1024), shift_range_lat=50.0, shift_range_lon=50.0)
    assert cols == _brute_force_reach(512, (256, 1024), 50.0, 50.0, 10.0)
    assert cols[0] == 0 and c == 0
    assert promised_cols(0) == (0, 0, 0)


def test_trim_is_off_outside_its_scope():
    from highlyaccurate_amd.models_ford import LM_S2GP_Ford
    assert LM_S2GP(O.default_args(proj='polar')).sat_first_col32(512, 256, 1024) == 0
    assert LM_S2GP_Ford(O.default_args()).sat_first_col32(512, 256, 1024) == 0
    assert LM_S2GP(O.default_args(level=4)).sat_first_col32(512, 256, 1024) == 0


def test_walk_table_of_the_default_reach():
    need = _s2gp.reach_walk(20, 41, 81)
    assert {k: need[k] for k in ('x18', 'x15', 'conv10', 'x8', 'conv5', 'x3', 'conv2')} == \
        {'x18': 39, 'x15': 18, 'conv10': 34, 'x8': 33, 'conv5': 65, 'x3': 64, 'conv2': 128}


def test_walk_and_promise_agree():
    """The backward walk (which c do the columns the loop reads allow) and the forward rule (which columns does a forward started
    at c leave exact) describe one dependency cone: c is allowed exactly when its promised columns are not right of the reach."""
    rs = np.random.RandomState(0)
    for _ in range(4000):
        p = (int(rs.randint(0, 64)), int(rs.randint(0, 128)), int(rs.randint(0, 256)))
        c = _s2gp.first_col32_of_reach(p, 1 << 20)
        assert all(q <= r for q, r in zip(promised_cols(c), p)), (p, c)
        assert any(q > r for q, r in zip(promised_cols(c + 1), p)), (p, c)


def test_promised_columns_against_the_oracle_extractor():
    torch.manual_seed(0)
    net = O.VGGUnet(3).double()
    net.load_state_dict({k: v.double() for k, v in O.synth_vgg_state(np.random.RandomState(3), bias_scale=0.05).items()})
    x = torch.rand(1, 3, 64, 256, dtype=torch.float64)
    first_image_col = 128 - 2
    cols = promised_cols(1)
    with torch.no_grad():
        ref = net.raw_maps(x)[:3]
        y = x.clone()
        y[..., :first_image_col] = torch.rand(1, 3, 64, first_image_col, dtype=torch.float64)
        got = net.raw_maps(y)[:3]
        z = x.clone()
        z[..., :first_image_col + 1] = torch.rand(1, 3, 64, first_image_col + 1, dtype=torch.float64)
        moved = net.raw_maps(z)[:3]
    for l in range(3):
        assert torch.equal(got[l][..., cols[l]:], ref[l][..., cols[l]:]), l
        assert not torch.equal(got[l][..., cols[l] - 1:], ref[l][..., cols[l] - 1:]), l      # the promise is tight
        assert not torch.equal(moved[l][..., cols[l]:], ref[l][..., cols[l]:]), l


def test_trim_cases_of_the_gpu_suite():
    """tests/test_sat_reach_gpu.py's cases: legal trims, c = 1, 2 and 3, ragged last tiles at every resolution, at most 64
    sum-of-squares slots per sample and level -- so that a lost or stale slot (about 1 / slots of the sum) cannot hide inside
    either inv_norm gate --, and where the promised columns lie beyond the map."""
    assert {c for *_, c in SC.TRIM_CASES} == {1, 2, 3}
    assert 1.0 / SC.MAX_SLOTS > 4 * SC.TOL_INV_FP16 > SC.TOL_INV_FP32
    assert SC.TOL_INV_FP16 == 2 * 2.0 ** -10
    vacuous = set()
    for precision, feat16, B, H, W, c in SC.TRIM_CASES:
        assert 128 * c < W and W % 8 == 0 and H % 8 == 0, (W, c)
        assert not feat16 or precision in ('bf16', 'fp16')
        slots = SC.slot_counts(H, W)
        assert all(1 <= n <= SC.MAX_SLOTS for n in slots), (H, W, slots)
        for l, (strip, first) in enumerate(zip(SC.strip_cols(c), promised_cols(c))):
            width = W >> (3 - l)
            assert strip < width and strip < first                 # something is computed, and its first columns are not promised
            if first >= width:
                vacuous.add((W, c, l))
    assert vacuous == {(W, c, l) for W, c in ((264, 2), (392, 3)) for l in range(3)}      # (392 / 8 = 49 < 16 * 3 + 2)
    for W in (264, 296, 392):
        assert all((W >> s) % 32 for s in (1, 2, 3)), W             # ragged last tile at H/2, H/4 and on the pooled H/8 map
    assert max(SC.slot_counts(128, 512)) == SC.MAX_SLOTS
