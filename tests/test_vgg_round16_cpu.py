"""CPU checks of ``vgg_round16``, the rounding-aware fp64 emulation of the bf16 / fp16 VGG forward that
``test_vgg_kernels_vs_fp64.py`` gates the GPU against."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
import vgg_round16 as R16


def _case(B, H, W, seed):
    rs = np.random.RandomState(seed)
    sd = O.synth_vgg_state(rs, bias_scale=0.05)
    x = torch.from_numpy(rs.random_sample((B, 3, H, W)).astype(np.float32))
    return sd, x


@pytest.mark.parametrize('level', [3, 4])
def test_rounding_off_is_the_oracle(level):
    """With rounding off the emulation is O.VGGUnet in fp64, maps and confidence maps alike."""
    sd, x = _case(2, 16, 48, 5)
    onet = O.VGGUnet(level)
    onet.load_state_dict(sd)
    with torch.no_grad():
        f64, c64 = onet.double()(x.double())
        f, c, _ = R16.forward(sd, x, level)
    assert len(f) == len(f64) == level and len(c) == len(c64) == level
    for a, b in zip(f + c, f64 + c64):
        assert a.dtype == torch.float64 and a.shape == b.shape
        assert (a - b).abs().max() <= 1e-15 * b.abs().max(), float((a - b).abs().max())


# the small cases of the GPU module's shape matrix, with its seeds: (B, H, W, level)
_GPU_CASES = [(1, 8, 8, 3), (1, 8, 8, 4), (1, 16, 296, 4)]


@pytest.mark.parametrize('name,dtype', list(R16.DTYPES.items()))
def test_gate_regimes_and_teeth(name, dtype):
    """``vgg_round16.gate`` on the GPU module's small cases.  Teeth: on every flip-free map (no rounding flip between the fp32-
    and fp64-accumulated emulations) the modelled rounding relL2(emu64, exact) is >= 10 x the gate, and both types have such
    maps.  On flip-free and partial maps an unrounded forward (the exact fp64 maps) fails the gate.  Saturated maps -- one flip
    cascading through the following layers -- are reported: there the gate is floored at half the rounding error."""
    seen = {'flip-free': 0, 'partial': 0, 'saturated': 0}
    for B, H, W, level in _GPU_CASES:
        sd, x = _case(B, H, W, 7919 * H + 31 * W + 3 * B + level)
        onet = O.VGGUnet(level)
        onet.load_state_dict(sd)
        with torch.no_grad():
            f64, c64 = onet.double()(x.double())
            e64 = R16.forward(sd, x, level, dtype)
            e32 = R16.forward(sd, x, level, dtype, torch.float32)
        for i, (a, b, ex) in enumerate(zip(e64[0] + e64[1], e32[0] + e32[1], f64 + c64)):
            g = R16.gate(a, b, ex)
            seen[g['regime']] += 1
            print(f"{name} {(B, H, W)} L{level} map {i} [{g['regime']}]: rounding {g['rnd_l2']:.2e}, noise {g['noise_l2']:.2e}, "
                  f"gate {g['l2']:.2e}")
            assert g['rnd_l2'] > 1e-5, (i, g)      # the rounding is on at all
            if g['regime'] == 'flip-free':
                assert g['rnd_l2'] >= 10 * g['l2'], (i, g)
            if g['regime'] != 'saturated':
                assert R16.rel_l2(ex, a) > g['l2'], (i, g)
    print(name, seen)
    assert seen['flip-free'] >= 3, seen


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_every_rounding_class_is_visible(dtype):
    """Operand rounding is idempotent (already-rounded weights and image give the same maps bit for bit), and the stored
    activations' rounding alone moves the maps by far more than fp64 noise: it is not a no-op a missing kernel rounding
    could hide behind."""
    sd, x = _case(1, 16, 48, 11)
    with torch.no_grad():
        base = R16.forward(sd, x, 3, dtype)[0]
        sd_r = {k: v.to(dtype).float() if k.endswith('weight') and not k.startswith('conf') else v for k, v in sd.items()}
        x_r = x.to(dtype).float()
        # rounded weights / input given as already-rounded values: re-rounding is the identity, the maps do not move
        same = R16.forward(sd_r, x_r, 3, dtype)[0]
        for a, b in zip(base, same):
            assert (a - b).abs().max() <= 1e-15 * b.abs().max()
        # with rounding off but the rounded weights and image fed in, only the activations' rounding is missing: visible
        part = R16.forward(sd_r, x_r, 3, None)[0]
    for a, b in zip(base, part):
        assert R16.rel_l2(b, a) > 1e-4
