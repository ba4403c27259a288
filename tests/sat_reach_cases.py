"""The cases of the trimmed satellite extractor (hla_vgg_forward_cols, first_col32 = c) that tests/test_sat_reach_gpu.py runs, and
what tests/test_sat_reach_cpu.py asserts about them without a GPU: the sum-of-squares slots per sample and the inv_norm gates."""

# (precision, feat16, B, H, W, c).  Widths 264 / 296 / 392 leave ragged last tiles at all three resolutions (W / 4 = 66 / 74 / 98
# against the 32-pixel tile); B = 9 runs the gate patterns; H = 128, B = 8 keeps the layers above CONV_SMALL_GRID: the 8-row kernels.
TRIM_CASES = [('bf16', True, 2, 64, 512, 1), ('bf16', True, 2, 64, 512, 2), ('bf16', True, 2, 64, 512, 3),
              ('bf16', True, 2, 64, 264, 1), ('bf16', True, 2, 64, 264, 2),
              ('bf16', True, 9, 64, 392, 1), ('bf16', True, 9, 64, 392, 3),
              ('fp16', True, 2, 64, 512, 3), ('fp16', True, 2, 64, 296, 2),
              ('fp32', False, 2, 64, 512, 2), ('fp32', False, 2, 64, 512, 3), ('fp32', False, 2, 64, 264, 1), ('fp32', False, 2, 64, 264, 2),
              ('bf16', False, 2, 64, 392, 2),
              ('bf16', True, 8, 128, 512, 3)]

# inv_norm against fp64: inv[l, b] * sqrt(sum of map^2 over the computed columns) = 1 to within
TOL_INV_FP32 = 1e-4          # fp32 maps
TOL_INV_FP16 = 2.0 ** -9     # fp16 maps: an element is rounded to 2^-11, a sum of squares to 2^-10; twice that
MAX_SLOTS = 64               # a lost or stale slot moves a sample's sum by about 1 / slots >= 1 / 64: above both gates


def tol_inv(feat16):
    return TOL_INV_FP16 if feat16 else TOL_INV_FP32


def slot_counts(H, W):
    """Sum-of-squares partials per sample of the three feature layers -- conv14 (H/4 x W/4, 256 channels in two blocks of 128),
    dec1.3 (H/4 x W/4), dec2.3 (H/2 x W/2) --: one per 8-row x 32-column tile and 128-channel block (csrc/vgg_layers.h, vgg_plan)."""
    tiles = lambda h, w: ((h + 7) // 8) * ((w + 31) // 32)
    return (tiles(H // 4, W // 4) * 2, tiles(H // 4, W // 4), tiles(H // 2, W // 2))


def strip_cols(c):
    """Columns of (x15, x18, x21) a forward with first_col32 = c never writes."""
    return tuple((16 * c) << l for l in range(3))
