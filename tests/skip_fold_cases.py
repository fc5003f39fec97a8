"""The operands and the case tables of the skip-convolution fold's kernel tests (conv3halo.hip TAIL; sdmi_k_igemm_tail), shared by
tests/test_skip_fold_gpu.py, tests/test_skip_fold_shapes_gpu.py and the CPU control tests/test_skip_fold_shapes_host.py.  torch alone: what is
drawn here on the CPU is what the GPU tests copy to the device, so the control judges the very numbers the kernels see.

Operand scales (the ones the split-fp16 bar of tests/test_model_shapes_gpu.py, _tol_split, assumes): conv activations fp16 N(0, 1) against
weights / sqrt(9 CA); tail activations fp32 N(0, 4) against weights / sqrt(Cin)."""
import math

import torch

from model_shapes import HALO_TILES  # noqa: F401  (tests/model_shapes.py imports nothing but json and os at module level)

HALO_BM = {14: 256, 15: 256, 16: 128, 17: 128}


def tol_split(Kd):
    """the project's split-fp16 max-abs bar, tests/test_model_shapes_gpu.py _tol_split (derivation there), written out so that the CPU control
    needs torch alone; tests/test_skip_fold_shapes_gpu.py asserts in every case that the two are the same number"""
    return 3e-5 * max(1.0, math.sqrt(Kd / 1920.0))


def seed(name, Cout, Cin, passes):
    return 1000 * Cout + 10 * Cin + passes + sum(map(ord, name))


def draw(name, B, H, W, ca, Cout, Cin, passes):
    """the fp32 draws of one case, on the CPU, in a fixed order: conv activation a [M, ca] (the kernels read a.half()), conv weight w
    [Cout, ca, 3, 3], tail activation x [M, Cin], tail weight ws [Cout, Cin], the two biases"""
    g = torch.Generator().manual_seed(seed(name, Cout, Cin, passes))
    M = B * H * W
    a = torch.randn((M, ca), generator=g)
    w = torch.randn((Cout, ca, 3, 3), generator=g) / math.sqrt(9 * ca)
    x = 2.0 * torch.randn((M, Cin), generator=g)
    ws = torch.randn((Cout, Cin), generator=g) / math.sqrt(Cin)
    b2, bs = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    return a, w, x, ws, b2, bs


# ---- tests/test_skip_fold_shapes_gpu.py: (name, B, H, W), CA, tile, Cout, tail Cin, passes, the (tile, split-K) requests ----------------
# Widths: on a 32-wide map a 128- / 256-row tile is 4 / 8 image rows, on a 64-wide one 2 / 4: most tiles are interior (no image border in the
# halo), unlike every tile of an 8- or 16-wide map.  32x32 at B = 2 on tile 15: the sample boundary is a tile boundary (tile 4 of 8).
WIDTH_SHAPES = [('32x32_b1', 1, 32, 32), ('64x64_b1', 1, 64, 64)]
WIDTHS = [(s, 384, t, co, 192, ps, (1, 3)) for s in WIDTH_SHAPES for t in HALO_TILES for co in (64, 320) for ps in (1, 3)]
WIDTHS.append((('32x32_b2', 2, 32, 32), 384, 15, 320, 192, 3, (1, 3)))
# Splits: CA = 1280 is 20 chunks, which 4, 5 and 10 divide (the committed table's halo rows use them: 512 1280 11520 -> tile 15, split 10).
# Tail 640 x 3 passes = 30 k-tiles, dealt 8 | 7, 6 and 3 per split; tail 64 x 1 pass = one k-tile, every split but one holds an empty range.
SPLITS = [(('16x16_b2_ca1280', 2, 16, 16), 1280, t, 320, ci, ps, (4, 5, 10)) for t in (15, 16) for ci, ps in ((640, 3), (64, 1))]
# Length and width: SD v1's 8 x 8 and 16 x 16 sites (Cout = 1280: 10 / 20 N tiles; one-pass tail of 2560 channels = 40 k-tiles), forced to the
# committed table's choice and as launched (tile -1, split-K 0: the table decides); and output_blocks.6 at 32 x 32, the longest tail (1920 x 3
# passes = 90 k-tiles), as launched.
SITES = [(('8x8_b2_sdv1', 2, 8, 8), 1280, 1280, 2560, 1, ((16, 10), (-1, 0))),
         (('16x16_b2_sdv1', 2, 16, 16), 1280, 1280, 2560, 1, ((15, 10), (-1, 0))),
         (('32x32_b2_sdv1', 2, 32, 32), 640, 640, 1920, 3, ((-1, 0),))]


def three_pass_cases():
    """(shape, CA, Cout, Cin) of every three-pass case above, once each"""
    seen, out = set(), []
    for s, ca, _, co, ci, ps, _ in WIDTHS + SPLITS:
        if ps == 3 and (s, ca, co, ci) not in seen:
            seen.add((s, ca, co, ci))
            out.append((s, ca, co, ci))
    out += [(s, ca, co, ci) for s, ca, co, ci, ps, _ in SITES if ps == 3]
    return out
