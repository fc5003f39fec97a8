"""Sharpness control of tests/test_skip_fold_shapes_gpu.py, on the CPU with torch alone: at the operands those cases draw
(tests/skip_fold_cases.py: same generators, same seeds), the two terms a subtly wrong tail launch would lose are each worth more than four
times the max-abs bar the GPU cases hold, so neither can hide under it:

  lo pass        max |x_lo w_hi^T| -- what a three-pass tail that dropped its [lo | w_hi] pass would be off by
  last chunk     max |conv3x3(a[..., last 64 channels], w[:, last 64 channels])| -- what a conv whose chunk loop (or a split's range) ended
                 one 64-channel chunk early would be off by

The bar is the split-fp16 bar of tests/test_model_shapes_gpu.py, from skip_fold_cases.tol_split (the same formula, which the GPU module pins
against the original in every case), so that this control imports torch and nothing of the library.  If a case missed the factor 4 the
remedy would be its operand scale, never the bar."""
import pytest
import torch.nn.functional as F

import skip_fold_cases as SC
from skip_fold_cases import tol_split


CASES = SC.three_pass_cases()


def test_there_are_three_pass_cases_of_every_family():
    assert {s[0] for s, _, _, _ in CASES} >= {'32x32_b1', '64x64_b1', '32x32_b2', '16x16_b2_ca1280', '32x32_b2_sdv1'}


@pytest.mark.parametrize('shape,ca,Cout,Cin', CASES, ids=[f'{s[0]}-ca{ca}-n{co}-c{ci}' for s, ca, co, ci in CASES])
def test_a_dropped_lo_pass_or_conv_chunk_exceeds_the_bar_fourfold(shape, ca, Cout, Cin):
    name, B, H, W = shape
    a, w, x, ws, _, _ = SC.draw(name, B, H, W, ca, Cout, Cin, 3)
    bar = tol_split(9 * ca + Cin)
    x_hi = x.half()
    x_lo = (x - x_hi.float()).half()                  # sdmi_k_cast_f16's low half
    lo_term = float((x_lo.double() @ ws.half().double().t()).abs().max())
    a_last = a.half().double().reshape(B, H, W, ca)[..., ca - 64:].permute(0, 3, 1, 2)
    chunk = float(F.conv2d(a_last, w[:, ca - 64:].half().double(), None, padding=1).abs().max())
    print(f'[skip fold control {name} ca{ca} n{Cout} c{Cin}] bar {bar:.2e}: max |x_lo w_hi^T| = {lo_term:.2e} ({lo_term / bar:.0f} x), '
          f'max |last conv chunk| = {chunk:.2e} ({chunk / bar:.0f} x)')
    assert lo_term > 4 * bar
    assert chunk > 4 * bar
