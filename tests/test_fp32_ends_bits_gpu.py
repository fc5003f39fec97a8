"""The fp32 ends of csrc/small.hip give the bits they gave before their sliced / wide kernel copies were merged: every case of
tests/fp32_ends_cases.py (output head on both pixel forms and every slice count, input conv on both patch sizes, the 1x1 quant convs, the
conv weight packers, the two GELUs; return codes and refusal messages included) against the SHA-256 recorded from the parent build in
tests/golden/fp32_ends_parent_bits.json.

A case fails at its input digest first when this machine does not generate the recorded inputs.

The digests pin what one compiler emitted.  A compiler upgrade may legitimately contract the FMAs of these loops differently and move
them (the fp64-bounded tests of the same kernels -- test_kernels_gpu.py, test_wide_ends_kernels_gpu.py, test_kl_f16_kernels_gpu.py -- say
whether the new bits are still right).  Then, and only then, re-record them on the GPU with

    python tools/record_fp32_ends_bits.py
"""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

import fp32_ends_cases as FC  # noqa: E402


@pytest.fixture(scope='module')
def recorded(golden_dir):
    with open(os.path.join(golden_dir, 'fp32_ends_parent_bits.json')) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(FC.CASES)


@pytest.mark.parametrize('name', list(FC.CASES))
def test_bits_equal_the_parents(name, recorded):
    assert FC.input_digest(name) == recorded[name]['input_sha256'], 'the inputs differ from the recorded ones'
    assert FC.run_case(name) == recorded[name]['output_sha256'], f'recorded at {recorded[name]["commit"]}'
