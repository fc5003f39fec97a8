"""The one-pass attention kernel's cases and routing, checked on the CPU before a GPU sees them:

  * every case of tests/test_attn_small_gpu.py is live under the attention probes (tests/attn_probes.py): each query row has an output on
    which a softmax weight, not fp16's subnormal grid, is measured, and at least 10 % of the non-empty outputs are such (with fewer than 8
    keys there are too few columns for a share: the rule of test_attention_probes_host.py).  No case is skipped: one that is not live fails;
  * the routing predicate sdmi_attn_small_takes (csrc/attn.hip: the table behind SDMI_ATTN_SMALL): knob 0 never takes the one-pass kernel,
    knob 2 takes it exactly where it is instantiated (d = 80 / 160, non-causal, at most 256 keys), and the default rule is the measured
    table of profiles/attn_small_ab.txt -- a subset of knob 2, with the waves per workgroup that were measured."""
import pytest

import attn_probes as A
import attn_small_cases as S


@pytest.mark.parametrize('d', S.D)
def test_gpu_cases_are_live(d):
    worst = 1.0
    for dd, nq, nkv in S.cases():
        if dd != d:
            continue
        for regime in A.REGIMES:
            q, k = A.make_qk(regime, S.B * S.HEADS, nq, nkv, d, S.seed(d, nq, nkv, regime))
            P, _ = A.softmax_ref(q, k, d ** -0.5)
            for name, col in A.codings(regime, nkv, d):
                share, rows = A.liveness(P, col, d)
                assert rows, (nq, nkv, regime, name)
                if nkv >= 8:
                    assert share >= 0.10, (nq, nkv, regime, name, share)
                    worst = min(worst, share)
    print(f'[probe liveness small d{d}] smallest live share {worst:.3f}', flush=True)


def _takes(d, nq, nkv, causal, knob):
    from stable_diffusion_amd import _lib
    return _lib.load().sdmi_attn_small_takes(d, nq, nkv, causal, knob)


def test_knob_0_and_2():
    for d, nq, nkv in S.cases():
        assert _takes(d, nq, nkv, 0, 0) == 0
        assert _takes(d, nq, nkv, 0, 2) in (1, 2, 4)
        assert _takes(d, nq, nkv, 1, 2) == 0                       # causal: never
    for d in S.D:
        assert _takes(d, 256, S.NKV_LIMIT + 1, 0, 2) == 0          # one key too many: the ring kernel
        assert _takes(d, 256, 4096, 0, 2) == 0
    for d in (24, 32, 40, 48, 64, 96, 128, 192):                   # head dims without an instantiation
        assert _takes(d, 256, 77, 0, 2) == 0 and _takes(d, 256, 77, 0, 1) == 0


def test_default_rule_is_the_measured_table():
    """the launch classes of the SD-v1 UNet below 64 x 64, and the rule's edges"""
    # 64 x 64 latents.  16 x 16 level (d = 160): cross-attention over 77 keys and self-attention over 256 -- one wave per workgroup
    assert _takes(160, 256, 77, 0, 1) == 1
    assert _takes(160, 256, 256, 0, 1) == 1
    # 8 x 8 mid block (d = 160, 64 queries): self-attention over 64 keys, cross-attention over 77
    assert _takes(160, 64, 64, 0, 1) == 1
    assert _takes(160, 64, 77, 0, 1) == 1
    # 32 x 32 level (d = 80): cross-attention over 77 keys, two waves per workgroup; its 1024-key self-attention stays on the ring kernel
    assert _takes(80, 1024, 77, 0, 1) == 2
    assert _takes(80, 1024, 1024, 0, 1) == 0
    # 32 x 32 latents: the d = 80 level has 256 queries
    assert _takes(80, 256, 77, 0, 1) == 1
    assert _takes(80, 256, 256, 0, 1) == 1
    # classes that were not measured stay on the ring kernel: 96 x 96 latents (576 / 2304 queries), more than 1024 queries
    assert _takes(160, 576, 77, 0, 1) == 0 and _takes(160, 576, 77, 0, 2) > 0
    assert _takes(80, 2304, 77, 0, 1) == 0 and _takes(80, 2304, 77, 0, 2) > 0
    assert _takes(80, 1024, 256, 0, 1) == 0
    # the default rule never goes where knob 2 does not
    for d in S.D:
        for nq in (1, 32, 33, 64, 256, 257, 1024, 1025, 4096):
            for nkv in (1, 64, 77, 128, 129, 256, 257):
                if _takes(d, nq, nkv, 0, 1):
                    assert _takes(d, nq, nkv, 0, 2) == _takes(d, nq, nkv, 0, 1)
