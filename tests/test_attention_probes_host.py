"""The attention probes (tests/attn_probes.py) checked on the CPU, before a GPU sees them:

  * the plain-torch restatement of the kernels' loop stays inside the per-weight tolerance with a factor in hand (err / tol <= 0.6) in every
    score regime x V coding, with one key group and with two;
  * each planted defect of that loop exceeds the tolerance by >= 50x in the regime / coding built to catch it -- and the two defects that
    random inputs at long key counts let through (no tail mask under diffuse scores, keys permuted inside a tile under the segment coding)
    do pass there, which is why those regimes and codings exist;
  * every case of tests/test_attention_probes_gpu.py is live: each query row has an output on which a weight, not fp16's subnormal grid, is
    measured, and at least 10 % of the non-empty outputs are such."""
import pytest
import torch

import attn_probes as A

BH, NQ = 2, 48
ONE_GROUP = [1000, 337, 4031]
TWO_GROUPS = [2176, 4096]


def _ratios(d, nkv, kvs, ones, mutant, regimes=A.REGIMES):
    """{(regime, coding): worst err / tol} of the emulator (coding names without their window offset)"""
    out = {}
    for regime in regimes:
        q, k = A.make_qk(regime, BH, NQ, nkv, d, 5 + nkv)
        P, _ = A.softmax_ref(q, k, d ** -0.5)
        for name, col in A.codings(regime, nkv, d):
            got = A.emulate(q, k, A.dense_v(col, BH, d), d ** -0.5, kvs=kvs, ones=ones, mutant=mutant).double()
            j = A.judge(got, P, col, A.R_MIXED)
            assert j['zeros_exact'] or mutant is not None
            out[(regime, name.split('@')[0])] = j['worst']
    return out


def test_coded_sum_is_p_times_v():
    """the reference's per-column sum equals P @ V with the dense indicator matrix, (batch, head) rotation included"""
    d, nkv = 40, 203
    q, k = A.make_qk('rising', 4, 33, nkv, d, 1)
    P, _ = A.softmax_ref(q, k, d ** -0.5)
    for regime in ('diffuse', 'rising'):
        for name, col in A.codings(regime, nkv, d):
            v = A.dense_v(col, 4, d, torch.float64)
            assert set(v.unique().tolist()) <= {0.0, 1.0} and bool((v.sum(-1) <= 1).all())
            assert torch.allclose(A.coded(P, col, d), P @ v, rtol=0, atol=1e-15), name
            assert torch.equal(A.key_counts(col, 4, 33, d), v.sum(1, keepdim=True).expand(4, 33, d)), name


def test_regimes_shift_the_scores():
    """dimension 0 carries b_j: the fp64 scores of a regime differ from b_j by what N(0, 1) in the other dimensions gives"""
    d, nkv = 64, 130
    for regime in A.REGIMES[1:]:
        q, k = A.make_qk(regime, 2, 5, nkv, d, 3)
        assert torch.equal(q[..., 0], torch.full((2, 5), 8.0, dtype=q.dtype))
        s0 = q[..., :1].double() @ k[..., :1].double().transpose(1, 2) * d ** -0.5
        assert float((s0 - A.shift(regime, nkv)).abs().max()) <= 20 * 2.0 ** -11
    qa, ka = A.make_qk('diffuse', 2, 5, nkv, d, 3)
    assert not torch.equal(qa[0], qa[1]) and not torch.equal(ka[0], ka[1])
    qs, _ = A.make_qk('rising', 2, 5, nkv, d, 3, split=True)
    hi, lo = A.split16(qs)
    assert qs.dtype == torch.float32 and bool((lo[..., 0] == 0).all()) and bool((lo[..., 1:] != 0).any())


@pytest.mark.parametrize('d,ones', [(40, True), (64, False)])
@pytest.mark.parametrize('nkv', ONE_GROUP)
def test_emulator_one_group_inside_the_bar(d, ones, nkv):
    r = _ratios(d, nkv, 1, ones, None)
    print(f'[probe emulator d{d} nkv{nkv}] worst err / tol {max(r.values()):.3f}', flush=True)
    assert max(r.values()) <= 0.6, r


@pytest.mark.parametrize('nkv', TWO_GROUPS)
def test_emulator_two_groups_inside_the_bar(nkv):
    r = _ratios(40, nkv, 2, True, None)
    print(f'[probe emulator d40 nkv{nkv} two key groups] worst err / tol {max(r.values()):.3f}', flush=True)
    assert max(r.values()) <= 0.6, r


@pytest.mark.parametrize('nkv', ONE_GROUP)
def test_control_no_tail_mask(nkv):
    """a phantom key (score 0) takes the whole softmax when every true score is near -20"""
    r = _ratios(40, nkv, 1, True, 'nomask', ('diffuse', 'negative'))
    for coding in ('segments', 'stride', 'window0', 'window_end', 'window_seam'):
        assert r[('negative', coding)] >= 50, r
    if nkv == 4031:      # 4031 keys at random scores: one phantom key in 4032 is under the bar
        assert max(v for (regime, _), v in r.items() if regime == 'diffuse') < 1.0, r


@pytest.mark.parametrize('nkv,kvs', [(n, 1) for n in ONE_GROUP] + [(n, 2) for n in TWO_GROUPS])
def test_control_dropped_tile(nkv, kvs):
    r = _ratios(40, nkv, kvs, True, 'droptile')
    for regime in A.REGIMES:
        if regime != 'falling':      # (there the last tile's weights are e^-20 of the first's)
            assert r[(regime, 'segments')] >= 50, r


@pytest.mark.parametrize('nkv,kvs', [(n, 1) for n in ONE_GROUP] + [(n, 2) for n in TWO_GROUPS])
def test_control_keys_permuted_inside_a_tile(nkv, kvs):
    r = _ratios(40, nkv, kvs, True, 'perm')
    for regime in A.REGIMES:
        assert r[(regime, 'stride')] >= 50, r
    if nkv == 4096:      # 102.4 keys per segment: keys 4 .. 11 of a tile never straddle two segments
        assert max(v for (_, coding), v in r.items() if coding == 'segments') < 1.0, r


@pytest.mark.parametrize('mutant', ['merge_swapped', 'merge_unit', 'merge_l'])
@pytest.mark.parametrize('nkv', TWO_GROUPS)
def test_control_key_group_merge(nkv, mutant):
    r = _ratios(40, nkv, 2, True, mutant, ('first_half', 'second_half'))
    assert min(r.values()) >= 50, r


@pytest.mark.parametrize('family,d', [('split16', 160), ('wide_split16', 1024)])
def test_split_score_rounding_term(family, d):
    """The extra relative term of the split-fp16 kernels (attn_probes.score_rounding) is what fp32 accumulation of a score of magnitude
    20 sqrt(d) costs.  A restatement of that accumulation alone, everything else exact and no fp16 anywhere, uses 0.7 .. 1.15 of the bar at
    R = 1e-5 alone under `negative` and `rising` -- the fp16 floors of P_lo and out_lo, which the kernels have on top, take up to 0.5 of
    it (the emulator tests above; `diffuse` and `falling` on the GPU) -- and 0.6 at most with the term; under `diffuse` it uses 0.07."""
    nq, nkv = 130, 203
    scale = d ** -0.5
    for regime in ('diffuse', 'negative', 'rising'):
        q, k = A.make_qk(regime, 2, nq, nkv, d, 11, split=True)
        (qh, ql), (kh, kl) = A.split16(q), A.split16(k)
        P, smax = A.softmax_ref(qh.double() + ql.double(), kh.double() + kl.double(), scale)
        W = A.emulate_split_weights(q, k, scale, family)
        _, col = A.codings(regime, nkv, d)[1]                     # stride: at most two keys per column
        got = A.coded(W, col, d)
        bare = A.judge(got, P, col, A.R_SPLIT)['worst']
        with_term = A.judge(got, P, col, A.R_SPLIT, extra=A.score_rounding(family, d, scale, smax))['worst']
        print(f'[probe split score rounding {family} d{d} {regime}] err / tol {bare:.3f} at R alone, {with_term:.3f} with the term', flush=True)
        assert with_term <= 0.6
        assert bare <= 0.1 if regime == 'diffuse' else bare >= 0.7


def _liveness_params():
    fams = {}
    for fam, d, nq, nkv in A.gpu_cases():
        fams.setdefault((fam, d), []).append((nq, nkv))
    return [pytest.param(fam, d, shapes, id=f'{fam}-d{d}') for (fam, d), shapes in fams.items()]


@pytest.mark.parametrize('family,d,shapes', _liveness_params())
def test_gpu_cases_are_live(family, d, shapes):
    causal = family == 'causal'
    split = family in ('split16', 'wide_split16')
    worst = 1.0
    for nq, nkv in shapes:
        B, heads = A.batch_heads(family, nq, nkv)
        bh = 1 if nq >= 1030 else B * heads              # (the largest references: one (batch, head) pair is enough here)
        for regime in A.REGIMES:
            q, k = A.make_qk(regime, bh, nq, nkv, d, A.case_seed(family, d, nq, nkv, regime), split)
            if split:
                (qh, ql), (kh, kl) = A.split16(q), A.split16(k)
                q, k = qh.double() + ql.double(), kh.double() + kl.double()
            P, _ = A.softmax_ref(q, k, d ** -0.5, causal)
            for name, col in A.codings(regime, nkv, d):
                share, rows = A.liveness(P, col, d, causal)
                assert rows, (nq, nkv, regime, name)
                if nkv >= 8:
                    assert share >= 0.10, (nq, nkv, regime, name, share)
                    worst = min(worst, share)
    print(f'[probe liveness {family} d{d}] smallest live share {worst:.3f}', flush=True)
