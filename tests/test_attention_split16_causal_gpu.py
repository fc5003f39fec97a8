"""The causal split-fp16 attention kernel alone (attn_split16_kernel<D, 4, CAUSAL = true> through sdmi_k_attention_split16_causal: the
self-attention of the full-precision CLIP text encoder) against an fp64 softmax(Q K^T scale + causal mask) V on the CPU.

Shapes: d = 32 / 64 / 128 (every instantiation), B = 2, heads = 2 (BH = 4), n = 1, 8, 31, 32, 33, 63, 64, 65, 77 -- one key, one partial
wave, the wave boundary (32 queries per wave), the key-tile boundary (64 keys per tile; at 65 and 77 the second tile is all-masked for the
first two waves), n_pad = n and n_pad > n, CLIP's own length.  One workgroup of four waves covers every query of a (batch, head) pair, so
waves without queries run both barriers of every key tile.

Every operand and both outputs live in guarded buffers (tests/guard.py): a write past out / out_lo fails the guard check, a read past an
operand brings NaN into the result.  Operands are fp32 normals split into hi / lo, so the low halves carry 11 more bits of every value;
the reference sees hi + lo.  The V^T pad columns n .. n_pad are zero (the contract in include/sdmi.h).

Per case:
  * the result (hi + lo) against fp64, relative to max|O|, at most TOL; and TOL is never above a tenth of the error that the mixed
    kernel (sdmi_k_attention_causal on the fp16 roundings of the same operands) makes against the same reference, computed here;
  * the softmax weights per element through probe V (tests/attn_probes.py): windows of min(d, 64) consecutive keys, one launch per window
    (a 64-key range at d >= 64, two halves of it at d = 32), key j of the window alone in its column -- every weight is held to the
    split-fp16 bar of test_attention_probes_gpu.py (R = 1e-5 + the score-rounding term + the fp16 floors), and every weight above the
    diagonal must be exactly 0.0 (attn_probes.judge: an output whose column holds no visible key);
  * changing key / value j (hi and lo) leaves the output rows of the queries < j bit-identical and changes row j.

Measured on an MI355X (profiles/full_precision_text_encoder.txt): max-abs / max|O| 0 .. 3.00e-7 over the 27 cases (worst d = 128, n = 32),
the mixed kernel 3.0e-4 .. 6.2e-4 on the same inputs (1500 .. 5300 times more); probe weights at most 0.50 of their bar.  The 79 tests
take 3 s together.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import _lib  # noqa: E402

import attn_probes as A  # noqa: E402
import guard  # noqa: E402
import kernels as K  # noqa: E402

DEV = 'cuda'
B, HEADS = 2, 2
BH = B * HEADS
D = [32, 64, 128]
N = [1, 8, 31, 32, 33, 63, 64, 65, 77]
# worst max-abs / max|O| of hi + lo against fp64 over the 27 cases, MI355X (printed per case by the test)
MEASURED = 3.0e-7
TOL = 1.25 * MEASURED


def _run(pool, ops, n, d, scale):
    """ops: q, q_lo, k, k_lo, vt, vt_lo already in guarded buffers -> (out, out_lo) [B, n, HEADS * d] in guarded buffers of `pool`"""
    out = pool.new('out', (B, n, HEADS * d), torch.float16)
    out_lo = pool.new('out_lo', (B, n, HEADS * d), torch.float16)
    _lib.check(_lib.load().sdmi_k_attention_split16_causal(*[o.data_ptr() for o in ops], out.data_ptr(), out_lo.data_ptr(), BH, HEADS, n,
                                                           ops[4].shape[2], d, float(scale), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out, out_lo


def _put_split(pool, name, x):
    hi, lo = A.split16(x)
    return pool.put(name, hi.to(DEV)), pool.put(name + '_lo', lo.to(DEV))


def _ref(q, k, v, scale):
    """fp64 causal attention, [BH, n, d]"""
    P, _ = A.softmax_ref(q, k, scale, causal=True)
    return P @ v.double()


@pytest.mark.parametrize('n', N)
@pytest.mark.parametrize('d', D)
def test_result_against_fp64_and_the_mixed_kernel(d, n):
    g = torch.Generator().manual_seed(7000 + 131 * d + n)
    scale = d ** -0.5
    q, k, v = (torch.randn((BH, n, d), generator=g) for _ in range(3))
    vt = A.vt_padded(v, 0.0)
    pool = guard.Pool(DEV)
    ops = [*_put_split(pool, 'q', q), *_put_split(pool, 'k', k), *_put_split(pool, 'vt', vt)]
    assert all(bool((o[1].float().abs() > 0).any()) for o in (ops[0:2], ops[2:4], ops[4:6]))        # the low halves matter
    out, out_lo = _run(pool, ops, n, d, scale)
    pool.check(f'causal split16 d{d} n{n}')
    # the reference sees what the kernel receives: hi + lo
    qs, ks, vs = (ops[i].double().cpu() + ops[i + 1].double().cpu() for i in (0, 2, 4))
    ref = _ref(qs, ks, vs[:, :, :n].transpose(1, 2), scale)
    got = A.heads_first(out.double().cpu() + out_lo.double().cpu(), HEADS)
    rel = float((got - ref).abs().max() / ref.abs().max())
    # the mixed kernel on the fp16 roundings (the hi halves) of the same operands, against the same reference
    mixed = K.attention_causal(ops[0], ops[2], ops[4], HEADS, scale)
    torch.cuda.synchronize()
    pool.check(f'causal mixed d{d} n{n}')
    rel_mixed = float((A.heads_first(mixed.double().cpu(), HEADS) - ref).abs().max() / ref.abs().max())
    print(f'[attention split16 causal d{d} n{n}] max-abs / max|O| {rel:.3e} (mixed kernel {rel_mixed:.3e}, ratio {rel_mixed / max(rel, 1e-30):.0f}; '
          f'tol {min(TOL, 0.1 * rel_mixed):.3e})', flush=True)
    assert bool(torch.isfinite(got).all())
    assert TOL <= 0.1 * rel_mixed, (TOL, rel_mixed)
    assert rel <= TOL
    # the low half is one: finite, at most half an fp16 step of hi
    h = out.float().abs()
    step = torch.where(h == 0, torch.full_like(h, 2.0 ** -25), 2.0 ** (torch.floor(torch.log2(h.clamp_min(2.0 ** -14))) - 11))
    assert bool((out_lo.float().abs() <= step * (1 + 2.0 ** -10)).all())


@pytest.mark.parametrize('n', N)
@pytest.mark.parametrize('d', D)
def test_softmax_weights_per_element(d, n):
    scale = d ** -0.5
    w = min(d, 64)
    j = torch.arange(n)
    bad, worst = [], 0.0
    for regime in ('diffuse', 'rising'):
        q, k = A.make_qk(regime, BH, n, n, d, 9000 + 131 * d + n + (1 if regime == 'rising' else 0), split=True)
        Pqk = guard.Pool(DEV)
        qk = [*_put_split(Pqk, 'q', q), *_put_split(Pqk, 'k', k)]
        P, smax = A.softmax_ref(qk[0].double() + qk[1].double(), qk[2].double() + qk[3].double(), scale, causal=True)
        extra = A.score_rounding('split16', d, scale, smax)
        seen = torch.zeros(n, dtype=torch.bool)
        for j0 in range(0, n, w):
            col = torch.where((j >= j0) & (j < j0 + w), j - j0, torch.full_like(j, -1))
            seen |= col >= 0
            Pv = guard.Pool(DEV)
            vt = A.vt_padded(A.dense_v(col, BH, d, torch.float32), 0.0)
            out, out_lo = _run(Pv, qk + [*_put_split(Pv, 'vt', vt)], n, d, scale)
            tag = f'probe causal split16 d{d} n{n} {regime} keys {j0}..{min(n, j0 + w) - 1}'
            Pqk.check(tag)
            Pv.check(tag)
            r = A.judge(A.heads_first(out.double() + out_lo.double(), HEADS), P, col, A.R_SPLIT, True, extra)
            print(f'[{tag}] worst err / tol {r["worst"]:.3f}, weights above the diagonal (and empty columns) exactly 0: {r["zeros_exact"]}',
                  flush=True)
            worst = max(worst, r['worst'])
            if not (r['worst'] <= 1.0 and r['zeros_exact']):
                bad.append((regime, j0, r))
        assert bool(seen.all())                     # every key's weight was read
    print(f'[probe causal split16 d{d} n{n} SUMMARY] worst err / tol {worst:.3f}', flush=True)
    assert not bad, bad


@pytest.mark.parametrize('n', [n for n in N if n > 1])
@pytest.mark.parametrize('d', D)
def test_rows_before_a_changed_key_keep_their_bits(d, n):
    g = torch.Generator().manual_seed(11000 + 131 * d + n)
    scale = d ** -0.5
    q, k, v = (torch.randn((BH, n, d), generator=g) for _ in range(3))
    pool = guard.Pool(DEV)
    qo = [*_put_split(pool, 'q', q)]
    base = _run(pool, qo + [*_put_split(pool, 'k', k), *_put_split(pool, 'vt', A.vt_padded(v, 0.0))], n, d, scale)
    for jc in sorted({1, n // 2, n - 1}):
        k2, v2 = k.clone(), v.clone()
        k2[:, jc] = torch.randn((BH, d), generator=g) * 3
        v2[:, jc] = torch.randn((BH, d), generator=g) * 3
        got = _run(pool, qo + [*_put_split(pool, 'k2', k2), *_put_split(pool, 'vt2', A.vt_padded(v2, 0.0))], n, d, scale)
        for a, b, name in ((base[0], got[0], 'out'), (base[1], got[1], 'out_lo')):
            assert torch.equal(a[:, :jc].view(torch.int16), b[:, :jc].view(torch.int16)), (name, jc)
        assert not torch.equal(base[0][:, jc], got[0][:, jc]), jc          # ... and query jc sees the change
    pool.check(f'causal split16 bits d{d} n{n}')


def test_refusals():
    lib = _lib.load()
    t = torch.zeros(4 * 8 * 40, dtype=torch.float16, device=DEV)
    p = [t.data_ptr()] * 8
    assert lib.sdmi_k_attention_split16_causal(*p, 4, 2, 8, 8, 40, 0.1, _lib.stream_ptr()) != 0
    assert b'head dim 40 has no instantiation (32, 64, 128)' in lib.sdmi_last_error()
    assert lib.sdmi_k_attention_split16_causal(*p, 4, 2, 9, 12, 32, 0.1, _lib.stream_ptr()) != 0         # n_pad % 8
    assert lib.sdmi_k_attention_split16_causal(*p[:7], None, 4, 2, 8, 8, 32, 0.1, _lib.stream_ptr()) != 0  # null out_lo
