"""Every attention kernel's softmax weights against fp64, read back through an indicator V (tests/attn_probes.py).

The other attention tests draw q, k, v ~ N(0, 1) and hold max-abs to 3e-3 / 4e-3 (mixed) or to 1e-5 of max|O| per tensor (split-fp16): with
diffuse weights the output is an average of nkv values, the bar sits 20 .. 75 times above the arithmetic's own error, and only query row 0
of (batch, head) pair 0 has a dominant key.  Here V has entries 0 or 1, so an output element IS a sum of softmax weights, and each is held
to

    tol = R ref + 2^-24 n_c rowmax_j(P) + 2^-24        (n_c = keys coded into the column; R = 2^-9 mixed, 1e-5 split-fp16)

(for the split-fp16 kernels R + 2 scale 2^-24 max_j |q k_j| sqrt(n_acc): the fp32 rounding of a score accumulated over n_acc MFMA passes,
derived in attn_probes.score_rounding; 2e-7 under `diffuse`, up to 2e-5 where the regime shifts the scores by 20) against the fp64 softmax of the operands as the kernel receives them (fp16 values; hi + lo for the split kernels), under six score regimes
that put the rescale, the tail mask, fp16-subnormal P and far-apart key-group merge weights into every lane of every wave, and V codings
that show a lost tile (`segments`), keys permuted inside a tile (`stride`) and single weights (`window`: the first keys, the ragged end, the
key-split seam).  An output with no key coded into its column must be exactly 0.0.  The V^T pad columns nkv .. nkv_pad are zero for d <= 160
(the contract in include/sdmi.h) and NaN for the wide kernels.  Operands and outputs live in guarded buffers (tests/guard.py).

Each case asserts, from the reference alone, that it is live (attn_probes.live): every query row that sees a coded key has a live output,
and >= 10 % of the non-empty outputs are live (cases with fewer than 8 keys are exempt from the share).  A causal row before a window sees
none of its keys: the whole row must then be exactly 0, and the row rule cannot apply to it.  For the split-fp16 kernels liveness is taken
at the mixed kernels' 2^-9 as well -- their own R = 1e-5 exceeds 8 x the fp16 floors of P_lo and out_lo only on weights above 0.048 -- and
the share at R = 1e-5 is printed beside it.

Kernels reached (dispatch: attn.hip launch_d, attn_wide.hip launch_wide_d, attn_split16.hip):
  dma           attn_dma_kernel<D, 2 | 4 | 8 waves>, all nine D: 1, 2, 3, 4, 6, 8 and 16 key tiles against rings of 4 (3 at d = 160) stages
  kvsplit       attn_dma_kernel<40, 16, 4, false, 0, 2>: nq > 1024, nkv % 128 == 0, 2048 <= nkv <= 4096; (1030, 2112) is the one-group
                kernel one tile past the seam
  causal        attn_kernel<D, 2, true>, D = 32 / 64 / 128
  wide          attn_wide_kernel<D, 2 | 4>, D = 192 / 448 / 1024
  split16       attn_split16_kernel<D, 4>, D = 24 / 40 / 64 / 160
  wide_split16  attn_wide_split16.hip, D = 192 / 1024
Not here: st_mid_ctx's in-launch cross-attention (tests/test_rowchain_gpu.py holds it bit-identical to sdmi_k_attention), and the non-causal
attn_kernel instantiations, which the dispatch cannot reach: every instantiated D is a multiple of 8, so (nkv * D) % 8 != 0 never holds.

Measured on an MI355X, worst err / tol over every regime x coding of a family (smallest live share beside it):
  family                                        cases   worst err / tol   smallest live share
  dma, 2 waves (nq <= 96)                          36        0.499              27.4 %
  dma, 4 waves (97 .. 1024)                        27        0.497              28.2 %
  dma, 8 waves (nq > 1024)                          9        0.491              28.4 %
  key split (2048, 2176, 4096 keys)                 3        0.480              30.5 %
  one group, one tile past the seam (2112 keys)     1        0.462              31.8 %
  causal                                           18        0.497              48.5 %
  wide, 2 waves                                     9        0.498              26.6 %
  wide, 4 waves                                     3        0.498              22.2 %
  split16 d = 24 / 40 / 64 / 160                   16        0.485 / 0.494 / 0.555 / 0.694      27.6 %
  wide split16 d = 192 / 1024                       6        0.590 / 0.801      26.7 %
The mixed kernels sit where a CPU restatement of their arithmetic does (0.47, tests/test_attention_probes_host.py): half the bar is the
fp16 rounding of P and of the output.  The split-fp16 kernels WITHOUT the score-rounding term: 0.49 / 0.60 / 0.92 / 1.43 at d = 24 / 40 / 64 /
160 and 1.03 / 2.01 at d = 192 / 1024, the excess under `negative` and `rising` only (`diffuse`, `falling`: 0.43 .. 0.50 at every d); with
it no family has more than a factor 2 in hand.  Their live share at R = 1e-5 itself is 0 .. 7 %.
The 128 cases take 7 s together.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import _lib  # noqa: E402

import attn_probes as A  # noqa: E402
import guard  # noqa: E402
import kernels as K  # noqa: E402

DEV = 'cuda'


def _cases(family):
    return [pytest.param(d, nq, nkv, id=f'd{d}-nq{nq}-nkv{nkv}') for f, d, nq, nkv in A.gpu_cases() if f == family]


def _run(family, d, nq, nkv, monkeypatch):
    monkeypatch.delenv('SDMI_ATTN_KVS', raising=False)          # the dispatch under test is the default one
    B, heads = A.batch_heads(family, nq, nkv)
    BH = B * heads
    causal = family == 'causal'
    split = family in ('split16', 'wide_split16')
    R = A.case_R(family)
    scale = d ** -0.5
    pad_fill = float('nan') if d > 160 else 0.0
    lib = _lib.load()
    bad, worst, least, least_own = [], 0.0, 1.0, 1.0
    for regime in A.REGIMES:
        q, k = A.make_qk(regime, BH, nq, nkv, d, A.case_seed(family, d, nq, nkv, regime), split)
        Pqk = guard.Pool(DEV)
        if split:
            (qh, ql), (kh, kl) = (K.cast_f16(t.to(DEV).contiguous(), want_lo=True) for t in (q, k))
            qk_ops = [Pqk.put('q', qh), Pqk.put('q_lo', ql), Pqk.put('k', kh), Pqk.put('k_lo', kl)]
            P, smax = A.softmax_ref(qh.double() + ql.double(), kh.double() + kl.double(), scale)
        else:
            qk_ops = [Pqk.put('q', q.to(DEV)), Pqk.put('k', k.to(DEV))]
            P, smax = A.softmax_ref(qk_ops[0], qk_ops[1], scale, causal)
        extra = A.score_rounding(family, d, scale, smax)
        for name, col in A.codings(regime, nkv, d):
            tag = f'probe {family} d{d} nq{nq} nkv{nkv} BH{BH} {regime}/{name}'
            Pv = guard.Pool(DEV)
            out = Pv.new('out', (B, nq, heads * d), torch.float16)
            if split:
                vt = A.vt_padded(A.dense_v(col, BH, d, torch.float32), 0.0).to(DEV)
                vh, vl = K.cast_f16(vt, want_lo=True)
                vh[:, :, nkv:] = pad_fill
                vl[:, :, nkv:] = pad_fill
                vh, vl = Pv.put('vt', vh), Pv.put('vt_lo', vl)
                out_lo = Pv.new('out_lo', (B, nq, heads * d), torch.float16)
                _lib.check(lib.sdmi_k_attention_split16(qk_ops[0].data_ptr(), qk_ops[1].data_ptr(), qk_ops[2].data_ptr(), qk_ops[3].data_ptr(),
                                                        vh.data_ptr(), vl.data_ptr(), out.data_ptr(), out_lo.data_ptr(), BH, heads, nq, nkv,
                                                        vh.shape[2], d, float(scale), _lib.stream_ptr()))
            else:
                vt = Pv.put('vt', A.vt_padded(A.dense_v(col, BH, d), pad_fill).to(DEV))
                if causal:
                    _lib.check(lib.sdmi_k_attention_causal(qk_ops[0].data_ptr(), qk_ops[1].data_ptr(), vt.data_ptr(), out.data_ptr(), BH, heads,
                                                           nq, vt.shape[2], d, float(scale), _lib.stream_ptr()))
                else:
                    _lib.check(lib.sdmi_k_attention(qk_ops[0].data_ptr(), qk_ops[1].data_ptr(), vt.data_ptr(), out.data_ptr(), BH, heads, nq,
                                                    nkv, vt.shape[2], d, float(scale), _lib.stream_ptr()))
            torch.cuda.synchronize()
            Pqk.check(tag)
            Pv.check(tag)
            got = out.double() + out_lo.double() if split else out.double()
            j = A.judge(A.heads_first(got, heads), P, col, R, causal, extra)
            own = f' (at R = 1e-5: {100 * j["share_own"]:.1f} %)' if split else ''
            print(f'[{tag}] worst err / tol {j["worst"]:.3f} at flat {j["at"]}, live {100 * j["share"]:.1f} %{own}, every row live '
                  f'{j["rows_live"]}, empty columns exactly 0: {j["zeros_exact"]}', flush=True)
            worst = max(worst, j['worst'])
            if nkv >= 8:
                least, least_own = min(least, j['share']), min(least_own, j['share_own'])
            if not (j['worst'] <= 1.0 and j['zeros_exact'] and j['rows_live'] and (nkv < 8 or j['share'] >= 0.10)):
                bad.append((regime, name, j))
    own = f' (at R = 1e-5: {100 * least_own:.1f} %)' if split else ''
    print(f'[probe {family} d{d} nq{nq} nkv{nkv} BH{BH} SUMMARY] worst err / tol {worst:.3f}, smallest live share {100 * least:.1f} %{own}',
          flush=True)
    assert not bad, bad


@pytest.mark.parametrize('d,nq,nkv', _cases('dma'))
def test_probe_dma(d, nq, nkv, monkeypatch):
    _run('dma', d, nq, nkv, monkeypatch)


@pytest.mark.parametrize('d,nq,nkv', _cases('kvsplit'))
def test_probe_key_split(d, nq, nkv, monkeypatch):
    _run('kvsplit', d, nq, nkv, monkeypatch)


@pytest.mark.parametrize('d,nq,nkv', _cases('causal'))
def test_probe_causal(d, nq, nkv, monkeypatch):
    _run('causal', d, nq, nkv, monkeypatch)


@pytest.mark.parametrize('d,nq,nkv', _cases('wide'))
def test_probe_wide(d, nq, nkv, monkeypatch):
    _run('wide', d, nq, nkv, monkeypatch)


@pytest.mark.parametrize('d,nq,nkv', _cases('split16'))
def test_probe_split16(d, nq, nkv, monkeypatch):
    _run('split16', d, nq, nkv, monkeypatch)


@pytest.mark.parametrize('d,nq,nkv', _cases('wide_split16'))
def test_probe_wide_split16(d, nq, nkv, monkeypatch):
    _run('wide_split16', d, nq, nkv, monkeypatch)
