"""The one-pass attention kernel for at most 256 keys (csrc/attn_small.hip) through sdmi_k_attention with SDMI_ATTN_SMALL=2, held to the
attention probes of tests/attn_probes.py: softmax weights read back through an indicator V, per element against the fp64 softmax of the
operands as the kernel receives them,

    tol = 2^-9 ref + 2^-24 n_c rowmax_j(P) + 2^-24        (attn_probes.tolerance with R_MIXED: the bar of the ring kernel)

under all six score regimes and every V coding, with q / k / V^T / out in guarded buffers (tests/guard.py).  The cases are
tests/attn_small_cases.py (d = 80 / 160, two batches of two heads, 32 / 96 / 40 queries, every edge of the 32-key score blocks up to 256
keys); tests/test_attn_small_host.py holds every one of them live on the CPU.  Each case runs at the routing's waves per workgroup and at
four (96 queries then leave the fourth wave of a workgroup without a slice); the two outputs must be the same bits.  An output with no key coded into its column must be
exactly 0.0, and a row of the output past nq or a column past a head's d is a guard or a neighbour's payload: the guards must be intact.

Knob on against knob off: the ring kernel (SDMI_ATTN_SMALL=0) runs on the same operands, is held to the same bar, and the two outputs may
differ per element by the sum of the two tolerances -- they are not bit-identical, the ring kernel exponentiates against a running maximum.
257 keys are one too many for the one-pass kernel: knob 2 must fall back to the ring kernel there, bit for bit.

Measured on an MI355X over the 66 cases (every regime x coding): worst err / tol 0.515 for the one-pass kernel and 0.515 for the ring kernel on the
same operands, worst |on - off| / (tol + tol) 0.480; one and four waves per workgroup bit-equal everywhere.  The 68 tests take 6 s together.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import _lib  # noqa: E402

import attn_probes as A  # noqa: E402
import attn_small_cases as S  # noqa: E402
import guard  # noqa: E402

DEV = 'cuda'


def _launch(knob, monkeypatch, q, k, vt, out, heads, nkv, d, nw=None):
    monkeypatch.setenv('SDMI_ATTN_SMALL', str(knob))
    if nw is None:
        monkeypatch.delenv('SDMI_ATTN_SMALL_NW', raising=False)
    else:
        monkeypatch.setenv('SDMI_ATTN_SMALL_NW', str(nw))         # (waves per workgroup of the one-pass kernel; the ring kernel ignores it)
    BH, nq = q.shape[0], q.shape[1]
    _lib.check(_lib.load().sdmi_k_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), BH, heads, nq, nkv, vt.shape[2], d,
                                            float(d ** -0.5), _lib.stream_ptr()))
    torch.cuda.synchronize()


@pytest.mark.parametrize('d,nq,nkv', [pytest.param(*c, id='d%d-nq%d-nkv%d' % c) for c in S.cases()])
def test_probe_small(d, nq, nkv, monkeypatch):
    for name in ('SDMI_ATTN_KVS', 'SDMI_ATTN_NW', 'SDMI_ATTN_SMALL_NW'):
        monkeypatch.delenv(name, raising=False)
    lib = _lib.load()
    assert lib.sdmi_attn_small_takes(d, nq, nkv, 0, 2) > 0
    BH = S.B * S.HEADS
    bad, worst, worst_off, worst_pair = [], 0.0, 0.0, 0.0
    for regime in A.REGIMES:
        q, k = A.make_qk(regime, BH, nq, nkv, d, S.seed(d, nq, nkv, regime))
        Pqk = guard.Pool(DEV)
        qd, kd = Pqk.put('q', q.to(DEV)), Pqk.put('k', k.to(DEV))
        P, _ = A.softmax_ref(qd, kd, d ** -0.5)
        rowmax = P.max(dim=-1, keepdim=True).values
        for name, col in A.codings(regime, nkv, d):
            tag = f'probe small d{d} nq{nq} nkv{nkv} BH{BH} {regime}/{name}'
            Pv = guard.Pool(DEV)
            vt = Pv.put('vt', A.vt_padded(A.dense_v(col, BH, d), 0.0).to(DEV))
            out = Pv.new('out', (S.B, nq, S.HEADS * d), torch.float16)
            off = Pv.new('out_ring', (S.B, nq, S.HEADS * d), torch.float16)
            out4 = Pv.new('out_4waves', (S.B, nq, S.HEADS * d), torch.float16)
            _launch(2, monkeypatch, qd, kd, vt, out, S.HEADS, nkv, d)
            _launch(2, monkeypatch, qd, kd, vt, out4, S.HEADS, nkv, d, nw=4)
            _launch(0, monkeypatch, qd, kd, vt, off, S.HEADS, nkv, d)
            Pqk.check(tag)
            Pv.check(tag)
            got, ring = A.heads_first(out.double(), S.HEADS), A.heads_first(off.double(), S.HEADS)
            j, j0 = A.judge(got, P, col, A.R_MIXED), A.judge(ring, P, col, A.R_MIXED)
            tol = A.tolerance(A.coded(P, col, d), rowmax, A.key_counts(col, BH, nq, d, False, P.device), A.R_MIXED)
            diff = (got - ring).abs()
            pair = float(torch.where(torch.isfinite(diff), diff / (2 * tol), torch.full_like(diff, float('inf'))).max())
            print(f'[{tag}] worst err / tol {j["worst"]:.3f} (ring kernel {j0["worst"]:.3f}), |on - off| / (tol + tol) {pair:.3f}, live '
                  f'{100 * j["share"]:.1f} %, every row live {j["rows_live"]}, empty columns exactly 0: {j["zeros_exact"]}', flush=True)
            worst, worst_off, worst_pair = max(worst, j['worst']), max(worst_off, j0['worst']), max(worst_pair, pair)
            same4 = torch.equal(out, out4)        # the waves of a workgroup share nothing: the grouping cannot change a bit
            if not (same4 and j['worst'] <= 1.0 and j['zeros_exact'] and j['rows_live'] and (nkv < 8 or j['share'] >= 0.10) and pair <= 1.0):
                bad.append((regime, name, j, pair, same4))
    print(f'[probe small d{d} nq{nq} nkv{nkv} BH{BH} SUMMARY] worst err / tol {worst:.3f} (ring kernel {worst_off:.3f}), '
          f'|on - off| / (tol + tol) {worst_pair:.3f}', flush=True)
    assert not bad, bad


@pytest.mark.parametrize('d', S.D)
def test_one_key_too_many_falls_back_to_the_ring_kernel(d, monkeypatch):
    for name in ('SDMI_ATTN_KVS', 'SDMI_ATTN_NW', 'SDMI_ATTN_SMALL_NW'):
        monkeypatch.delenv(name, raising=False)
    nq, nkv, BH = 40, S.NKV_LIMIT + 1, S.B * S.HEADS
    assert _lib.load().sdmi_attn_small_takes(d, nq, nkv, 0, 2) == 0
    q, k = A.make_qk('rising', BH, nq, nkv, d, S.seed(d, nq, nkv, 'rising'))
    _, col = A.codings('rising', nkv, d)[1]
    pool = guard.Pool(DEV)
    qd, kd = pool.put('q', q.to(DEV)), pool.put('k', k.to(DEV))
    vt = pool.put('vt', A.vt_padded(A.dense_v(col, BH, d), 0.0).to(DEV))
    outs = [pool.new(f'out_knob{knob}', (S.B, nq, S.HEADS * d), torch.float16) for knob in (2, 0)]
    _launch(2, monkeypatch, qd, kd, vt, outs[0], S.HEADS, nkv, d)
    _launch(0, monkeypatch, qd, kd, vt, outs[1], S.HEADS, nkv, d)
    pool.check(f'small fallback d{d}')
    assert torch.equal(outs[0], outs[1])
    P, _ = A.softmax_ref(qd, kd, d ** -0.5)
    assert A.judge(A.heads_first(outs[0].double(), S.HEADS), P, col, A.R_MIXED)['worst'] <= 1.0
