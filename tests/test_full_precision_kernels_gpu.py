"""Kernels of the full-precision UNet mode (split-fp16 operands) against fp64 torch, through the C ABI.

Inputs are fp32 and split on the host into hi = fp16(x), lo = fp16(x - hi); the reference sees the fp32 values."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import _lib  # noqa: E402

DEV = 'cuda'


def _s():
    return _lib.stream_ptr()


def _split(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


def _join(hi, lo):
    return hi.double() + lo.double()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _reconstructs(hi, lo, ref):
    """hi + lo equals the fp32 value to 2^-21 relative (+ half an fp16 subnormal step for values whose low half underflows)"""
    err = (_join(hi, lo) - ref.double()).abs()
    bound = ref.double().abs() * 2.0 ** -21 + 2.0 ** -25
    return float((err - bound).max()) <= 0.0, float((err / ref.double().abs().clamp_min(1e-30)).max())


def attention_split16(q, k, vt, heads, nkv):
    """q [BH,nq,d], k [BH,nkv,d], vt [BH,d,nkv_pad] fp32 -> [B, nq, heads*d] (hi, lo)"""
    BH, nq, d = q.shape
    (qh, ql), (kh, kl), (vh, vl) = _split(q), _split(k), _split(vt)
    out = torch.empty((BH // heads, nq, heads * d), dtype=torch.float16, device=q.device)
    out_lo = torch.empty_like(out)
    _lib.check(_lib.load().sdmi_k_attention_split16(qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(), vh.data_ptr(), vl.data_ptr(),
                                                    out.data_ptr(), out_lo.data_ptr(), BH, heads, nq, nkv, vt.shape[2], d, d ** -0.5, _s()))
    torch.cuda.synchronize()
    return out, out_lo


def _attention_ref(q, k, vt, heads, nkv):
    """fp64, one (batch, head) pair at a time (the 9216-token score matrices stay small)"""
    BH, nq, d = q.shape
    out = torch.empty((BH, nq, d), dtype=torch.float64, device=q.device)
    for i in range(BH):
        s = (q[i].double() @ k[i, :nkv].double().T) * d ** -0.5
        out[i] = torch.softmax(s, dim=-1) @ vt[i, :, :nkv].double().T
    return out.reshape(BH // heads, heads, nq, d).permute(0, 2, 1, 3).reshape(BH // heads, nq, heads * d)


ATTN_CASES = [(d, n, n) for d in (40, 80, 160) for n in (64, 1024, 4096, 9216)] + [(d, 1024, 77) for d in (40, 80, 160)]
# the d = 32 / 64 / 128 instantiations; ragged query tails (one wave = 32 queries, one workgroup = 128); short and ragged key
# tiles (64 keys per tile, nkv_pad = round8(nkv))
ATTN_CASES += [(d, n, n) for d in (32, 64, 128) for n in (64, 1024)] + [(d, 1024, 77) for d in (32, 64, 128)] + [(64, 4096, 4096)]
ATTN_CASES += [(40, 1, 77), (64, 31, 1024), (80, 33, 77), (128, 129, 130), (32, 4095, 4095)]
ATTN_CASES += [(32, 64, 1), (40, 129, 3), (64, 33, 31), (80, 256, 33), (128, 64, 63), (160, 128, 65), (64, 1024, 130)]


def _half_step(hi):
    """half the fp16 spacing at each hi (the subnormal spacing at 0)"""
    h = hi.float().abs()
    return torch.where(h == 0, torch.full_like(h, 2.0 ** -25), 2.0 ** (torch.floor(torch.log2(h.clamp_min(2.0 ** -14))) - 11))


def _lo_is_a_low_half(hi, lo):
    return bool(torch.isfinite(lo.float()).all()) and bool((lo.float().abs() <= _half_step(hi) * (1 + 2.0 ** -10)).all())


@pytest.mark.parametrize('d,nq,nkv', ATTN_CASES)
def test_attention_split16(d, nq, nkv):
    """softmax(q k^T d^-1/2) v with every operand split-fp16: max-abs error relative to max|O| <= 1e-5 (fp16-operand attention: ~1e-3).
    B * heads = 16; cross-attention over 77 context tokens padded to 80 (pad keys of v^T zero, as the executor writes them).
    The low halves are finite and at most half an fp16 step of hi.  (Measured on an MI355X over these cases and the head-layout /
    large-logit ones below: <= 3.3e-6.)"""
    g = _g(1000 + d + nq + nkv)
    BH, heads = 16, 8
    nkv_pad = (nkv + 7) // 8 * 8
    q = torch.randn((BH, nq, d), generator=g).to(DEV)
    k = torch.randn((BH, nkv, d), generator=g).to(DEV)
    vt = torch.zeros((BH, d, nkv_pad), device=DEV)
    vt[:, :, :nkv] = torch.randn((BH, d, nkv), generator=g).to(DEV)
    out, out_lo = attention_split16(q, k, vt, heads, nkv)
    ref = _attention_ref(q, k, vt, heads, nkv)
    rel = float((_join(out, out_lo) - ref).abs().max() / ref.abs().max())
    rel_hi = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f'[attention split16 d{d} nq{nq} nkv{nkv}] max-abs / max|O| {rel:.2e} (hi alone {rel_hi:.2e})', flush=True)
    assert bool(torch.isfinite(out.float()).all()) and rel <= 1e-5
    assert _lo_is_a_low_half(out, out_lo)


def _attention_inputs(g, BH, d, nq, nkv):
    nkv_pad = (nkv + 7) // 8 * 8
    q = torch.randn((BH, nq, d), generator=g).to(DEV)
    k = torch.randn((BH, nkv, d), generator=g).to(DEV)
    vt = torch.zeros((BH, d, nkv_pad), device=DEV)
    vt[:, :, :nkv] = torch.randn((BH, d, nkv), generator=g).to(DEV)
    return q, k, vt


@pytest.mark.parametrize('BH,heads,d,nq,nkv', [(2, 1, 64, 129, 65), (2, 1, 160, 33, 77), (10, 5, 40, 31, 77), (10, 5, 128, 256, 33),
                                               (10, 5, 80, 1024, 1024)])
def test_attention_split16_head_layouts(BH, heads, d, nq, nkv):
    """one head, and an odd head count: the output's [b][q][head * d] addressing of (batch, head) pair bh"""
    q, k, vt = _attention_inputs(_g(2000 + BH + d + nq + nkv), BH, d, nq, nkv)
    out, out_lo = attention_split16(q, k, vt, heads, nkv)
    ref = _attention_ref(q, k, vt, heads, nkv)
    rel = float((_join(out, out_lo) - ref).abs().max() / ref.abs().max())
    print(f'[attention split16 BH{BH} heads{heads} d{d} nq{nq} nkv{nkv}] max-abs / max|O| {rel:.2e}', flush=True)
    assert bool(torch.isfinite(out.float()).all()) and rel <= 1e-5
    assert _lo_is_a_low_half(out, out_lo)


@pytest.mark.parametrize('d,nq,nkv', [(64, 256, 1024), (40, 129, 77), (160, 64, 130)])
def test_attention_split16_large_logits(d, nq, nkv):
    """|score * scale| up to ~60 with every query's maximum in the LAST key tile: the running max jumps there and the earlier
    tiles' sums and outputs are rescaled by alpha = exp(m_old - m_new).  Every query leans on a unit direction u (60 u) that only the
    last key has (sqrt(d) u): its score is 60 + N(0, 10); the other keys are orthogonal to u and score ~N(0, 10^2), so in some
    rows the earlier tiles come within ~10 of the maximum and their rescaled share is well above the bar."""
    g = _g(3000 + d + nq + nkv)
    BH, heads = 4, 2
    q, k, vt = _attention_inputs(g, BH, d, nq, nkv)
    u = torch.randn((BH, 1, d), generator=g).to(DEV)
    u = u / u.norm(dim=-1, keepdim=True)
    q = q * 10 ** 0.5 + 60.0 * u
    k = k * 10 ** 0.5
    k = k - (k @ u.transpose(1, 2)) * u              # no other key sees u
    k[:, nkv - 1] = d ** 0.5 * u[:, 0]
    s = (q.double() @ k.double().transpose(1, 2)) * d ** -0.5
    last_tile = (nkv - 1) // 64 * 64
    assert float(s.abs().max()) >= 55.0 and bool((s.argmax(dim=-1) >= last_tile).all())
    out, out_lo = attention_split16(q, k, vt, heads, nkv)
    ref = _attention_ref(q, k, vt, heads, nkv)
    rel = float((_join(out, out_lo) - ref).abs().max() / ref.abs().max())
    print(f'[attention split16 large logits d{d} nq{nq} nkv{nkv}] max |s scale| {float(s.abs().max()):.1f}, '
          f'max-abs / max|O| {rel:.2e}', flush=True)
    assert bool(torch.isfinite(out.float()).all()) and rel <= 1e-5
    assert _lo_is_a_low_half(out, out_lo)


@pytest.mark.parametrize('kind,ntok', [(0, 77), (0, 256), (1, 77), (1, 256)])
def test_split_heads(kind, ntok):
    """the per-head scatter of q / k (kind 0) and v^T (kind 1, pad tokens zero) reconstructs its fp32 source"""
    g = _g(7 + kind + ntok)
    B, heads, dh, ld, col0 = 2, 8, 40, 3 * 320, 320
    ntok_pad = (ntok + 7) // 8 * 8
    src = (torch.randn((B * ntok, ld), generator=g) * 3).to(DEV)
    shape = (B * heads, ntok, dh) if kind == 0 else (B * heads, dh, ntok_pad)
    hi = torch.full(shape, float('nan'), dtype=torch.float16, device=DEV)
    lo = torch.full(shape, float('nan'), dtype=torch.float16, device=DEV)
    _lib.check(_lib.load().sdmi_k_split_heads(src.data_ptr(), ld, col0, hi.data_ptr(), lo.data_ptr(), kind, B, ntok, ntok_pad, heads, dh, _s()))
    torch.cuda.synchronize()
    x = src[:, col0:col0 + heads * dh].reshape(B, ntok, heads, dh).permute(0, 2, 1, 3).reshape(B * heads, ntok, dh)
    if kind == 1:
        x = torch.cat([x.transpose(1, 2), torch.zeros((B * heads, dh, ntok_pad - ntok), device=DEV)], dim=2)
    ok, worst = _reconstructs(hi, lo, x)
    print(f'[split heads kind {kind} ntok {ntok}] worst relative reconstruction error {worst:.2e}', flush=True)
    assert ok


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('dh', [32, 64, 80, 160])
@pytest.mark.parametrize('seg', [0, 1, 2])
@pytest.mark.parametrize('ntok', [1, 3, 4096])
def test_split_heads_edges(kind, dh, seg, ntok):
    """head widths 32 .. 160, every column segment of a [q | k | v] source (col0 = 0, C, 2C), 1, 3 and 4096 tokens; kind 1
    writes its pad tokens as exactly +0 in hi and lo (NaN before), which attn_split16 multiplies by zero probabilities"""
    g = _g(17 + kind + dh + seg + ntok)
    B, heads = 2, 8
    C = heads * dh
    ld, col0 = 3 * C, seg * C
    ntok_pad = (ntok + 7) // 8 * 8
    src = (torch.randn((B * ntok, ld), generator=g) * 3).to(DEV)
    shape = (B * heads, ntok, dh) if kind == 0 else (B * heads, dh, ntok_pad)
    hi = torch.full(shape, float('nan'), dtype=torch.float16, device=DEV)
    lo = torch.full(shape, float('nan'), dtype=torch.float16, device=DEV)
    _lib.check(_lib.load().sdmi_k_split_heads(src.data_ptr(), ld, col0, hi.data_ptr(), lo.data_ptr(), kind, B, ntok, ntok_pad, heads, dh, _s()))
    torch.cuda.synchronize()
    x = src[:, col0:col0 + C].reshape(B, ntok, heads, dh).permute(0, 2, 1, 3).reshape(B * heads, ntok, dh)
    if kind == 1:
        x = x.transpose(1, 2)
        for t in (hi, lo):
            pad = t[:, :, ntok:].contiguous().view(torch.int16)
            assert torch.equal(pad, torch.zeros_like(pad))
        hi, lo = hi[:, :, :ntok], lo[:, :, :ntok]
    ok, worst = _reconstructs(hi, lo, x)
    print(f'[split heads kind {kind} dh {dh} col0 {col0} ntok {ntok}] worst relative reconstruction error {worst:.2e}', flush=True)
    assert ok


def test_geglu_split():
    """value * gelu(gate) (erf form, attention.py:222-225) as hi / lo: lo is at most half an fp16 step of hi, and hi + lo is within
    2e-6 relative of fp64 (erff and the products in fp32; + half an fp16 subnormal step where the low half underflows)"""
    g = _g(11)
    M, Fd = 300, 1280
    src = (torch.randn((M, 2 * Fd), generator=g) * 2).to(DEV)
    hi = torch.empty((M, Fd), dtype=torch.float16, device=DEV)
    lo = torch.empty_like(hi)
    _lib.check(_lib.load().sdmi_k_geglu_split(src.data_ptr(), M, Fd, hi.data_ptr(), lo.data_ptr(), _s()))
    torch.cuda.synchronize()
    s64 = src.double()
    ref = s64[:, :Fd] * F.gelu(s64[:, Fd:])
    v = _join(hi, lo)
    step = torch.where(hi.float() == 0, torch.full_like(hi.float(), 2.0 ** -24),
                       2.0 ** (torch.floor(torch.log2(hi.float().abs().clamp_min(2.0 ** -14))) - 10))
    assert bool((lo.float().abs() <= 0.5 * step * (1 + 2.0 ** -10)).all())
    err = (v - ref).abs()
    worst = float((err / ref.abs().clamp_min(1e-3)).max())
    print(f'[geglu split] worst relative error vs fp64 (|y| >= 1e-3) {worst:.2e}', flush=True)
    assert float((err - (2e-6 * ref.abs() + 2.0 ** -25)).max()) <= 0.0


@pytest.mark.parametrize('C', [64, 320, 1280])
def test_layernorm_split(C):
    """LayerNorm (attention.py:211-215, eps 1e-5) as hi / lo: within 1e-6 of fp64 relative to the largest output"""
    g = _g(C)
    M = 257
    x = (torch.randn((M, C), generator=g) * 4 + 1).to(DEV)
    gamma = (torch.rand((C,), generator=g) + 0.5).to(DEV)
    beta = torch.randn((C,), generator=g).to(DEV)
    hi = torch.empty((M, C), dtype=torch.float16, device=DEV)
    lo = torch.empty_like(hi)
    _lib.check(_lib.load().sdmi_k_layernorm_split(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), hi.data_ptr(), lo.data_ptr(), M, C, 1e-5, _s()))
    torch.cuda.synchronize()
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    err = float((_join(hi, lo) - ref).abs().max() / ref.abs().max())
    print(f'[layernorm split C{C}] max-abs / max|y| {err:.2e}', flush=True)
    assert err <= 1e-6


def test_resampler_operand_reconstructs():
    """the operand of a full-mode Downsample / Upsample (sdmi_k_cast_f16 with out_lo) reconstructs the fp32 residual stream"""
    g = _g(5)
    x = (torch.randn((2 * 32 * 32 * 320,), generator=g) * 10).to(DEV)
    hi = torch.empty(x.shape, dtype=torch.float16, device=DEV)
    lo = torch.empty_like(hi)
    _lib.check(_lib.load().sdmi_k_cast_f16(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), x.numel(), _s()))
    torch.cuda.synchronize()
    ok, worst = _reconstructs(hi, lo, x)
    assert ok, worst
