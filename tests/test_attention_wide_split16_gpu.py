"""Split-fp16 flash attention for wide heads (csrc/attn_wide_split16.hip: 160 < d <= 1024, d % 64 == 0) against fp64 torch, through
sdmi_k_attention_split16, which dispatches to it by head dim.

Inputs are fp32 and split on the host into hi = fp16(x), lo = fp16(x - hi); the reference sees the fp32 values.  Every operand and
both outputs live in guarded buffers (tests/guard.py): a read outside an operand reaches the result as NaN, a write outside the
output is seen by the guard check.  The bar is the project's own for split-fp16 attention (tests/test_full_precision_kernels_gpu.py):
max-abs / max|O| <= 1e-5 against fp64, finite outputs, lo at most half an fp16 step of hi.  Measured on an MI355X over every case of
this file: <= 8.6e-7 (profiles/attn_wide_split16.txt)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import _lib  # noqa: E402

from guard import Pool  # noqa: E402

DEV = 'cuda'
BAR = 1e-5


def _s():
    return _lib.stream_ptr()


def _split(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


def _join(hi, lo):
    return hi.double() + lo.double()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _half_step(hi):
    """half the fp16 spacing at each hi (the subnormal spacing at 0)"""
    h = hi.float().abs()
    return torch.where(h == 0, torch.full_like(h, 2.0 ** -25), 2.0 ** (torch.floor(torch.log2(h.clamp_min(2.0 ** -14))) - 11))


def _lo_is_a_low_half(hi, lo):
    return bool(torch.isfinite(lo.float()).all()) and bool((lo.float().abs() <= _half_step(hi) * (1 + 2.0 ** -10)).all())


def _attention_ref(q, k, vt, heads, nkv):
    """fp64, one (batch, head) pair at a time"""
    BH, nq, d = q.shape
    out = torch.empty((BH, nq, d), dtype=torch.float64, device=q.device)
    for i in range(BH):
        s = (q[i].double() @ k[i, :nkv].double().T) * d ** -0.5
        out[i] = torch.softmax(s, dim=-1) @ vt[i, :, :nkv].double().T
    return out.reshape(BH // heads, heads, nq, d).permute(0, 2, 1, 3).reshape(BH // heads, nq, heads * d)


def _inputs(g, BH, d, nq, nkv, nkv_pad=None, pad_fill=0.0):
    nkv_pad = (nkv + 7) // 8 * 8 if nkv_pad is None else nkv_pad
    q = torch.randn((BH, nq, d), generator=g).to(DEV)
    k = torch.randn((BH, nkv, d), generator=g).to(DEV)
    vt = torch.full((BH, d, nkv_pad), pad_fill, device=DEV)
    vt[:, :, :nkv] = torch.randn((BH, d, nkv), generator=g).to(DEV)
    return q, k, vt


def attention_split16(q, k, vt, heads, nkv, case=''):
    """q [BH,nq,d], k [BH,nkv,d], vt [BH,d,nkv_pad] fp32 -> [B, nq, heads*d] (hi, lo), all in guarded buffers"""
    BH, nq, d = q.shape
    pool = Pool(DEV)
    ops = []
    for name, t in (('q', q), ('k', k), ('vt', vt)):
        hi, lo = _split(t)
        ops += [pool.put(name, hi), pool.put(name + '_lo', lo)]
    out = pool.new('out', (BH // heads, nq, heads * d), torch.float16)
    out_lo = pool.new('out_lo', (BH // heads, nq, heads * d), torch.float16)
    _lib.check(_lib.load().sdmi_k_attention_split16(*[o.data_ptr() for o in ops], out.data_ptr(), out_lo.data_ptr(), BH, heads, nq, nkv,
                                                    vt.shape[2], d, d ** -0.5, _s()))
    torch.cuda.synchronize()
    pool.check(case)
    return out.clone(), out_lo.clone()


def _check(tag, out, out_lo, ref):
    rel = float((_join(out, out_lo) - ref).abs().max() / ref.abs().max())
    rel_hi = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f'[attention wide split16 {tag}] max-abs / max|O| {rel:.2e} (hi alone {rel_hi:.2e})', flush=True)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(out_lo.float()).all())
    assert rel <= BAR
    assert _lo_is_a_low_half(out, out_lo)
    return rel


# ragged query tails (a workgroup owns 32 queries), a ragged last key tile (64 keys per tile), one key; at (256, 77) nkv_pad = 80: a
# pad range in V^T.  d = 192 and 960: d / 32 is no multiple of 4 (waves 0 / 1 own one output tile more than waves 2 / 3).
SHAPES = [(64, 64), (33, 65), (1, 1), (129, 130), (256, 77)]


@pytest.mark.parametrize('BH,heads', [(2, 1), (4, 2)])
@pytest.mark.parametrize('nq,nkv', SHAPES)
@pytest.mark.parametrize('d', [192, 512, 960, 1024])
def test_attention_wide_split16(d, nq, nkv, BH, heads):
    q, k, vt = _inputs(_g(1000 + d + 7 * nq + nkv + BH), BH, d, nq, nkv)
    tag = f'd{d} nq{nq} nkv{nkv} BH{BH} heads{heads}'
    out, out_lo = attention_split16(q, k, vt, heads, nkv, tag)
    _check(tag, out, out_lo, _attention_ref(q, k, vt, heads, nkv))


def test_attention_wide_split16_first_stage_shape():
    """the mid block of the SD first stage at a 32 x 32 latent: 1024 tokens, one head of 512"""
    q, k, vt = _inputs(_g(77), 1, 512, 1024, 1024)
    out, out_lo = attention_split16(q, k, vt, 1, 1024, 'first stage')
    _check('d512 nq1024 nkv1024 BH1 heads1', out, out_lo, _attention_ref(q, k, vt, 1, 1024))


def test_attention_wide_split16_pad_columns_may_hold_anything():
    """V^T pad columns nkv .. nkv_pad (hi and lo) are NaN: the kernel replaces them by zeros after the load"""
    d, nq, nkv, nkv_pad = 512, 64, 3, 16
    q, k, vt = _inputs(_g(5), 2, d, nq, nkv, nkv_pad, pad_fill=float('nan'))
    assert bool(torch.isnan(vt[:, :, nkv:]).all())
    out, out_lo = attention_split16(q, k, vt, 1, nkv, 'NaN pads')
    _check(f'd{d} nq{nq} nkv{nkv} nkv_pad{nkv_pad} NaN pads', out, out_lo, _attention_ref(q, k, vt, 1, nkv))


@pytest.mark.parametrize('d', [192, 512, 1024])
def test_attention_wide_split16_one_key(d):
    """one key: P = 1 exactly, so hi + lo of the output is hi + lo of V, bit for bit"""
    BH, heads, nq = 4, 2, 33
    q, k, vt = _inputs(_g(9 + d), BH, d, nq, 1)
    out, out_lo = attention_split16(q, k, vt, heads, 1, f'one key d{d}')
    vh, vl = _split(vt)
    v = _join(vh, vl)[:, :, 0]                                                     # [BH, d]
    want = v.reshape(BH // heads, 1, heads * d).expand(-1, nq, -1)
    assert torch.equal(_join(out, out_lo), want)


def test_attention_wide_split16_large_logits():
    """|score * scale| up to ~60 with every query's maximum in the LAST key tile (see test_attention_split16_large_logits): the running
    max jumps there and the earlier tiles' sums and outputs are rescaled by alpha = exp(m_old - m_new)"""
    d, nq, nkv = 512, 64, 130
    g = _g(3000 + d + nq + nkv)
    BH, heads = 4, 2
    q, k, vt = _inputs(g, BH, d, nq, nkv)
    u = torch.randn((BH, 1, d), generator=g).to(DEV)
    u = u / u.norm(dim=-1, keepdim=True)
    q = q * 10 ** 0.5 + 60.0 * u
    k = k * 10 ** 0.5
    k = k - (k @ u.transpose(1, 2)) * u              # no other key sees u
    k[:, nkv - 1] = d ** 0.5 * u[:, 0]
    s = (q.double() @ k.double().transpose(1, 2)) * d ** -0.5
    last_tile = (nkv - 1) // 64 * 64
    assert float(s.abs().max()) >= 55.0 and bool((s.argmax(dim=-1) >= last_tile).all())
    out, out_lo = attention_split16(q, k, vt, heads, nkv, 'large logits')
    print(f'[attention wide split16 large logits] max |s scale| {float(s.abs().max()):.1f}', flush=True)
    _check(f'large logits d{d} nq{nq} nkv{nkv}', out, out_lo, _attention_ref(q, k, vt, heads, nkv))


def test_attention_wide_split16_is_repeatable():
    """fixed summation order, no atomics: two launches agree bit for bit"""
    q, k, vt = _inputs(_g(21), 2, 512, 129, 130)
    a = attention_split16(q, k, vt, 1, 130, 'repeat 1')
    b = attention_split16(q, k, vt, 1, 130, 'repeat 2')
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('d', [176, 1088])
def test_attention_wide_split16_unsupported_head_dim(d):
    """head dims in neither kernel's list fail by name and launch nothing"""
    q, k, vt = _inputs(_g(3), 1, d, 8, 8)
    with pytest.raises(_lib.SdmiError, match=f'head dim {d}'):
        attention_split16(q, k, vt, 1, 8, f'd{d}')
