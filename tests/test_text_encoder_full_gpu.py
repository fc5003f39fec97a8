"""The full-precision text encoders (FrozenCLIPEmbedderHIP / BERTEmbedderHIP with hip_precision='full': every MFMA operand split-fp16)
on the GPU, and the pieces only they use: the hi / lo activation producers and the split-fp16 GEMM at text-encoder row counts.

Reference for the encoders: the fp64 evaluation of the same network -- oracle.clip_ref.clip_text_forward / bert_ref.bert_forward run
unchanged on a .double() state dict.  The committed fp32 goldens (clip_*.npz, bert_*.npz) are the second check, held to the fp64 pin plus
the distance between the fp32 and the fp64 evaluation of the oracle on that case, computed here.

Hard bars: a tenth of the mixed mode's pins (tests/test_clip_gpu.py CLIP_TOL, tests/test_bert_gpu.py BARS) -- a mode that costs three MFMA
passes has to buy an order of magnitude.  Per-case pins: 1.25 x the max-abs measured on an MI355X (profiles/full_precision_text_encoder.txt),
never above the hard bar.  The mixed mode's error on the same inputs is printed beside each."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import clip_ref  # noqa: E402
from stable_diffusion_amd import _lib  # noqa: E402

import bert_ref  # noqa: E402
import guard  # noqa: E402
import kernels as K  # noqa: E402
from test_bert_gpu import BARS as BERT_MIXED_BARS  # noqa: E402
from test_clip_gpu import CLIP_TOL, _FakeTokenizer, _text_config  # noqa: E402

DEV = 'cuda'
CLIP_CFGS = {'tiny': clip_ref.TINY_CLIP, 'sd': clip_ref.SD_CLIP}
CLIP_CASES = ['tiny_b2', 'tiny_b3_L40', 'sd_b2']
BERT_CASES = ['tiny_b2', 'tiny_b3_L40', 'laion_d2_b2', 'laion_b2']
CLIP_HARD = 0.1 * CLIP_TOL
BERT_HARD = {k: 0.1 * v for k, v in BERT_MIXED_BARS.items()}
SEEDS = [0, 1, 2]
# max-abs against the fp64 oracle measured on an MI355X, weight seeds 0 / 1 / 2 (profiles/full_precision_text_encoder.txt); pin = 1.25 x
CLIP_MEASURED = {'tiny_b2': (2.413e-6, 2.581e-6, 2.673e-6), 'tiny_b3_L40': (3.090e-6, 2.321e-6, 2.827e-6),
                 'sd_b2': (7.204e-6, 8.914e-6, 8.256e-6),
                 'tiny_props': (3.521e-6,)}          # the property tests' own inputs (B = 4, ids seed 3; the fake tokenizer's ids)
BERT_MEASURED = {'tiny_b2': (2.502e-6, 2.583e-6, 2.453e-6), 'tiny_b3_L40': (2.205e-6, 2.769e-6, 3.087e-6),
                 'laion_d2_b2': (6.166e-6, 6.743e-6, 7.234e-6), 'laion_b2': (1.246e-5, 1.167e-5, 1.004e-5),
                 'tiny_props': (3.042e-6,)}          # the property tests' own inputs (B = 3, ids seed 3; the fake tokenizer's ids)


class _Double(dict):
    """a state dict that hands out .double() copies on access (the 32-layer BERT never exists twice in fp64)"""

    def __getitem__(self, key):
        return dict.__getitem__(self, key).double()


_cache = {}


def _models(family, cfg_name, wseed):
    """(state dict, full module, mixed module) of one weight set; one weight set at a time lives on the GPU"""
    key = (family, cfg_name, wseed)
    if key not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        from stable_diffusion_amd import BERTEmbedderHIP, FrozenCLIPEmbedderHIP
        mods = []
        if family == 'clip':
            cfg = CLIP_CFGS[cfg_name]
            sd = clip_ref.make_clip_state_dict(cfg, wseed)
            for prec in ('full', 'mixed'):
                m = FrozenCLIPEmbedderHIP(text_config=_text_config(cfg), tokenizer=_FakeTokenizer(cfg.vocab_size), hip_precision=prec)
                missing, unexpected = m.load_state_dict({'transformer.' + k: v for k, v in sd.items()}, strict=False)
                assert not unexpected and missing == ['transformer.text_model.embeddings.position_ids']
                mods.append(m.cuda())
        else:
            cfg = bert_ref.CFGS[cfg_name]
            sd = bert_ref.make_bert_state_dict(cfg, wseed)
            for prec in ('full', 'mixed'):
                m = BERTEmbedderHIP(**cfg.embedder_kwargs(), use_tokenizer=False, hip_precision=prec)
                m.load_state_dict({'transformer.' + k: v for k, v in sd.items()}, strict=True)
                mods.append(m.cuda())
        _cache[key] = (sd, mods[0], mods[1])
    return _cache[key]


def _pin(measured, case, wseed, hard):
    return min(hard, 1.25 * measured[case][wseed])


def _check(tag, full, mixed, ref64, pin, hard, gold=None, ref32=None):
    err = (full.double().cpu() - ref64).abs()
    mx, rms = float(err.max()), float(err.pow(2).mean().sqrt())
    mx_mixed = float((mixed.double().cpu() - ref64).abs().max())
    line = (f'[text encoder full {tag}] vs fp64 max-abs {mx:.3e} rms {rms:.3e} (mixed mode on the same inputs {mx_mixed:.3e}) '
            f'|ref|max {float(ref64.abs().max()):.3f} (pin {pin:.2e}, hard bar {hard:.2e})')
    if gold is not None:
        d3264 = float((ref32.double() - ref64).abs().max())
        gerr = float((full.float().cpu() - gold).abs().max())
        line += f' | vs fp32 golden max-abs {gerr:.3e} (oracle fp32 vs fp64 {d3264:.3e})'
    print(line, flush=True)
    assert full.dtype == torch.float32 and bool(torch.isfinite(full).all())
    assert pin <= hard
    assert mx <= pin
    if gold is not None:
        assert gerr <= pin + d3264


# ---- whole encoders against the fp64 oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wseed', SEEDS)
@pytest.mark.parametrize('case', CLIP_CASES)
def test_clip_full_against_fp64(case, wseed, golden_dir):
    z = np.load(os.path.join(golden_dir, f'clip_{case}.npz'))
    cfg_name = str(z['cfg'])
    cfg = CLIP_CFGS[cfg_name]
    sd, full, mixed = _models('clip', cfg_name, wseed)
    ids = clip_ref.make_clip_ids(cfg, int(z['batch']), int(z['L']), seed=int(z['input_seed']))
    ref64 = clip_ref.clip_text_forward(_Double(sd), cfg, ids)
    assert ref64.dtype == torch.float64
    is_gold = wseed == int(z['weight_seed'])
    out, out_mixed = full.encode_ids(ids.cuda()), mixed.encode_ids(ids.cuda())
    torch.cuda.synchronize()
    _check(f'clip {case} weight seed {wseed}', out, out_mixed, ref64, _pin(CLIP_MEASURED, case, wseed, CLIP_HARD), CLIP_HARD,
           torch.from_numpy(z['out']) if is_gold else None, clip_ref.clip_text_forward(sd, cfg, ids) if is_gold else None)


@pytest.mark.parametrize('wseed', SEEDS)
@pytest.mark.parametrize('case', BERT_CASES)
def test_bert_full_against_fp64(case, wseed, golden_dir):
    z = np.load(os.path.join(golden_dir, f'bert_{case}.npz'))
    cfg_name = str(z['cfg'])
    cfg = bert_ref.CFGS[cfg_name]
    sd, full, mixed = _models('bert', cfg_name, wseed)
    ids = bert_ref.make_bert_ids(cfg, int(z['batch']), int(z['L']), seed=int(z['input_seed']))
    with torch.no_grad():
        ref64 = bert_ref.bert_forward(_Double(sd), cfg, ids)
        is_gold = wseed == int(z['weight_seed'])
        ref32 = bert_ref.bert_forward(sd, cfg, ids) if is_gold else None
    assert ref64.dtype == torch.float64
    out, out_mixed = full(ids.cuda()), mixed(ids.cuda())
    torch.cuda.synchronize()
    hard = BERT_HARD[cfg_name]
    _check(f'bert {case} weight seed {wseed}', out, out_mixed, ref64, _pin(BERT_MEASURED, case, wseed, hard), hard,
           torch.from_numpy(z['out']) if is_gold else None, ref32)


# ---- the properties the mixed tests hold ---------------------------------------------------------------------------------------------------
def test_clip_full_is_causal_repeatable_and_batch_independent():
    cfg = clip_ref.TINY_CLIP
    sd, m, _ = _models('clip', 'tiny', 0)
    assert m.hip_precision == 'full' and m._handle.lib.sdmi_clip_precision(m._handle.h) == 1
    pin = _pin(CLIP_MEASURED, 'tiny_props', 0, CLIP_HARD)
    ids = clip_ref.make_clip_ids(cfg, 4, 77, seed=3).cuda()
    a = m.encode_ids(ids)
    assert torch.equal(a, m.encode_ids(ids))
    ids2 = ids.clone(); ids2[:, 50] = (ids2[:, 50] + 1) % (cfg.vocab_size - 2)
    b = m.encode_ids(ids2)
    assert torch.equal(a[:, :50], b[:, :50]) and not torch.equal(a[:, 50:], b[:, 50:])
    one = m.encode_ids(ids[1:2])
    ref = clip_ref.clip_text_forward(_Double(sd), cfg, ids.cpu())
    d_one, d_ref = (one - a[1:2]).abs().max().item(), (a.double().cpu() - ref).abs().max().item()
    print(f'[text encoder full clip tiny props] vs fp64 max-abs {d_ref:.3e}, row alone vs in the batch {d_one:.3e} (pin {pin:.2e})', flush=True)
    assert d_one <= pin and d_ref <= pin


def test_bert_full_is_repeatable_and_batch_independent():
    cfg = bert_ref.TINY_BERT
    sd, m, _ = _models('bert', 'tiny', 0)
    assert m.hip_precision == 'full' and m._handle.lib.sdmi_bert_precision(m._handle.h) == 1
    pin = _pin(BERT_MEASURED, 'tiny_props', 0, BERT_HARD['tiny'])
    ids = bert_ref.make_bert_ids(cfg, 3, 77, seed=3).cuda()
    a = m(ids)
    assert torch.equal(a, m(ids))
    d_one = max((m(ids[b:b + 1]) - a[b:b + 1]).abs().max().item() for b in range(3))
    ids2 = ids.clone()
    ids2[1, 60] = (ids2[1, 60] + 1) % cfg.vocab_size
    c = m(ids2)
    assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2]) and not torch.equal(a[1, :60], c[1, :60])
    with torch.no_grad():
        ref = bert_ref.bert_forward(_Double(sd), cfg, ids.cpu())
    d_ref = (a.double().cpu() - ref).abs().max().item()
    print(f'[text encoder full bert tiny props] vs fp64 max-abs {d_ref:.3e}, a row alone vs in the batch {d_one:.3e} (pin {pin:.2e})', flush=True)
    assert d_one <= pin and d_ref <= pin


def test_full_text_interface_and_refusals():
    cfg = clip_ref.TINY_CLIP
    _, m, _ = _models('clip', 'tiny', 0)
    z = m.encode(['a photograph of an astronaut riding a horse', ''])
    assert z.shape == (2, 77, cfg.hidden_size) and torch.isfinite(z).all()
    assert torch.equal(z, m(['a photograph of an astronaut riding a horse', '']))
    bcfg = bert_ref.TINY_BERT

    class _Tok:
        def __call__(self, text, truncation=True, max_length=77, padding='max_length', return_tensors='pt', **kw):
            text = [text] if isinstance(text, str) else list(text)
            ids = torch.zeros((len(text), max_length), dtype=torch.long)
            for i, s in enumerate(text):
                toks = [101] + [103 + (b * 37) % (bcfg.vocab_size - 103) for b in s.encode()][:max_length - 2] + [102]
                ids[i, :len(toks)] = torch.tensor(toks)
            return {'input_ids': ids}

    from stable_diffusion_amd import BERTEmbedderHIP
    sd, _, _ = _models('bert', 'tiny', 0)
    mb = BERTEmbedderHIP(**bcfg.embedder_kwargs(), tokenizer=_Tok(), hip_precision='full')
    mb.load_state_dict({'transformer.' + k: v for k, v in sd.items()}, strict=True)
    mb = mb.cuda()
    text = ['a painting of a virus monster playing guitar', '']
    zb = mb.encode(text)
    assert zb.shape == (2, 77, bcfg.dim) and torch.equal(zb, mb(text))
    with torch.no_grad():
        ref = bert_ref.bert_forward(_Double(sd), bcfg, _Tok()(text)['input_ids'])
    d_ref = (zb.double().cpu() - ref).abs().max().item()
    print(f'[text encoder full bert tiny encode(text)] vs fp64 max-abs {d_ref:.3e}', flush=True)
    assert d_ref <= _pin(BERT_MEASURED, 'tiny_props', 0, BERT_HARD['tiny'])
    for mod, vocab in ((m, cfg.vocab_size), (mb, bcfg.vocab_size)):
        with pytest.raises(RuntimeError, match='no CPU'):
            mod.encode_ids(torch.zeros(1, 77, dtype=torch.long))
        with pytest.raises(IndexError):
            mod.encode_ids(torch.full((1, 77), vocab, dtype=torch.long, device='cuda'))
        with pytest.raises(ValueError):
            mod.encode_ids(torch.zeros(1, 78, dtype=torch.long, device='cuda'))


def test_mixed_keyword_is_the_default_path_bit_for_bit():
    """hip_precision='mixed' == no argument == a handle from sdmi_clip_create / sdmi_bert_create, the entry points from before the keyword"""
    import ctypes as C
    from stable_diffusion_amd import BERTEmbedderHIP, FrozenCLIPEmbedderHIP
    cfg = clip_ref.TINY_CLIP
    sd, _, mixed = _models('clip', 'tiny', 0)
    ids = clip_ref.make_clip_ids(cfg, 2, 77, seed=4).cuda()
    outs = [mixed.encode_ids(ids)]
    for kw in ({}, {'hip_precision': 'mixed'}):
        m = FrozenCLIPEmbedderHIP(text_config=_text_config(cfg), tokenizer=_FakeTokenizer(cfg.vocab_size), **kw)
        m.load_state_dict({'transformer.' + k: v for k, v in sd.items()}, strict=False)
        if not kw:                                     # the handle the module made before this mode existed
            lib, h = m._handle.lib, C.c_void_p()
            lib.sdmi_clip_destroy(m._handle.h)
            _lib.check(lib.sdmi_clip_create(C.byref(m._cfg), C.byref(h)))
            m._handle.h = h
        outs.append(m.cuda().encode_ids(ids))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    bcfg = bert_ref.TINY_BERT
    bsd, _, bmixed = _models('bert', 'tiny', 0)
    bids = bert_ref.make_bert_ids(bcfg, 2, 77, seed=4).cuda()
    want = bmixed(bids)
    for kw in ({}, {'hip_precision': 'mixed'}):
        m = BERTEmbedderHIP(**bcfg.embedder_kwargs(), use_tokenizer=False, **kw)
        m.load_state_dict({'transformer.' + k: v for k, v in bsd.items()}, strict=True)
        if not kw:
            lib, h = m._handle.lib, C.c_void_p()
            lib.sdmi_bert_destroy(m._handle.h)
            _lib.check(lib.sdmi_bert_create(C.byref(m._cfg), C.byref(h)))
            m._handle.h = h
        assert torch.equal(want, m.cuda()(bids))


# ---- the activation producers ------------------------------------------------------------------------------------------------------------
def _ulp16(y):
    """the fp16 spacing at |y| (float64 in, float64 out; the subnormal spacing below 2^-14)"""
    a = y.abs().clamp_min(2.0 ** -14)
    return 2.0 ** (torch.floor(torch.log2(a)) - 10)


# worst |hi + lo - f(x)| in fp16 ulps of f(x) over the 4096 points, measured on an MI355X; bar = 1.25 x
ACT_MEASURED = {'quick_gelu': 0.4999, 'gelu_erf': 0.4970}


@pytest.mark.parametrize('name', ['quick_gelu', 'gelu_erf'])
def test_activation_producers(name):
    """4096 values over [-12, 12] with 0 and -0: hi is the fp16 kernel's output bit for bit, hi + lo against the fp64 function in fp16 ulps of
    the result, bar 1.25 x measured, and the bar itself must be below one fp16 ulp.

    quick_gelu: lo = fp16(y - hi) is a low half (at most half a step of hi).  gelu_erf: the shared `gelu_erf` (igemm_dev.h; Abramowitz-Stegun,
    1.5e-7 absolute on erf, 1 + erf cancelling for negative x) is up to 2.06 fp16 ulps off around x = -4.04 (f = -1.08e-4) -- measured here
    with lo = fp16(y - hi), where hi + lo missed the one-ulp bar; tests/test_bert_gpu.py pins the same 2 ulp on the fp16 kernel.  hi keeps
    those bits, and lo is taken against the erfc form of the function instead, so it is up to 2.6 steps of hi there and the sum is the GELU.
    Both sums reach half an ulp only where the result is an fp16 subnormal (the low half underflows)."""
    lib = _lib.load()
    x = torch.cat([torch.linspace(-12, 12, 4092, dtype=torch.float32), torch.tensor([0.0, -0.0, 12.0, -12.0])])
    assert x.numel() == 4096 and bool((x == 0).sum() >= 2)
    pool = guard.Pool(DEV)
    xd = pool.put('x', x.to(DEV))
    hi, lo, h16 = (pool.new(n, (4096,), torch.float16) for n in ('hi', 'lo', 'f16'))
    split, plain = ((lib.sdmi_k_quick_gelu_split, lib.sdmi_k_quick_gelu) if name == 'quick_gelu' else
                    (lib.sdmi_k_gelu_erf_split, lib.sdmi_k_gelu_erf))
    _lib.check(split(xd.data_ptr(), hi.data_ptr(), lo.data_ptr(), 4096, _lib.stream_ptr()))
    _lib.check(plain(xd.data_ptr(), h16.data_ptr(), 4096, _lib.stream_ptr()))
    torch.cuda.synchronize()
    pool.check(name)
    x64 = x.double()
    ref = x64 * torch.sigmoid(1.702 * x64) if name == 'quick_gelu' else F.gelu(x64)
    got = hi.double().cpu() + lo.double().cpu()
    ulps = (got - ref).abs() / _ulp16(ref)
    worst, at = float(ulps.max()), int(ulps.argmax())
    bar = 1.25 * ACT_MEASURED[name]
    print(f'[{name} split] worst |hi + lo - f(x)| = {worst:.4f} fp16 ulp of f(x) at x = {float(x[at]):.4f} (f = {float(ref[at]):.4e}); '
          f'bar {bar:.4f}', flush=True)
    # hi is the fp16 kernel's output bit for bit; lo is a low half
    assert torch.equal(hi.view(torch.int16), h16.view(torch.int16))
    lo_steps = float((lo.double().cpu().abs() / _ulp16(hi.double().cpu())).max())
    print(f'[{name} split] largest |lo| = {lo_steps:.4f} fp16 steps of hi', flush=True)
    assert bool(torch.isfinite(lo.float()).all()) and lo_steps <= (0.5 if name == 'quick_gelu' else 2.6) * (1 + 2.0 ** -10)
    zeros = got[x == 0]
    assert zeros.numel() >= 2 and bool((zeros == 0).all())
    assert bar < 1.0            # by construction of the split: hi + lo carries the fp32 value, far below one fp16 ulp
    assert worst <= bar
    bad = torch.empty(8, device=DEV)
    assert split(bad.data_ptr(), hi.data_ptr(), lo.data_ptr(), 6, _lib.stream_ptr()) != 0          # n % 4 refused


# ---- the split-fp16 GEMM at text-encoder row counts ---------------------------------------------------------------------------------------
# worst max-abs / max|out| of the split-fp16 GEMM against fp64 over the 12 shapes x {bias, bias + in-place residual} x {no split-K, auto},
# measured on an MI355X; bar = 1.25 x
GEMM_MEASURED = 7.790e-7


@pytest.mark.parametrize('Kd', [128, 512])
@pytest.mark.parametrize('N', [128, 384])
@pytest.mark.parametrize('M', [77, 120, 154])
def test_split16_gemm_at_text_row_counts(M, N, Kd):
    """M = L, an odd multiple of nothing, 2 L: no multiple of the 64-row tile.  fp32 operands; the split-fp16 GEMM sees hi / lo and the packed
    [hi | hi | lo] weights, the single-pass GEMM their fp16 roundings; both against the fp64 product of the fp32 values."""
    g = torch.Generator().manual_seed(5000 + 7 * M + 3 * N + Kd)
    x = torch.randn((M, Kd), generator=g)
    w = torch.randn((N, Kd), generator=g) / Kd ** 0.5
    bias = torch.randn((N,), generator=g) * 0.05
    res = torch.randn((M, N), generator=g)
    prod = x.double() @ w.double().t() + bias.double()
    w3 = K.pack_split3(w.to(DEV))
    w16 = K.pack_conv_weight(w.to(DEV).view(N, Kd, 1, 1))
    worst, worst16 = 0.0, 0.0
    for residual in (False, True):
        ref = prod + (res.double() if residual else 0)
        scale = float(ref.abs().max())
        for splitk in (1, 0):
            pool = guard.Pool(DEV)
            hi, lo = pool.put('a_hi', x.half().to(DEV)), pool.put('a_lo', (x - x.half().float()).half().to(DEV))
            w3g, bg = pool.put('w3', w3), pool.put('bias', bias.to(DEV))
            out = pool.new('out', (M, N), torch.float32)
            if residual:
                out.copy_(res)
            ws = pool.new('ws', (1 << 20,), torch.float32) if splitk == 0 else None
            cnt = pool.new('cnt', (8192,), torch.int32, fill=0) if splitk == 0 else None
            K.igemm(hi, w3g, N, 1, M, 1, M, 1, a1=lo, bias=bg, residual=out if residual else None, out_f32=out, splitk=splitk, split16=True,
                    ws=ws, cnt=cnt)
            torch.cuda.synchronize()
            tag = f'split16 gemm M{M} N{N} K{Kd} residual {residual} splitk {splitk}'
            pool.check(tag)
            assert bool(torch.isfinite(out).all()), tag
            worst = max(worst, float((out.double().cpu() - ref).abs().max()) / scale)
        out16 = torch.empty((M, N), device=DEV)
        if residual:
            out16.copy_(res)
        K.igemm(x.half().to(DEV), w16, N, 1, M, 1, M, 1, bias=bias.to(DEV), residual=out16 if residual else None, out_f32=out16)
        torch.cuda.synchronize()
        worst16 = max(worst16, float((out16.double().cpu() - ref).abs().max()) / scale)
    bar = 1.25 * GEMM_MEASURED
    print(f'[split16 gemm M{M} N{N} K{Kd}] max-abs / max|out| {worst:.3e} (single-pass fp16 GEMM {worst16:.3e}, ratio {worst16 / worst:.0f}); '
          f'bar {bar:.3e}', flush=True)
    assert bar <= 0.1 * worst16
    assert worst <= bar
