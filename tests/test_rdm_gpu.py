"""The retrieval-augmented UNet (configs/retrieval-augmented-diffusion/768x768.yaml) and layout-to-image's on the MI355X: SpatialTransformers
whose heads come from num_head_channels = 32 (14 / 28 / 42 / 56 heads), widths 448 / 896 / 1344 / 1792, 16 latent channels in and out.

Kernels against fp64 in guarded buffers (tests/guard.py) at the bars tests/test_model_shapes_gpu.py holds for the same launch kind (its
helpers are imported, not restated; B = 2): the output head for 9 .. 16 channels on both of its forms, conv_in at 16 input channels, the
3x3 convs / 1x1 convs / dense GEMMs at every width and concat pair of the model on an 8 x 8 and a 6 x 6 map (M = 72 is a multiple of no
tile height) at the executor's own tile and split request in both precisions, with GroupNorm-statistics targets at 14 .. 112 channels per
group; GroupNorm stand-alone at the same pairs; LayerNorm at the four widths, folded where the executor's guard admits it; attention at
head dim 32 with 14 .. 56 heads, self and over 1 / 11 / 21 context tokens, mixed and split-fp16.
Whole UNets against goldens of the reference's own UNetModel (tools/make_golden_rdm.py): full at 2e-5, mixed at 1e-3, every case; the
fixture's fp16-operand floor (computed from the reference) is printed beside the error.  A case measured above 1e-3 would go into
FLOOR_CASES and be held to 1.25 x its floor (README's rule of the outlier family); the list is empty.  Launch tapes replayed across timesteps and shapes.  The body of scripts/knn2img.py up to samples_ddim against the
reference DDIM loop at the fixture's bar.  Packed blobs."""
import contextlib
import ctypes as C
import io
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import kernels as K  # noqa: E402
import test_ln_fold_gpu as LNF  # noqa: E402  (its _Stream helper: the fold's producers and consumers with their references and bars)
import test_model_shapes_gpu as TMS  # noqa: E402  (helpers and bars only: _Case, _conv_ref64, _tol32, _tol_split, _report, ...)
from stable_diffusion_amd import _lib, synthetic  # noqa: E402

DEV = 'cuda'
B = TMS.B
MIXED_TOL = 1e-3        # tests/test_faces_gpu.py: the project's one mixed-precision bar
FULL_TOL = 2e-5         # ... and its full-mode bar
WIDTHS = [448, 896, 1344, 1792]
# (h | skip) -> N of the output ResBlocks, in execution order back to front (csrc/unet.cpp UNet::build)
CONCATS = [(448, 448, 448), (896, 448, 448), (896, 896, 896), (1344, 896, 896), (1344, 1344, 1344), (1792, 1344, 1344), (1792, 1792, 1792)]
CASES = {'rdm64': ['8x8_b2', '48x48_b1', '16x16_b10', '16x16_b2_ctx1', '16x16_b2_ctx0'], 'rdm448x2': ['8x8_b2', '24x24_b1'],
         'rdm320x1': ['16x16_b2'], 'layout': ['8x8_b2', '32x32_b1']}
FLOOR_CASES = ()        # (tag, case) measured above MIXED_TOL in mixed precision: none
_models = {}


# ---- the output head for 9 .. 16 channels ---------------------------------------------------------------------------------------
def _conv_out_guarded(P, h, w, b, Bn, H, W):
    Cout, Cin = w.shape[0], w.shape[1]
    lib = _lib.load()
    w_d = P.put('w', w)
    wp = P.new('w_ohwi', (Cout, 3, 3, Cin), torch.float32)
    _lib.check(lib.sdmi_k_pack_conv_out(w_d.data_ptr(), wp.data_ptr(), Cout, Cin, _lib.stream_ptr()))
    out = P.new('out', (Bn, Cout, H, W), torch.float32)
    rc = lib.sdmi_k_conv_out(h.data_ptr(), wp.data_ptr(), b.data_ptr(), out.data_ptr(), Bn, H, W, Cin, Cout, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, wp


@pytest.mark.parametrize('Cin', [64, 448, 512, 576])
def test_conv_out_9_to_16_channels_vs_fp64(Cin):
    """W % 4 == 0 and Cin <= 512 take the 4-pixel form (both channel passes at 448 / 512, one at 64), everything else -- (1, 1), (3, 6),
    Cin = 576 -- the one-wave-per-pixel form; 9 and 12 outputs leave the upper half of 8 partly empty.  Bar _tol32(9 Cin)."""
    tol = TMS._tol32(9 * Cin)
    errs = []
    for Cout in (9, 12, 16):
        for H, W in ((1, 1), (3, 6), (8, 8), (2, 48)):
            g = TMS._g(TMS._seed(Cin, Cout, H, W, 1))
            P = guard.Pool(DEV)
            h = P.put('h', TMS._randn((B, H * W, Cin), g))
            w = TMS._randn((Cout, Cin, 3, 3), g, 1.0 / math.sqrt(9 * Cin))
            b = P.put('bias', TMS._randn((Cout,), g, 0.1))
            keep = h.clone(), b.clone()
            rc, out, wp = _conv_out_guarded(P, h, w, b, B, H, W)
            _lib.check(rc)
            wp_keep = wp.clone()
            ref = (TMS._conv_ref64(h.reshape(B * H * W, Cin), w, B, H, W, 3, 1, 0) + b.double()[None]).reshape(B, H, W, Cout)
            tag = f'conv_out {Cin}->{Cout} {H}x{W}'
            errs.append(TMS._report(tag, out.permute(0, 2, 3, 1), ref, tol))
            P.check(tag)
            assert torch.equal(h, keep[0]) and torch.equal(b, keep[1]) and torch.equal(wp, wp_keep), f'{tag}: an input was modified'
    assert max(errs) < tol, (errs, tol)


def test_conv_out_17_channels_is_refused():
    P = guard.Pool(DEV)
    g = TMS._g(17)
    h = P.put('h', TMS._randn((B, 64, 64), g))
    b = P.put('bias', TMS._randn((17,), g))
    rc, out, _ = _conv_out_guarded(P, h, TMS._randn((17, 64, 3, 3), g), b, B, 8, 8)
    assert rc != 0 and b'out_channels <= 16' in _lib.load().sdmi_last_error()
    P.check('conv_out 17')
    assert bool(torch.isnan(out).all())          # (nothing was launched: the output keeps its poison)


@pytest.mark.parametrize('Cout', [8, 4, 3])
def test_conv_out_up_to_8_channels_is_unchanged(Cout):
    """the heads every other model uses keep their kernels: the same bar as tests/test_model_shapes_gpu.py::test_conv_out"""
    g = TMS._g(TMS._seed(Cout, 320))
    P = guard.Pool(DEV)
    h = P.put('h', TMS._randn((B, 64, 320), g))
    w = TMS._randn((Cout, 320, 3, 3), g, 1.0 / math.sqrt(9 * 320))
    b = P.put('bias', TMS._randn((Cout,), g, 0.1))
    rc, out, _ = _conv_out_guarded(P, h, w, b, B, 8, 8)
    _lib.check(rc)
    ref = (TMS._conv_ref64(h.reshape(B * 64, 320), w, B, 8, 8, 3, 1, 0) + b.double()[None]).reshape(B, 8, 8, Cout)
    e = TMS._report(f'conv_out 320->{Cout}', out.permute(0, 2, 3, 1), ref, 2e-5)
    P.check('conv_out <= 8')
    assert e < 2e-5


@pytest.mark.parametrize('hw', [8, 6])
def test_conv_in_16_channels_vs_fp64(hw):
    """conv_in sits on its bound (K = 144 = the kernel's patch width); bar of tests/test_model_shapes_gpu.py::test_conv_in"""
    Cin, Cout = 16, 448
    g = TMS._g(TMS._seed(Cin, Cout, hw))
    P = guard.Pool(DEV)
    x = P.put('x', TMS._randn((B, Cin, hw, hw), g))
    w = P.put('w', TMS._randn((Cout, Cin, 3, 3), g, 1.0 / math.sqrt(9 * Cin)))
    b = P.put('bias', TMS._randn((Cout,), g, 0.1))
    out = P.new('out', (B, hw * hw, Cout), torch.float32)
    _lib.check(_lib.load().sdmi_k_conv_in(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), B, Cin, hw, hw, Cout, _lib.stream_ptr()))
    torch.cuda.synchronize()
    ref = TMS._conv_ref64(x.permute(0, 2, 3, 1).reshape(B * hw * hw, Cin), w, B, hw, hw, 3, 1, 0) + b.double()[None]
    e = TMS._report(f'conv_in 16->{Cout} hw{hw}', out, ref, 2e-5)
    P.check('conv_in 16')
    assert e < 2e-5


# ---- GEMMs and convs at the model's widths -----------------------------------------------------------------------------------------
def _run_both_precisions(name, kw, split):
    """the executor's request (tile -1, splitk 0) on fp16 operands and on the split-fp16 form of the full-precision mode"""
    res = [TMS._Case(name, **kw).run(-1, 0, as_executor=True)]
    res.append(TMS._Case(name + ' split', **dict(kw, **{split: True})).run(-1, 0, want16=False, as_executor=True))
    for errs, st in res:
        TMS._assert_case(errs, st)


@pytest.mark.parametrize('hw', [8, 6])
@pytest.mark.parametrize('c0,c1,N', CONCATS, ids=[f'{a}|{b}-{n}' for a, b, n in CONCATS])
def test_concat_conv3_and_skip_vs_fp64(c0, c1, N, hw):
    """in_layers' 3x3 conv of an output ResBlock over the (h | skip) concat -- K = 9 (c0 + c1) up to 32 256 -- with the embedding row and
    the statistics of out_layers' GroupNorm (N / 32 = 14 .. 56 channels per group), and the block's 1x1 skip convolution"""
    st = [(N // 32, 0)] if (hw * hw) % 32 == 0 else []          # (the epilogue statistics need H W % 32 == 0: the 6 x 6 map runs the kernel)
    conv = dict(c0=c0, c1=c1, N=N, Hin=hw, Win=hw, Hout=hw, Wout=hw, ksize=3, rowvec=True, gn=st)
    _run_both_precisions(f'conv1 {c0}|{c1}->{N} hw{hw}', conv, 'split3')
    skip = dict(c0=c0 + c1, c1=0, N=N, Hin=hw, Win=hw, Hout=hw, Wout=hw, resid=True, gn=st, bare_as_executor=True)
    _run_both_precisions(f'skip {c0 + c1}->{N} hw{hw}', skip, 'split16')


@pytest.mark.parametrize('hw', [8, 6])
@pytest.mark.parametrize('C_', WIDTHS)
def test_conv3_at_every_width_vs_fp64(C_, hw):
    """out_layers' 3x3 conv (residual epilogue) at one width; its output is read by the next block's GroupNorm (C / 32 per group) and,
    from the skip stack, as the SECOND source of a concat GroupNorm: (c0 + C) / 32 = 28 .. 112 channels per group at offset c0"""
    c0 = {448: 896, 896: 1344, 1344: 1792, 1792: 1792}[C_]
    st = [(C_ // 32, 0), ((c0 + C_) // 32, c0)] if (hw * hw) % 32 == 0 else []      # (epilogue statistics need H W % 32 == 0)
    kw = dict(c0=C_, c1=0, N=C_, Hin=hw, Win=hw, Hout=hw, Wout=hw, ksize=3, resid=True, gn=st)
    _run_both_precisions(f'conv2 {C_} hw{hw}', kw, 'split3')
    if C_ == 448 and st:          # ... and as the FIRST source of the last concat (448 | 448: 28 per group)
        TMS._assert_case(*TMS._Case('conv2 448 first', **dict(kw, gn=[(28, 0)])).run(-1, 0, as_executor=True))


@pytest.mark.parametrize('ntok', [64, 36])
@pytest.mark.parametrize('C_', WIDTHS)
def test_transformer_gemms_vs_fp64(C_, ntok):
    """the dense GEMMs of a BasicTransformerBlock at one width: an out-projection (K = C, in place on the token stream), FF-out
    (K = 4 C up to 7168, in place), proj_out with the statistics of the next GroupNorm, and the GEGLU projection (8 C columns, up to 14 336)"""
    dense = dict(c1=0, N=C_, Hin=ntok, Win=1, Hout=ntok, Wout=1)
    _run_both_precisions(f'attn_out {C_} ntok{ntok}', dict(dense, c0=C_, resid=True, inplace=True), 'split16')
    _run_both_precisions(f'ff2 {4 * C_}->{C_} ntok{ntok}', dict(dense, c0=4 * C_, resid=True, inplace=True), 'split16')
    _run_both_precisions(f'proj_out {C_} ntok{ntok}', dict(dense, c0=C_, resid=True, gn=[(C_ // 32, 0)] if ntok % 32 == 0 else []), 'split16')
    M, N = B * ntok, 8 * C_
    g = TMS._g(TMS._seed(M, C_, N))
    a = TMS._r16((M, C_), g)
    w = TMS._r16((N, C_), g, 1.0 / math.sqrt(C_))
    b = TMS._randn((N,), g, 0.1)
    val, gate = (a.double() @ w.double().t() + b.double()).chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    P = guard.Pool(DEV)
    wp, bp = K.pack_geglu(w.float(), b)
    a_d, wp, bp = P.put('a', a), P.put('w', wp), P.put('bias', bp)
    out = P.new('out', (M, N // 2), torch.float16)
    K.igemm(a_d, wp, N, B, ntok, 1, ntok, 1, bias=bp, out_f16=out, mode=1, tile=-1)
    torch.cuda.synchronize()
    e = TMS._report(f'geglu {C_}->{N} ntok{ntok}', out, ref, 4e-3)
    P.check('geglu')
    assert e < 4e-3          # (tests/test_model_shapes_gpu.py::test_geglu)


@pytest.mark.parametrize('L', [1, 11, 21])
@pytest.mark.parametrize('C_', WIDTHS)
def test_context_kv_projection_vs_fp64(C_, L):
    """K | V of the cross-attention from 768 context channels: 2 C columns, B L = 2 / 22 / 42 rows, fp16 and split-fp16 operands"""
    kw = dict(c0=768, c1=0, N=2 * C_, Hin=L, Win=1, Hout=L, Wout=1, bias=False)
    _run_both_precisions(f'kv 768->{2 * C_} L{L}', kw, 'split16')


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------
GN_PAIRS = [(c, 0) for c in WIDTHS] + [(a, b) for a, b, _ in CONCATS]


@pytest.mark.parametrize('HW', [1, 36, 576])
@pytest.mark.parametrize('c0,c1', GN_PAIRS, ids=[f'{a}|{b}' for a, b in GN_PAIRS])
def test_groupnorm_vs_fp64(c0, c1, HW):
    """14 / 28 / 42 / 56 channels per group and 28 .. 112 over the concats (3584 channels): groups that straddle the seam between the two
    sources (1344 | 896: 70 per group, the seam is inside group 19); bars of tests/test_model_shapes_gpu.py::test_groupnorm"""
    g = TMS._g(TMS._seed(c0, c1, HW, 3))
    C_ = c0 + c1
    P = guard.Pool(DEV)
    x0 = P.put('x0', TMS._randn((B, HW, c0), g, 1.5) + 0.3)
    x1 = P.put('x1', TMS._randn((B, HW, c1), g, 0.7) - 0.2) if c1 else None
    gamma = P.put('gamma', 1 + 0.1 * TMS._randn((C_,), g))
    beta = P.put('beta', 0.1 * TMS._randn((C_,), g))
    x = x0 if x1 is None else torch.cat([x0, x1], dim=2)
    x64 = x.double().reshape(B, HW, 32, C_ // 32)
    mean = x64.mean((1, 3), keepdim=True)
    var = ((x64 - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((x64 - mean) / torch.sqrt(var + 1e-5)).reshape(B, HW, C_) * gamma.double() + beta.double()
    ref = y * torch.sigmoid(y)
    o = TMS._groupnorm_guarded(P, x0, x1, gamma, beta, 1e-5, 1)
    tag = f'groupnorm {c0}|{c1} HW{HW}'
    e = [(TMS._report(f'{tag} f32', o['f32'], ref, 2e-5), 2e-5), (TMS._report(f'{tag} f16', o['f16'], ref, 4e-3), 4e-3),
         (TMS._report(f'{tag} raw', o['raw'], x, 4e-3), 4e-3),
         (TMS._report(f'{tag} hi+lo', o['f16'].float() + o['lo'].float(), o['f32'], 4e-6), 4e-6),
         (TMS._report(f'{tag} raw hi+lo', o['raw'].float() + o['raw_lo'].float(), x, 4e-6), 4e-6)]
    P.check(tag)
    for err, tol in e:
        assert err < tol, (tag, err, tol)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [2, 72, 288, 1152])
@pytest.mark.parametrize('C_', WIDTHS)
def test_layernorm_vs_fp64(C_, rows):
    """the stand-alone kernel (what 1344 / 1792 and the 1 / 36 / 144-token levels run): fp16 out against fp64.  Bar: the output is
    N(0, 1) * gamma + beta, below 8 in magnitude, stored as fp16 -- half an ulp there is 2^-9 = 2.0e-3 -- plus the fp32 arithmetic (1e-5)"""
    g = TMS._g(TMS._seed(C_, rows, 5))
    P = guard.Pool(DEV)
    x = P.put('x', TMS._randn((rows, C_), g, 1.5) + 0.3)
    gamma = P.put('gamma', 1 + 0.1 * TMS._randn((C_,), g))
    beta = P.put('beta', 0.1 * TMS._randn((C_,), g))
    out = P.new('out', (rows, C_), torch.float16)
    keep = x.clone()
    _lib.check(_lib.load().sdmi_k_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, C_, 1e-5, _lib.stream_ptr()))
    torch.cuda.synchronize()
    x64 = x.double()
    mu = x64.mean(1, keepdim=True)
    ref = (x64 - mu) / torch.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + 1e-5) * gamma.double() + beta.double()
    assert float(ref.abs().max()) < 8.0
    tol = 2.0 ** -9 + 1e-5
    e = TMS._report(f'layernorm C{C_} rows{rows}', out, ref, tol)
    P.check('layernorm')
    assert torch.equal(x, keep) and e < tol


@pytest.mark.parametrize('C_', [448, 896])
def test_layernorm_fold_at_the_widths_that_take_it(C_):
    """C <= 1280 with 576 tokens per sample (rows 1152) is what the executor folds in this model (448 at 2304 / 576 tokens, 896 at 576):
    the producer / consumer comparisons of tests/test_ln_fold_gpu.py (its _Stream: guarded buffers, fp64 references, its own bars) at the
    dispatch request, 14 and 28 partial blocks per row, on its four distributions -- the fp16 and the in-place out-projection producers,
    the split-fp16 proj_in form, and the consumers q | k | v at head dim 32, GEGLU and a plain projection"""
    for dist in LNF.DISTS:
        s = LNF._Stream(C_, 2, 576, dist)
        x, a16, part = s.produce('f16', -1)
        xi, a16i, parti = s.produce('f16-inplace', -1)
        assert torch.equal(x, xi) and torch.equal(a16, a16i) and torch.equal(part, parti), f'{s.tag}: in place != out of place'
        s.prepare(x, a16, part)
        s.consume('heads', x, a16, part, dh=32)
        s.consume('geglu', x, a16, part)
        s.consume('plain', x, a16, part)
        xs, a16s, parts = s.produce('split16', -1)              # proj_in's form feeds norm1 -> q | k | v
        s.prepare(xs, a16s, parts, kinds=('heads',))
        s.consume('heads', xs, a16s, parts, dh=32, src='split16')


# ---- attention at head dim 32 ----------------------------------------------------------------------------------------------------------
def _attn_d32(heads, nq, nkv, full, zero_kv=False):
    d = 32
    g = TMS._g(TMS._seed(heads, nq, nkv, 32))
    BH, nkp, scale = B * heads, (nkv + 7) // 8 * 8, d ** -0.5
    q, k, v = TMS._randn((BH, nq, d), g), TMS._randn((BH, nkv, d), g), TMS._randn((BH, nkv, d), g)
    if zero_kv:
        k, v = torch.zeros_like(k), torch.zeros_like(v)
    vt = torch.zeros((BH, d, nkp), device=DEV)
    vt[:, :, :nkv] = v.transpose(1, 2)
    lib = _lib.load()
    P = guard.Pool(DEV)
    out = P.new('out', (B, nq, heads * d), torch.float16)
    tag = f'attention d32 h{heads} nq{nq} nkv{nkv} {"split16" if full else "mixed"}'
    if full:
        ops = []
        for nm, t in (('q', q), ('k', k), ('vt', vt)):
            hi, lo = K.cast_f16(t.contiguous(), want_lo=True)
            ops += [P.put(nm, hi), P.put(nm + '_lo', lo)]
        out_lo = P.new('out_lo', (B, nq, heads * d), torch.float16)
        _lib.check(lib.sdmi_k_attention_split16(*[o.data_ptr() for o in ops], out.data_ptr(), out_lo.data_ptr(), BH, heads, nq, nkv, nkp, d,
                                                float(scale), _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = out.double() + out_lo.double()
        ref = TMS._attn_ref64(q, k, v, heads, scale)
        err, bar = float((got - ref).abs().max()), 1e-5 * max(float(ref.abs().max()), 1e-30)       # (test_attention: max-abs / max|O| <= 1e-5)
    else:
        qh, kh, vh = P.put('q', q.half()), P.put('k', k.half()), P.put('vt', vt.half())
        _lib.check(lib.sdmi_k_attention(qh.data_ptr(), kh.data_ptr(), vh.data_ptr(), out.data_ptr(), BH, heads, nq, nkv, nkp, d, float(scale),
                                        _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = out.double()
        ref = TMS._attn_ref64(qh, kh, vh[:, :, :nkv].transpose(1, 2), heads, scale)
        err, bar = float((got - ref).abs().max()), 4e-3
    print(f'[{tag}] max-abs {err:.3e} (bar {bar:.1e})', flush=True)
    P.check(tag)
    assert bool(torch.isfinite(got).all())
    return got, err, bar


@pytest.mark.parametrize('full', [False, True], ids=['mixed', 'split16'])
@pytest.mark.parametrize('heads', [14, 28, 42, 56])
def test_attention_d32_vs_fp64(heads, full):
    """self-attention at the token counts of the 48 x 48 and the 8 x 8 latent's levels, cross-attention over knn 0 / 10 / 20"""
    res = [_attn_d32(heads, n, n, full)[1:] for n in (1, 4, 36, 144, 576)]
    res += [_attn_d32(heads, nq, nkv, full)[1:] for nq in (36, 576) for nkv in (1, 11, 21)]
    for err, bar in res:
        assert err <= bar, (err, bar)


@pytest.mark.parametrize('full', [False, True], ids=['mixed', 'split16'])
def test_attention_over_a_zero_context_is_exactly_zero(full):
    """uc = zeros_like(c): every key and value is zero, the softmax is uniform and the output is 0 -- not a rounding of it"""
    got, _, _ = _attn_d32(14, 36, 11, full, zero_kv=True)
    assert int((got != 0).sum()) == 0


# ---- the UNets against the reference goldens ------------------------------------------------------------------------------------
def _unet(tag, prec, **over):
    key = (tag, prec, tuple(sorted(over.items())))
    if key not in _models:
        for k in [k for k in _models if k[0] != tag]:       # (one model family on the device at a time)
            del _models[k]
        torch.cuda.empty_cache()
        from stable_diffusion_amd import UNetModelHIP
        m = UNetModelHIP(**dict(synthetic.RDM_STANDINS[tag], **over), hip_precision=prec)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models[key] = m.cuda()
    return _models[key]


def _inputs(z, kw):           # (tools/make_golden_rdm.py unet_inputs / context_inputs)
    b, h, w = int(z['batch']), int(z['h']), int(z['w'])
    x = torch.randn(b, kw['in_channels'], h, w, generator=torch.Generator().manual_seed(int(z['input_seed'])))
    t = torch.tensor([int(v) for v in z['t']], dtype=torch.int64)
    L = int(z['ctx_tokens'])
    if str(z['ctx_kind']) == 'zero':
        c = torch.zeros(b, L, kw['context_dim'])
    else:
        c = torch.randn(b, L, kw['context_dim'], generator=torch.Generator().manual_seed(int(z['ctx_seed'])))
    return x.cuda(), t.cuda(), c.cuda()


@pytest.mark.parametrize('prec', ['mixed', 'full'])
@pytest.mark.parametrize('tag,case', [(t, c) for t in CASES for c in CASES[t]])
def test_unet_matches_reference(tag, case, prec, golden_dir):
    """rdm64 8x8_b2: the smallest legal latent (64 / 16 / 4 / 1 tokens); 48x48_b1: the native latent (2304 / 576 / 144 / 36 tokens: the
    LayerNorm fold on at the first two levels); 16x16_b10: the 8 + 2 chunking, 21 context tokens; ctx1: the one-token copy shortcut with
    heads from num_head_channels; ctx0: the all-zero unconditional context.  rdm448x2: the real 14 / 28 heads and 14 .. 56 channels per
    group.  rdm320x1: 10 heads of 32 at the one width whose SpatialTransformer runs as row-strip chain launches (st_head, st_mid, the
    FF tail; 512 token rows: the fold is on).  layout: transformer_depth 3 over 92 tokens, three output channels"""
    z = np.load(os.path.join(golden_dir, f'{tag}_unet_{case}.npz'))
    assert int(z['weight_seed']) == 0
    x, t, c = _inputs(z, synthetic.RDM_STANDINS[tag])
    ref = torch.from_numpy(z['eps'])
    eps = _unet(tag, prec)(x, t, context=c)
    torch.cuda.synchronize()
    err = (eps.float().cpu() - ref).abs()
    mx, rms = float(err.max()), float(err.pow(2).mean().sqrt())
    floor = float(z['floor_maxabs'])
    tol = FULL_TOL if prec == 'full' else (max(MIXED_TOL, 1.25 * floor) if (tag, case) in FLOOR_CASES else MIXED_TOL)
    print(f'[{tag} unet {case} {prec}] max-abs {mx:.3e} rms {rms:.3e} |eps|max {ref.abs().max():.3f} (tol {tol:.2e}; fp16-operand floor {floor:.2e})',
          flush=True)
    assert eps.shape == ref.shape and bool(torch.isfinite(eps).all())
    assert mx <= tol


def test_zero_context_gives_the_bias_of_the_out_projection(golden_dir):
    """c = 0: the cross-attention adds exactly to_out's bias, whatever the queries are -- two different all-zero-context calls of one x
    differ in nothing, a zero context of another length gives the same eps bit for bit, and eps is finite"""
    z = np.load(os.path.join(golden_dir, 'rdm64_unet_16x16_b2_ctx0.npz'))
    x, t, c = _inputs(z, synthetic.RDM64_UNET_KWARGS)
    m = _unet('rdm64', 'mixed')
    a = m(x, t, context=c).clone()
    b = m(x, t, context=torch.zeros(2, 1, 768, device=DEV)).clone()          # (the one-token shortcut copies V = 0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def test_rdm_unet_tape_replay_across_timesteps_and_shapes():
    """a replayed tape must add the embedding row of ITS timestep, and a second shape gets its own tape"""
    m = _unet('rdm64', 'mixed')
    lib = m._handle.lib

    def stats():
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.sdmi_unet_tape_stats(m._handle.h, C.byref(a), C.byref(b)))
        return a.value, b.value
    ctx = torch.randn(2, 11, 768, generator=torch.Generator().manual_seed(9)).cuda()
    for hw in (16, 8):
        x = torch.randn(2, 16, hw, hw, generator=torch.Generator().manual_seed(5)).cuda()
        t981, t1 = torch.full((2,), 981, dtype=torch.long, device=DEV), torch.full((2,), 1, dtype=torch.long, device=DEV)
        with _env('SDMI_REPLAY', '0'):
            un981, un1 = m(x, t981, context=ctx).clone(), m(x, t1, context=ctx).clone()
        assert not torch.equal(un981, un1)
        m.cache_timesteps([981, 1])
        try:
            r0, c0 = stats()
            m.hint_timestep(981)
            a = m(x, t981, context=ctx).clone()
            r1, c1 = stats()
            m.hint_timestep(1)
            b = m(x, t1, context=ctx).clone()
            r2, c2 = stats()
            m.hint_timestep(981)
            c = m(x, t981, context=ctx).clone()
            r3, c3 = stats()
        finally:
            m.cache_timesteps([])
        torch.cuda.synchronize()
        assert (r1, c1) in ((r0, c0 + 1), (r0 + 1, c0)) and (r2, c2) == (r1 + 1, c1) and (r3, c3) == (r2 + 1, c2), ((r0, c0), (r1, c1), (r2, c2), (r3, c3))
        assert torch.equal(a, un981) and torch.equal(b, un1) and torch.equal(c, un981)


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def test_rdm_pipeline_matches_reference_loop(golden_dir):
    """The body of scripts/knn2img.py:357-377 up to samples_ddim on HIP classes: c = cat([text, nn]) of unit-norm rows, uc = zeros_like(c),
    DDIM at the script's default scale -- against the reference DDIMSampler loop on the CPU, at the fixture's bar: how far `samples` of
    that reference loop moves when every eps of every step is off by 1e-3 on every element."""
    from stable_diffusion_amd import DDIMSamplerHIP, LatentDiffusionHIP
    z = np.load(os.path.join(golden_dir, 'rdm64_pipeline_16.npz'))
    steps, b, h, w = int(z['steps']), int(z['batch']), int(z['h']), int(z['w'])
    assert float(z['perturb']) == MIXED_TOL
    kw = synthetic.RDM64_UNET_KWARGS
    ld = LatentDiffusionHIP(_unet('rdm64', 'mixed'), **synthetic.RDM_SCHEDULE).cuda()
    x_T = torch.randn(b, kw['in_channels'], h, w, generator=torch.Generator().manual_seed(int(z['input_seed'])))
    c = torch.randn(b, 1 + int(z['knn']), kw['context_dim'], generator=torch.Generator().manual_seed(int(z['ctx_seed'])))
    c = (c / c.norm(dim=-1, keepdim=True)).cuda()
    uc = torch.zeros_like(c)
    with contextlib.redirect_stdout(io.StringIO()):
        samples, _ = DDIMSamplerHIP(ld).sample(S=steps, conditioning=c, batch_size=b, shape=[kw['in_channels'], h, w], verbose=False,
                                               x_T=x_T.cuda(), unconditional_guidance_scale=float(z['scale']),
                                               unconditional_conditioning=uc, eta=float(z['eta']))
    torch.cuda.synchronize()
    e_s = float((samples.cpu() - torch.from_numpy(z['samples'])).abs().max())
    bar_s = float(z['bar_samples'])
    print(f'[rdm64 pipeline] samples max-abs {e_s:.3e} (bar {bar_s:.3e})', flush=True)
    assert bool(torch.isfinite(samples).all()) and e_s <= bar_s, (e_s, bar_s)


# ---- packed blobs ---------------------------------------------------------------------------------------------------------------
def test_packed_blob_round_trip_and_family_check(tmp_path, golden_dir):
    """a blob reproduces eps bit for bit in a fresh module; a blob from a num_heads handle of equal shapes (one level of 64 channels:
    2 heads of 32 either way) is refused by the num_head_channels handle, and the other way round"""
    from stable_diffusion_amd import UNetModelHIP
    z = np.load(os.path.join(golden_dir, 'rdm64_unet_8x8_b2.npz'))
    x, t, c = _inputs(z, synthetic.RDM64_UNET_KWARGS)
    m = _unet('rdm64', 'mixed')
    eps = m(x, t, context=c).clone()
    path = str(tmp_path / 'rdm64.sdmipk')
    assert m.save_packed(path) > 0
    fresh = UNetModelHIP(**synthetic.RDM64_UNET_KWARGS).cuda().load_packed(path)
    again = fresh(x, t, context=c)
    torch.cuda.synchronize()
    assert torch.equal(again, eps)
    del fresh
    one = dict(synthetic.RDM64_UNET_KWARGS, channel_mult=[1], attention_resolutions=[1])
    by_nhc = UNetModelHIP(**one).cuda()
    by_heads = UNetModelHIP(**dict(one, num_head_channels=-1, num_heads=2)).cuda()
    sd = synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in by_nhc.state_dict().items()], 0)
    assert [k for k in by_heads.state_dict()] == [k for k in by_nhc.state_dict()]
    by_nhc.load_state_dict(sd, strict=True)
    by_heads.load_state_dict(sd, strict=True)
    x1 = x[:, :, :4, :4].contiguous()
    assert torch.equal(by_nhc(x1, t, context=c), by_heads(x1, t, context=c))          # (the same network ...)
    p_heads, p_nhc = str(tmp_path / 'heads.sdmipk'), str(tmp_path / 'nhc.sdmipk')
    assert by_heads.save_packed(p_heads) == by_nhc.save_packed(p_nhc)
    with pytest.raises(_lib.SdmiError, match='different UNet configuration|num_head_channels'):      # (... but not the same blob family)
        by_nhc.load_packed(p_heads)
    with pytest.raises(_lib.SdmiError, match='different UNet configuration|num_head_channels'):
        by_heads.load_packed(p_nhc)
