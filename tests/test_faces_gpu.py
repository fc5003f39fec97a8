"""The face / bedroom LDMs (models/ldm/celeba256, ffhq256, lsun_beds256) and bsr_sr's UNet on the MI355X: widths 224 and 160.

Kernels against fp64 in guarded buffers (tests/guard.py), at the bars tests/test_model_shapes_gpu.py holds for the same launch kind
(its helpers are imported, not restated): the half k-tile of the implicit-GEMM family -- A sources of 32 (mod 64) channels, 1x1 / 3x3 /
stride 2 / folded x2 upsampling, two-source concats with the tail on either side or on both, on the LDS-DMA and the register-staged
path, split-K 1 / 2 / 3, tiles 3 / 5 / the launcher's own choice, the two split-fp16 forms -- with every A row followed by a pitch gap
of NaNs (0xFF bytes): the upper half of a half tile must not be read, not read and multiplied by zero weights.  Launches whose sources
are multiples of 64 through the new packer entry: the same packed bytes and the same output bits as through the old one.  GroupNorm at
7 .. 49 and 5 channels per group, stand-alone and as GEMM-epilogue statistics.  Attention at head dim 32 with 14 / 21 / 28 / 20 heads.
Whole UNets against goldens of the reference's own UNetModel (tools/make_golden_faces.py): mixed at 1e-3, full at 2e-5.  Launch tapes
replayed across timesteps.  The body of scripts/sample_diffusion.py against the reference DDIM loop at the fixture's bar."""
import contextlib
import ctypes as C
import io
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import kernels as K  # noqa: E402
import test_model_shapes_gpu as TMS  # noqa: E402  (helpers and bars only: _conv_ref64, _tol32, _tol_split, _report, _stats_errors, ...)
from stable_diffusion_amd import _lib, synthetic  # noqa: E402

DEV = 'cuda'
B = 2
MIXED_TOL = 1e-3        # tests/test_churches_gpu.py: the project's one mixed-precision bar
FULL_TOL = 2e-5         # ... and its full-mode bar
FACES_CASES = ['8x8_b2', '16x16_b2', '32x32_b1', '64x64_b1', '16x16_b10']
BSR_CASES = ['16x16_b2', '32x32_b1']
GAP = 40                # halves behind every A row, all 0xFF = NaN: more than the 32 halves a whole k-tile would read past a half one
_models = {}


def pack_conv_weight_src(w, split):
    """[O,I,KH,KW] fp32 cuda -> fp16 [O, KH*KW*I], K chunk-major per source of `split` (sdmi_k_pack_conv_weight_src)"""
    O, I, KH, KW = w.shape
    c = list(split) + [0] * (3 - len(split))
    dst = torch.empty((O, KH * KW * I), dtype=torch.float16, device=w.device)
    _lib.check(_lib.load().sdmi_k_pack_conv_weight_src(w.contiguous().data_ptr(), dst.data_ptr(), O, I, KH, KW, c[0], c[1], c[2], _lib.stream_ptr()))
    return dst


# ---- the half k-tile -------------------------------------------------------------------------------------------------------
class _Tail:
    """one GEMM / conv geometry with its sources in separate guarded buffers at ONE row pitch of max(c) + GAP halves (gap = NaN)"""

    def __init__(self, name, split, N, Hin, Win, Hout, Wout, ksize=1, stride=1, up=0, gn=(), gap=GAP):
        self.name, self.split, self.N, self.gn = name, tuple(split), N, list(gn)
        self.geom = (B, Hin, Win, Hout, Wout, ksize, stride, up)
        Cin = sum(split)
        self.Kd = ksize * ksize * Cin
        self.M, self.HW = B * Hout * Wout, Hout * Wout
        g = TMS._g(TMS._seed(Cin, len(split), N, Hin, Hout, ksize, stride, up))
        self.P = P = guard.Pool(DEV)
        x = TMS._r16((B * Hin * Win, Cin), g)
        w = TMS._r16((N, Cin, ksize, ksize), g, 1.0 / math.sqrt(self.Kd))
        ld = max(split) + gap
        self.a, c = [], 0
        for i, cs in enumerate(split):
            self.a.append(P.put(f'a{i}', x[:, c:c + cs].contiguous(), ld=ld))
            c += cs
        self.w = P.put('w', pack_conv_weight_src(w.float(), split))
        self.bias = P.put('bias', TMS._randn((N,), g))
        self.ref = TMS._conv_ref64(x, w, B, Hin, Win, ksize, stride, up) + self.bias.double()[None]
        self.inputs = [(v, v.clone()) for v in self.a + [self.w, self.bias]]
        self.cnt = P.new('splitk_cnt', (8192,), torch.int32, fill=0)

    def run(self, tile, splitk, dma):
        P, M, N = self.P, self.M, self.N
        tag = f'{self.name} tile{tile} k{splitk} dma{dma}'
        n0 = len(P.bufs)
        out = P.new('out_f32', (M, N), torch.float32, ld=N + 8)
        out16 = P.new('out_f16', (M, N), torch.float16, ld=N + 8)
        ws = P.new('splitk_ws', (TMS._ws_floats(M, N),), torch.float32, row_bytes=4 * ((N + 255) // 256 * 256))
        accs = [P.new(f'gn_acc{i}', (B, 32, 8, 16), torch.int64, fill=0) for i in range(len(self.gn))]
        gn = [(acc, cpg, cbase) for acc, (cpg, cbase) in zip(accs, self.gn)] or None
        Bn, Hin, Win, Hout, Wout, ksize, stride, up = self.geom
        K.igemm(self.a[0], self.w, N, Bn, Hin, Win, Hout, Wout, ksize, stride, up, a1=self.a[1] if len(self.a) > 1 else None,
                a2=self.a[2] if len(self.a) > 2 else None, bias=self.bias, out_f32=out, out_f16=out16, ldo=N + 8, tile=tile, splitk=splitk,
                dma=dma, gn=gn, ws=ws, cnt=self.cnt)
        torch.cuda.synchronize()
        tol = TMS._tol32(self.Kd)
        errs = {'f32': (TMS._report(f'{tag} f32', out, self.ref, tol), tol), 'f16': (TMS._report(f'{tag} f16', out16, self.ref, 6e-3), 6e-3)}
        st = TMS._stats_errors(out, self.HW, self.gn, accs)
        for (cpg, cbase), (e1, e2, bar) in zip(self.gn, st):
            print(f'[{tag} gn-stats cpg{cpg} cbase{cbase}] |sum err| {e1:.3e} (tol {bar:.1e}) rel sumsq err {e2:.3e} (tol 1.0e-05)', flush=True)
        P.check(tag)
        assert int(self.cnt.abs().max()) == 0, f'{tag}: split-K tile counters not left zero'
        for v, keep in self.inputs:
            assert torch.equal(v, keep), f'{tag}: an input operand was modified'
        self.last = out.clone()
        del P.bufs[n0:]
        return errs, st


# name, sources, N, Hin, Hout, ksize, stride, up, statistics targets (cpg, cbase)
TAIL_CASES = [
    ('1x1 32', (32,), 64, 8, 8, 1, 1, 0, ()),                          # the whole K is one half tile
    ('1x1 96', (96,), 64, 8, 8, 1, 1, 0, ()),
    ('1x1 224', (224,), 224, 8, 8, 1, 1, 0, [(7, 0)]),
    ('3x3 96', (96,), 64, 8, 8, 3, 1, 0, ()),
    ('3x3 224', (224,), 224, 8, 8, 3, 1, 0, [(7, 0), (21, 448)]),     # N tail on the 128-wide tile; cpg 7 / 21, cbase 0 / 448
    ('3x3 s2 224', (224,), 224, 16, 8, 3, 2, 0, ()),
    ('3x3 up 224', (224,), 224, 4, 8, 3, 1, 1, ()),
    ('3x3 96|64', (96, 64), 64, 8, 8, 3, 1, 0, ()),                    # 27 k-tiles: odd
    ('3x3 64|96', (64, 96), 64, 8, 8, 3, 1, 0, ()),
    ('3x3 96|96', (96, 96), 64, 8, 8, 3, 1, 0, ()),
    ('3x3 224|224', (224, 224), 224, 8, 8, 3, 1, 0, [(7, 0)]),
    ('1x1 96|64|32', (96, 64, 32), 64, 8, 8, 1, 1, 0, ()),
    ('3x3 224 6x6', (224,), 224, 6, 6, 3, 1, 0, ()),                   # M = 72: no multiple of any BM
]


@pytest.mark.parametrize('name,split,N,hin,hout,ksize,stride,up,gn', TAIL_CASES, ids=[c[0].replace(' ', '-') for c in TAIL_CASES])
def test_half_k_tile_vs_fp64(name, split, N, hin, hout, ksize, stride, up, gn):
    """every case on the LDS-DMA and the register-staged path, at split-K 1 and 2 (3 where the k-tile count is odd), on tiles 3 and 5 and
    the launcher's own choice; every A row is followed by NaNs, so a finite in-bar output shows that a half tile reads 64 bytes per row"""
    c = _Tail(name, split, N, hin, hin, hout, hout, ksize, stride, up, gn)
    ntiles = ksize * ksize * sum((s + 63) // 64 for s in split)
    res = []
    for dma in (1, 0):
        for tile in (3, 5, -1):
            for sk in (1, 2) + ((3,) if ntiles % 2 and ntiles > 3 and tile == 5 else ()):
                res.append(c.run(tile, sk, dma))
        res.append(c.run(-1, 0, dma))                          # the executor's request: table / heuristic tile and split
    for errs, st in res:
        TMS._assert_case(errs, st)


def test_half_k_tile_ignores_the_next_pixel():
    """at the executor's pitch (lda = C) the bytes behind a row's last 32 channels are the next pixel's: the result must not depend on them.
    Same launch twice, the second time with every OTHER source row turned into NaN / Inf through a 1x1 conv that reads row m only for
    output m: rows whose own input is finite must keep their bits."""
    g = TMS._g(7)
    C_, N, hw = 224, 64, 8
    M = B * hw * hw
    x = TMS._r16((M, C_), g)
    w = TMS._r16((N, C_, 1, 1), g, 1.0 / math.sqrt(C_))
    P = guard.Pool(DEV)
    a = P.put('a', x)
    wp = P.put('w', K.pack_conv_weight(w.float()))
    outs = []
    for poison in (False, True):
        if poison:
            a[1::2, :64] = float('nan')
            a[1::2, 64:] = float('inf')
        for dma in (1, 0):
            out = P.new('out', (M, N), torch.float32)
            K.igemm(a, wp, N, B, hw, hw, hw, hw, out_f32=out, tile=5, dma=dma)
            torch.cuda.synchronize()
            outs.append(out.clone())
    P.check('next pixel')
    ref = x.double() @ w.double().reshape(N, C_).t()
    assert TMS._report('1x1 224 lda=C', outs[0], ref, TMS._tol32(C_)) < TMS._tol32(C_)
    assert torch.equal(outs[0], outs[1])
    for clean, dirty in ((outs[0], outs[2]), (outs[1], outs[3])):
        assert bool(torch.isfinite(dirty[0::2]).all()) and torch.equal(clean[0::2], dirty[0::2])
        assert not bool(torch.isfinite(dirty[1::2]).any())


@pytest.mark.parametrize('Cin', [96, 224])
@pytest.mark.parametrize('form', ['conv3_split3', 'gemm_split16', 'dense_split3'])
def test_half_k_tile_split_fp16_forms(form, Cin):
    """the K-concatenated 3-pass 3x3 conv ([hi | lo | hi] x [w_hi | w_hi | w_lo]: three sources that all end in a half tile), the
    split-fp16 dense GEMM family and the K-concatenated 1x1 form it replaces; fp32 N(0, 4) operands, bar _tol_split"""
    ksize = 3 if form == 'conv3_split3' else 1
    N, hw = 224, 8
    M, Kd = B * hw * hw, ksize * ksize * Cin
    g = TMS._g(TMS._seed(Cin, ksize, 16))
    x = TMS._randn((M, Cin), g, 2.0)
    w = TMS._randn((N, Cin, ksize, ksize), g, 1.0 / math.sqrt(Kd))
    hi, lo = K.cast_f16(x, want_lo=True)
    P = guard.Pool(DEV)
    a_hi, a_lo = P.put('a_hi', hi, ld=Cin + GAP), P.put('a_lo', lo, ld=Cin + GAP)
    wp = P.put('w', K.pack_conv_split3(w) if ksize == 3 else K.pack_split3(w.reshape(N, Cin).contiguous()))
    bias = P.put('bias', TMS._randn((N,), g))
    ref = TMS._conv_ref64(x, w, B, hw, hw, ksize, 1, 0) + bias.double()[None]
    tol = TMS._tol_split(Kd)
    cnt = P.new('splitk_cnt', (8192,), torch.int32, fill=0)
    errs = []
    for tile, sk in ((5, 1), (5, 2), (-1, 0)) + (((3, 1), (3, 2)) if form != 'gemm_split16' else ((2, 1), (8, 2))):
        out = P.new('out', (M, N), torch.float32, ld=N + 8)
        ws = P.new('splitk_ws', (TMS._ws_floats(M, N),), torch.float32, row_bytes=4 * ((N + 255) // 256 * 256))
        K.igemm(a_hi, wp, N, B, hw, hw, hw, hw, ksize, a1=a_lo, a2=None if form == 'gemm_split16' else a_hi, bias=bias, out_f32=out,
                ldo=N + 8, tile=tile, splitk=sk, split16=form == 'gemm_split16', ws=ws, cnt=cnt)
        torch.cuda.synchronize()
        errs.append(TMS._report(f'{form} Cin{Cin} tile{tile} k{sk}', out, ref, tol))
        P.check(f'{form} Cin{Cin} tile{tile} k{sk}')
        del P.bufs[-2:]
    assert max(errs) < tol, (errs, tol)


@pytest.mark.parametrize('split', [(128,), (64, 64)])
@pytest.mark.parametrize('ksize', [1, 3])
def test_whole_chunk_launches_are_bit_identical(split, ksize):
    """sources that are multiples of 64: the new packer entry (split given) writes the old entry's bytes, and the launch gives the same
    output bits with either"""
    Cin, N, hw = sum(split), 64, 8
    M = B * hw * hw
    g = TMS._g(TMS._seed(Cin, len(split), ksize))
    x = TMS._r16((M, Cin), g)
    w = TMS._r16((N, Cin, ksize, ksize), g, 1.0 / math.sqrt(ksize * ksize * Cin))
    old, new = K.pack_conv_weight(w.float()), pack_conv_weight_src(w.float(), split)
    torch.cuda.synchronize()
    assert torch.equal(old.view(torch.int16), new.view(torch.int16))
    if ksize == 3:
        w3 = TMS._randn((N, Cin, 3, 3), g)
        s3 = K.pack_conv_split3(w3)
        virt = torch.cat([w3.half().float(), w3.half().float(), (w3 - w3.half().float())], dim=1)
        assert torch.equal(s3.view(torch.int16), K.pack_conv_weight(virt).view(torch.int16))
    srcs = [x[:, :split[0]]] + ([x[:, split[0]:]] if len(split) > 1 else [])
    outs = []
    for wp in (old, new):
        for tile, sk, dma in ((5, 1, 1), (5, 2, 1), (3, 1, 0), (-1, 0, -1)):
            out = torch.empty((M, N), dtype=torch.float32, device=DEV)
            K.igemm(srcs[0], wp, N, B, hw, hw, hw, hw, ksize, a1=srcs[1] if len(srcs) > 1 else None, out_f32=out, tile=tile, splitk=sk, dma=dma)
            outs.append(out)
    torch.cuda.synchronize()
    for a, b in zip(outs[:4], outs[4:]):
        assert torch.equal(a, b)
    ref = TMS._conv_ref64(x, w, B, hw, hw, ksize, 1, 0)
    assert TMS._report(f'whole chunks {split} k{ksize}', outs[0], ref, 3e-4) < 3e-4


def test_launcher_still_refuses_other_widths():
    x = torch.zeros((B * 64, 48), dtype=torch.float16, device=DEV)
    w = torch.zeros((64, 48), dtype=torch.float16, device=DEV)
    out = torch.empty((B * 64, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.SdmiError, match='multiples of 32'):
        K.igemm(x, w, 64, B, 8, 8, 8, 8, out_f32=out)
    with pytest.raises(_lib.SdmiError, match='multiple of 32'):
        pack_conv_weight_src(torch.zeros((64, 112, 3, 3), device=DEV), (64, 48))


# ---- GroupNorm at odd channels per group ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('HW', [1, 4, 64, 1024])
@pytest.mark.parametrize('c0,c1', [(128, 96), (448, 224), (672, 448), (896, 672), (160, 0), (224, 0), (224, 224), (320, 160)])
def test_groupnorm_odd_channels_per_group(c0, c1, HW):
    """7 / 21 / 35 / 49 / 5 / 7 / 14 / 15 channels per group: quads that straddle two groups at every offset, seams inside a group"""
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


# ---- attention at head dim 32 ---------------------------------------------------------------------------------------------------
def _split(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


# (input recipe and bars of tests/test_churches_gpu.py::test_attention_d24_d48_vs_fp64; B = 2)
@pytest.mark.parametrize('n', [1, 16, 64, 1024])
@pytest.mark.parametrize('heads', [14, 21, 28, 20])
@pytest.mark.parametrize('full', [False, True])
def test_attention_d32_vs_fp64(n, heads, full):
    torch.manual_seed(n + heads)
    d, nq, nkv = 32, n, n
    BH, nkv_pad = B * heads, (nkv + 7) // 8 * 8
    q = torch.randn(BH, nq, d, device=DEV)
    k = torch.randn(BH, nkv, d, device=DEV)
    v = torch.randn(BH, nkv, d, device=DEV)
    vt = torch.zeros(BH, d, nkv_pad, device=DEV)
    vt[:, :, :nkv] = v.transpose(1, 2)
    scale = d ** -0.5
    lib = _lib.load()
    pool = guard.Pool()
    out = pool.new('out', (B, nq, heads * d), torch.float16)
    if full:
        ops = [pool.put(nm, t) for nm, t in zip(('q', 'q_lo', 'k', 'k_lo', 'vt', 'vt_lo'), _split(q) + _split(k) + _split(vt))]
        out_lo = pool.new('out_lo', (B, nq, heads * d), torch.float16)
        _lib.check(lib.sdmi_k_attention_split16(*[t.data_ptr() for t in ops], out.data_ptr(), out_lo.data_ptr(), BH, heads, nq, nkv, nkv_pad, d,
                                                scale, _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = out.double() + out_lo.double()
        qr, kr, vr = q.double(), k.double(), v.double()
        tol = 2e-5
    else:
        qh, kh, vh = pool.put('q', q.half()), pool.put('k', k.half()), pool.put('vt', vt.half())
        _lib.check(lib.sdmi_k_attention(qh.data_ptr(), kh.data_ptr(), vh.data_ptr(), out.data_ptr(), BH, heads, nq, nkv, nkv_pad, d, scale,
                                        _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = out.double()
        qr, kr, vr = qh.double(), kh.double(), vh[:, :, :nkv].transpose(1, 2).double()
        tol = 4e-3
    pool.check(f'attention d32 heads={heads} n={n}')
    ref = torch.softmax(qr @ kr.transpose(1, 2) * scale, dim=-1) @ vr
    ref = ref.view(B, heads, nq, d).permute(0, 2, 1, 3).reshape(B, nq, heads * d)
    err = float((got - ref).abs().max())
    print(f'[attn d32 heads={heads} n={n} full={full}] max-abs {err:.3e}', flush=True)
    assert err <= tol


# ---- the UNets against the reference goldens ------------------------------------------------------------------------------------
def _unet(tag, prec):
    if (tag, prec) not in _models:
        for key in [k for k in _models if k[0] != tag]:       # (one model family on the device at a time)
            del _models[key]
        torch.cuda.empty_cache()
        from stable_diffusion_amd import UNetModelHIP
        m = UNetModelHIP(**(synthetic.FACES_UNET_KWARGS if tag == 'faces' else synthetic.BSR_UNET_KWARGS), hip_precision=prec)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models[(tag, prec)] = m.cuda()
    return _models[(tag, prec)]


def _unet_inputs(batch, channels, h, w, ts, seed=1):       # (tools/make_golden_faces.py unet_inputs)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, channels, h, w, generator=g), torch.tensor(ts, dtype=torch.int64)


@pytest.mark.parametrize('prec', ['mixed', 'full'])
@pytest.mark.parametrize('tag,case', [('faces', c) for c in FACES_CASES] + [('bsr', c) for c in BSR_CASES])
def test_unet_matches_reference(tag, case, prec, golden_dir):
    """faces 8x8_b2: the smallest legal latent (the middle block sees one pixel); 64x64_b1: the native latent (4096 / 1024 / 256 / 64
    tokens); 16x16_b10: the 8 + 2 chunking of a sample_diffusion.py batch; bsr: six input channels, 20 heads"""
    z = np.load(os.path.join(golden_dir, f'{tag}_unet_{case}.npz'))
    assert int(z['weight_seed']) == 0
    x, t = _unet_inputs(int(z['batch']), 6 if tag == 'bsr' else 3, int(z['h']), int(z['w']), tuple(int(v) for v in z['t']), seed=int(z['input_seed']))
    ref = torch.from_numpy(z['eps'])
    eps = _unet(tag, prec)(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    err = (eps.float().cpu() - ref).abs()
    mx, rms = float(err.max()), float(err.pow(2).mean().sqrt())
    tol = MIXED_TOL if prec == 'mixed' else FULL_TOL
    print(f'[{tag} unet {case} {prec}] max-abs {mx:.3e} rms {rms:.3e} |eps|max {ref.abs().max():.3f} (tol {tol:.1e})', flush=True)
    assert eps.shape == ref.shape and bool(torch.isfinite(eps).all())
    assert mx <= tol


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


def test_faces_unet_tape_replay_across_timesteps_and_shapes():
    """a replayed tape must add the embedding row of ITS timestep, and a second shape gets its own tape"""
    m = _unet('faces', 'mixed')
    lib = m._handle.lib

    def stats():
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.sdmi_unet_tape_stats(m._handle.h, C.byref(a), C.byref(b)))
        return a.value, b.value
    for hw in (16, 8):
        x, _ = _unet_inputs(2, 3, hw, hw, (981, 981), seed=5)
        x = x.cuda()
        t981, t1 = torch.full((2,), 981, dtype=torch.long, device=DEV), torch.full((2,), 1, dtype=torch.long, device=DEV)
        with _env('SDMI_REPLAY', '0'):
            un981, un1 = m(x, t981).clone(), m(x, t1).clone()
        assert not torch.equal(un981, un1)
        m.cache_timesteps([981, 1])
        try:
            r0, c0 = stats()
            m.hint_timestep(981)
            a = m(x, t981).clone()
            r1, c1 = stats()
            m.hint_timestep(1)
            b = m(x, t1).clone()
            r2, c2 = stats()
            m.hint_timestep(981)
            c = m(x, t981).clone()
            r3, c3 = stats()
        finally:
            m.cache_timesteps([])
        torch.cuda.synchronize()
        assert (r1, c1) in ((r0, c0 + 1), (r0 + 1, c0)) and (r2, c2) == (r1 + 1, c1) and (r3, c3) == (r2 + 1, c2), ((r0, c0), (r1, c1), (r2, c2), (r3, c3))
        assert torch.equal(a, un981) and torch.equal(b, un1) and torch.equal(c, un981)


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def _pipeline_noise(seed, steps, shape):          # (tools/make_golden_faces.py pipeline_noise)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), [torch.randn(shape, generator=g) for _ in range(steps)]


VQ_DEC_PIN = 6.1e-3      # tests/test_cin_gpu.py VQ_PINS['dec_q']: the same VQ-f4 decoder (mid-block attention on) on codebook rows


def test_faces_pipeline_matches_reference_loop(golden_dir):
    """The body of scripts/sample_diffusion.py's make_convolutional_sample on HIP classes: DDIM at eta 1.0 with no conditioning (the
    per-step noise handed out from the seeded sequence the golden tool used) -- against the reference DDIMSampler loop on the CPU, at the
    fixture's bar: how far `samples` of that reference loop moves when every eps of every step is off by 1e-3 on every element.  The VQ-f4
    decode is compared on the golden's own latent at its own code indices (a code flip near a cell boundary is not the UNet's)."""
    from stable_diffusion_amd import DDIMSamplerHIP, LatentDiffusionHIP, VQModelInterfaceHIP
    z = np.load(os.path.join(golden_dir, 'faces_pipeline_16.npz'))
    steps, b, h, w = int(z['steps']), int(z['batch']), int(z['h']), int(z['w'])
    assert float(z['perturb']) == MIXED_TOL
    unet = _unet('faces', 'mixed')
    vq = VQModelInterfaceHIP(**synthetic.FACES_VQ_KWARGS)
    dec_keys = [(k, tuple(v.shape)) for k, v in vq.state_dict().items() if k.startswith(('decoder.', 'post_quant_conv.', 'quantize.'))]
    sd = {k: v for k, v in vq.state_dict().items()}
    sd.update(synthetic.synthetic_named_state_dict(dec_keys, int(z['weight_seed'])))
    vq.load_state_dict(sd, strict=True)
    vq = vq.cuda()
    ld = LatentDiffusionHIP(unet, **synthetic.FACES_SCHEDULE).cuda()
    x_T, noises = _pipeline_noise(int(z['noise_seed']), steps, (b, 3, h, w))
    seq = [n.cuda() for n in noises]
    smp = DDIMSamplerHIP(ld)
    smp._noise_like = lambda shape, device: seq.pop(0)
    with contextlib.redirect_stdout(io.StringIO()):
        samples, _ = smp.sample(steps, batch_size=b, shape=(3, h, w), eta=float(z['eta']), verbose=False, x_T=x_T.cuda())
    e = sd['quantize.embedding.weight']
    zq = e[torch.from_numpy(z['idx']).long()].permute(0, 3, 1, 2).contiguous()          # the golden's own quantized latent
    x_dec = vq.decode(zq.cuda(), force_not_quantize=True)
    torch.cuda.synchronize()
    assert not seq and bool(torch.isfinite(samples).all()) and bool(torch.isfinite(x_dec).all())
    e_s = float((samples.cpu() - torch.from_numpy(z['samples'])).abs().max())
    e_x = float((x_dec.cpu() - torch.from_numpy(z['x_dec'])).abs().max())
    bar_s = float(z['bar_samples'])
    print(f'[faces pipeline] samples max-abs {e_s:.3e} (bar {bar_s:.3e}); decode of the golden latent max-abs {e_x:.3e} (pin {VQ_DEC_PIN:.1e})', flush=True)
    assert e_s <= bar_s and e_x <= VQ_DEC_PIN, (e_s, bar_s, e_x)
