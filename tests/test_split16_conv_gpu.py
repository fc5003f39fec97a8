"""Three-source (K-concatenated) split-fp16 convolutions against fp64 torch, through the C ABI.

An fp32 activation x is split by sdmi_k_cast_f16 into separate buffers hi = fp16(x), lo = fp16(x - hi); the conv reads the
operand [hi | lo | hi] (a0, a1, a2; K = 27 Cin for a 3x3) against weights packed by sdmi_k_pack_conv_split3 as
[w_hi | w_hi | w_lo], i.e. hi w_hi + lo w_hi + hi w_lo with fp32 accumulation.  This is the default mode's last ResBlock
(both 3x3 convs), the per-prompt context K / V projection (1x1, head-scatter epilogue) and, in the full mode, every ResBlock
conv and resampler.  The reference sees the fp32 x and w in float64.

Bars (from the arithmetic: operands to ~2^-22, fp32 accumulation): max-abs <= 3e-5 on O(1) outputs, <= 1/20 of the same conv
on one fp16 source with fp16 weights, two runs bit-identical.  The drop-`lo` controls show that the bars separate a correct
kernel from one that silently lost a term.  Each case prints its measured error.

Measured on an MI355X: small cases <= 8.1e-6 on every generic and halo tile and split; SD shapes 7.1e-6 .. 2.2e-5 (the worst:
the bench's 640 -> 320 conv as the planner runs it, halo tile 14 without split-K, one fp32 accumulator over K = 17280), 105 -
639x under the fp16-operand conv; the drop-lo controls 41 - 55x over the bar."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import kernels as K  # noqa: E402  (tests/ is on sys.path via conftest's rootdir insertion)

DEV = 'cuda'
BAR = 3e-5          # max-abs on O(1) outputs (the bar of test_gemm_split16)

ALL_TILES = list(range(14)) + [18, 19, 20, 21]     # generic implicit GEMM tiles (include/sdmi.h)
HALO_TILES = {14: 256, 15: 256, 16: 128, 17: 128}  # halo-staged 3x3 conv tile -> BM


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _with_outliers(x, g, scale=30.0):
    """a few entries at |x| ~ 30 (the residual stream's outlier scale); x is modified in place"""
    flat = x.view(-1)
    n = max(4, flat.numel() // 2048)
    idx = torch.randint(0, flat.numel(), (n,), generator=g)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    flat[idx] = sign * scale * (1.0 + 0.1 * torch.rand(n, generator=g))
    return x


def _ordered(h):
    """fp16 bit patterns -> integers in value order (adjacent fp16 values differ by 1; +0 and -0 coincide)"""
    b = h.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


# ---- 1. the weight packer ---------------------------------------------------------------------------------------------

def _host_pack_conv(w):
    """pack_conv_weight's chunk-major K order restated on the host: [O][I][3][3] -> [O][9 I],
    k = ((i / 64) * 9 + ky * 3 + kx) * 64 + i % 64"""
    O, I = w.shape[:2]
    return w.reshape(O, I // 64, 64, 3, 3).permute(0, 1, 3, 4, 2).reshape(O, 9 * I)


@pytest.mark.parametrize('I', [64, 320, 640, 1280])
@pytest.mark.parametrize('O', [64, 320, 72])
def test_pack_conv_split3_matches_packing_the_virtual_tensor(O, I):
    """sdmi_k_pack_conv_split3(w) is, bit for bit, pack_conv_weight of the virtual [O][3 I][3][3] tensor cat([w_hi, w_hi, w_lo])
    -- packed on the host and by sdmi_k_pack_conv_weight on the device"""
    g = _g(O * 7 + I)
    w = torch.randn((O, I, 3, 3), generator=g) / math.sqrt(9 * I)
    w.view(-1)[::97] *= 1e-3          # small weights: their low halves are fp16 subnormals
    w_hi = w.half()
    w_lo = (w - w_hi.float()).half()
    virt = torch.cat([w_hi, w_hi, w_lo], dim=1)
    got = K.pack_conv_split3(w.to(DEV)).cpu()
    assert got.shape == (O, 27 * I)
    assert torch.equal(got.view(torch.int16), _host_pack_conv(virt).contiguous().view(torch.int16))
    dev = K.pack_conv_weight(virt.float().to(DEV)).cpu()
    assert torch.equal(got.view(torch.int16), dev.view(torch.int16))


def test_pack_conv_split3_refuses_a_ragged_channel_count():
    from stable_diffusion_amd import _lib
    w = torch.zeros((8, 72, 3, 3), device=DEV)
    with pytest.raises(_lib.SdmiError, match='% 64'):
        K.pack_conv_split3(w)


# ---- 2. three-source 3x3 conv ----------------------------------------------------------------------------------------

_CASES = {}


def _conv_case(name, B, Hin, Win, Cin, N, stride, up):
    """inputs on the device (x split into separate hi / lo buffers, packed split3 and fp16 weights, epilogue terms) and the
    float64 reference, built once per case"""
    if name in _CASES:
        return _CASES[name]
    g = _g(sum(map(ord, name)))
    x = _with_outliers(torch.randn((B * Hin * Win, Cin), generator=g), g)
    w = torch.randn((N, Cin, 3, 3), generator=g) / math.sqrt(9 * Cin)
    Hout = 2 * Hin if up else (Hin - 1) // stride + 1
    Wout = 2 * Win if up else (Win - 1) // stride + 1
    M = B * Hout * Wout
    bias = torch.randn(N, generator=g)
    rowvec = torch.randn(B, N, generator=g)
    resid = torch.randn(M, N, generator=g)
    xd, wd = x.to(DEV), w.to(DEV)
    hi, lo = K.cast_f16(xd, want_lo=True)
    xi = xd.double().reshape(B, Hin, Win, Cin).permute(0, 3, 1, 2)
    if up:
        xi = F.interpolate(xi, scale_factor=2, mode='nearest')
    ref = F.conv2d(xi, wd.double(), None, stride=stride, padding=1)
    assert ref.shape == (B, N, Hout, Wout)
    ref = ref.permute(0, 2, 3, 1).reshape(M, N) + bias.double().to(DEV)[None] + \
        rowvec.double().to(DEV).repeat_interleave(Hout * Wout, dim=0) + resid.double().to(DEV)
    c = dict(B=B, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, Cin=Cin, N=N, stride=stride, up=up, M=M, hi=hi, lo=lo,
             w3=K.pack_conv_split3(wd), w16=K.pack_conv_weight(wd), bias=bias.to(DEV), rowvec=rowvec.to(DEV),
             resid=resid.to(DEV), ref=ref)
    torch.cuda.synchronize()
    _CASES[name] = c
    return c


def _run3(c, tile, splitk, dma=-1, a1=None, fused_splitk=True):
    """the three-source conv a0 = hi, a1 = lo, a2 = hi (c0 = c1 = c2 = Cin, K = 27 Cin) with bias, rowvec and residual"""
    out = torch.full((c['M'], c['N']), float('nan'), device=DEV)
    K.igemm(c['hi'], c['w3'], c['N'], c['B'], c['Hin'], c['Win'], c['Hout'], c['Wout'], 3, c['stride'], c['up'],
            a1=c['lo'] if a1 is None else a1, a2=c['hi'], bias=c['bias'], rowvec=c['rowvec'], residual=c['resid'], out_f32=out,
            splitk=splitk, tile=tile, dma=dma, fused_splitk=fused_splitk)
    torch.cuda.synchronize()
    return out


def _err(out, ref):
    return float((out.double() - ref).abs().max()) if bool(torch.isfinite(out).all()) else float('inf')


def _check(label, c, tile, splitk, dma=-1, fused_splitk=True):
    out = _run3(c, tile, splitk, dma, fused_splitk=fused_splitk)
    err = _err(out, c['ref'])
    print(f'[split16 conv {label} tile{tile} k{splitk} dma{dma}] max-abs {err:.2e} (bar {BAR:.0e}) '
          f'max|ref| {float(c["ref"].abs().max()):.2f}', flush=True)
    assert err <= BAR
    out2 = _run3(c, tile, splitk, dma, fused_splitk=fused_splitk)
    assert torch.equal(out, out2)
    return err


SMALL = [
    # name, B, Hin, Win, Cin, N, stride, up
    ('s1', 2, 12, 12, 64, 128, 1, 0),
    ('s1_ntail', 2, 8, 8, 64, 72, 1, 0),                  # N tail inside every tile
    ('down_even', 2, 12, 12, 64, 64, 2, 0),
    ('down_odd', 1, 7, 9, 128, 64, 2, 0),
    ('down_1x3', 2, 2, 6, 64, 64, 2, 0),                  # tiny_8x24's last Downsample: a 1x3 output
    ('up_odd', 1, 5, 7, 64, 72, 1, 1),                    # Upsample folded into the gather, odd input, N tail
]


@pytest.mark.parametrize('case', SMALL, ids=[c[0] for c in SMALL])
@pytest.mark.parametrize('tile', ALL_TILES)
@pytest.mark.parametrize('dma', [0, 1])
@pytest.mark.parametrize('splitk', [1, 2, 3])
def test_split16_conv3_generic_tiles(case, tile, dma, splitk):
    """every generic tile, register and LDS-DMA staging: split-K 3 starts its splits exactly on the source changes
    (9 Cin / 64 k-tiles per source), split-K 2 starts one inside a source, mid-chunk"""
    c = _conv_case(*case)
    _check(case[0], c, tile, splitk, dma)


HALO = [
    # name, B, H, W, Cin, N -- three sources of Cin / 64 chunks each
    ('h16_c320', 1, 16, 16, 320, 64),        # 15 chunks: splits 3 (5 + 5 + 5) on the source changes at 5 and 10, 5 and 2 inside
    ('h8_4img', 4, 8, 8, 128, 128),          # whole images per tile (BM = 128: two, 256: four)
    ('h32_ntail', 1, 32, 32, 64, 72),        # one chunk per source, N tail
]


def _halo_supported(B, H, W, bm):
    """igemm.hip halo_supported() for a stride-1 3x3 conv"""
    HW = H * W
    if not (8 <= W <= 64 and W & (W - 1) == 0 and bm % W == 0):
        return False
    cap = (((bm // 64 + 2) * 66 + bm // 4 - 1) // (bm // 4)) * (bm // 4)
    if bm <= HW:
        return HW % bm == 0 and (bm // W + 2) * (W + 2) <= cap
    return bm % HW == 0 and (B * HW) % bm == 0 and (bm // HW) * (H + 2) * (W + 2) <= cap


HALO_RUNS = [(c, t) for c in HALO for t, bm in HALO_TILES.items() if _halo_supported(c[1], c[2], c[3], bm)]


@pytest.mark.parametrize('case,tile', HALO_RUNS, ids=[f'{c[0]}-t{t}' for c, t in HALO_RUNS])
@pytest.mark.parametrize('splitk', [1, 2, 3, 5])
def test_split16_conv3_halo_tiles(case, tile, splitk):
    """the halo-staged conv picks its source per 64-channel chunk and splits K at chunk granularity: split boundaries on and
    inside the source changes"""
    name, B, H, W, Cin, N = case
    c = _conv_case(name, B, H, W, Cin, N, 1, 0)
    _check(name, c, tile, splitk)


SD = [
    # name, B, Hin, Win, Cin, N, stride, up, pinned (tile, splitk) runs beside the planner's (-1, auto)
    ('last_res_in', 2, 64, 64, 640, 320, 1, 0, [(15, 5), (5, 3)]),      # bench shape, conv 1 of the last ResBlock
    ('last_res_out', 2, 64, 64, 320, 320, 1, 0, [(14, 5)]),             # ... conv 2
    ('full_8x8', 2, 8, 8, 1280, 1280, 1, 0, [(2, 15)]),                 # full mode: deep K, split-K
    ('full_8x8_cat', 2, 8, 8, 2560, 1280, 1, 0, [(19, 16)]),
    ('full_16x16_cat', 2, 16, 16, 1920, 1280, 1, 0, [(15, 4)]),         # 90 chunks, splits of 23 inside the sources
    ('full_32x32', 2, 32, 32, 640, 640, 1, 0, []),
    ('full_down', 2, 64, 64, 320, 320, 2, 0, []),                       # Downsample 64 -> 32
    ('full_up', 2, 8, 8, 1280, 1280, 1, 1, []),                         # Upsample 8 -> 16
]
SD_RUNS = [(c, t, k) for c in SD for t, k in [(-1, 0)] + c[8]]


@pytest.mark.parametrize('case,tile,splitk', SD_RUNS, ids=[f'{c[0]}-t{t}-k{k}' for c, t, k in SD_RUNS])
def test_split16_conv3_sd_shapes(case, tile, splitk):
    """SD-scale shapes of the default mode's last ResBlock and the full mode's ResBlocks / resamplers: the planner's choice
    (tuning table, auto split-K, as the executor launches them) and pinned tiles / splits"""
    c = _conv_case(*case[:8])
    _check(case[0], c, tile, splitk)


@pytest.mark.parametrize('case', [s[:8] for s in SMALL[:1] + SMALL[3:]] + [s[:8] for s in SD],
                         ids=[s[0] for s in SMALL[:1] + SMALL[3:]] + [s[0] for s in SD])
def test_split16_conv3_beats_fp16_operands(case):
    """the planner's three-source conv is within 1/20 of the error of the same conv on one fp16 source with fp16 weights"""
    c = _conv_case(*case)
    err3 = _err(_run3(c, -1, 0), c['ref'])
    out1 = torch.full((c['M'], c['N']), float('nan'), device=DEV)
    K.igemm(c['hi'], c['w16'], c['N'], c['B'], c['Hin'], c['Win'], c['Hout'], c['Wout'], 3, c['stride'], c['up'],
            bias=c['bias'], rowvec=c['rowvec'], residual=c['resid'], out_f32=out1, splitk=0)
    torch.cuda.synchronize()
    err1 = _err(out1, c['ref'])
    print(f'[split16 conv {case[0]}] max-abs {err3:.2e}, fp16 operands {err1:.2e} (ratio {err1 / max(err3, 1e-30):.0f})', flush=True)
    assert err3 <= BAR and err3 <= err1 / 20


@pytest.mark.parametrize('case,tile,splitk', [(SD[0][:8], -1, 0), (SMALL[0], 5, 2), (HALO[0][:6] + (1, 0), 15, 5)],
                         ids=['last_res_in', 's1-t5-k2', 'h16_c320-t15-k5'])
def test_split16_conv3_dropped_lo_term_fails_the_bar(case, tile, splitk):
    """negative control: the same conv with a1 pointing to zeros (the lo x w_hi term dropped) misses the bar by >= 10x"""
    c = _conv_case(*case)
    zeros = torch.zeros_like(c['lo'])
    err = _err(_run3(c, tile, splitk, a1=zeros), c['ref'])
    print(f'[split16 conv {case[0]} tile{tile} k{splitk} without lo] max-abs {err:.2e} = {err / BAR:.0f} x the bar', flush=True)
    assert err >= 10 * BAR


# ---- 3. three-source 1x1 with the per-head scatter: the context K / V projection -------------------------------------

KV = [(320, 8), (640, 8), (1280, 8), (768, 12)]      # (C, heads): dh = 40, 80, 160, 64
NCTX, DCTX, BKV = 77, 768, 2


_KV = {}


def _kv_case(C, heads):
    if (C, heads) in _KV:
        return _KV[(C, heads)]
    g = _g(C + heads)
    ctx = _with_outliers(torch.randn((BKV * NCTX, DCTX), generator=g), g)
    w = torch.randn((2 * C, DCTX), generator=g) / math.sqrt(DCTX)
    ctxd, wd = ctx.to(DEV), w.to(DEV)
    hi, lo = K.cast_f16(ctxd, want_lo=True)
    dh = C // heads
    y = (ctxd.double() @ wd.double().t()).reshape(BKV, NCTX, 2, heads, dh)
    kref = y[:, :, 0].permute(0, 2, 1, 3).reshape(BKV * heads, NCTX, dh)
    vref = y[:, :, 1].permute(0, 2, 3, 1).reshape(BKV * heads, dh, NCTX)
    c = dict(C=C, heads=heads, dh=dh, hi=hi, lo=lo, w3=K.pack_split3(wd), w16=wd.half(), kref=kref, vref=vref)
    _KV[(C, heads)] = c
    return c


def _kv_run(c, tile, splitk, a1='lo', single=False):
    """mode 2: k [B heads][77][dh], v^T [B heads][dh][80] pre-filled with NaN, v^T pad columns zeroed first (as context_kv does)"""
    heads, dh, C = c['heads'], c['dh'], c['C']
    ntp = (NCTX + 7) // 8 * 8
    k = torch.full((BKV * heads, NCTX, dh), float('nan'), dtype=torch.float16, device=DEV)
    vt = torch.full((BKV * heads, dh, ntp), float('nan'), dtype=torch.float16, device=DEV)
    vt[:, :, NCTX:] = 0
    hd = dict(segs=[(k, 0), (vt, 1)], heads=heads, dh=dh, ntok=NCTX, ntok_pad=ntp, segC=C)
    if single:
        K.igemm(c['hi'], c['w16'], 2 * C, BKV, NCTX, 1, NCTX, 1, mode=2, splitk=splitk, tile=tile, heads=hd)
    else:
        K.igemm(c['hi'], c['w3'], 2 * C, BKV, NCTX, 1, NCTX, 1, a1=c['lo'] if a1 == 'lo' else a1, a2=c['hi'], mode=2,
                splitk=splitk, tile=tile, heads=hd)
    torch.cuda.synchronize()
    return k, vt


ULP_FLOOR = 2.0 ** -6


def _ulp_stats(got, ref64):
    """(max fp16-ulp distance to fp16(ref), fraction not equal to it).  Below |ref| = 2^-6 the distance is counted in the fp16
    spacing at 2^-6 (2^-16 = 1.5e-5): there the spacing shrinks toward the absolute error of fp32 accumulation, O(2^-24 sum|x w|)
    ~ 1e-6 here, which no fp32-accumulating kernel avoids where the dot product cancels (measured on an MI355X: 14 - 20 ulps on a
    few outputs below 1e-4, whose spacing is the subnormal 6e-8)."""
    want = ref64.float().half()      # (through fp32: differs from one rounding of the fp64 value only at exact fp32-level ties)
    if not bool(torch.isfinite(got).all()):
        return float('inf'), 1.0
    d = (_ordered(got) - _ordered(want)).abs()
    frac = float((d != 0).double().mean())
    small = ref64.abs() < ULP_FLOOR
    d = torch.where(small, (got.double() - want.double()).abs() / (ULP_FLOOR * 2.0 ** -10), d.double())
    return float(d.max()), frac


def _kv_stats(c, k, vt):
    mk, fk = _ulp_stats(k, c['kref'])
    mv, fv = _ulp_stats(vt[:, :, :NCTX], c['vref'])
    return max(mk, mv), max(fk, fv)


@pytest.mark.parametrize('C,heads', KV, ids=[f'C{c}h{h}' for c, h in KV])
@pytest.mark.parametrize('tile', [-1, 0, 3, 5, 8])
@pytest.mark.parametrize('splitk', [1, 2, 3])
def test_split16_context_kv_head_scatter(C, heads, tile, splitk):
    """the default K / V^T projection of the context (unet.cpp context_kv: three sources, K = 3 x 768, per-head scatter):
    fp16 outputs within 1 ulp of fp16(fp64 reference) everywhere (the ulp at 2^-6 below 2^-6, see _ulp_stats) and equal to it on
    >= 99 %; the v^T pad columns stay +0;
    two runs bit-identical.  (split-K 3 starts its splits on the source changes, 2 inside one.)  Measured on an MI355X: 1 ulp,
    <= 0.42 % not equal, on every shape, tile and split."""
    c = _kv_case(C, heads)
    k, vt = _kv_run(c, tile, splitk)
    mx, frac = _kv_stats(c, k, vt)
    print(f'[split16 K/V C{C} h{heads} tile{tile} k{splitk}] max {mx:.2f} ulp, {100 * frac:.3f} % not equal to fp16(fp64)', flush=True)
    assert mx <= 1 and frac <= 0.01
    assert torch.equal(vt[:, :, NCTX:].view(torch.int16), torch.zeros_like(vt[:, :, NCTX:]).view(torch.int16))
    k2, vt2 = _kv_run(c, tile, splitk)
    assert torch.equal(k.view(torch.int16), k2.view(torch.int16)) and torch.equal(vt.view(torch.int16), vt2.view(torch.int16))


@pytest.mark.parametrize('C,heads', KV[:2], ids=[f'C{c}h{h}' for c, h in KV[:2]])
def test_split16_context_kv_controls(C, heads):
    """the bars separate: fp16 operands, and the three-source GEMM with a1 pointing to zeros (lo dropped), each miss the
    1-ulp bar by >= 10x and the 1 % equality bar by >= 10x (measured on an MI355X: fp16 operands 146 ulp / 50 %, lo dropped
    72 - 94 ulp / 42 %)"""
    c = _kv_case(C, heads)
    for label, run in (('fp16 operands', lambda: _kv_run(c, -1, 1, single=True)),
                       ('without lo', lambda: _kv_run(c, -1, 1, a1=torch.zeros_like(c['lo'])))):
        mx, frac = _kv_stats(c, *run())
        print(f'[split16 K/V C{C} h{heads} {label}] max {mx:.1f} ulp, {100 * frac:.1f} % not equal to fp16(fp64)', flush=True)
        assert mx >= 10 and frac >= 0.10
