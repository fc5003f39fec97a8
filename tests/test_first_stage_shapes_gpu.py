"""Every distinct launch geometry of the mixed-precision first stage (the walk of tests/first_stage_shapes.py over KL-f8, VQ-f4 and VQ-f4 without
mid attention, at a 64 x 64 latent) through the C ABI, in guarded buffers (tests/guard.py), against an fp64 reference computed with torch
on the device; the materialised attention chain of VFwd::attn_block on probe operands; and csrc/vae.cpp's own composition of that chain under
a peaked softmax, against an fp64 decoder, at the case's fp16-operand floor.

Operands are fp16-representable (except the split-fp16 runs, whose operands are fp32) and weights are scaled 1 / sqrt(K), so the fp64 value is the
exact one and the error is the kernel's.  The bars are the project's own:
  fp32 GEMM / conv   3e-4 max(1, sqrt(K / 11520))  (test_model_shapes_gpu._tol32);  fp16 copy 6e-3;  split-fp16 3e-5 max(1, sqrt(K / 1920))
                     (test_model_shapes_gpu._tol_split)
  GroupNorm          f32 2e-5, f16 4e-3, raw 4e-3, raw hi + lo 4e-6 (test_groupnorm of test_model_shapes_gpu.py, test_kernels_gpu.py)
  conv_in, conv_out  2e-5 (test_conv_in_out);  pointwise_nchw 1e-5;  cast_f16 bit-exact;  vq_quantize as test_quantizer_vs_restatement
  softmax_rows       2^-10 ref + 2^-24 per weight;  the chain 2^-9 ref + 2^-25 n_c + 2^-24 per output (first_stage_shapes.softmax_tol / chain_judge;
                     derived there and held against a CPU restatement in test_first_stage_shapes_host.py);  dense V 3e-3 (the attention bar)
  decode             1.5 x the case's fp16-operand floor (FLOOR_MAX_FACTOR of tests/test_unet_gpu.py), the floor from first_stage_shapes.decode64
(a) Every GEMM / conv runs once as the executor requests it -- tile -1, splitk 0 or 1 as csrc/vae.cpp sets it, the executor's 8 Mi-float split-K
workspace, the role's epilogue, batch 1 where a map side is 256 or more and batch 2 below (and batch 1 there as well: the tuning table's rows
for those levels are keyed by the batch-1 M), so that the (M, N, K) keys of the tuning table are the product's -- and again at a 32-pixel map side (1024 tokens for the attention GEMMs), batch 2, on the forced axis of test_model_shapes_gpu.py
(tiles 3 and 5, split-K 1 and 2) with output rows at a pitch of N + 8.  The split-fp16 nin_shortcut runs as launched only (its kernel family
has its own tiles; test_model_shapes_gpu.py does the same).
The Upsample convs run here as the 3x3 conv with the nearest x2 folded into its gather (up = 1), which is what the executor launches under
SDMI_UP_PHASE=0; by default it launches them as the four 2x2 phase convs of one launch wherever the committed phase table has the winning
row (csrc/vae.cpp decode).  That form of every Upsample site of this walk is run by test_model_shapes_gpu.py::test_upsample_conv_in_both_forms
and, for every row of tune_up_phase_gfx950.txt, by tests/test_up_phase_tiles_gpu.py.
After every launch every buffer's guards are checked, inputs must be unchanged bits and the split-K tile counters zero again.

(b) The chain runs each chunk of first_stage_shapes.CHAIN_SHAPES at its row offset r0, at C = 512 and C = 128, under the six score regimes
and the V codings of tests/attn_probes.py.  Liveness (every row has a live output, >= 10 % of the non-empty outputs are live) is asserted from
the fp64 reference for every case but the single-weight `window` codings of the 9216-key softmax (first_stage_shapes.must_be_live: there
fp16 stores most single weights as subnormals; 12 of 348 (chunk, regime, coding) cases, which still meet the bar and the exact zeros).

Skipped cases: none.

Measured on an MI355X (worst max-abs per family | bar):
  3x3 conv fp32 as launched (batch 1 and 2) / forced axis        6.4e-6 / 5.1e-6     | 3e-4
  Upsample / Downsample conv as launched / forced axis            6.7e-6 / 5.2e-6     | 3e-4
  attention GEMMs, fp32 out (scores, proj_out) launched / forced  2.1e-6 / 1.7e-6     | 3e-4
  attention GEMMs, fp16 out (q, k, v^T, P v) launched / forced    1.95e-3 / 1.95e-3   | 6e-3
  split-fp16 nin_shortcut, K = 128 / 256 / 512                    8.6e-6              | 3e-5
  GroupNorm f32 / f16 / raw / raw hi + lo                         9.5e-7 / 1.95e-3 / 2.9e-3 / 9.5e-7 | 2e-5 / 4e-3 / 4e-3 / 4e-6
  conv_in / conv_out / pointwise_nchw                             1.9e-6 / 7.2e-7 / 1.9e-6            | 2e-5 / 2e-5 / 1e-5
  cast_f16, vq_quantize                                           bit-exact; every clear-gap pixel picks the reference's code
  softmax_rows per weight, err / tol                              0.500 at every shape and regime (the fp16 rounding itself)
  chain per output, err / tol (smallest asserted live share)      C = 512: 0.333 .. 0.708 (13.6 %), C = 128: 0.333 .. 0.655 (14.2 %)
      per shape, C = 512 | 128: 64: 0.333 | 0.333, 192: 0.333 | 0.490, 576: 0.494 | 0.647, 1024: 0.498 | 0.644, 1088: 0.587 | 0.655,
      2304: 0.663 | 0.565, 4096: 0.708 | 0.507, rows 8192 .. 9215 of 9216: 0.629 | 0.417  (CPU restatement of the arithmetic: 0.333 .. 0.655)
  chain with dense V and a V bias                                 2.6e-3              | 3e-3
  decode under a peaked softmax, measured / floor                 8 x 8: 0.862 (floor 1.09e-3), 48 x 48: 0.900 (1.25e-3), 64 x 64: 0.945 (1.32e-3) | 1.5
  controls: conv reference without its last 64-channel chunk off by 1.89 (bar 3e-4); the 2304-token chain against a reference whose tail chunk
  is shifted by one row fails on every case of the tail chunk and on none of the first chunk, worst err / tol 9.7e4
Guard findings: none.  The 116 cases take 5 s together."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_probes as A  # noqa: E402
import first_stage_shapes as FS  # noqa: E402
import guard  # noqa: E402
import kernels as K  # noqa: E402
from stable_diffusion_amd import _lib  # noqa: E402
from test_model_shapes_gpu import FORCED, _g, _r16, _randn, _report, _seed, _tol32, _tol_split, _ws_floats  # noqa: E402

DEV = 'cuda'
EXEC_WS_FLOATS = 8 << 20           # run_two_pass: begin_pass((int64_t)8 << 20)
FORCED_SIDE = 32
FLOOR_MAX_FACTOR = 1.50            # tests/test_unet_gpu.py


def _batch(side):
    return 1 if side >= 256 else 2


def _conv_ref64(a, w, Bn, Hin, ksize, stride, up, asym):
    """a [Bn * Hin * Hin, C], w [N, C, k, k] -> fp64 [M, N]: nine shifted fp64 matmuls (no library convolution); asym: zero pad on the right
    and at the bottom only (F.pad(x, (0, 1, 0, 1)) + conv(stride 2, padding 0), model.py:71-79)"""
    C, N = a.shape[1], w.shape[0]
    w64 = w.double()
    if ksize == 1:
        return a.double() @ w64.reshape(N, C).t()
    x = a.double().reshape(Bn, Hin, Hin, C)
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    H = x.shape[1]
    lo = 0 if asym else 1
    Ho = (H + lo + 1 - 3) // stride + 1
    xp = torch.nn.functional.pad(x, (0, 0, lo, 1, lo, 1))
    out = torch.zeros((Bn * Ho * Ho, N), dtype=torch.float64, device=a.device)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Ho - 1) + 1:stride, :]
            out += xs.reshape(-1, C) @ w64[:, :, ky, kx].t()
    return out


class _Gemm:
    """one igemm launch site: operands in guarded buffers, the fp64 reference, `run` for one (tile, split-K) request"""

    def __init__(self, name, Bn, c, N, hin, hout, ksize=1, stride=1, up=0, asym=0, bias=True, resid=False, out='f32', split16=False,
                 splitk=0, ref_drop=0):
        self.name, self.N, self.split16, self.out, self.splitk = name, N, split16, out, splitk
        win, wout = (hin, hout) if ksize == 3 else (1, 1)          # dense: Hin = Hout = the rows of one sample, Win = Wout = 1
        self.geom = (Bn, hin, win, hout, wout, ksize, stride, up)
        self.asym = asym
        self.Kd = ksize * ksize * c
        self.M = M = Bn * hout * wout
        g = _g(_seed(Bn, c, N, hin, hout, ksize, stride, up, split16, asym))
        self.P = P = guard.Pool(DEV)
        rows_in = Bn * hin * win
        if split16:         # fp32 operands: hi | lo halves from the cast kernel, weights [hi | hi | lo] (N(0, 4) operands: test_gemm_split16)
            x = _randn((rows_in, c), g, 2.0)
            w = _randn((N, c, 1, 1), g, 1.0 / math.sqrt(self.Kd))
            hi, lo = K.cast_f16(x, want_lo=True)
            self.a, self.a_lo = P.put('a_hi', hi), P.put('a_lo', lo)
            self.w = P.put('w_split3', K.pack_split3(w.reshape(N, c).contiguous()))
        else:
            x = _r16((rows_in, c), g)
            w = _r16((N, c, ksize, ksize), g, 1.0 / math.sqrt(self.Kd))
            self.a, self.a_lo = P.put('a', x), None
            self.w = P.put('w', K.pack_conv_weight(w.float()))
        if ref_drop:        # control: the reference (only) loses the last `ref_drop` input channels
            x = x.clone()
            x[:, c - ref_drop:] = 0
        ref = _conv_ref64(x, w, Bn, hin, ksize, stride, up, asym)
        self.bias = self.resid0 = None
        if bias:
            self.bias = P.put('bias', _randn((N,), g))
            ref += self.bias.double()[None]
        if resid:
            self.resid0 = _randn((M, N), g)
            ref = ref + self.resid0.double()
        self.ref = ref
        self.inputs = [(v, v.clone()) for v in (self.a, self.a_lo, self.w, self.bias) if v is not None]
        self.cnt = P.new('splitk_cnt', (8192,), torch.int32, fill=0)

    def run(self, tile, splitk, gap=0, as_executor=False):
        P, M, N = self.P, self.M, self.N
        tag = f'{self.name} tile{tile} k{splitk}'
        ldo = N + gap
        n0 = len(P.bufs)
        o32 = P.new('out_f32', (M, N), torch.float32, ld=ldo) if self.out == 'f32' else None
        o16 = P.new('out_f16', (M, N), torch.float16, ld=ldo) if self.out == 'f16' else None
        resid = P.put('residual', self.resid0, ld=ldo) if self.resid0 is not None else None
        ws = P.new('splitk_ws', (EXEC_WS_FLOATS if as_executor else _ws_floats(M, N),), torch.float32, row_bytes=4 * ((N + 255) // 256 * 256))
        Bn, hin, win, hout, wout, ksize, stride, up = self.geom
        K.igemm(self.a, self.w, N, Bn, hin, win, hout, wout, ksize, stride, up, a1=self.a_lo, bias=self.bias, residual=resid, out_f32=o32,
                out_f16=o16, ldo=ldo, tile=tile, splitk=splitk, asym_pad=self.asym, split16=self.split16, ws=ws, cnt=self.cnt)
        torch.cuda.synchronize()
        if self.out == 'f16':
            tol, got = 6e-3, o16
        else:
            tol, got = (_tol_split(self.Kd) if self.split16 else _tol32(self.Kd)), o32
        e = _report(f'{tag} {self.out}', got, self.ref, tol)
        P.check(tag)
        assert int(self.cnt.abs().max()) == 0, f'{tag}: split-K tile counters not left zero'
        for v, keep in self.inputs:
            assert torch.equal(v, keep), f'{tag}: an input operand was modified'
        del P.bufs[n0:]
        return e, tol


def _gemm_kwargs(kind, d, forced):
    """walk dict -> _Gemm arguments at the product size, or at the forced axis' 32-pixel side / 1024 tokens"""
    if kind == 'conv3':
        hin = FORCED_SIDE if forced else d['hin']
        hout = hin * d['hout'] // d['hin']
        return dict(Bn=2 if forced else _batch(max(d['hin'], d['hout'])), c=d['C'], N=d['N'], hin=hin, hout=hout, ksize=3, stride=d['stride'],
                    up=d['up'], asym=d['asym_pad'], resid=d['role'] == 'conv2')
    if kind == 'nin':
        hw = FORCED_SIDE if forced else d['hw']
        return dict(Bn=2 if forced else _batch(d['hw']), c=d['K'], N=d['N'], hin=hw * hw, hout=hw * hw, split16=True)
    nt = FORCED_SIDE * FORCED_SIDE
    M, Kd, N = d['M'], d['K'], d['N']
    if forced:          # a 32 x 32 latent: every token count of the geometry becomes 1024
        M, Kd, N = (nt if d['role'] != 'vt' else M), (nt if d['role'] == 'pv' else Kd), (nt if d['role'] in ('vt', 'scores') else N)
    return dict(Bn=1 if d['per_image'] else 2, c=Kd, N=N, hin=M, hout=M, bias=d['bias'], resid=d['resid'], out=d['out'], splitk=d['splitk'])


def _gemm_cases():
    seen, out = set(), []
    for kind, d in FS.distinct(kinds=('conv3', 'nin', 'dense')):
        d = {k: v for k, v in d.items() if k != 'r0'}          # (a chunk's row offset moves pointers only: the chain test launches at r0)
        key = (kind, tuple(sorted(d.items())))
        if key not in seen:
            seen.add(key)
            out.append(pytest.param(kind, d, id=FS.case_id(kind, d)))
    return out


@pytest.mark.parametrize('kind,d', _gemm_cases())
def test_gemm_and_conv(kind, d):
    """3x3 convs (bias; bias + residual; nearest x2 folded; stride 2 with the pad on the right and bottom only), the split-fp16 nin_shortcut and
    the six GEMMs of the attention block (activations as the `w` operand, ldo = ntok, K = ntok), as launched and on the forced axis"""
    name = FS.case_id(kind, d)
    kw = _gemm_kwargs(kind, d, False)
    res = []
    # (the tuning table's rows for the levels below 256^2 were collected at batch 1: M = 4096 / 16384.  Batch 2 there takes the heuristic
    # branch of launch_igemm, batch 1 the table's tile where it has a row; both are launches the product makes)
    for Bn in ((2, 1) if kw['Bn'] == 2 and not d.get('per_image') else (kw['Bn'],)):
        c = _Gemm(f'{name} B{Bn}', **dict(kw, Bn=Bn))
        res.append(c.run(-1, c.splitk, as_executor=True))
        del c
        torch.cuda.empty_cache()
    if kind != 'nin':
        f = _Gemm(name + f' side{FORCED_SIDE}', **_gemm_kwargs(kind, d, True))
        res += [f.run(t, k, gap=8) for t, k in FORCED]
    for e, tol in res:
        assert e < tol, (e, tol)


# ---- GroupNorm, cast, the fp32 ends -----------------------------------------------------------------------------------------------------------
def _cases_of(kind):
    return [pytest.param(d, id=FS.case_id(kind, d)) for _, d in FS.distinct(kinds=(kind,))]


@pytest.mark.parametrize('d', _cases_of('gn'))
def test_groupnorm(d):
    """GroupNorm(32, eps 1e-6) at 4 .. 16 channels per group over up to 262 144 pixels, with exactly the outputs the executor asks for: f16
    (+ SiLU), f16 | raw | raw_lo in front of a nin_shortcut, f32 in front of conv_out, f16 without SiLU in front of the attention"""
    C, hw, silu, outs = d['C'], d['hw'], d['silu'], d['outs']
    Bn, HW = _batch(hw), hw * hw
    g = _g(_seed(C, hw, silu, len(outs)))
    P = guard.Pool(DEV)
    x = P.put('x', _randn((Bn, HW, C), g, 1.5) + 0.3)
    gamma, beta = P.put('gamma', 1 + 0.1 * _randn((C,), g)), P.put('beta', 0.1 * _randn((C,), g))
    keep = x.clone()
    o = {nm: P.new(nm, (Bn, HW, C), torch.float32 if nm == 'f32' else torch.float16) for nm in outs}
    n = _lib.load().sdmi_k_groupnorm_ws_floats(Bn, HW)
    ws = P.new('gn_ws', (n,), torch.float32)
    _lib.check(_lib.load().sdmi_k_groupnorm(x.data_ptr(), None, C, 0, Bn, HW, gamma.data_ptr(), beta.data_ptr(), 1e-6, silu, _lib.ptr(o.get('f16')),
                                            _lib.ptr(o.get('f32')), _lib.ptr(o.get('raw')), None, _lib.ptr(o.get('raw_lo')), ws.data_ptr(), n,
                                            _lib.stream_ptr()))
    torch.cuda.synchronize()
    x64 = x.double().reshape(Bn, HW, 32, C // 32)
    mean = x64.mean((1, 3), keepdim=True)
    var = ((x64 - mean) ** 2).mean((1, 3), keepdim=True)
    ref = ((x64 - mean) / torch.sqrt(var + 1e-6)).reshape(Bn, HW, C) * gamma.double() + beta.double()
    if silu:
        ref = ref * torch.sigmoid(ref)
    tag = FS.case_id('gn', d)
    e = []
    if 'f32' in o:
        e.append((_report(f'{tag} f32', o['f32'], ref, 2e-5), 2e-5))
    if 'f16' in o:
        e.append((_report(f'{tag} f16', o['f16'], ref, 4e-3), 4e-3))
    if 'raw' in o:
        e.append((_report(f'{tag} raw', o['raw'], x, 4e-3), 4e-3))
        e.append((_report(f'{tag} raw hi+lo', o['raw'].float() + o['raw_lo'].float(), x, 4e-6), 4e-6))
    P.check(tag)
    assert torch.equal(x, keep)
    for err, tol in e:
        assert err < tol, (err, tol)


@pytest.mark.parametrize('d', _cases_of('cast'))
def test_cast_f16(d):
    """the fp16 copy of the stream in front of a resampling conv: the round-to-nearest fp16 of every element, bit for bit"""
    hw, C = d['hw'], d['C']
    n = _batch(hw) * hw * hw * C
    P = guard.Pool(DEV)
    x = P.put('x', _randn((n,), _g(_seed(hw, C)), 2.0))
    hi = P.new('hi', (n,), torch.float16)
    _lib.check(_lib.load().sdmi_k_cast_f16(x.data_ptr(), hi.data_ptr(), None, n, _lib.stream_ptr()))
    torch.cuda.synchronize()
    P.check(FS.case_id('cast', d))
    assert torch.equal(hi, x.half())


@pytest.mark.parametrize('d', _cases_of('conv_in'))
def test_conv_in(d):
    Cin, Cout, hw = d['cin'], d['N'], d['hw']
    Bn = _batch(hw)
    g = _g(_seed(Cin, Cout, hw))
    P = guard.Pool(DEV)
    x = P.put('x', _randn((Bn, Cin, hw, hw), g))
    w = P.put('w', _randn((Cout, Cin, 3, 3), g, 1.0 / math.sqrt(9 * Cin)))
    b = P.put('bias', _randn((Cout,), g, 0.1))
    out = P.new('out', (Bn, hw * hw, Cout), torch.float32)
    _lib.check(_lib.load().sdmi_k_conv_in(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), Bn, Cin, hw, hw, Cout, _lib.stream_ptr()))
    torch.cuda.synchronize()
    xn = x.permute(0, 2, 3, 1).reshape(Bn * hw * hw, Cin)
    ref = _conv_ref64(xn, w, Bn, hw, 3, 1, 0, 0) + b.double()[None]
    e = _report(FS.case_id('conv_in', d), out, ref, 2e-5)
    P.check('conv_in')
    assert e < 2e-5           # (test_conv_in_out)


@pytest.mark.parametrize('d', _cases_of('conv_out'))
def test_conv_out(d):
    Cin, Cout, hw = d['cin'], d['N'], d['hw']
    Bn = _batch(hw)
    g = _g(_seed(Cin, Cout, hw, 1))
    P = guard.Pool(DEV)
    h = P.put('h', _randn((Bn, hw * hw, Cin), g))
    w = _randn((Cout, Cin, 3, 3), g, 1.0 / math.sqrt(9 * Cin))
    b = P.put('bias', _randn((Cout,), g, 0.1))
    w_d = P.put('w', w)
    wp = P.new('w_ohwi', (Cout, 3, 3, Cin), torch.float32)
    lib = _lib.load()
    _lib.check(lib.sdmi_k_pack_conv_out(w_d.data_ptr(), wp.data_ptr(), Cout, Cin, _lib.stream_ptr()))
    out = P.new('out', (Bn, Cout, hw, hw), torch.float32)
    _lib.check(lib.sdmi_k_conv_out(h.data_ptr(), wp.data_ptr(), b.data_ptr(), out.data_ptr(), Bn, hw, hw, Cin, Cout, _lib.stream_ptr()))
    torch.cuda.synchronize()
    ref = (_conv_ref64(h.reshape(Bn * hw * hw, Cin), w, Bn, hw, 3, 1, 0, 0) + b.double()[None]).reshape(Bn, hw, hw, Cout)
    e = _report(FS.case_id('conv_out', d), out.permute(0, 2, 3, 1), ref, 2e-5)
    P.check('conv_out')
    assert e < 2e-5


@pytest.mark.parametrize('d', _cases_of('pointwise'))
def test_pointwise_nchw(d):
    """post_quant_conv (3 -> 3; 4 -> 4 with the latent's 1 / scale_factor as in_scale) and quant_conv (3 -> 3, 8 -> 8)"""
    Cin, Cout, hw = d['cin'], d['N'], d['hw']
    Bn = _batch(hw)
    scale = 1.0 / 0.18215 if d['in_scale'] else 1.0
    g = _g(_seed(Cin, Cout, hw, 2))
    P = guard.Pool(DEV)
    x, w, b = P.put('x', _r16((Bn, Cin, hw, hw), g).float()), P.put('w', _randn((Cout, Cin), g, 1.0 / math.sqrt(Cin))), P.put('b', _randn((Cout,), g))
    out = P.new('out', (Bn, Cout, hw, hw), torch.float32)
    _lib.check(_lib.load().sdmi_k_pointwise_nchw(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), Bn, Cin, Cout, hw * hw, scale,
                                                 _lib.stream_ptr()))
    torch.cuda.synchronize()
    s32 = float(torch.tensor(scale, dtype=torch.float32))           # the fp32 value the kernel receives
    ref = torch.einsum('oc,bchw->bohw', w.double(), x.double() * s32) + b.double()[None, :, None, None]
    e = _report(FS.case_id('pointwise', d), out.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1), 1e-5)
    P.check('pointwise_nchw')
    assert e < 1e-5           # (test_model_shapes_gpu._ep_pointwise_nchw)


@pytest.mark.parametrize('d', _cases_of('vq_quantize'))
def test_vq_quantize(d):
    """the 8192 x 3 codebook over a 64 x 64 code: the checks of test_inpaint_gpu.py::test_quantizer_vs_restatement, in guarded buffers"""
    import vq_ref
    n_embed, D, hw = d['n_embed'], d['D'], d['hw']
    Bn = _batch(hw)
    g = torch.Generator().manual_seed(n_embed + D)
    e, z = torch.randn(n_embed, D, generator=g), torch.randn(Bn, D, hw, hw, generator=g)
    P = guard.Pool(DEV)
    z_d, e_d = P.put('z', z.to(DEV)), P.put('codebook', e.to(DEV))
    zq, idx = P.new('zq', (Bn, D, hw, hw), torch.float32), P.new('idx', (Bn, hw * hw), torch.int32)
    norms = P.new('norms_ws', (n_embed,), torch.float32)
    _lib.check(_lib.load().sdmi_k_vq_quantize(z_d.data_ptr(), 1.0, e_d.data_ptr(), norms.data_ptr(), n_embed, D, zq.data_ptr(), idx.data_ptr(), Bn,
                                              hw * hw, _lib.stream_ptr()))
    torch.cuda.synchronize()
    P.check('vq_quantize')
    assert torch.equal(z_d.cpu(), z) and torch.equal(e_d.cpu(), e)
    _, ref_idx = vq_ref.quantize(z, e)
    dist = vq_ref.distances(z, e).double()
    best = dist.gather(1, ref_idx.view(-1, 1)).squeeze(1)
    second = dist.scatter(1, ref_idx.view(-1, 1), float('inf')).min(1).values
    clear = (second - best) > 1e-5 * best.abs().clamp_min(1e-30)
    mine = idx.long().cpu().view(-1)
    assert torch.equal(mine[clear], ref_idx.view(-1)[clear])
    db = dist.gather(1, mine.view(-1, 1)).squeeze(1)
    assert bool(((db - best) <= 1e-5 * best.abs().clamp_min(1e-30) + 1e-6).all())
    assert torch.equal(zq.cpu(), vq_ref.straight_through(z, e, idx.long().cpu().view(Bn, hw, hw)))


# ---- the materialised attention chain ------------------------------------------------------------------------------------------------------------
class _Chain:
    """q [ntok, C], k [ntok, C] in guarded buffers; `scores_softmax` and `pv` launch one chunk exactly as VFwd::attn_block does: the fp32
    score GEMM with the k activations as `w` and ldo = ntok, softmax_rows, then P v^T with K = ntok and the V bias, all with splitk = 1 and
    pointer offsets r0"""

    def __init__(self, C, ntok, q, k):
        self.C, self.ntok, self.scale = C, ntok, 1.0 / math.sqrt(C)
        self.P = P = guard.Pool(DEV)
        self.q, self.k = P.put('q', q.to(DEV)), P.put('k', k.to(DEV))
        qc = min(ntok, FS.QC_MAX)
        self.S = P.new('S', (qc, ntok), torch.float32)
        self.Pm = P.new('P', (qc, ntok), torch.float16)
        self.cnt = P.new('splitk_cnt', (8192,), torch.int32, fill=0)
        self.ws = P.new('splitk_ws', (EXEC_WS_FLOATS,), torch.float32, row_bytes=4 * 512)
        self.keep = [(v, v.clone()) for v in (self.q, self.k)]

    def scores_softmax(self, r0, rows):
        C, ntok = self.C, self.ntok
        self.S.view(torch.int32).fill_(-1)
        self.Pm.view(torch.int16).fill_(-1)
        K.igemm(self.q[r0:r0 + rows], self.k, ntok, 1, rows, 1, rows, 1, out_f32=self.S, ldo=ntok, splitk=1, ws=self.ws, cnt=self.cnt)
        _lib.check(_lib.load().sdmi_k_softmax_rows(self.S.data_ptr(), self.Pm.data_ptr(), rows, ntok, self.scale, _lib.stream_ptr()))
        torch.cuda.synchronize()
        if rows < self.S.shape[0]:          # a tail chunk writes its own rows only
            assert bool((self.S[rows:].view(torch.int32) == -1).all()) and bool((self.Pm[rows:].view(torch.int16) == -1).all())
        return self.S[:rows], self.Pm[:rows]

    def pv(self, r0, rows, vt, bias, ao):
        K.igemm(self.Pm[:rows], vt, self.C, 1, rows, 1, rows, 1, bias=bias, out_f16=ao[r0:r0 + rows], ldo=self.C, splitk=1, ws=self.ws,
                cnt=self.cnt)
        torch.cuda.synchronize()

    def check(self, tag):
        self.P.check(tag)
        assert int(self.cnt.abs().max()) == 0, f'{tag}: split-K tile counters not left zero'
        for v, keep in self.keep:
            assert torch.equal(v, keep), f'{tag}: an input operand was modified'


def _chain_cases():
    return [pytest.param(C, ntok, ch, id=f'C{C}-ntok{ntok}-rows{sum(r for _, r in ch)}') for C in FS.CHAIN_C for ntok, ch in FS.CHAIN_SHAPES]


def _run_chain_probes(C, ntok, chunk_list, ref_shift=0):
    """-> (worst chain err / tol, worst softmax err / tol, smallest asserted live share, list of failures); ref_shift: the control -- the
    REFERENCE weights of a tail chunk (the last one launched) are shifted by that many rows"""
    bad, worst, worst_sm, least = [], 0.0, 0.0, 1.0
    zero_bias = None
    for ri, regime in enumerate(A.REGIMES):
        q, k = A.make_qk(regime, 1, ntok, ntok, C, FS.chain_seed(C, ntok, ri))
        ch = _Chain(C, ntok, q[0], k[0])
        Pv = guard.Pool(DEV)
        zero_bias = Pv.put('bias', torch.zeros((C,), device=DEV))
        codes = A.codings(regime, ntok, C)
        vts = [Pv.put(f'vt {name}', A.dense_v(col, 1, C)[0].t().contiguous().to(DEV)) for name, col in codes]
        aos = [Pv.new(f'ao {name}', (ntok, C), torch.float16) for name, _ in codes]
        for ci, (r0, rows) in enumerate(chunk_list):
            tag = f'chain C{C} ntok{ntok} r0 {r0} rows {rows} {regime}'
            S, Pm = ch.scores_softmax(r0, rows)
            Pref, _ = A.softmax_ref(ch.q[r0:r0 + rows][None], ch.k[None], ch.scale)
            Pref = Pref[0]
            # softmax_rows alone, per element, against the fp64 softmax of the fp32 scores it was given
            Psm = torch.softmax(S.double() * float(torch.tensor(ch.scale, dtype=torch.float32)), dim=1)
            sm = float(((Pm.double() - Psm).abs() / FS.softmax_tol(Psm)).max())
            sm = sm if math.isfinite(sm) else float('inf')
            worst_sm = max(worst_sm, sm)
            if ref_shift and ci == len(chunk_list) - 1:
                Pref = Pref.roll(ref_shift, 0)
            for (name, col), vt, ao in zip(codes, vts, aos):
                ch.pv(r0, rows, vt, zero_bias, ao)
                j = FS.chain_judge(ao[r0:r0 + rows].double(), Pref, col, C)
                must = FS.must_be_live(name, ntok)
                print(f'[{tag}/{name}] chain worst err / tol {j["worst"]:.3f} at flat {j["at"]}, softmax alone {sm:.3f}, live {100 * j["share"]:.1f} %'
                      f'{"" if must else " (single weights, not asserted)"}, every row live {j["rows_live"]}, empty columns exactly 0: '
                      f'{j["zeros_exact"]}', flush=True)
                worst = max(worst, j['worst'])
                if must:
                    least = min(least, j['share'])
                if not (j['worst'] <= 1.0 and sm <= 1.0 and j['zeros_exact'] and (not must or (j['rows_live'] and j['share'] >= 0.10))):
                    bad.append((regime, name, r0, j, sm))
            ch.check(tag)
            Pv.check(tag)
    print(f'[chain C{C} ntok{ntok} SUMMARY] worst err / tol: chain {worst:.3f}, softmax alone {worst_sm:.3f}; smallest live share {100 * least:.1f} %',
          flush=True)
    return worst, worst_sm, least, bad


@pytest.mark.parametrize('C,ntok,chunk_list', _chain_cases())
def test_attention_chain_probes(C, ntok, chunk_list):
    """S = q_chunk k^T, softmax_rows, P v^T with an indicator V under the six score regimes: every output is a sum of softmax weights and is
    held to 2^-9 ref + 2^-25 n_c + 2^-24; softmax_rows' own output to 2^-10 ref + 2^-24 per weight; an output that codes no key is exactly 0"""
    _, _, _, bad = _run_chain_probes(C, ntok, chunk_list)
    assert not bad, bad


@pytest.mark.parametrize('C,ntok,chunk_list', _chain_cases())
def test_attention_chain_dense_v(C, ntok, chunk_list):
    """the same launches with v ~ N(0, 1) and a non-zero V bias, at the project's 3e-3 attention bar"""
    g = _g(_seed(C, ntok, 3))
    q, k, v = _r16((ntok, C), g), _r16((ntok, C), g), _r16((ntok, C), g)
    q[0] *= 6.0
    k[ntok - 1] *= 6.0          # (a few large scores, as test_model_shapes_gpu.test_attention)
    ch = _Chain(C, ntok, q, k)
    Pv = guard.Pool(DEV)
    vt, bias = Pv.put('vt', v.t().contiguous()), Pv.put('bias', _randn((C,), g))
    ao = Pv.new('ao', (ntok, C), torch.float16)
    worst = 0.0
    for r0, rows in chunk_list:
        ch.scores_softmax(r0, rows)
        ch.pv(r0, rows, vt, bias, ao)
        ref = torch.softmax(ch.q[r0:r0 + rows].double() @ ch.k.double().t() * ch.scale, dim=1) @ v.double() + bias.double()
        worst = max(worst, _report(f'chain dense V C{C} ntok{ntok} r0 {r0} rows {rows}', ao[r0:r0 + rows], ref, 3e-3))
        ch.check('chain dense V')
        Pv.check('chain dense V')
    assert worst < 3e-3


# ---- csrc/vae.cpp's own composition under a peaked softmax ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('latent', [8, 48, 64])
def test_decode_with_peaked_attention(latent):
    """the tiny first stage with the sharpened q / k and the enlarged V bias (first_stage_shapes.peaked_state_dict; conditions and mutant controls
    in test_first_stage_shapes_host.py) through AutoencoderKLHIP, batch 2: one chunk (64 tokens), a chunk and a tail (2304), two chunks (4096),
    the per-image loop, the bias behind P v.  Against the fp64 decoder, at 1.5 x the case's own fp16-operand floor."""
    from oracle import vae_ref
    from stable_diffusion_amd import AutoencoderKLHIP
    cfg = vae_ref.VAEConfig(ch=64, ch_mult=(1, 2), num_res_blocks=1)
    sd = FS.peaked_state_dict(cfg, 0)
    m = AutoencoderKLHIP(cfg.ddconfig(), None, cfg.embed_dim)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    z = vae_ref.make_vae_inputs(cfg, 2, latent, latent, seed=1).to(DEV)
    img = m.decode(z)
    torch.cuda.synchronize()
    info = {}
    ref = FS.decode64(sd, cfg, z, info=info)
    floor = float((FS.decode64(sd, cfg, z, r16=True) - ref).abs().max())
    err = float((img.double() - ref).abs().max())
    print(f'[peaked decode latent {latent}] max-abs {err:.3e}, fp16-operand floor {floor:.3e}, measured / floor {err / floor:.3f} (bar '
          f'{FLOOR_MAX_FACTOR}), |img| max {float(ref.abs().max()):.3f}, mean row maximum {float(info["rowmax"].mean()):.3f}', flush=True)
    assert bool(torch.isfinite(img).all())
    assert err <= FLOOR_MAX_FACTOR * floor, (err, floor)


# ---- controls: the checks above cannot pass vacuously -------------------------------------------------------------------------------------------
def test_control_conv_reference_without_one_chunk():
    """512 -> 512, 3x3 at 64 x 64 (K = 4608): with the last 64-channel chunk dropped from the REFERENCE only, the error must miss that case's bar
    at least tenfold"""
    kw = dict(Bn=2, c=512, N=512, hin=64, hout=64, ksize=3)
    assert any(k == 'conv3' and (d['C'], d['N'], d['hin'], d['role']) == (512, 512, 64, 'conv1') for k, d in FS.distinct())
    e, tol = _Gemm('control conv, reference without the last chunk', ref_drop=64, **kw).run(-1, 0, as_executor=True)
    assert tol == _tol32(4608) and e > 10 * tol, (e, tol)
    e, tol = _Gemm('control conv, whole reference', **kw).run(-1, 0, as_executor=True)
    assert e < tol


def test_control_chain_reference_with_a_shifted_tail():
    """the 2304-token chain (a chunk of 2048 rows, a tail of 256) checked against a reference whose tail chunk is shifted by one row must fail"""
    ntok, chunk_list = FS.CHAIN_SHAPES[5]
    assert ntok == 2304 and chunk_list == [(0, 2048), (2048, 256)]
    worst, _, _, bad = _run_chain_probes(128, ntok, chunk_list, ref_shift=1)
    assert bad and all(r0 == 2048 for _, _, r0, _, _ in bad) and worst > 10.0
