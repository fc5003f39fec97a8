"""Every distinct launch geometry of the class-conditional ImageNet (CIN), latent-inpainting and LAION-400M UNets (the walk of
tests/model_shapes.py, at the product sizes and batch 2) through the C ABI, in guarded buffers (tests/guard.py), against an fp64
reference computed with torch on the device.

Operands are fp16-representable (except the split-fp16 runs, whose operands are fp32), so the fp64 value is the exact one and the
error is the kernel's.  The bars are the project's own, written once here:
  GEMM / conv   fp32 output 3e-4 max-abs up to K = 11520 (test_igemm_splitk_sd_shapes), 3e-4 sqrt(K / 11520) beyond (same operands, weights
                scaled 1 / sqrt(K): the rounding error of the accumulation grows as sqrt(K)); fp16 copy 6e-3; GEGLU 4e-3 (test_igemm_geglu);
                head scatter 4e-3, 6e-3 when split along K (test_igemm_head_scatter(_splitk)); split-fp16 3e-5 (test_gemm_split16)
  GroupNorm     2e-5 / 4e-3 / 4e-6 (test_groupnorm)
  statistics    sum of squares 1e-5 relative; sum 2e-3 absolute up to 40 960 elements per group (test_conv3halo holds it at that size), linear
                in the element count above (each element adds at most one fp32 rounding of an O(1) value before the exact fixed-point add)
  attention     3e-3, 4e-3 for the wide-head and the causal kernels; split-fp16 1e-5 of max|O| (test_attention_split16)
Every GEMM / conv runs once with the executor's dispatch request (tile = -1, splitk = 0, a workspace given), its source layout (a concat
is one buffer of c0 + c1 channels) and the bias / row vector / residual / statistics epilogue of its role; again on split-fp16 operands
for the roles that have them (the 1x1 convs and projections on the stream; the two 3x3 convs of the last ResBlock as the K-concatenated
three-source product); and on a thin forced axis that pins what the heuristic of launch_igemm can choose (tiles 3 and 5, split-K 1 and 2;
there the concat is launched as two sources a0 | a1, the skip conv also carries a residual and a statistics target, and output rows are
at a pitch of N + 8, so that a store past the N tail of a row lands in a gap).
Two roles are launched by the executor in another form than that request since the skip fold and the phase convs, and run here in that form
too, for these models and for SD v1 (model_shapes 'sdv1': oracle.plan.SD_V1 at a 64 x 64 latent, 77 tokens):
  conv2 + skip   where the committed table sends conv2 to a halo-staged tile the skip convolution is the 1x1 tail of conv2's launch
                 (sdmi_k_igemm_tail; bias2 + bias_skip, no residual): test_conv2_with_the_skip_tail_as_launched runs every distinct folding
                 site (model_shapes.folds, pinned against sdmi_unet_skip_fold_plan on the CPU) at the bars of test_skip_fold_shapes_gpu.py.
                 test_plain_gemm_and_conv above runs the same sites as the two launches of SDMI_SKIP_FOLD=0 (and of every block that does
                 not fold)
  up             the Upsample conv is the four 2x2 phase convs of one launch where the table's phase row beats the up = 1 row by 3 %
                 (SDMI_UP_PHASE=1, the default), the 3x3 conv with the folded upsampling otherwise: test_upsample_conv_in_both_forms runs
                 every distinct site, the first stages' included, in both forms, which is each setting of the knob without restating the rule
NOT run here -- these launch variants of the executor stay covered by the whole-UNet goldens (and, at SD's shapes only, by their own
kernel tests): GroupNorm + SiLU applied inside the split-K reduction of a ResBlock's conv1 (pgn_*; test_igemm_splitk_reduce_groupnorm_
behind_a_grid_barrier runs 40 / 20 / 16 channels per group, the new models have 18 .. 32); out_lo of the last FF-out; the one-token context
broadcast that replaces to_q and the nkv = 1 attention in CIN by default (SDMI_CTX1; the general path it replaces IS run here); and the
statistics conv_in emits itself (the C ABI of sdmi_k_conv_in has no statistics arguments; the walk lists its targets).
The LayerNorm fold of the transformer blocks (f16_scale + lnp_out producers, lnf_* consumers without bias) is run by tests/test_ln_fold_gpu.py,
at every transformer width of these models; the dense cases here run the plain bias / residual epilogues.
The split-fp16 bar is 3e-5 up to K = 1920 and grows as sqrt(K) beyond (_tol_split: derivation and the one case it matters for).
After every launch every buffer's guards are checked, the split-K tile counters must be zero again, and inputs must be unchanged bits.

Skipped cases: none.  Contract notes: the key-split attention kernel is dispatched only for nkv % 128 == 0, so its ragged case is ragged
in nq alone; the register-staged attention kernel is reached only by causal launches (every head dim is a multiple of 8), so the causal
case is its ragged case."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import kernels as K  # noqa: E402
import model_shapes as MS  # noqa: E402
from stable_diffusion_amd import _lib  # noqa: E402

DEV = 'cuda'
B = 2
FORCED = [(3, 1), (3, 2), (5, 1), (5, 2)]


def _g(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, device=DEV) * scale


def _r16(shape, g, scale=1.0):
    return _randn(shape, g, scale).half()


def _seed(*xs):
    return sum((i + 1) * 7919 * int(x) for i, x in enumerate(xs)) % (2 ** 31)


def _report(name, got, ref, tol):
    """K.report on the row that holds the worst element (the whole tensors stay on the device); NaN anywhere is reported as inf"""
    got2 = got.reshape(-1, got.shape[-1])
    ref2 = ref.reshape(-1, ref.shape[-1])
    d = (got2.double() - ref2.double()).abs()
    if not bool(torch.isfinite(got2.float()).all()):
        bad = (~torch.isfinite(got2.float())).nonzero()[0].tolist()
        print(f'[{name}] non-finite output at row {bad[0]} col {bad[1]} of {tuple(got2.shape)}', flush=True)
        return float('inf')
    r = int(d.max(1).values.argmax())
    return K.report(name, got2[r], ref2[r].float(), tol)


def _tol32(Kd):
    return 3e-4 * max(1.0, math.sqrt(Kd / 11520.0))


def _tol_split(Kd):
    """split-fp16 products on N(0, 4) operands with weights scaled 1 / sqrt(K): 3e-5 is the bar test_gemm_split16 holds with exactly these
    operands, whose longest K is 1920.  Beyond that K the same law as _tol32 applies, for the same reason: the operands are exact to 2^-22,
    what is left is the rounding of one fp32 accumulator chain over K products of fixed variance, which grows as sqrt(K).  The split16 1x1
    convs / projections of the two UNets have K <= 1920 (bar 3e-5 unchanged) but for the inpainting K = 2048 skip conv (3.1e-5; 7.6e-6 measured); the last ResBlock's three-source 3x3 convs have K = 9 Cin = 1728 ..
    4608 algorithmic products (the lo terms ride in the same chain, a factor 2^-11 smaller): 3e-5 .. 4.65e-5.
    Measured on an MI355X: (256 | 256) -> 256 at 128 x 128, K = 4608, as launched (tile 3, no split-K): 3.05e-5 on outputs up to 12.1, i.e.
    2.5e-6 relative -- over a flat 3e-5, inside 4.65e-5; the other three stay under 3e-5 (1.1e-5 .. 2.4e-5)."""
    return 3e-5 * max(1.0, math.sqrt(Kd / 1920.0))


def _conv_ref64(a, w, Bn, Hin, Win, ksize, stride, up):
    """a [Bn*Hin*Win, C] fp16 / fp32, w [N, C, k, k] -> fp64 [M, N]: nine shifted fp64 matmuls (no library convolution)"""
    C = a.shape[1]
    N = w.shape[0]
    x = a.double().reshape(Bn, Hin, Win, C)
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    H, W_ = x.shape[1], x.shape[2]
    w64 = w.double()
    if ksize == 1:
        return x.reshape(-1, C) @ w64.reshape(N, C).t()
    Ho, Wo = (H - 1) // stride + 1, (W_ - 1) // stride + 1
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros((Bn * Ho * Wo, N), dtype=torch.float64, device=a.device)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]
            out += xs.reshape(-1, C) @ w64[:, :, ky, kx].t()
    return out


def _ws_floats(M, N):
    """slabs for every split the auto choice of launch_igemm can want (so the workspace never limits it) and for the forced splits"""
    rM, rN = (M + 255) // 256 * 256, (N + 255) // 256 * 256
    blocks = (rM // 256) * ((N + 127) // 128)
    return min(16, 2 * max(1, -(-512 // blocks))) * rM * rN


def _stats_errors(out, HW, targets, accs):
    """[(|sum err|, rel sumsq err, sum bar)] of the accumulated GroupNorm statistics against fp64 sums over the stored output"""
    Bn = out.shape[0] // HW
    N = out.shape[1]
    v = out.double().reshape(Bn, HW, N)
    cs, css = v.sum(1), (v * v).sum(1)
    res = []
    for (cpg, cbase), acc in zip(targets, accs):
        gi = (cbase + torch.arange(N, device=out.device)) // cpg
        ng = max(32, (cbase + N - 1) // cpg + 1)         # (a control's shifted reference may reach a 33rd group: kept in range, then cut)
        rs = torch.zeros((Bn, ng), dtype=torch.float64, device=out.device).index_add_(1, gi, cs)[:, :32].cpu()
        rss = torch.zeros((Bn, ng), dtype=torch.float64, device=out.device).index_add_(1, gi, css)[:, :32].cpu()
        s, ss = K.gn_acc_sums(acc)
        res.append(((s - rs).abs().max().item(), ((ss - rss).abs() / (1.0 + rss)).max().item(), 2e-3 * max(1.0, HW * cpg / 40960.0)))
    return res


class _Case:
    """one GEMM / conv geometry: operands in guarded buffers, the fp64 reference, and `run` for one (tile, split-K) choice"""

    def __init__(self, name, c0, c1, N, Hin, Win, Hout, Wout, ksize=1, stride=1, up=0, bias=True, rowvec=False, resid=False, inplace=False,
                 gn=(), split16=False, split3=False, ref_drop=0, bare_as_executor=False):
        self.name, self.N, self.ksize, self.split16, self.inplace = name, N, ksize, split16, inplace
        self.geom = (B, Hin, Win, Hout, Wout, ksize, stride, up)
        self.c0, self.c1 = c0, c1
        Cin = c0 + c1
        self.Kd = ksize * ksize * Cin
        self.M = M = B * Hout * Wout
        self.HW = Hout * Wout
        self.targets = list(gn)
        self.bare_as_executor = bare_as_executor
        g = _g(_seed(c0, c1, N, Hin, Hout, ksize, stride, up, split16))
        self.P = P = guard.Pool(DEV)
        self.split3 = split3
        if split3:          # the last ResBlock: fp32 operands as the K-concatenated 3-pass product [hi | lo | hi] x [w_hi | w_hi | w_lo]; the
            # N(0, 4) operands of the split16 cases below and of test_gemm_split16, bar _tol_split (see there)
            x = _randn((B * Hin * Win, Cin), g, 2.0)
            w = _randn((N, Cin, ksize, ksize), g, 1.0 / math.sqrt(self.Kd))
            hi, lo = K.cast_f16(x, want_lo=True)
            self.a, self.a_lo = P.put('a_hi', hi), P.put('a_lo', lo)
            self.w = P.put('w_conv_split3', K.pack_conv_split3(w))
            self.c0, self.c1 = Cin, 0
        elif split16:       # fp32 operands: hi | lo halves from the cast kernel, weights [hi | hi | lo]
            x = _randn((B * Hin * Win, Cin), g, 2.0)
            w = _randn((N, Cin, ksize, ksize), g, 1.0 / math.sqrt(self.Kd))
            hi, lo = K.cast_f16(x, want_lo=True)
            self.a, self.a_lo = P.put('a_hi', hi), P.put('a_lo', lo)
            self.w = P.put('w_split3', K.pack_split3(w.reshape(N, Cin).contiguous()))
        else:               # the channel concat is one buffer: the two sources are column slices at one row pitch, as in the executor
            x = _r16((B * Hin * Win, Cin), g)
            w = _r16((N, Cin, ksize, ksize), g, 1.0 / math.sqrt(self.Kd))
            self.a, self.a_lo = P.put('a', x), None
            self.w = P.put('w', K.pack_conv_weight(w.float()))
        if ref_drop:        # control: the reference (only) loses the last `ref_drop` channels of the second source
            x = x.clone()
            x[:, Cin - ref_drop:] = 0
        ref = _conv_ref64(x, w, B, Hin, Win, ksize, stride, up)
        self.bias = self.rowvec = self.resid0 = None
        if bias:
            self.bias = P.put('bias', _randn((N,), g))
            ref += self.bias.double()[None]
        if rowvec:
            self.rowvec = P.put('rowvec', _randn((B, N), g))
            ref += self.rowvec.double().repeat_interleave(self.HW, dim=0)
        self.ref_bare = ref
        if resid:
            self.resid0 = _randn((M, N), g)
            ref = ref + self.resid0.double()
        self.ref = ref
        self.inputs = [(v, v.clone()) for v in (self.a, self.a_lo, self.w, self.bias, self.rowvec) if v is not None]
        self.cnt = P.new('splitk_cnt', (8192,), torch.int32, fill=0)

    def run(self, tile, splitk, gap=0, want16=True, as_executor=False):
        P, M, N = self.P, self.M, self.N
        tag = f'{self.name} tile{tile} k{splitk}'
        ldo = N + gap
        n0 = len(P.bufs)
        out = P.new('out_f32', (M, N), torch.float32, ld=ldo)
        resid = None
        # as_executor: the concat is ONE buffer of c0 + c1 channels (GroupNorm wrote it), and the skip conv has a bias only (csrc/unet.cpp
        # res_block); the forced runs keep the two-source launch and the residual + statistics epilogue on the skip conv (a superset)
        bare = as_executor and self.bare_as_executor
        ref = self.ref_bare if bare else self.ref
        targets = [] if bare else self.targets
        if self.resid0 is not None and not bare:
            if self.inplace:
                out.copy_(self.resid0)
                resid = out
            else:
                resid = P.put('residual', self.resid0, ld=ldo)
        out16 = P.new('out_f16', (M, N), torch.float16, ld=ldo) if want16 else None
        ws = P.new('splitk_ws', (_ws_floats(M, N),), torch.float32, row_bytes=4 * ((N + 255) // 256 * 256))
        accs = [P.new(f'gn_acc{i}', (B, 32, 8, 16), torch.int64, fill=0) for i in range(len(targets))]
        gn = [(acc, cpg, cbase) for acc, (cpg, cbase) in zip(accs, targets)] or None
        two = self.c1 and not as_executor
        a0 = self.a[:, :self.c0] if two else self.a
        a1 = self.a[:, self.c0:] if two else self.a_lo
        Bn, Hin, Win, Hout, Wout, ksize, stride, up = self.geom
        K.igemm(a0, self.w, N, Bn, Hin, Win, Hout, Wout, ksize, stride, up, a1=a1, bias=self.bias, rowvec=self.rowvec, residual=resid,
                out_f32=out, out_f16=out16, ldo=ldo, tile=tile, splitk=splitk, gn=gn, split16=self.split16, ws=ws, cnt=self.cnt,
                a2=self.a if self.split3 else None)
        torch.cuda.synchronize()
        tol = _tol_split(self.Kd) if (self.split16 or self.split3) else _tol32(self.Kd)
        errs = {'f32': (_report(f'{tag} f32', out, ref, tol), tol)}
        if want16:
            errs['f16'] = (_report(f'{tag} f16', out16, ref, 6e-3), 6e-3)
        st = _stats_errors(out, self.HW, targets, accs)
        for (cpg, cbase), (e1, e2, bar) in zip(targets, st):
            print(f'[{tag} gn-stats cpg{cpg} cbase{cbase}] |sum err| {e1:.3e} (tol {bar:.1e}) rel sumsq err {e2:.3e} (tol 1.0e-05)', flush=True)
        P.check(tag)
        assert int(self.cnt.abs().max()) == 0, f'{tag}: split-K tile counters not left zero'
        for v, keep in self.inputs:
            assert torch.equal(v, keep), f'{tag}: an input operand was modified'
        self.last = (out, accs)
        del P.bufs[n0:]         # this run's outputs and scratch (the operands stay for the next run)
        return errs, st


def _assert_case(errs, st):
    for what, (e, tol) in errs.items():
        assert e < tol, (what, e, tol)
    for e1, e2, bar in st:
        assert e1 < bar and e2 < 1e-5, (e1, e2, bar)


def _conv_kwargs(kind, d):
    if kind == 'conv3':
        role = d['role']
        kw = dict(c0=d['c0'], c1=d['c1'], N=d['N'], Hin=d['hin'], Win=d['hin'], Hout=d['hout'], Wout=d['hout'], ksize=3, stride=d['stride'],
                  up=d['up'], gn=d['gn'], rowvec=role == 'conv1', resid=role == 'conv2')
    elif kind == 'conv1x1':       # the skip convolution reads the raw fp16 copy of the concat: one source; statistics as for conv2 (next norm)
        kw = dict(c0=d['K'], c1=0, N=d['N'], Hin=d['hw'], Win=d['hw'], Hout=d['hw'], Wout=d['hw'], resid=True, gn=[(d['N'] // 32, 0)], bare_as_executor=True)
    else:
        role = d['role']
        kw = dict(c0=d['K'], c1=0, N=d['N'], Hin=d['M'], Win=1, Hout=d['M'], Wout=1, resid=role in ('attn_out', 'ff2', 'proj_out'),
                  inplace=role in ('attn_out', 'ff2'), gn=d.get('gn', []))
    return kw


SPLIT16_ROLES = ('skip', 'proj_in', 'proj_out', 'qkv_legacy')      # dense1x1(..., precise) in csrc/unet.cpp


def _plain_cases():
    out = []
    for model in ('cin', 'inpaint'):
        for kind, d in MS.distinct(model, ('conv3', 'conv1x1', 'dense')):
            if d.get('mode', 'plain') == 'plain':
                out.append(pytest.param(model, kind, d, id=f'{model}-{MS.case_id(kind, d)}'))
    return out


@pytest.mark.parametrize('model,kind,d', _plain_cases())
def test_plain_gemm_and_conv(model, kind, d):
    """3x3 convs (stride 1 / 2, folded x2 upsampling, two-source concat), 1x1 skip convs and the plain-mode dense GEMMs of the transformer /
    legacy attention blocks, with the role's epilogue and the statistics targets of the real consumers"""
    name = f'{model} {MS.case_id(kind, d)}'
    c = _Case(name, **_conv_kwargs(kind, d))
    res = [c.run(-1, 0, as_executor=True)]
    res += [c.run(t, k, gap=8) for t, k in FORCED]
    if d['role'] in SPLIT16_ROLES:
        kw = _conv_kwargs(kind, d)
        s = _Case(name + ' split16', split16=True, **kw)
        res.append(s.run(-1, 0, want16=False, as_executor=True))
    if d.get('p3'):
        s = _Case(name + ' split3', split3=True, **_conv_kwargs(kind, d))
        res.append(s.run(-1, 0, want16=False, as_executor=True))
    for errs, st in res:
        _assert_case(errs, st)


def _mode_cases(mode):
    out = []
    for model in ('cin', 'laion') if mode == 'kv' else ('cin',):
        for kind, d in MS.distinct(model, ('dense', 'kv')):
            if (kind == 'kv') == (mode == 'kv') and (kind == 'kv' or d['mode'] == mode):
                out.append(pytest.param(model, d, id=f'{model}-{MS.case_id(kind, d)}'))
    return out


@pytest.mark.parametrize('model,d', _mode_cases('geglu'))
def test_geglu(model, d):
    """FeedForward / GEGLU (attention.py:37-64) at the CIN widths: value * gelu(gate) in fp16; tile -1 (0 by the heuristic) and the forced 3"""
    M, Kd, N = B * d['M'], d['K'], d['N']
    g = _g(_seed(M, Kd, N))
    a = _r16((M, Kd), g)
    w = _r16((N, Kd), g, 1.0 / math.sqrt(Kd))
    b = _randn((N,), g, 0.1)
    y = a.double() @ w.double().t() + b.double()
    val, gate = y.chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    P = guard.Pool(DEV)
    wp, bp = K.pack_geglu(w.float(), b)
    a_d, wp, bp = P.put('a', a), P.put('w', wp), P.put('bias', bp)
    res = []
    for tile in (-1, 3):
        out = P.new('out', (M, N // 2), torch.float16)
        K.igemm(a_d, wp, N, B, d['M'], 1, d['M'], 1, bias=bp, out_f16=out, mode=1, tile=tile)
        torch.cuda.synchronize()
        res.append(_report(f'{model} {MS.case_id("dense", d)} tile{tile}', out, ref, 4e-3))
        P.check(f'geglu tile{tile}')
    assert max(res) < 4e-3


def _heads_run(tag, P, a0, wp, N, ntok, segs, heads, dh, segC, refs, tile, splitk, bias=None, a1=None, a2=None):
    ntp = (ntok + 7) // 8 * 8
    outs = []
    for i, kind in enumerate(segs):
        if kind == 0:
            outs.append(P.new(f'seg{i}', (B * heads, ntok, dh), torch.float16))
        else:       # V^T: the pad tokens are zero by contract (the executor clears the buffer when ntok_pad != ntok)
            outs.append(P.new(f'seg{i}_vt', (B * heads, dh, ntp), torch.float16, fill=0 if ntp != ntok else None))
    ws = P.new('splitk_ws', (_ws_floats(B * ntok, N),), torch.float32, row_bytes=4 * ((N + 255) // 256 * 256))
    cnt = P.new('splitk_cnt', (8192,), torch.int32, fill=0)
    K.igemm(a0, wp, N, B, ntok, 1, ntok, 1, a1=a1, a2=a2, mode=2, bias=bias, tile=tile, splitk=splitk, ws=ws, cnt=cnt,
            heads=dict(segs=list(zip(outs, segs)), heads=heads, dh=dh, ntok=ntok, ntok_pad=ntp, segC=segC))
    torch.cuda.synchronize()
    tol = 4e-3 if splitk == 1 else 6e-3
    worst = 0.0
    for i, (o, kind, r) in enumerate(zip(outs, segs, refs)):
        got = o if kind == 0 else o[:, :, :ntok]
        worst = max(worst, _report(f'{tag} tile{tile} k{splitk} seg{i}', got, r, tol))
        if kind == 1 and ntp != ntok:
            assert float(o[:, :, ntok:].abs().max()) == 0.0
    P.check(f'{tag} tile{tile} k{splitk}')
    assert int(cnt.abs().max()) == 0
    return worst, tol


def _head_refs(y, ntok, nseg, heads, dh, kinds):
    y = y.reshape(B, ntok, nseg, heads, dh)
    return [y[:, :, i].permute(0, 2, 1, 3).reshape(B * heads, ntok, dh) if kind == 0 else
            y[:, :, i].permute(0, 2, 3, 1).reshape(B * heads, dh, ntok) for i, kind in enumerate(kinds)]


@pytest.mark.parametrize('model,d', _mode_cases('heads'))
def test_head_scatter(model, d):
    """q | k | v and to_q of the CIN transformer blocks ('b n (h d) -> (b h) n d', v transposed): one head of 384 / 576 / 960 channels"""
    ntok, Kd, N, heads, dh = d['M'], d['K'], d['N'], d['heads'], d['dh']
    C = heads * dh
    nseg = N // C
    kinds = [0, 0, 1][:nseg] if nseg == 3 else [0]
    g = _g(_seed(ntok, Kd, N))
    a = _r16((B * ntok, Kd), g)
    w = _r16((N, Kd), g, 1.0 / math.sqrt(Kd))
    refs = _head_refs(a.double() @ w.double().t(), ntok, nseg, heads, dh, kinds)
    P = guard.Pool(DEV)
    a_d, w_d = P.put('a', a), P.put('w', w)
    tag = f'{model} {MS.case_id("dense", d)}'
    res = [_heads_run(tag, P, a_d, w_d, N, ntok, kinds, heads, dh, C, refs, -1, 1)]          # the executor: splitk = 1, tile from the heuristic (2)
    res += [_heads_run(tag, P, a_d, w_d, N, ntok, kinds, heads, dh, C, refs, t, k) for t, k in FORCED]
    for e, tol in res:
        assert e < tol


@pytest.mark.parametrize('model,d', _mode_cases('kv'))
def test_context_kv_projection(model, d):
    """to_k | to_v over the context (attention.py:174-176): K = 512 (CIN, one class token) and K = 1280 (LAION, 77 tokens), scattered as K and
    V^T per head, on fp16 operands and as the 3-pass split-fp16 product [hi | lo | hi] x [w_hi | w_hi | w_lo] the executor runs"""
    ntok, Kd, N, heads, dh = d['ntok'], d['K'], d['N'], d['heads'], d['dh']
    C = heads * dh
    g = _g(_seed(ntok, Kd, N))
    tag = f'{model} {MS.case_id("kv", d)}'
    a = _r16((B * ntok, Kd), g)
    w = _r16((N, Kd), g, 1.0 / math.sqrt(Kd))
    refs = _head_refs(a.double() @ w.double().t(), ntok, 2, heads, dh, [0, 1])
    P = guard.Pool(DEV)
    res = [_heads_run(tag, P, P.put('a', a), P.put('w', w), N, ntok, [0, 1], heads, dh, C, refs, -1, 1)]
    x = _randn((B * ntok, Kd), g, 2.0)
    w32 = _randn((N, Kd), g, 1.0 / math.sqrt(Kd))
    refs = _head_refs(x.double() @ w32.double().t(), ntok, 2, heads, dh, [0, 1])
    hi, lo = K.cast_f16(x, want_lo=True)
    P = guard.Pool(DEV)
    hi_d, lo_d = P.put('a_hi', hi), P.put('a_lo', lo)
    res.append(_heads_run(tag + ' split-fp16', P, hi_d, P.put('w_split3', K.pack_split3(w32)), N, ntok, [0, 1], heads, dh, C, refs, -1, 1,
                          a1=lo_d, a2=hi_d))
    for e, tol in res:
        assert e < tol


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------
def _gn_cases():
    seen, out = set(), []
    for model in ('cin', 'inpaint'):
        for kind, d in MS.distinct(model, ('gn',)):
            key = (d['c0'], d['c1'], d['hw'])
            if key not in seen:
                seen.add(key)
                out.append(pytest.param(model, d['c0'], d['c1'], d['hw'] ** 2, id=f'{model}-{d["c0"]}|{d["c1"]}-hw{d["hw"]}'))
    return out


def _groupnorm_guarded(P, x0, x1, gamma, beta, eps, silu):
    Bn, HW, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[2]
    C = c0 + c1
    o = dict(f16=P.new('out_f16', (Bn, HW, C), torch.float16), f32=P.new('out_f32', (Bn, HW, C), torch.float32),
             raw=P.new('raw_f16', (Bn, HW, C), torch.float16), lo=P.new('out_lo', (Bn, HW, C), torch.float16),
             raw_lo=P.new('raw_lo', (Bn, HW, C), torch.float16))
    n = _lib.load().sdmi_k_groupnorm_ws_floats(Bn, HW)
    ws = P.new('gn_ws', (n,), torch.float32)
    _lib.check(_lib.load().sdmi_k_groupnorm(x0.data_ptr(), _lib.ptr(x1), c0, c1, Bn, HW, gamma.data_ptr(), beta.data_ptr(), float(eps), int(silu),
                                            o['f16'].data_ptr(), o['f32'].data_ptr(), o['raw'].data_ptr(), o['lo'].data_ptr(),
                                            o['raw_lo'].data_ptr(), ws.data_ptr(), n, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('model,c0,c1,HW', _gn_cases())
def test_groupnorm(model, c0, c1, HW):
    """GroupNorm32 + SiLU over every (C, c0 | c1, HW) of the two UNets: 6 .. 64 channels per group, groups that straddle the seam between the
    two sources ((384 | 192): 18 per group, the seam is inside group 21), all five outputs"""
    g = _g(_seed(c0, c1, HW))
    C = c0 + c1
    P = guard.Pool(DEV)
    x0 = P.put('x0', _randn((B, HW, c0), g, 1.5) + 0.3)
    x1 = P.put('x1', _randn((B, HW, c1), g, 0.7) - 0.2) if c1 else None
    gamma = P.put('gamma', 1 + 0.1 * _randn((C,), g))
    beta = P.put('beta', 0.1 * _randn((C,), g))
    x = x0 if x1 is None else torch.cat([x0, x1], dim=2)
    x64 = x.double().reshape(B, HW, 32, C // 32)
    mean = x64.mean((1, 3), keepdim=True)
    var = ((x64 - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((x64 - mean) / torch.sqrt(var + 1e-5)).reshape(B, HW, C) * gamma.double() + beta.double()
    ref = y * torch.sigmoid(y)
    o = _groupnorm_guarded(P, x0, x1, gamma, beta, 1e-5, 1)
    tag = f'{model} groupnorm {c0}|{c1} HW{HW}'
    e = [(_report(f'{tag} f32', o['f32'], ref, 2e-5), 2e-5), (_report(f'{tag} f16', o['f16'], ref, 4e-3), 4e-3),
         (_report(f'{tag} raw', o['raw'], x, 4e-3), 4e-3),
         (_report(f'{tag} hi+lo', o['f16'].float() + o['lo'].float(), o['f32'], 4e-6), 4e-6),
         (_report(f'{tag} raw hi+lo', o['raw'].float() + o['raw_lo'].float(), x, 4e-6), 4e-6)]
    P.check(tag)
    for err, tol in e:
        assert err < tol


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _attn_ref64(q, k, v, heads, scale, causal=False):
    BH, nq, d = q.shape
    out = torch.empty((BH, nq, d), dtype=torch.float64, device=q.device)
    for i in range(BH):
        s = (q[i].double() @ k[i].double().t()) * scale
        if causal:
            s = s + torch.full((nq, nq), float('-inf'), dtype=torch.float64, device=q.device).triu(1)
        out[i] = torch.softmax(s, dim=-1) @ v[i].double()
    return out.reshape(BH // heads, heads, nq, d).permute(0, 2, 1, 3).reshape(BH // heads, nq, heads * d)


def _attn_cases():
    seen, out = set(), []
    for model in ('cin', 'inpaint', 'laion'):
        for kind, d in MS.distinct(model, ('attn',)):
            key = (d['d'], d['heads'], d['nq'], d['nkv'])
            if key not in seen:
                seen.add(key)
                out.append(pytest.param(model, 'walk', *key, id=f'{model}-d{key[0]}-h{key[1]}-nq{key[2]}-nkv{key[3]}'))
    # one ragged shape per kernel family (nq % 32 != 0, nkv % 64 != 0)
    out.append(pytest.param('ragged', 'dma', 80, 2, 333, 203, id='ragged-lds-dma'))
    out.append(pytest.param('ragged', 'dma', 40, 2, 4096 + 40, 2048 + 128, id='ragged-key-split'))       # (nkv % 128 == 0: see the module docstring)
    out.append(pytest.param('ragged', 'dma', 384, 2, 77, 45, id='ragged-wide'))
    out.append(pytest.param('ragged', 'causal', 64, 2, 77, 77, id='ragged-causal-register-staged'))
    out.append(pytest.param('ragged', 'split16', 64, 2, 100, 77, id='ragged-split16'))
    return out


@pytest.mark.parametrize('model,family,d,heads,nq,nkv', _attn_cases())
def test_attention(model, family, d, heads, nq, nkv):
    """softmax(q k^T d^-1/2) v at the three models' (d, heads, nq, nkv) -- one head of 384 .. 960 channels (CIN), 8 heads of 64 / 96 / 128
    (inpainting), LAION's 32 x 32-latent token counts against 77 context tokens -- and one ragged shape per kernel family.  The V^T pad columns
    nkv .. nkv_pad are zero where the contract says so (include/sdmi.h) and NaN for the wide-head kernel, which accepts anything there."""
    g = _g(_seed(d, heads, nq, nkv))
    BH = B * heads
    scale = d ** -0.5
    nkp = (nkv + 7) // 8 * 8
    wide = d > 160
    tag = f'{model} attention {family} d{d} h{heads} nq{nq} nkv{nkv}'
    P = guard.Pool(DEV)
    out = P.new('out', (B, nq, heads * d), torch.float16)
    lib = _lib.load()
    if family == 'split16':
        q, k, v = _randn((BH, nq, d), g), _randn((BH, nkv, d), g), _randn((BH, nkv, d), g)
        vt = torch.zeros((BH, d, nkp), device=DEV)
        vt[:, :, :nkv] = v.transpose(1, 2)
        ops = []
        for nm, t in (('q', q), ('k', k), ('vt', vt)):
            hi, lo = K.cast_f16(t.contiguous(), want_lo=True)
            ops += [P.put(nm, hi), P.put(nm + '_lo', lo)]
        out_lo = P.new('out_lo', (B, nq, heads * d), torch.float16)
        _lib.check(lib.sdmi_k_attention_split16(*[o.data_ptr() for o in ops], out.data_ptr(), out_lo.data_ptr(), BH, heads, nq, nkv, nkp, d,
                                                float(scale), _lib.stream_ptr()))
        torch.cuda.synchronize()
        ref = _attn_ref64(q, k, v, heads, scale)
        rel = float((out.double() + out_lo.double() - ref).abs().max() / ref.abs().max())
        print(f'[{tag}] max-abs / max|O| {rel:.2e} (tol 1.0e-05)', flush=True)
        P.check(tag)
        assert bool(torch.isfinite(out.float()).all()) and rel <= 1e-5
        return
    q, k, v = _r16((BH, nq, d), g), _r16((BH, nkv, d), g), _r16((BH, nkv, d), g)
    if family != 'causal':          # a few large scores so the online-softmax rescale path runs
        q[0, 0] *= 6.0
        k[0, nkv - 1] *= 6.0
        k[0, nkv // 2] *= 5.0
    vt = torch.full((BH, d, nkp), float('nan') if wide else 0.0, device=DEV, dtype=torch.float16)
    vt[:, :, :nkv] = v.transpose(1, 2)
    q_d, k_d, vt_d = P.put('q', q), P.put('k', k), P.put('vt', vt)
    if family == 'causal':
        _lib.check(lib.sdmi_k_attention_causal(q_d.data_ptr(), k_d.data_ptr(), vt_d.data_ptr(), out.data_ptr(), BH, heads, nq, nkp, d, float(scale),
                                               _lib.stream_ptr()))
    else:
        _lib.check(lib.sdmi_k_attention(q_d.data_ptr(), k_d.data_ptr(), vt_d.data_ptr(), out.data_ptr(), BH, heads, nq, nkv, nkp, d, float(scale),
                                        _lib.stream_ptr()))
    torch.cuda.synchronize()
    ref = _attn_ref64(q, k, v, heads, scale, causal=family == 'causal')
    tol = 4e-3 if (wide or family == 'causal') else 3e-3
    err = _report(tag, out, ref, tol)
    P.check(tag)
    assert err < tol


# ---- the other kernels of a forward -----------------------------------------------------------------------------------------------------
def _distinct_of(kind, keys):
    seen, out = set(), []
    for model in ('cin', 'inpaint'):
        for _, d in MS.distinct(model, (kind,)):
            key = tuple(d[k] for k in keys)
            if key not in seen:
                seen.add(key)
                out.append(pytest.param(*key, id=f'{model}-' + '-'.join(f'{k}{d[k]}' for k in keys)))
    return out


@pytest.mark.parametrize('hw,C,dir_', _distinct_of('resample', ('hw', 'C', 'dir')))
def test_resample2(hw, C, dir_):
    """2x2 average pool / nearest x2 of the inpainting UNet's resampling ResBlocks (openaimodel.py:253-259): fp32, and fp16 hi | lo"""
    g = _g(_seed(hw, C, dir_ + 2))
    P = guard.Pool(DEV)
    x = P.put('x', _randn((B, hw, hw, C), g))
    ho = hw // 2 if dir_ > 0 else 2 * hw
    o32 = P.new('out_f32', (B, ho, ho, C), torch.float32)
    hi, lo = P.new('out_f16', (B, ho, ho, C), torch.float16), P.new('out_lo', (B, ho, ho, C), torch.float16)
    lib = _lib.load()
    _lib.check(lib.sdmi_k_resample2(x.data_ptr(), o32.data_ptr(), None, None, B, hw, hw, C, dir_, _lib.stream_ptr()))
    _lib.check(lib.sdmi_k_resample2(x.data_ptr(), None, hi.data_ptr(), lo.data_ptr(), B, hw, hw, C, dir_, _lib.stream_ptr()))
    torch.cuda.synchronize()
    x64 = x.double()
    if dir_ > 0:
        ref = x64.reshape(B, ho, 2, ho, 2, C).mean((2, 4))
    else:
        ref = x64.repeat_interleave(2, 1).repeat_interleave(2, 2)
    tag = f'resample2 hw{hw} C{C} dir{dir_}'
    e = _report(tag, o32, ref, 1e-6)
    P.check(tag)
    assert e <= 1e-6 * float(ref.abs().max())          # (one fp32 rounding of a sum of four: test_resample2_matches_torch)
    assert torch.equal(hi, o32.half()) and torch.equal(lo, (o32 - hi.float()).half())


@pytest.mark.parametrize('Cin,Cout,hw', _distinct_of('conv_in', ('cin', 'N', 'hw')))
def test_conv_in(Cin, Cout, hw):
    """the first conv on fp32 NCHW input: 3 channels (CIN) and 7 (inpainting: latent | masked latent | mask)"""
    g = _g(_seed(Cin, Cout, hw))
    P = guard.Pool(DEV)
    x = P.put('x', _randn((B, Cin, hw, hw), g))
    w = P.put('w', _randn((Cout, Cin, 3, 3), g, 1.0 / math.sqrt(9 * Cin)))
    b = P.put('bias', _randn((Cout,), g, 0.1))
    out = P.new('out', (B, hw * hw, Cout), torch.float32)
    _lib.check(_lib.load().sdmi_k_conv_in(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), B, Cin, hw, hw, Cout, _lib.stream_ptr()))
    torch.cuda.synchronize()
    xn = x.permute(0, 2, 3, 1).reshape(B * hw * hw, Cin)
    ref = _conv_ref64(xn, w, B, hw, hw, 3, 1, 0) + b.double()[None]
    e = _report(f'conv_in {Cin}->{Cout} hw{hw}', out, ref, 2e-5)
    P.check('conv_in')
    assert e < 2e-5           # (test_conv_in_out)


@pytest.mark.parametrize('Cin,Cout,hw', _distinct_of('conv_out', ('cin', 'N', 'hw')))
def test_conv_out(Cin, Cout, hw):
    """the `out` head (openaimodel.py:533-537) with 3 output channels, from 192 / 256 input channels"""
    g = _g(_seed(Cin, Cout, hw, 1))
    P = guard.Pool(DEV)
    h = P.put('h', _randn((B, hw * hw, Cin), g))
    w = _randn((Cout, Cin, 3, 3), g, 1.0 / math.sqrt(9 * Cin))
    b = P.put('bias', _randn((Cout,), g, 0.1))
    w_d = P.put('w', w)
    wp = P.new('w_ohwi', (Cout, 3, 3, Cin), torch.float32)
    lib = _lib.load()
    _lib.check(lib.sdmi_k_pack_conv_out(w_d.data_ptr(), wp.data_ptr(), Cout, Cin, _lib.stream_ptr()))
    out = P.new('out', (B, Cout, hw, hw), torch.float32)
    _lib.check(lib.sdmi_k_conv_out(h.data_ptr(), wp.data_ptr(), b.data_ptr(), out.data_ptr(), B, hw, hw, Cin, Cout, _lib.stream_ptr()))
    torch.cuda.synchronize()
    ref = (_conv_ref64(h.reshape(B * hw * hw, Cin), w, B, hw, hw, 3, 1, 0) + b.double()[None]).reshape(B, hw, hw, Cout).permute(0, 3, 1, 2)
    e = _report(f'conv_out {Cin}->{Cout} hw{hw}', out.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1), 2e-5)
    P.check('conv_out')
    assert e < 2e-5


@pytest.mark.parametrize('Kd,N', _distinct_of('small_linear', ('K', 'N')))
@pytest.mark.parametrize('silu', [0, 1])
def test_small_linear(Kd, N, silu):
    """time_embed and the emb_layers of the two UNets: K = 192 / 256 (timestep embedding) and 768 / 1024 (time_embed_dim)"""
    g = _g(_seed(Kd, N, silu))
    P = guard.Pool(DEV)
    x = P.put('x', _randn((B, Kd), g, 2.0))
    w = P.put('w', _randn((N, Kd), g, 1.0 / math.sqrt(Kd)))
    b = P.put('bias', _randn((N,), g, 0.1))
    out = P.new('out', (B, N), torch.float32)
    _lib.check(_lib.load().sdmi_k_small_linear(x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), out.data_ptr(), N, B, N, Kd, silu,
                                               _lib.stream_ptr()))
    torch.cuda.synchronize()
    x64 = x.double()
    ref = (x64 * torch.sigmoid(x64) if silu else x64) @ w.double().t() + b.double()
    e = _report(f'small_linear K{Kd} N{N} silu{silu}', out, ref, 2e-5)
    P.check('small_linear')
    assert e < 2e-5           # (test_time_embedding_path)


@pytest.mark.parametrize('dim', [192, 256])
def test_timestep_embedding(dim):
    from oracle.unet_ref import timestep_embedding as ref_temb
    t = torch.tensor([981, 481, 1, 0, 999], dtype=torch.int64)
    P = guard.Pool(DEV)
    t_d = P.put('t', t.to(DEV))
    tf_d = P.put('t_f32', t.float().to(DEV))
    ref = ref_temb(t, dim)
    lib = _lib.load()
    for nm, args in (('int64', (t_d.data_ptr(), None)), ('fp32', (None, tf_d.data_ptr()))):
        out = P.new('out ' + nm, (5, dim), torch.float32)
        _lib.check(lib.sdmi_k_timestep_embedding(*args, out.data_ptr(), 5, dim, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert _report(f'timestep_embedding dim{dim} {nm}', out, ref.to(DEV), 2e-4) < 2e-4       # (test_time_embedding_path)
    P.check('timestep_embedding')


# ---- controls: the checks above cannot pass vacuously -------------------------------------------------------------------------------------
def test_control_longest_k_reference_without_one_chunk():
    """(1024 | 1024) -> 1024, 3x3, K = 18432: with the last 64-channel chunk of the second source dropped from the REFERENCE only, the
    error must exceed that case's bar at least tenfold (a kernel that skipped the chunk would be as far off)"""
    kw = dict(c0=1024, c1=1024, N=1024, Hin=16, Win=16, Hout=16, Wout=16, ksize=3, rowvec=True)
    assert any(k == 'conv3' and (d['c0'], d['c1'], d['N'], d['hin']) == (1024, 1024, 1024, 16) for k, d in MS.distinct('inpaint'))
    errs, _ = _Case('control longest-K, reference without the last chunk', ref_drop=64, **kw).run(-1, 0)
    e, tol = errs['f32']
    assert tol == _tol32(18432) and e > 10 * tol, (e, tol)
    errs, st = _Case('control longest-K, whole reference', **kw).run(-1, 0)
    _assert_case(errs, st)


def test_control_statistics_target_off_by_one_channel():
    """the (384 | 192) seam, 18 channels per group: the statistics of the 192-channel source accumulated for cbase = 384 (inside group 21) must
    FAIL the bars when checked against a reference with cbase + 1"""
    tgt = (18, 384)
    d = next(d for k, d in MS.distinct('cin') if k == 'conv3' and d['N'] == 192 and tgt in d['gn'])
    c = _Case('control gn target', **_conv_kwargs('conv3', d))
    errs, st = c.run(-1, 0)
    _assert_case(errs, st)
    out, accs = c.last
    i = c.targets.index(tgt)
    (e1, e2, bar), = _stats_errors(out, c.HW, [(18, 385)], [accs[i]])
    print(f'[control gn target cbase+1] |sum err| {e1:.3e} (tol {bar:.1e}) rel sumsq err {e2:.3e}', flush=True)
    assert not (e1 < bar and e2 < 1e-5)
    assert e2 > 10 * 1e-5


def test_guarded_buffers_on_the_device():
    """the helper's self-check with torch writes on the device: one byte poked into each guard and into a pitch gap makes `check` raise"""
    g = guard.guarded((70, 40), torch.float16, ld=48)
    assert torch.isnan(g.view).all() and g.view.data_ptr() % 16 == 0
    g.view.zero_()
    g.check('payload')
    for off in (g.guard - 1, g.guard + g.nbytes, g.guard + 3 * g.pitch + 40 * 2 + 1):
        g.raw[off] = 0
        with pytest.raises(AssertionError, match='outside the payload'):
            g.check('poke')
        g.raw[off] = guard.FILL
    g.check('restored')


# ---- the remaining kernel-level entry points of include/sdmi.h: guards at one tail shape, values against their existing reference ------
def _s():
    return _lib.stream_ptr()


def _ord16(h):
    i = h.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _ep_layernorm(P):
    g = _g(1)
    M, C = 9, 772
    x, ga, be = P.put('x', _randn((M, C), g, 2.0) + 0.5), P.put('gamma', 1 + 0.1 * _randn((C,), g)), P.put('beta', 0.1 * _randn((C,), g))
    out = P.new('out', (M, C), torch.float16)
    _lib.check(_lib.load().sdmi_k_layernorm(x.data_ptr(), ga.data_ptr(), be.data_ptr(), out.data_ptr(), M, C, 1e-5, _s()))
    ref = F.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5)
    assert _report('layernorm', out, ref, 4e-3) < 4e-3


def _ep_layernorm_split(P):
    g = _g(2)
    M, C = 33, 324
    x, ga, be = P.put('x', _randn((M, C), g, 4.0) + 1), P.put('gamma', torch.rand((C,), generator=g, device=DEV) + 0.5), P.put('beta', _randn((C,), g))
    hi, lo = P.new('hi', (M, C), torch.float16), P.new('lo', (M, C), torch.float16)
    _lib.check(_lib.load().sdmi_k_layernorm_split(x.data_ptr(), ga.data_ptr(), be.data_ptr(), hi.data_ptr(), lo.data_ptr(), M, C, 1e-5, _s()))
    ref = F.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5)
    assert float((hi.double() + lo.double() - ref).abs().max() / ref.abs().max()) <= 1e-6


def _ep_cast_f16(P):
    x = P.put('x', _randn((10004,), _g(3), 2.0))
    hi, lo = P.new('hi', (10004,), torch.float16), P.new('lo', (10004,), torch.float16)
    _lib.check(_lib.load().sdmi_k_cast_f16(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), 10004, _s()))
    assert torch.equal(hi, x.half()) and float((hi.float() + lo.float() - x).abs().max()) < 2e-6


def _ep_split_heads(P, kind):
    Bn, heads, dh, ld, col0, ntok = 2, 8, 40, 960, 320, 77
    ntp = 80
    src = P.put('src', _randn((Bn * ntok, ld), _g(4 + kind), 3.0))
    shape = (Bn * heads, ntok, dh) if kind == 0 else (Bn * heads, dh, ntp)
    hi, lo = P.new('hi', shape, torch.float16), P.new('lo', shape, torch.float16)
    _lib.check(_lib.load().sdmi_k_split_heads(src.data_ptr(), ld, col0, hi.data_ptr(), lo.data_ptr(), kind, Bn, ntok, ntp, heads, dh, _s()))
    x = src[:, col0:col0 + heads * dh].reshape(Bn, ntok, heads, dh).permute(0, 2, 1, 3).reshape(Bn * heads, ntok, dh)
    if kind == 1:       # the pad tokens are written as zeros (NaN before)
        x = torch.cat([x.transpose(1, 2), torch.zeros((Bn * heads, dh, ntp - ntok), device=DEV)], dim=2)
    err = (hi.double() + lo.double() - x.double()).abs()
    assert float((err - (x.double().abs() * 2.0 ** -21 + 2.0 ** -25)).max()) <= 0.0


def _ep_geglu_split(P):
    M, Fd = 37, 324
    src = P.put('src', _randn((M, 2 * Fd), _g(6), 2.0))
    hi, lo = P.new('hi', (M, Fd), torch.float16), P.new('lo', (M, Fd), torch.float16)
    _lib.check(_lib.load().sdmi_k_geglu_split(src.data_ptr(), M, Fd, hi.data_ptr(), lo.data_ptr(), _s()))
    s64 = src.double()
    ref = s64[:, :Fd] * F.gelu(s64[:, Fd:])
    assert float(((hi.double() + lo.double() - ref).abs() - (2e-6 * ref.abs() + 2.0 ** -25)).max()) <= 0.0


def _ep_softmax_rows(P):
    rows, cols = 37, 4004
    S = P.put('S', _randn((rows, cols), _g(7), 40.0))
    out = P.new('P', (rows, cols), torch.float16)
    _lib.check(_lib.load().sdmi_k_softmax_rows(S.data_ptr(), out.data_ptr(), rows, cols, 0.044, _s()))
    assert _report('softmax_rows', out, torch.softmax(S.double() * 0.044, dim=1), 5e-4) < 5e-4


def _ep_pointwise_nchw(P):
    g = _g(8)
    x, w, b = P.put('x', _randn((2, 4, 9, 7), g)), P.put('w', _randn((8, 4), g)), P.put('b', _randn((8,), g))
    out = P.new('out', (2, 8, 9, 7), torch.float32)
    _lib.check(_lib.load().sdmi_k_pointwise_nchw(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), 2, 4, 8, 63, 3.0, _s()))
    ref = torch.einsum('oc,bchw->bohw', w.double(), x.double() * 3.0) + b.double()[None, :, None, None]
    assert _report('pointwise_nchw', out.permute(0, 2, 3, 1), ref.permute(0, 2, 3, 1), 1e-5) < 1e-5


def _ep_vq_quantize(P):
    import vq_ref
    g = torch.Generator().manual_seed(9)
    n_embed, D, Bn, H, W = 37, 3, 2, 9, 7
    e, z = torch.randn(n_embed, D, generator=g), torch.randn(Bn, D, H, W, generator=g)
    z_d, e_d = P.put('z', z.to(DEV)), P.put('codebook', e.to(DEV))
    zq, idx = P.new('zq', (Bn, D, H, W), torch.float32), P.new('idx', (Bn, H * W), torch.int32)
    norms = P.new('norms_ws', (n_embed,), torch.float32)
    _lib.check(_lib.load().sdmi_k_vq_quantize(z_d.data_ptr(), 1.0, e_d.data_ptr(), norms.data_ptr(), n_embed, D, zq.data_ptr(), idx.data_ptr(), Bn,
                                              H * W, _s()))
    torch.cuda.synchronize()
    _, ref_idx = vq_ref.quantize(z, e)
    d = vq_ref.distances(z, e).double()
    best = d.gather(1, ref_idx.view(-1, 1)).squeeze(1)
    second = d.scatter(1, ref_idx.view(-1, 1), float('inf')).min(1).values
    clear = (second - best) > 1e-5 * best.abs().clamp_min(1e-30)
    mine = idx.long().cpu().view(-1)
    assert torch.equal(mine[clear], ref_idx.view(-1)[clear])
    assert torch.equal(zq.cpu(), vq_ref.straight_through(z, e, idx.long().cpu().view(Bn, H, W)))


def _ep_gelu_erf(P):
    n = 4 * 333
    x = P.put('x', _randn((n,), _g(10), 3.0))
    out = P.new('out', (n,), torch.float16)
    _lib.check(_lib.load().sdmi_k_gelu_erf(x.data_ptr(), out.data_ptr(), n, _s()))
    assert int((_ord16(out) - _ord16(F.gelu(x.double()).half())).abs().max()) <= 2


def _ep_pack_kernels(P):
    g = _g(11)
    lib = _lib.load()
    O, I = 72, 64
    w = P.put('w_oihw', _randn((O, I, 3, 3), g))
    dst = P.new('pack_conv_weight', (O, 9 * I), torch.float16)
    _lib.check(lib.sdmi_k_pack_conv_weight(w.data_ptr(), dst.data_ptr(), O, I, 3, 3, _s()))
    assert torch.equal(dst, K.pack_conv_weight(w)) and torch.equal(dst.float().sort(1).values, w.half().float().reshape(O, -1).sort(1).values)
    dst3 = P.new('pack_conv_split3', (O, 27 * I), torch.float16)
    _lib.check(lib.sdmi_k_pack_conv_split3(w.data_ptr(), dst3.data_ptr(), O, I, 3, 3, _s()))
    hi = w.half()
    lo = (w - hi.float()).half()
    want = torch.cat([hi, hi, lo], dim=1).float().reshape(O, -1)
    assert torch.equal(dst3, K.pack_conv_split3(w)) and torch.equal(dst3.float().sort(1).values, want.sort(1).values)
    dsto = P.new('pack_conv_out', (3, 3, 3, I), torch.float32)
    _lib.check(lib.sdmi_k_pack_conv_out(w.data_ptr(), dsto.data_ptr(), 3, I, _s()))
    assert torch.equal(dsto, w[:3].permute(0, 2, 3, 1))
    N, Kd = 70, 100
    w2 = P.put('w', _randn((N, Kd), g))
    d2 = P.new('pack_split3', (N, 3 * Kd), torch.float16)
    _lib.check(lib.sdmi_k_pack_split3(w2.data_ptr(), d2.data_ptr(), N, Kd, _s()))
    h2 = w2.half()
    assert torch.equal(d2, torch.cat([h2, h2, (w2 - h2.float()).half()], dim=1))
    N, Kd = 128, 72
    w3, b3 = P.put('w_geglu', _randn((N, Kd), g)), P.put('b_geglu', _randn((N,), g))
    wd, bd = P.new('pack_geglu w', (N, Kd), torch.float16), P.new('pack_geglu b', (N,), torch.float32)
    _lib.check(lib.sdmi_k_pack_geglu(w3.data_ptr(), b3.data_ptr(), wd.data_ptr(), bd.data_ptr(), N, Kd, _s()))
    wr, br = K.pack_geglu(w3, b3)
    assert torch.equal(wd, wr) and torch.equal(bd, br)


def _ep_ln_fold_prep(P):
    g = _g(12)
    N, Kd, ldw = 70, 96, 104
    w = P.put('w', _r16((N, Kd), g), ld=ldw)
    ga, be, bias = P.put('gamma', 1 + 0.1 * _randn((Kd,), g)), P.put('beta', 0.1 * _randn((Kd,), g)), P.put('bias', _randn((N,), g))
    cs, dn = P.new('cs', (N,), torch.float32), P.new('d', (N,), torch.float32)
    _lib.check(_lib.load().sdmi_k_ln_fold_prep(w.data_ptr(), N, Kd, ldw, ga.data_ptr(), be.data_ptr(), bias.data_ptr(), cs.data_ptr(), dn.data_ptr(), _s()))
    assert _report('ln_fold_prep cs', cs[None], (w.double() @ ga.double())[None], 1e-4) < 1e-4
    assert _report('ln_fold_prep d', dn[None], (w.double() @ be.double() + bias.double())[None], 1e-4) < 1e-4


def _gcopy(P, c, keys):
    """guarded copies of the named device tensors of a case dict (the chain kernels' operands)"""
    return {k: P.put(k, c[k].contiguous()) for k in keys}


def _ep_ff_tail(P, head):
    """sdmi_k_ff_tail / sdmi_k_st_tail at C = 320, three samples of 128 tokens: the bits of the separate launches (tests/test_rowchain_gpu.py)"""
    import test_rowchain_gpu as RC
    Bn, ntok = 3, 128
    c = RC._ff_tail_case(Bn, ntok, 77)
    M, C_ = c['M'], c['C']
    ref_acc = torch.zeros((Bn, 32, 8, 16), dtype=torch.int64, device=DEV)
    out_ref, copy_ref, _, _, _ = RC._three_launches(c, gn=[(ref_acc, 30, 640)])
    o = _gcopy(P, c, ['ln16', 'part', 'csd', 'wp', 'wff2', 'bff2', 't', 'wpo3', 'bpo', 'x_in', 'ao', 'wo2', 'bo2', 't_prev', 'dgamma'])
    out, copy = P.new('out', (M, C_), torch.float32), P.new('out_f16', (M, C_), torch.float16)
    acc = P.new('gn_acc', (Bn, 32, 8, 16), torch.int64, fill=0)
    if head:
        K.st_tail(o['ao'], o['wo2'], o['bo2'], o['t_prev'], o['dgamma'], 1e-5, o['csd'], o['wp'], o['wff2'], o['bff2'], o['wpo3'], o['bpo'], o['x_in'],
                  out, Bn, ntok, out_f16=copy, gn=[(acc, 30, 640)])
        assert torch.equal(o['t_prev'], c['t'])
    else:
        K.ff_tail(o['ln16'], o['part'], 1e-5, o['csd'], o['wp'], o['wff2'], o['bff2'], o['t'], o['wpo3'], o['bpo'], o['x_in'], out, Bn, ntok,
                  out_f16=copy, gn=[(acc, 30, 640)])
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref) and torch.equal(copy, copy_ref)
    (s, ss), (s0, ss0) = K.gn_acc_sums(acc), K.gn_acc_sums(ref_acc)
    assert torch.allclose(s, s0, rtol=1e-6, atol=1e-3) and torch.allclose(ss, ss0, rtol=1e-6, atol=1e-3)


def _ep_st_head(P):
    import test_rowchain_gpu as RC
    Bn, ntok = 3, 128
    c = RC._st_head_case(Bn, ntok, 78)
    M, C_, heads, dh = c['M'], c['C'], c['heads'], c['dh']
    t0, q0, k0, vt0, cs, dn = RC._st_head_launches(c)
    o = _gcopy(P, c, ['dgn_g', 'dgn_b', 'w_in3', 'db_in', 'dln_g', 'wqkv16'])
    x = P.put('x', c['dx'].view(M, C_))
    cs, dn = P.put('cs', cs), P.put('d', dn)
    t, q, k = P.new('t', (M, C_), torch.float32), P.new('q', q0.shape, torch.float16), P.new('k', k0.shape, torch.float16)
    vt = P.new('vt', vt0.shape, torch.float16, fill=0)
    n = _lib.load().sdmi_k_groupnorm_ws_floats(Bn, ntok)
    ws = P.new('gn_ws', (n,), torch.float32)
    _lib.check(_lib.load().sdmi_k_st_head(x.data_ptr(), ws.data_ptr(), n, o['dgn_g'].data_ptr(), o['dgn_b'].data_ptr(), 1e-6, o['w_in3'].data_ptr(),
                                          o['db_in'].data_ptr(), t.data_ptr(), o['dln_g'].data_ptr(), 1e-5, o['wqkv16'].data_ptr(), cs.data_ptr(),
                                          dn.data_ptr(), q.data_ptr(), k.data_ptr(), vt.data_ptr(), Bn, ntok, vt.shape[2], heads, dh, C_, _s()))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in ((t, t0), (q, q0), (k, k0), (vt, vt0)))


def _ep_st_mid(P, ctx):
    """sdmi_k_st_mid / sdmi_k_st_mid_ctx: guarded launch against the unguarded one (itself pinned bit for bit by tests/test_rowchain_gpu.py)"""
    g = _g(13 + ctx)
    Bn, ntok, nkv, C_, heads = (1, 32, 5, 320, 8) if ctx else (3, 128, 0, 320, 8)
    dh, M, nkp = C_ // heads, Bn * ntok, 8
    ao, wo, bo = _r16((M, C_), g, 0.7), _r16((C_, C_), g, 1 / math.sqrt(C_)), _randn((C_,), g, 0.1)
    t_prev = _randn((M, C_), g, 1.5) + 0.3
    ln_g, ln_b, wq = 1 + 0.2 * _randn((C_,), g), 0.1 * _randn((C_,), g), _r16((C_, C_), g, 1 / math.sqrt(C_))
    cs, dn = K.ln_fold_prep(wq, C_, ln_g, ln_b)
    o = {k: P.put(k, v) for k, v in dict(ao=ao, wo=wo, bo=bo, ln_g=ln_g, wq=wq, cs=cs, dn=dn).items()}
    t0, t = t_prev.clone(), P.put('t', t_prev)
    if ctx:
        ck = _r16((Bn * heads, nkv, dh), g, 1.2)
        cvt = torch.zeros((Bn * heads, dh, nkp), dtype=torch.float16, device=DEV)
        cvt[:, :, :nkv] = _r16((Bn * heads, dh, nkv), g)
        a0 = torch.full((M, C_), float('nan'), dtype=torch.float16, device=DEV)
        K.st_mid_ctx(ao, wo, bo, t0, ln_g, 1e-5, wq, cs, dn, ck, cvt, nkv, dh ** -0.5, a0, Bn, ntok, heads, dh)
        a1 = P.new('ao_out', (M, C_), torch.float16)
        K.st_mid_ctx(o['ao'], o['wo'], o['bo'], t, o['ln_g'], 1e-5, o['wq'], o['cs'], o['dn'], P.put('ctx_k', ck), P.put('ctx_vt', cvt), nkv, dh ** -0.5,
                     a1, Bn, ntok, heads, dh)
        torch.cuda.synchronize()
        assert torch.equal(a1, a0) and torch.equal(t, t0)
    else:
        q0 = torch.full((Bn * heads, ntok, dh), float('nan'), dtype=torch.float16, device=DEV)
        K.st_mid(ao, wo, bo, t0, ln_g, 1e-5, wq, cs, dn, q0, Bn, ntok, heads, dh)
        q = P.new('q', q0.shape, torch.float16)
        K.st_mid(o['ao'], o['wo'], o['bo'], t, o['ln_g'], 1e-5, o['wq'], o['cs'], o['dn'], q, Bn, ntok, heads, dh)
        torch.cuda.synchronize()
        assert torch.equal(q, q0) and torch.equal(t, t0)
    t_ref = t_prev.double() + ao.double() @ wo.double().t() + bo.double()
    assert _report('st_mid t', t, t_ref, 2e-3) < 2e-3


def _ep_gn_conv3(P):
    import test_gnconv_gpu as GC
    Bn, H, W = 3, 5, 96
    c = GC._case(Bn, H, W, 256, 0, 79)
    N = c['N']
    ref_acc = torch.zeros((Bn, 32, 8, 16), dtype=torch.int64, device=DEV)
    out_ref, copy_ref = GC._two_launches(c, True, gn=[(ref_acc, 10, 0)], want_copy=True)
    o = _gcopy(P, c, ['x0', 'dgamma', 'dbeta', 'wp', 'dbias', 'dresid'])
    out, copy = P.new('out', (Bn * H * W, N), torch.float32), P.new('out_f16', (Bn * H * W, N), torch.float16)
    acc = P.new('gn_acc', (Bn, 32, 8, 16), torch.int64, fill=0)
    d = _lib.IGemmDesc()
    d.c0 = 256; d.lda0 = 256
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.ksize, d.stride, d.up = Bn, H, W, H, W, 3, 1, 0
    d.w = o['wp'].data_ptr(); d.N = N; d.mode = 0; d.splitk = 1; d.tile = -1; d.dma = -1
    d.bias = o['dbias'].data_ptr(); d.residual = o['dresid'].data_ptr(); d.ldr = N
    d.out_f32 = out.data_ptr(); d.out_f16 = copy.data_ptr(); d.ldo = N
    d.gn_n = 1; d.gn_acc[0] = acc.data_ptr(); d.gn_cpg[0] = 10; d.gn_cbase[0] = 0
    n = _lib.load().sdmi_k_groupnorm_ws_floats(Bn, H * W)
    ws = P.new('gn_ws', (n,), torch.float32)
    import ctypes
    _lib.check(_lib.load().sdmi_k_gn_conv3(ctypes.byref(d), o['x0'].data_ptr(), None, 256, 0, ws.data_ptr(), n, o['dgamma'].data_ptr(),
                                           o['dbeta'].data_ptr(), 1e-5, _s()))
    torch.cuda.synchronize()
    assert torch.equal(out, out_ref) and torch.equal(copy, copy_ref)
    (s, ss), (s0, ss0) = K.gn_acc_sums(acc), K.gn_acc_sums(ref_acc)
    assert torch.allclose(s, s0, rtol=1e-6, atol=1e-3) and torch.allclose(ss, ss0, rtol=1e-6, atol=1e-3)


ENTRY_POINTS = {
    'layernorm': _ep_layernorm, 'layernorm_split': _ep_layernorm_split, 'cast_f16': _ep_cast_f16,
    'split_heads_rows': lambda P: _ep_split_heads(P, 0), 'split_heads_vt': lambda P: _ep_split_heads(P, 1), 'geglu_split': _ep_geglu_split,
    'softmax_rows': _ep_softmax_rows, 'pointwise_nchw': _ep_pointwise_nchw, 'vq_quantize': _ep_vq_quantize, 'gelu_erf': _ep_gelu_erf,
    'pack_kernels': _ep_pack_kernels, 'ln_fold_prep': _ep_ln_fold_prep, 'ff_tail': lambda P: _ep_ff_tail(P, False),
    'st_tail': lambda P: _ep_ff_tail(P, True), 'st_head': _ep_st_head, 'st_mid': lambda P: _ep_st_mid(P, False),
    'st_mid_ctx': lambda P: _ep_st_mid(P, True), 'gn_conv3': _ep_gn_conv3,
}


# ---- conv2 + skip and the Upsample convs as the executor launches them since the skip fold and the phase convs --------------------------
FOLD_MODELS = ('sdv1', 'cin', 'inpaint', 'laion')
REDUCE_ABOVE = 16384          # source rows of an Upsample conv above which the site runs on a 32 x 32 source with the table's tile forced


def _fold_cases():
    """every distinct ResBlock of the four UNets whose skip convolution the executor folds at batch 2 (model_shapes.folds: not excluded,
    and the committed table sends conv2 to a halo-staged tile)"""
    seen, out = set(), []
    for model in FOLD_MODELS:
        for _, d in MS.distinct(model, ('conv2_tail',)):
            key = (d['hw'], d['N'], d['tail_c'], d['passes'], tuple(d['gn']))
            if MS.folds(d, B) and key not in seen:
                seen.add(key)
                out.append(pytest.param(model, d, id=f'{model}-{MS.case_id("conv2_tail", d)}'))
    return out


@pytest.mark.parametrize('model,d', _fold_cases())
def test_conv2_with_the_skip_tail_as_launched(model, d):
    """conv2 + skip_connection of a folding ResBlock as ONE launch (sdmi_k_igemm_tail, tile -1, split-K 0: the table's halo-staged tile and
    split), with the statistics targets of conv2's real consumers, at the bars of tests/test_skip_fold_shapes_gpu.py"""
    import test_skip_fold_gpu as SF
    import test_skip_fold_shapes_gpu as SFS
    shape = (f'{model}_{d["hw"]}x{d["hw"]}_b{B}', B, d['hw'], d['hw'])
    c = SF._operands(shape, d['N'], d['tail_c'], d['passes'], ca=d['N'])
    SFS.check_case(f'{model} {MS.case_id("conv2_tail", d)}', c, -1, 0, d['gn'], two_launches=False)
    SF._REFS.pop((shape, d['N'], d['tail_c'], d['passes'], d['N']))       # (one site per case: nothing to share, the largest is 100 MB)


def _up_cases():
    """every distinct Upsample conv of the four UNets and of the three first stages: (source side, C, N, statistics targets)"""
    import first_stage_shapes as FS
    seen, out = set(), []
    for model in FOLD_MODELS:
        for _, d in MS.distinct(model, ('conv3',)):
            key = (d['hin'], d['c0'], d['N'], tuple(d['gn']))
            if d['role'] == 'up' and key not in seen:
                seen.add(key)
                out.append(pytest.param(*key, id=f'{model}-{MS.case_id("conv3", d)}'))
    for _, d in FS.distinct(kinds=('conv3',)):
        key = (d['hin'], d['C'], d['N'], ())
        if d['role'] == 'up' and key not in seen:
            seen.add(key)
            out.append(pytest.param(*key, id=f'first_stage-{FS.case_id("conv3", d)}'))
    return out


@pytest.mark.parametrize('hin,C,N,targets', _up_cases())
def test_upsample_conv_in_both_forms(hin, C, N, targets):
    """an Upsample conv as the executor launches it under either setting of SDMI_UP_PHASE: the 3x3 conv with the nearest x2 folded into its
    gather (sdmi_k_igemm, up = 1) and the four 2x2 phase convs on derived weights (sdmi_k_igemm_up_phase), each with tile -1 and split-K 0 and
    the statistics targets of the real consumers, at batch 2.  A site of more than REDUCE_ABOVE source rows runs its (N, C) on a 32 x 32 source with the
    table's tile for the site forced (the tile index depends on the tile count, not on which rows a tile holds)."""
    import test_up_phase_gpu as UP
    import test_up_phase_tiles_gpu as UPT
    targets = list(targets)
    tag = f'up {C}->{N} {hin}x{hin} b{B}'
    rows = B * hin * hin
    old_req, ph_req, src = (-1, 0), (-1, 0), hin
    if rows > REDUCE_ABOVE:
        src = 32
        # (the table's rows for the first stages' levels are keyed by the batch-1 M: the site's row at this batch, else at batch 1, else none)
        old_req = MS.tune_lookup(4 * rows, N, 9 * C, 3, 1) or MS.tune_lookup(4 * rows // B, N, 9 * C, 3, 1) or (-1, 0)
        ph_req = MS.tune_lookup(rows, N, 4 * C, 2, 1) or MS.tune_lookup(rows // B, N, 4 * C, 2, 1) or (-1, 0)
        tag += f' reduced to 32x32 (3x3-up {old_req}, phase {ph_req})'
    old = _Case(tag + ' 3x3-up', c0=C, c1=0, N=N, Hin=src, Win=src, Hout=2 * src, Wout=2 * src, ksize=3, up=1, gn=targets)
    _assert_case(*old.run(*old_req, as_executor=True))
    c = UP._operands(B, src, src, C, N)
    UPT.check_launch(tag + ' phase', c, ph_req[0], splitk=0 if ph_req[0] < 0 else 1, targets=targets)
    UP._REFS.pop((c['B'], src, src, C, N), None)


@pytest.mark.parametrize('entry', list(ENTRY_POINTS))
def test_entry_point_stays_inside_its_buffers(entry):
    P = guard.Pool(DEV)
    ENTRY_POINTS[entry](P)
    torch.cuda.synchronize()
    P.check(entry)
