"""A ResBlock's skip_connection as the 1x1 tail phase of conv2's halo-staged launch (conv3halo.hip TAIL).

Kernel level (sdmi_k_igemm_tail): out = conv3x3(a) + x W_s^T + bias against the fp64 sum over the same fp16-rounded operands and weights
(the 3-pass form over the same hi / lo splits), with the fp16 copy and the GroupNorm-statistics targets where the epilogue (or the split-K
reduction) emits them, every operand and output in guarded buffers.  The bar is the standard fp32 accumulation bound, per element:

    |got - ref| <= (Ktot + S + 4) 2^-24 (sum_k |a_k w_k| + |bias|)

Ktot = the number of accumulated products (9 Ca of the conv + Kt of the tail), S = the number of splits (one more fp32 addition each in the
reduction), 4 = bias and the final roundings.  It is derived, not measured.  Every case prints its worst ratio to the bar, and beside it the
ratio of today's two launches (skip GEMM into fp32, conv2 with that residual) against the same reference.

Whole UNet: the committed TINY, SD-v1 16 x 16 and SD-v1 64 x 64 goldens with the fold on (the bars of tests/test_unet_gpu.py), fold on vs fold off, the
launch tapes' verify mode, and the launch count of an SD-v1 call at 64 x 64.

Measured on an MI355X: see profiles/skip_fold_ab.txt."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard  # noqa: E402  (tests/ is on sys.path via conftest's rootdir insertion)
import kernels as K  # noqa: E402
import skip_fold_cases as SC  # noqa: E402

DEV = 'cuda'
EPS32 = 2.0 ** -24
CA = 384            # conv2's input channels: 6 chunks of 64, so the halo tiles split 1, 2, 3 and 6 ways on chunk boundaries
SPLITS = (1, 2, 3, 6)
HALO_BM = SC.HALO_BM

# name, B, H, W, tiles: 8 x 8 maps are whole images per tile (two in BM = 128, four in BM = 256), 16 x 16 maps image rows (BM = 128: 8 rows, two
# tiles per image; BM = 256: the image)
SHAPES = [('8x8_b2', 2, 8, 8, (16, 17)), ('8x8_b4', 4, 8, 8, (14, 15)), ('16x16_b1', 1, 16, 16, (14, 15, 16, 17)),
          ('16x16_b2', 2, 16, 16, (14, 17))]
COUTS = (64, 128, 320)       # 320: a ragged N tile at BN = 128 (and five full ones at BN = 64)
CINS = (64, 192)             # 64 single-pass: ONE tail k-tile, shorter than its ring and fewer than 2, 3, 6 splits (empty tail ranges)
KCASES = [(s[0], t, co, ci, ps) for s in SHAPES for t in s[4] for co in (COUTS if s[0] != '16x16_b2' else (320,)) for ci in CINS
          for ps in (1, 3)]
_SHAPE = {s[0]: s for s in SHAPES}
_REFS = {}


def _operands(shape, Cout, Cin, passes, ca=CA):
    """device operands and the fp64 references of one geometry, built once and left unchanged.  shape: a name of SHAPES, or (name, B, H, W);
    ca: conv2's input channels (the draws: tests/skip_fold_cases.py, on the CPU, so that the CPU control sees the same numbers)"""
    if isinstance(shape, str):
        shape = _SHAPE[shape][:4]
    key = (shape, Cout, Cin, passes, ca)
    if key in _REFS:
        return _REFS[key]
    name, B, H, W = shape
    M = B * H * W
    CA = ca
    a, w, x, ws, b2, bs = (t.to(DEV) for t in SC.draw(name, B, H, W, ca, Cout, Cin, passes))
    a = a.half()
    bias = b2 + bs                                       # fp32, as finalize() folds the two biases
    wp = K.pack_conv_weight(w)
    x_hi, x_lo = K.cast_f16(x, want_lo=True)
    a64 = a.double().reshape(B, H, W, CA).permute(0, 3, 1, 2)
    w64 = w.half().double()
    conv = F.conv2d(a64, w64, None, padding=1).permute(0, 2, 3, 1).reshape(M, Cout)
    mag = F.conv2d(a64.abs(), w64.abs(), None, padding=1).permute(0, 2, 3, 1).reshape(M, Cout)
    if passes == 3:      # [hi | lo | hi] against [w_hi | w_hi | w_lo]
        wt = K.pack_split3(ws)
        w_hi, w_lo = wt[:, :Cin].double(), wt[:, 2 * Cin:].double()
        assert torch.equal(wt[:, :Cin], wt[:, Cin:2 * Cin])
        h64, l64 = x_hi.double(), x_lo.double()
        skip = h64 @ w_hi.t() + l64 @ w_hi.t() + h64 @ w_lo.t()
        mag = mag + h64.abs() @ w_hi.abs().t() + l64.abs() @ w_hi.abs().t() + h64.abs() @ w_lo.abs().t()
    else:
        wt = ws.half().contiguous()
        skip = x_hi.double() @ wt.double().t()
        mag = mag + x_hi.double().abs() @ wt.double().abs().t()
    ref = conv + skip + bias.double()[None]
    mag = mag + bias.double().abs()[None]
    torch.cuda.synchronize()
    c = dict(B=B, H=H, W=W, M=M, CA=CA, Cout=Cout, Cin=Cin, passes=passes, Kt=passes * Cin, a=a, wp=wp, x_hi=x_hi, x_lo=x_lo, wt=wt, b2=b2,
             bs=bs, bias=bias, ref=ref, mag=mag)
    _REFS[key] = c
    return c


def _desc(c, a, wp, bias, out, tile, splitk, ws, cnt, residual=None, out_f16=None, gn=None):
    from stable_diffusion_amd import _lib
    d = _lib.IGemmDesc()
    d.a0 = a.data_ptr(); d.c0 = c['CA']; d.lda0 = a.stride(0)
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.ksize, d.stride, d.up = c['B'], c['H'], c['W'], c['H'], c['W'], 3, 1, 0
    d.w = wp.data_ptr(); d.N = c['Cout']; d.mode = 0
    d.bias = bias.data_ptr()
    if residual is not None:
        d.residual = residual.data_ptr(); d.ldr = residual.stride(0)
    d.out_f32 = out.data_ptr(); d.ldo = out.stride(0); d.out_f16 = _lib.ptr(out_f16)
    d.splitk, d.tile, d.dma = splitk, tile, -1
    d.splitk_ws = ws.data_ptr(); d.splitk_ws_floats = ws.numel()
    d.splitk_cnt = cnt.data_ptr(); d.splitk_cnt_ints = cnt.numel()
    if gn is not None:          # (acc, cpg) at cbase 0, or a list of up to two (acc, cpg, cbase)
        gn = [gn + (0,)] if isinstance(gn, tuple) else gn
        d.gn_n = len(gn)
        for i, (acc, cpg, cbase) in enumerate(gn):
            d.gn_acc[i] = acc.data_ptr(); d.gn_cpg[i] = cpg; d.gn_cbase[i] = cbase
    return d


def _run(c, tile, splitk, extras, folded, targets=None):
    """one launch configuration in guarded buffers -> (out fp32, out fp16 | None, statistics accumulators | None).  splitk 0: the launcher
    chooses (slabs for 16 splits are given).  targets: the (cpg, cbase) statistics targets of a run with extras, [(N / 32, 0)] by default;
    when given, the accumulators come back as a list in that order.  After the launch: every guard intact, the split-K tile counters zero
    again, every operand bit-unchanged."""
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    P = guard.Pool(DEV)
    M, N, Cin = c['M'], c['Cout'], c['Cin']
    a, wp, wt = P.put('a', c['a']), P.put('w', c['wp']), P.put('w_tail', c['wt'])
    x_hi = P.put('x_hi', c['x_hi'])
    x_lo = P.put('x_lo', c['x_lo']) if c['passes'] == 3 else None
    out = P.new('out', (M, N), torch.float32)
    o16 = P.new('out_f16', (M, N), torch.float16) if extras else None
    tg = ([(N // 32, 0)] if targets is None else list(targets)) if extras else []
    accs = [P.new(f'gn_acc{i}', (c['B'], 32, 8, 16), torch.int64, fill=0) for i in range(len(tg))]
    acc = (accs[0] if targets is None else accs) if extras else None
    rM, rN = (M + 255) // 256 * 256, (N + 127) // 128 * 128
    ws = P.new('splitk_ws', ((splitk if splitk > 0 else 16) * rM * rN,), torch.float32, row_bytes=4 * rN)
    cnt = P.new('splitk_cnt', (8192,), torch.int32, fill=0)
    gn = [(ac, cpg, cbase) for ac, (cpg, cbase) in zip(accs, tg)] or None
    if folded:
        bias = P.put('bias', c['bias'])
        d = _desc(c, a, wp, bias, out, tile, splitk, ws, cnt, out_f16=o16, gn=gn)
        _lib.check(lib.sdmi_k_igemm_tail(C.byref(d), x_hi.data_ptr(), _lib.ptr(x_lo), x_hi.data_ptr() if x_lo is not None else None, Cin,
                                         x_hi.stride(0), wt.data_ptr(), c['Kt'], _lib.stream_ptr()))
    else:                # today's two launches: the skip GEMM into fp32, conv2 with that residual
        skip = P.new('skip', (M, N), torch.float32)
        b2, bs = P.put('b2', c['b2']), P.put('bs', c['bs'])
        K.igemm(x_hi, wt, N, c['B'], c['H'] * c['W'], 1, c['H'] * c['W'], 1, 1, a1=x_lo, bias=bs, out_f32=skip, split16=c['passes'] == 3)
        d = _desc(c, a, wp, b2, out, tile, splitk, ws, cnt, residual=skip, out_f16=o16, gn=gn)
        _lib.check(lib.sdmi_k_igemm(C.byref(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    tag = f'{"folded" if folded else "two launches"} tile {tile} split {splitk}'
    P.check(tag)
    assert int(cnt.abs().max()) == 0, f'{tag}: split-K tile counters not left zero'
    for v, k in ((a, 'a'), (wp, 'wp'), (wt, 'wt'), (x_hi, 'x_hi'), (x_lo, 'x_lo')):
        assert v is None or torch.equal(v.view(torch.int16), c[k].view(torch.int16)), f'{tag}: operand {k} was modified'
    for v, k in ((bias, 'bias'),) if folded else ((b2, 'b2'), (bs, 'bs')):
        assert torch.equal(v.view(torch.int32), c[k].view(torch.int32)), f'{tag}: operand {k} was modified'
    return out, o16, acc


def _ratio(c, out, splitk):
    """worst |got - ref| / bound over the elements (inf if anything is not finite)"""
    if not bool(torch.isfinite(out).all()):
        return float('inf')
    bound = (9 * c['CA'] + c['Kt'] + splitk + 4) * EPS32 * c['mag']
    return float(((out.double() - c['ref']).abs() / bound).max())


@pytest.mark.parametrize('shape,tile,Cout,Cin,passes', KCASES, ids=[f'{s}-t{t}-n{co}-c{ci}-p{ps}' for s, t, co, ci, ps in KCASES])
def test_conv3_with_1x1_tail_matches_fp64(shape, tile, Cout, Cin, passes):
    c = _operands(shape, Cout, Cin, passes)
    nkt_t = c['Kt'] // 64
    for splitk in SPLITS:
        for extras in ((False, True) if splitk in (1, 3) else (False,)):
            out, o16, acc = _run(c, tile, splitk, extras, folded=True)
            r = _ratio(c, out, splitk)
            two, _, _ = _run(c, tile, splitk, extras, folded=False)
            r2 = _ratio(c, two, splitk)
            print(f'[skip fold {shape} tile{tile} N{Cout} Cin{Cin} x{passes} split{splitk} (tail k-tiles {nkt_t}{", some splits empty" if splitk > nkt_t else ""})'
                  f'{" +f16 +stats" if extras else ""}] worst |err| / bound: folded {r:.2e}, two launches {r2:.2e}', flush=True)
            assert r <= 1.0
            if extras:
                # the fp16 copy is the fp16 rounding of the stored fp32 value
                assert torch.equal(o16, out.half())
                # statistics: fp32 partial sums of the stored values, n = HW * cpg per group -- the same accumulation bound over the stored output
                HW, cpg = c['H'] * c['W'], Cout // 32
                v = out.double().reshape(c['B'], HW, 32, cpg)
                s, ss = K.gn_acc_sums(acc)
                n = HW * cpg
                bs_ = (n + 4) * EPS32 * v.abs().sum((1, 3)).cpu() + n * 2.0 ** -40
                bss = (n + 4) * EPS32 * (v * v).sum((1, 3)).cpu() * 2 + n * 2.0 ** -40
                assert bool(((s - v.sum((1, 3)).cpu()).abs() <= bs_).all())
                assert bool(((ss - (v * v).sum((1, 3)).cpu()).abs() <= bss).all())


def test_a_tail_on_a_generic_tile_fails_loudly():
    """only the halo-staged tiles run the tail: anything else is an error, never a launch that drops the term"""
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    c = _operands('8x8_b2', 64, 64, 1)
    out = torch.zeros((c['M'], 64), device=DEV)
    ws = torch.zeros((1 << 20,), device=DEV)
    cnt = torch.zeros((8192,), dtype=torch.int32, device=DEV)
    for tile in (5, 7):
        d = _desc(c, c['a'], c['wp'], c['bias'], out, tile, 1, ws, cnt)
        rc = lib.sdmi_k_igemm_tail(C.byref(d), c['x_hi'].data_ptr(), None, None, 64, 64, c['wt'].data_ptr(), 64, _lib.stream_ptr())
        assert rc != 0 and b'tail' in lib.sdmi_last_error()
    # ... and a tail the kernel cannot run (channels not whole k-tiles) on a halo tile
    d = _desc(c, c['a'], c['wp'], c['bias'], out, 16, 1, ws, cnt)
    rc = lib.sdmi_k_igemm_tail(C.byref(d), c['x_hi'].data_ptr(), None, None, 32, 64, c['wt'].data_ptr(), 32, _lib.stream_ptr())
    assert rc != 0 and b'tail' in lib.sdmi_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# ---- whole UNet ------------------------------------------------------------------------------------------------------

import test_unet_gpu as U  # noqa: E402  (the goldens' loaders and bars: imported, not copied)


def _forward(case, golden_dir):
    from oracle.weights import make_inputs
    z = np.load(os.path.join(golden_dir, f'unet_{case}.npz'))
    cfg_name = case.split('_')[0]
    cfg = U.CFGS[cfg_name]
    m, _ = U._model(cfg_name, int(z['weight_seed']), U._style(z))
    x, t, ctx = make_inputs(cfg, int(z['batch']), int(z['h']), int(z['w']), seed=int(z['input_seed']), ctx_len=int(z['ctx_len']),
                            timesteps=tuple(int(v) for v in z['t']), style=U._style(z))
    return m, z, (x.cuda(), t.cuda(), ctx.cuda())


def _plan(m, B, H, W, L):
    buf = (C.c_int32 * 64)()
    n = m._handle.lib.sdmi_unet_skip_fold_plan(m._handle.h, B, H, W, L, buf, 64)
    assert n >= 0
    return list(buf[:n])


# (sdv1_64x64: the flagship shape, where 13 of the 14 skip convolutions fold; at 16 x 16 latents the committed tuning table sends no conv2 to a
# halo-staged tile, so those two cases pin that the knob then changes nothing)
@pytest.mark.parametrize('case', ['tiny_16x16', 'sdv1_16x16', 'sdv1_64x64'])
def test_unet_goldens_with_the_fold_on_and_off(case, golden_dir, monkeypatch):
    """fold on meets the case's bar, fold on and fold off differ by less than that bar, and the launch tapes' verify mode passes with the fold on"""
    m, z, (x, t, ctx) = _forward(case, golden_dir)
    ref = torch.from_numpy(z['eps'])
    bar_max, bar_rms, _ = U._bars(case, golden_dir, U._style(z))
    monkeypatch.setenv('SDMI_SKIP_FOLD', '1')
    plan = _plan(m, x.shape[0], x.shape[2], x.shape[3], ctx.shape[1])
    on = m(x, t, context=ctx).float().cpu()
    monkeypatch.setenv('SDMI_SKIP_FOLD', '0')
    off = m(x, t, context=ctx).float().cpu()
    e_on, e_off = (on - ref).abs(), (off - ref).abs()
    d = float((on - off).abs().max())
    print(f'[skip fold unet {case}] {sum(plan)} of {len(plan)} skip convolutions folded; vs reference max-abs: fold on {float(e_on.max()):.3e} '
          f'(rms {float(e_on.pow(2).mean().sqrt()):.3e}), fold off {float(e_off.max()):.3e}; max|on - off| {d:.3e} (bar {bar_max:.1e})', flush=True)
    assert float(e_on.max()) <= bar_max and float(e_on.pow(2).mean().sqrt()) <= bar_rms
    assert d < bar_max
    monkeypatch.setenv('SDMI_SKIP_FOLD', '1')
    again = m(x, t, context=ctx).float().cpu()            # (replayed from the tape recorded above)
    assert torch.equal(again, on)
    monkeypatch.setenv('SDMI_REPLAY_VERIFY', '1')         # the executor runs; its launch list must equal the patched tape
    assert torch.equal(m(x, t, context=ctx).float().cpu(), on)


def _launches(m, x, t, ctx):
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    m(x, t, context=ctx)
    torch.cuda.synchronize()
    _lib.check(lib.sdmi_profile_begin())
    m(x, t, context=ctx)
    cbuf = C.create_string_buffer(1 << 16)
    _lib.check(lib.sdmi_profile_end(cbuf, 1 << 16))
    tab = json.loads(cbuf.value.decode())
    return sum(r['launches'] for r in tab), tab


def test_sdv1_call_at_64x64_takes_21_fewer_launches(monkeypatch):
    """Of the 14 skip convolutions of an SD-v1 call, 13 fold at 64 x 64: output_blocks.11.0 runs its 3x3 convs as three-pass split-fp16 (no
    halo-staged launch) and keeps its skip GEMM.  13 skip launches and the 8 split-K reduce launches behind the split ones go: 21 fewer.
    (Counted from the profiler's per-kernel launch table: the launch tapes' statistics count forwards, not launches.)"""
    from oracle.plan import SD_V1
    from oracle.weights import make_inputs
    m, _ = U._model('sdv1', 0)
    x, t, ctx = make_inputs(SD_V1, 2, 64, 64, seed=3)
    x, t, ctx = x.cuda(), t.cuda(), ctx.cuda()
    monkeypatch.setenv('SDMI_SKIP_FOLD', '1')
    plan = _plan(m, 2, 64, 64, ctx.shape[1])
    n_on, tab_on = _launches(m, x, t, ctx)
    monkeypatch.setenv('SDMI_SKIP_FOLD', '0')
    n_off, tab_off = _launches(m, x, t, ctx)
    red = lambda tab: sum(r['launches'] for r in tab if r['name'].startswith('splitk_reduce'))
    print(f'[skip fold launches sdv1 64x64] fold off {n_off}, fold on {n_on}: {n_off - n_on} fewer ({sum(plan)} of {len(plan)} sites folded; '
          f'split-K reduce launches {red(tab_off)} -> {red(tab_on)})', flush=True)
    assert plan == [1] * 13 + [0]
    assert n_off - n_on == 21
