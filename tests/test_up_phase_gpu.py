"""The Upsample conv as the four 2x2 phase convs of one launch (igemm KIND_2X2: sdmi_k_igemm_up_phase, sdmi_k_up_phase_weights; DESIGN.md
section 4), every operand and output in guarded buffers (tests/guard.py).

Derived weights: bit for bit the fp16 rounding of the fp32 sum of the contributing taps (tests/up_phase.py, (ky, kx) order).

Kernel against fp64 over the same fp16 operands and the DERIVED fp16 weights, per element the fp32 accumulation bound of tests/test_skip_fold_gpu.py:

    |got - ref| <= (K' + S + 4) 2^-24 (sum_k |a_k w'_k| + |bias|),      K' = 4 Cin accumulated products, S = 1 (unsplit)

New path against old path (the KIND_3X3_UP launch over the packed 3x3 weights) on the same inputs: that bound plus what the ONE extra rounding of a
summed tap can move, 1.05 sum_k |a_k| 2^-11 |w'_k| (half an fp16 ulp of w'_k is at most 2^-11 |w'_k|; 1.05 covers the subnormal taps), per output in fp64.

GroupNorm statistics: the accumulator words against the sums over the launch's own stored output, the bound of tests/test_skip_fold_gpu.py.

Whole UNet (TINY and SD-v1 at a 16 x 16 latent): the committed goldens' bars with the knob on, tape replay = executor, launch count."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402  (tests/ is on sys.path via conftest's rootdir insertion)
import kernels as K  # noqa: E402
import up_phase as P  # noqa: E402

DEV = 'cuda'
EPS32 = 2.0 ** -24
# 1 x 1: every tap but one is padding, M' = B below any tile; 2 x 3 / 5 x 4: odd sizes, at B = 2 the sample boundary falls inside the one tile
# (M' = 12 / 40); 8 x 8: 64 rows per sample -- a whole 64-row tile per sample, two samples in a 128-row tile, and statistics (64 % 32 == 0)
MAPS = [(1, 1), (2, 3), (5, 4), (8, 8)]
CINS = (64, 128)             # (a source of 32 (mod 64) channels is refused: see test_refusals)
NS = (64, 96)                # 96: a ragged N tile at BN = 64 and at BN = 128
TILES = (-1, 5, 7)           # as launched (tuning table, then the heuristic), 64 x 64 (3 stages), 128 x 128 (3 stages)
_REFS = {}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _operands(B, H, W, Cin, N):
    """device operands and the fp64 references of one geometry, built once and left unchanged"""
    key = (B, H, W, Cin, N)
    if key in _REFS:
        return _REFS[key]
    g = _g(10000 * B + 1000 * H + 100 * W + Cin + N)
    M = B * H * W
    a = torch.randn((M, Cin), generator=g).to(DEV).half()
    w = (torch.randn((N, Cin, 3, 3), generator=g) / math.sqrt(9 * Cin)).to(DEV)
    w.view(-1)[::89] *= 2.0 ** -8                     # wide exponent spread inside the summed taps (and fp16 subnormals)
    bias = torch.randn(N, generator=g).to(DEV)
    wp = K.pack_conv_weight(w)                        # fp16 [N, 9 Cin]
    wph = P.derive_packed(wp, torch.float32)          # fp16 [4, N, 4 Cin]: RNE(fp32 sum)
    a64 = a.double().reshape(B, H, W, Cin).permute(0, 3, 1, 2)
    w4 = torch.stack([P.unpack_k(wph[ph].double(), 2, 2) for ph in range(4)])
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(4 * M, N)
    ref = nhwc(P.phase_conv(a64, w4)) + bias.double()[None]
    mag_w = nhwc(P.phase_conv(a64.abs(), w4.abs()))
    torch.cuda.synchronize()
    c = dict(B=B, H=H, W=W, M=M, Cin=Cin, N=N, a=a, wp=wp, wph=wph, bias=bias, ref=ref, mag_w=mag_w, mag=mag_w + bias.double().abs()[None])
    _REFS[key] = c
    return c


def _desc(c, a, w, bias, out, tile, out_f16=None, gn=None, up=1, splitk=1):
    from stable_diffusion_amd import _lib
    d = _lib.IGemmDesc()
    d.a0 = a.data_ptr(); d.c0 = c['Cin']; d.lda0 = a.stride(0)
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.ksize, d.stride, d.up = c['B'], c['H'], c['W'], 2 * c['H'], 2 * c['W'], 3, 1, up
    d.w = w.data_ptr(); d.N = c['N']; d.mode = 0
    d.bias = bias.data_ptr()
    d.out_f32 = out.data_ptr(); d.ldo = out.stride(0); d.out_f16 = _lib.ptr(out_f16)
    d.splitk, d.tile, d.dma = splitk, tile, -1          # (splitk 0 is the executor's request: the tuning table's key)
    if gn is not None:          # (acc, cpg) at cbase 0, or a list of up to two (acc, cpg, cbase)
        gn = [gn + (0,)] if isinstance(gn, tuple) else gn
        d.gn_n = len(gn)
        for i, (acc, cpg, cbase) in enumerate(gn):
            d.gn_acc[i] = acc.data_ptr(); d.gn_cpg[i] = cpg; d.gn_cbase[i] = cbase
    return d


def _run(c, tile, extras, phase, targets=None, splitk=1):
    """one launch in guarded buffers -> (out fp32 [4 M, N], out fp16 | None, statistics accumulators | None, derived weights as the device made
    them).  targets: the (cpg, cbase) statistics targets of a run with extras, [(N / 32, 0)] by default; when given, the accumulators come back
    as a list in that order.  After the launch: every guard intact, every operand bit-unchanged."""
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    Pl = guard.Pool(DEV)
    M, N, Cin = c['M'], c['N'], c['Cin']
    a, wp, bias = Pl.put('a', c['a']), Pl.put('w', c['wp']), Pl.put('bias', c['bias'])
    out = Pl.new('out', (4 * M, N), torch.float32)
    o16 = Pl.new('out_f16', (4 * M, N), torch.float16) if extras else None
    tg = ([(N // 32, 0)] if targets is None else list(targets)) if extras else []
    accs = [Pl.new(f'gn_acc{i}', (c['B'], 32, 8, 16), torch.int64, fill=0) for i in range(len(tg))]
    acc = (accs[0] if targets is None else accs) if extras else None
    gn = [(ac, cpg, cbase) for ac, (cpg, cbase) in zip(accs, tg)] or None
    wph = None
    if phase:
        wph = Pl.new('w_phase', (4, N, 4 * Cin), torch.float16)
        _lib.check(lib.sdmi_k_up_phase_weights(wp.data_ptr(), wph.data_ptr(), N, Cin, _lib.stream_ptr()))
        d = _desc(c, a, wph, bias, out, tile, out_f16=o16, gn=gn, splitk=splitk)
        _lib.check(lib.sdmi_k_igemm_up_phase(C.byref(d), _lib.stream_ptr()))
    else:
        d = _desc(c, a, wp, bias, out, tile, out_f16=o16, gn=gn)
        _lib.check(lib.sdmi_k_igemm(C.byref(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    tag = f'{"phase" if phase else "3x3 up"} tile {tile}'
    Pl.check(tag)
    assert torch.equal(a.view(torch.int16), c['a'].view(torch.int16)) and torch.equal(wp.view(torch.int16), c['wp'].view(torch.int16)) and \
        torch.equal(bias.view(torch.int32), c['bias'].view(torch.int32)), f'{tag}: an input operand was modified'
    return out, o16, acc, wph


@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('H,W', MAPS, ids=[f'{h}x{w}' for h, w in MAPS])
def test_phase_launch_matches_fp64_and_the_old_path(B, H, W):
    for Cin in CINS:
        for N in NS:
            c = _operands(B, H, W, Cin, N)
            Kp = 4 * Cin
            acc_bound = (Kp + 1 + 4) * EPS32 * c['mag']
            old, _, _, _ = _run(c, -1, False, phase=False)
            for tile in TILES:
                stats = (H * W) % 32 == 0
                out, o16, acc, wph = _run(c, tile, stats, phase=True)
                # derived weights: RNE(fp32 sum), bit for bit
                assert torch.equal(wph.view(torch.int16), c['wph'].view(torch.int16))
                assert bool(torch.isfinite(out).all()), 'an output row was not written (or a guard value was read)'
                r = float(((out.double() - c['ref']).abs() / acc_bound).max())
                ab_bound = acc_bound + 1.05 * 2.0 ** -11 * c['mag_w']
                r2 = float(((out.double() - old.double()).abs() / ab_bound).max())
                print(f'[up phase B{B} {H}x{W} Cin{Cin} N{N} tile{tile}{" +f16 +stats" if stats else ""}] worst |err| / bound: vs fp64 on derived weights '
                      f'{r:.2e}, vs the 3x3-up launch {r2:.2e}', flush=True)
                assert r <= 1.0
                assert r2 <= 1.0
                if stats:
                    assert torch.equal(o16, out.half())
                    HWo, cpg = 4 * H * W, N // 32
                    v = out.double().reshape(B, HWo, 32, cpg)
                    s, ss = K.gn_acc_sums(acc)
                    n = HWo * cpg
                    bs_ = (n + 4) * EPS32 * v.abs().sum((1, 3)).cpu() + n * 2.0 ** -40
                    bss = (n + 4) * EPS32 * (v * v).sum((1, 3)).cpu() * 2 + n * 2.0 ** -40
                    assert bool(((s - v.sum((1, 3)).cpu()).abs() <= bs_).all())
                    assert bool(((ss - (v * v).sum((1, 3)).cpu()).abs() <= bss).all())


def test_derived_k_order_is_the_pack_kernels():
    """the host restatement of the pack order (tests/up_phase.py pack_k) is what sdmi_k_pack_conv_weight writes, so the derived weights'
    chunk-major order is checked against the device's own"""
    g = _g(5)
    w = torch.randn((72, 128, 3, 3), generator=g).to(DEV)
    assert torch.equal(K.pack_conv_weight(w).view(torch.int16), P.pack_k(w.half()).contiguous().view(torch.int16))


def test_refusals():
    """what the phase launch cannot run is an error, never a wrong launch: a half k-tile source, split-K, a halo-staged tile, a residual"""
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    c = _operands(1, 8, 8, 64, 64)
    out = torch.zeros((4 * c['M'], 64), device=DEV)
    d = _desc(c, c['a'], c['wph'], c['bias'], out, -1)
    d.c0 = 32
    assert lib.sdmi_k_igemm_up_phase(C.byref(d), _lib.stream_ptr()) != 0
    d = _desc(c, c['a'], c['wph'], c['bias'], out, -1)
    d.splitk = 2
    assert lib.sdmi_k_igemm_up_phase(C.byref(d), _lib.stream_ptr()) != 0
    d = _desc(c, c['a'], c['wph'], c['bias'], out, 16)
    assert lib.sdmi_k_igemm_up_phase(C.byref(d), _lib.stream_ptr()) != 0
    d = _desc(c, c['a'], c['wph'], c['bias'], out, -1)
    d.residual = out.data_ptr(); d.ldr = 64
    assert lib.sdmi_k_igemm_up_phase(C.byref(d), _lib.stream_ptr()) != 0
    d = _desc(c, c['a'], c['wph'], c['bias'], out, -1, up=0)
    assert lib.sdmi_k_igemm_up_phase(C.byref(d), _lib.stream_ptr()) != 0
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


@pytest.mark.parametrize('case', ['tiny_16x16', 'sdv1_16x16'])
def test_unet_goldens_with_the_knob_on(case, golden_dir, monkeypatch):
    """SDMI_UP_PHASE=1 (by the tuning table, the default) and =2 (every Upsample conv the kernel can run) meet the case's bars, replay from the
    tape bit for bit and pass the tapes' verify mode; with the knob on the launch count is that of SDMI_UP_PHASE=0 (other kernels, same number)"""
    m, z, (x, t, ctx) = _forward(case, golden_dir)
    ref = torch.from_numpy(z['eps'])
    bar_max, bar_rms, _ = U._bars(case, golden_dir, U._style(z))
    monkeypatch.setenv('SDMI_UP_PHASE', '0')
    off = m(x, t, context=ctx).float().cpu()
    n_off, _ = _launches(m, x, t, ctx)
    for knob in ('1', '2'):
        monkeypatch.delenv('SDMI_REPLAY_VERIFY', raising=False)
        monkeypatch.setenv('SDMI_UP_PHASE', knob)
        on = m(x, t, context=ctx).float().cpu()
        e_on = (on - ref).abs()
        d = float((on - off).abs().max())
        n_on, tab = _launches(m, x, t, ctx)
        n_ph = sum(r['launches'] for r in tab if r['name'].endswith('_up2x2'))
        print(f'[up phase unet {case} SDMI_UP_PHASE={knob}] {n_ph} phase launches; vs reference max-abs {float(e_on.max()):.3e} (rms '
              f'{float(e_on.pow(2).mean().sqrt()):.3e}; bars {bar_max:.1e} / {bar_rms:.1e}); max|on - off| {d:.3e}; launches {n_on} (off: {n_off})', flush=True)
        assert float(e_on.max()) <= bar_max and float(e_on.pow(2).mean().sqrt()) <= bar_rms
        assert d < bar_max
        again = m(x, t, context=ctx).float().cpu()            # (replayed from the tape recorded above)
        assert torch.equal(again, on)
        monkeypatch.setenv('SDMI_REPLAY_VERIFY', '1')         # the executor runs; its launch list must equal the patched tape
        assert torch.equal(m(x, t, context=ctx).float().cpu(), on)
        if knob == '1':
            assert n_on == n_off
