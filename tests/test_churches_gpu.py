"""The unconditional LSUN-Churches model (models/ldm/lsun_churches256/config.yaml) on the MI355X.

Kernels against fp64 in guarded buffers (tests/guard.py): the GroupNorm-apply launch with the scale-shift rows of a
use_scale_shift_norm ResBlock, attention at head dims 24 and 48 in both precisions down to one key.  The whole UNet against
goldens of the reference's own UNetModel (tools/make_golden_churches.py; weights regenerated from the seeded per-key generator
over the HIP module's key list): mixed at the project's bar 1e-3, full at 2e-5.  Launch tapes replayed across timesteps (the
scale-shift row is a caller pointer of the tape).  The body of scripts/sample_diffusion.py's make_convolutional_sample against
the reference DDIM loop and decoder, at bars the golden tool derived from a reference UNet perturbed by the mixed bar."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from guard import Pool  # noqa: E402
from stable_diffusion_amd import synthetic  # noqa: E402

UNET_CASES = ['16x16_b2', '32x32_b1', '32x32_b2', '48x48_b1', '16x16_b10']
MIXED_TOL = 1e-3        # the project's one mixed-precision bar
FULL_TOL = 2e-5         # ~2 x the worst full-mode error recorded against any reference golden (1.03e-5); the full-mode attention bar
_models = {}


def _lib():
    from stable_diffusion_amd import _lib as L
    return L


def _unet(prec):
    if prec not in _models:
        torch.cuda.empty_cache()
        from stable_diffusion_amd import UNetModelHIP
        m = UNetModelHIP(**synthetic.CHURCHES_UNET_KWARGS, hip_precision=prec)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0),
                          strict=True)
        _models[prec] = m.cuda()
    return _models[prec]


def _unet_inputs(batch, h, w, ts, seed=1):       # (tools/make_golden_churches.py unet_inputs)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 4, h, w, generator=g), torch.tensor(ts, dtype=torch.int64)


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


# ---- kernels ------------------------------------------------------------------------------------------------------------
def _groupnorm_film(pool, x, gamma, beta, film, film_ld, eps=1e-5, silu=1):
    """sdmi_k_groupnorm_film over guarded operands; film None = NULL rows.  Returns the five outputs."""
    B, HW, Cc = x.shape
    L = _lib()
    lib = L.load()
    o = {k: pool.new(k, (B, HW, Cc), torch.float32 if k == 'f32' else torch.float16) for k in ('f16', 'f32', 'raw', 'lo', 'raw_lo')}
    n = lib.sdmi_k_groupnorm_ws_floats(B, HW)
    ws = torch.empty((n,), dtype=torch.float32, device='cuda')
    L.check(lib.sdmi_k_groupnorm_film(x.data_ptr(), None, Cc, 0, B, HW, gamma.data_ptr(), beta.data_ptr(), float(eps), int(silu),
                                      L.ptr(film), int(film_ld), o['f16'].data_ptr(), o['f32'].data_ptr(), o['raw'].data_ptr(),
                                      o['lo'].data_ptr(), o['raw_lo'].data_ptr(), ws.data_ptr(), n, L.stream_ptr()))
    torch.cuda.synchronize()
    return o


# (C, H*W, shared row): 6 channels per group -- a quad straddles two groups; 4 pixels; one pixel; 307 200 quads -- the U = 4 kernel;
# pitch 0 -- one row shared by every sample, what a timestep-table hit hands out
@pytest.mark.parametrize('Cc,HW,shared', [(192, 1024, False), (384, 4, False), (768, 1, False), (768, 1600, False), (192, 1024, True)])
def test_groupnorm_scale_shift_vs_fp64(Cc, HW, shared):
    import torch.nn.functional as F
    from kernels import report
    g = torch.Generator().manual_seed(Cc + HW)
    B = 2
    x = torch.randn(B, HW, Cc, generator=g) * 1.5 + 0.3           # (as in test_kernels_gpu.py::test_groupnorm)
    gamma = 1 + 0.1 * torch.randn(Cc, generator=g)
    beta = 0.1 * torch.randn(Cc, generator=g)
    rows = 0.25 * torch.randn(1 if shared else B, 2 * Cc, generator=g)          # [scale | shift] per sample, distinct rows
    xd = x.double()
    ref = F.group_norm(xd.permute(0, 2, 1).reshape(B, Cc, HW, 1), 32, gamma.double(), beta.double(), 1e-5).reshape(B, Cc, HW).permute(0, 2, 1)
    rd = rows.double().expand(B, 2 * Cc)
    ref = F.silu(ref * (1 + rd[:, None, :Cc]) + rd[:, None, Cc:])
    assert float(ref.abs().max()) < 8          # half an fp16 ulp below 8 is 3.9e-3
    pool = Pool()
    xg, gg, bg = pool.put('x', x.cuda()), pool.put('gamma', gamma.cuda()), pool.put('beta', beta.cuda())
    fg = pool.put('rows', rows.cuda())         # (guarded: a read past [B][2C] poisons the result)
    o = _groupnorm_film(pool, xg, gg, bg, fg, 0 if shared else 2 * Cc)
    pool.check(f'groupnorm film C={Cc} HW={HW}')
    tag = f'groupnorm film C={Cc} HW={HW} shared={shared}'
    assert report(tag + ' f32', o['f32'], ref, 2e-5) < 2e-5
    assert report(tag + ' f16', o['f16'], ref, 4e-3) < 4e-3
    assert report(tag + ' hi+lo', o['f16'].float() + o['lo'].float(), o['f32'], 4e-6) < 4e-6
    # the raw copies are the un-normalised input, untouched by the rows
    assert torch.equal(o['raw'], xg.half()) and torch.equal(o['raw_lo'], (xg - xg.half().float()).half())


@pytest.mark.parametrize('Cc,HW', [(192, 1024), (768, 1), (768, 1600)])
def test_groupnorm_null_rows_are_bit_identical_to_plain(Cc, HW):
    from kernels import groupnorm
    g = torch.Generator().manual_seed(Cc + HW + 1)
    x = (torch.randn(2, HW, Cc, generator=g) * 1.5 + 0.3).cuda()
    gamma = (1 + 0.1 * torch.randn(Cc, generator=g)).cuda()
    beta = (0.1 * torch.randn(Cc, generator=g)).cuda()
    pool = Pool()
    o = _groupnorm_film(pool, x, gamma, beta, None, 0)
    pool.check('groupnorm film, null rows')
    plain = groupnorm(x, None, gamma, beta, 1e-5, 1, want=('f16', 'f32', 'raw', 'lo', 'raw_lo'))
    torch.cuda.synchronize()
    for k in ('f16', 'f32', 'raw', 'lo', 'raw_lo'):
        assert torch.equal(o[k], plain[k]), k


def _split(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


# (input recipe and bars of tests/test_inpaint_gpu.py::test_attention_d96_vs_fp64; heads = 8, B = 2 as in the model)
@pytest.mark.parametrize('nq,nkv', [(1024, 1024), (144, 144), (36, 36), (9, 9), (4, 4), (1, 1), (33, 1001)])
@pytest.mark.parametrize('d', [24, 48])
@pytest.mark.parametrize('full', [False, True])
def test_attention_d24_d48_vs_fp64(nq, nkv, d, full):
    torch.manual_seed(nq + nkv)
    B, heads = 2, 8
    BH, nkv_pad = B * heads, (nkv + 7) // 8 * 8
    q = torch.randn(BH, nq, d, device='cuda')
    k = torch.randn(BH, nkv, d, device='cuda')
    v = torch.randn(BH, nkv, d, device='cuda')
    vt = torch.zeros(BH, d, nkv_pad, device='cuda')
    vt[:, :, :nkv] = v.transpose(1, 2)
    scale = d ** -0.5
    L = _lib()
    lib = L.load()
    pool = Pool()
    out = pool.new('out', (B, nq, heads * d), torch.float16)
    if full:
        ops = [pool.put(n, t) for n, t in zip(('q', 'q_lo', 'k', 'k_lo', 'vt', 'vt_lo'), _split(q) + _split(k) + _split(vt))]
        out_lo = pool.new('out_lo', (B, nq, heads * d), torch.float16)
        L.check(lib.sdmi_k_attention_split16(*[t.data_ptr() for t in ops], out.data_ptr(), out_lo.data_ptr(), BH, heads, nq, nkv, nkv_pad, d,
                                             scale, L.stream_ptr()))
        torch.cuda.synchronize()
        got = out.double() + out_lo.double()
        qr, kr, vr = q.double(), k.double(), v.double()
        tol = 2e-5
    else:
        qh, kh, vh = pool.put('q', q.half()), pool.put('k', k.half()), pool.put('vt', vt.half())
        L.check(lib.sdmi_k_attention(qh.data_ptr(), kh.data_ptr(), vh.data_ptr(), out.data_ptr(), BH, heads, nq, nkv, nkv_pad, d, scale,
                                     L.stream_ptr()))
        torch.cuda.synchronize()
        got = out.double()
        qr, kr, vr = qh.double(), kh.double(), vh[:, :, :nkv].transpose(1, 2).double()
        tol = 4e-3
    pool.check(f'attention d{d} nq={nq} nkv={nkv}')
    ref = torch.softmax(qr @ kr.transpose(1, 2) * scale, dim=-1) @ vr                # [BH][nq][d]
    ref = ref.view(B, heads, nq, d).permute(0, 2, 1, 3).reshape(B, nq, heads * d)
    err = float((got - ref).abs().max())
    print(f'[attn d{d} nq={nq} nkv={nkv} full={full}] max-abs {err:.3e}', flush=True)
    assert err <= tol


# ---- the UNet against the reference goldens -----------------------------------------------------------------------------
def _golden_unet(golden_dir, case):
    z = np.load(os.path.join(golden_dir, f'churches_unet_{case}.npz'))
    assert int(z['weight_seed']) == 0
    x, t = _unet_inputs(int(z['batch']), int(z['h']), int(z['w']), tuple(int(v) for v in z['t']), seed=int(z['input_seed']))
    return x, t, torch.from_numpy(z['eps'])


@pytest.mark.parametrize('prec', ['mixed', 'full'])
@pytest.mark.parametrize('case', UNET_CASES)
def test_churches_unet_matches_reference(case, prec, golden_dir):
    """16x16_b2: the smallest legal latent (the middle block sees one pixel), two rows with different scale / shift; 32x32: the
    native latent; 48x48_b1: token counts 2304 / 576 / 144 / 36 / 9; 16x16_b10: the 8 + 2 chunking of a sample_diffusion.py batch."""
    x, t, ref = _golden_unet(golden_dir, case)
    eps = _unet(prec)(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    err = (eps.float().cpu() - ref).abs()
    mx, rms = float(err.max()), float(err.pow(2).mean().sqrt())
    tol = MIXED_TOL if prec == 'mixed' else FULL_TOL
    print(f'[churches unet {case} {prec}] max-abs {mx:.3e} rms {rms:.3e} |eps|max {ref.abs().max():.3f} (tol {tol:.1e})', flush=True)
    assert eps.shape == ref.shape and bool(torch.isfinite(eps).all())
    assert mx <= tol


def test_churches_unet_tape_replay_across_timesteps():
    """The scale-shift rows come from the timestep table when a forward is hinted: a replayed tape must normalise with the row
    of ITS timestep, not with the row it was recorded at."""
    m = _unet('mixed')
    x, _ = _unet_inputs(2, 16, 16, (981, 981), seed=5)
    x = x.cuda()
    t981, t1 = torch.full((2,), 981, dtype=torch.long, device='cuda'), torch.full((2,), 1, dtype=torch.long, device='cuda')
    lib = m._handle.lib

    def stats():
        a, b = C.c_int64(0), C.c_int64(0)
        _lib().check(lib.sdmi_unet_tape_stats(m._handle.h, C.byref(a), C.byref(b)))
        return a.value, b.value
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
    # (the first hinted call records -- or replays, when an earlier test recorded this shape on the same workspace); the later two replay
    assert (r1, c1) in ((r0, c0 + 1), (r0 + 1, c0)) and (r2, c2) == (r1 + 1, c1) and (r3, c3) == (r2 + 1, c2), ((r0, c0), (r1, c1), (r2, c2), (r3, c3))
    assert torch.equal(a, un981) and torch.equal(b, un1) and torch.equal(c, un981)


# ---- pipeline -------------------------------------------------------------------------------------------------------------
def _pipeline_noise(seed, steps, shape):          # (tools/make_golden_churches.py pipeline_noise)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), [torch.randn(shape, generator=g) for _ in range(steps)]


def test_churches_pipeline_matches_reference_loop(golden_dir):
    """The body of scripts/sample_diffusion.py's make_convolutional_sample on HIP classes: DDIM at eta 1.0 with no conditioning
    (the per-step noise handed out from the seeded sequence the golden tool used), then the KL-f8 decode of samples / scale_factor
    -- against the reference DDIMSampler loop and the reference decoder on the CPU.  The bars are the fixture's: how far `samples`
    and `x_dec` of that reference loop move when every eps of every step is off by the mixed bar, 1e-3, on every element."""
    from stable_diffusion_amd import AutoencoderKLHIP, DDIMSamplerHIP, LatentDiffusionHIP
    z = np.load(os.path.join(golden_dir, 'churches_pipeline_16.npz'))
    steps, b, h, w = int(z['steps']), int(z['batch']), int(z['h']), int(z['w'])
    scale_factor = float(z['scale_factor'])
    assert scale_factor != 1.0 and float(z['perturb']) == MIXED_TOL
    unet = _unet('mixed')
    vae = AutoencoderKLHIP(synthetic.CHURCHES_VAE_DDCONFIG, None, 4)
    dec_keys = [(k, tuple(v.shape)) for k, v in vae.state_dict().items() if k.startswith(('decoder.', 'post_quant_conv.'))]
    sd = {k: v for k, v in vae.state_dict().items()}
    sd.update(synthetic.synthetic_named_state_dict(dec_keys, int(z['weight_seed'])))
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda()
    ld = LatentDiffusionHIP(unet, **synthetic.CHURCHES_SCHEDULE).cuda()
    x_T, noises = _pipeline_noise(int(z['noise_seed']), steps, (b, 4, h, w))
    seq = [n.cuda() for n in noises]
    smp = DDIMSamplerHIP(ld)
    smp._noise_like = lambda shape, device: seq.pop(0)
    with contextlib.redirect_stdout(io.StringIO()):
        samples, _ = smp.sample(steps, batch_size=b, shape=(4, h, w), eta=float(z['eta']), verbose=False, x_T=x_T.cuda())
    x_dec = vae.decode(samples / scale_factor)
    torch.cuda.synchronize()
    assert not seq and bool(torch.isfinite(samples).all()) and bool(torch.isfinite(x_dec).all())
    e_s = float((samples.cpu() - torch.from_numpy(z['samples'])).abs().max())
    e_x = float((x_dec.cpu() - torch.from_numpy(z['x_dec'])).abs().max())
    bar_s, bar_x = float(z['bar_samples']), float(z['bar_x_dec'])
    print(f'[churches pipeline] samples max-abs {e_s:.3e} (bar {bar_s:.3e}); x_dec max-abs {e_x:.3e} (bar {bar_x:.3e})', flush=True)
    assert e_s <= bar_s and e_x <= bar_x, (e_s, bar_s, e_x, bar_x)
