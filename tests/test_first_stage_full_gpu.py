"""The full-precision first stage (AutoencoderKLHIP / VQModelInterfaceHIP with hip_precision='full': every MFMA operand of the
ResBlocks, the resampling convs and the mid-block attention split-fp16) on the GPU.

Reference: an fp64 evaluation of the same network, built here from oracle.vae_ref's layer functions on a .double() state dict
(vae_decode / vae_encode_moments themselves cast their input to fp32).  The committed fp32 reference goldens are the second check.

Hard bars: a tenth of the mixed mode's pinned tolerances (tests/test_vae_gpu.py: decode 3.0e-3, encode moments 3.5e-3;
tests/test_cin_gpu.py / tests/test_inpaint_gpu.py for the VQ stages) -- a mode that costs three MFMA passes has to buy an order of
magnitude.  Per-case pins: 1.25 x the max-abs error measured on an MI355X (profiles/full_precision_first_stage.txt), never above
the hard bar."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import vae_ref  # noqa: E402
from oracle.vae_ref import SD_VAE, SMALL_VAE, TINY_VAE, VAEConfig, make_vae_inputs, make_vae_state_dict  # noqa: E402
from stable_diffusion_amd import synthetic  # noqa: E402

import vq_ref  # noqa: E402

DEC_HARD, ENC_HARD = 3.0e-4, 3.5e-4
WIDE192_VAE = VAEConfig(ch=64, ch_mult=(1, 3), num_res_blocks=1)          # mid width 192: the smallest wide head
CFGS = {'tiny': TINY_VAE, 'small': SMALL_VAE, 'sd': SD_VAE, 'wide192': WIDE192_VAE}

# max-abs against the fp64 oracle, 1.25 x measured on an MI355X (profiles/full_precision_first_stage.txt).  Measured: decode 2.476e-6 /
# 3.780e-6 / 8.419e-6 / 1.123e-5 / 9.022e-6 / 2.904e-6, encode 3.847e-6 / 1.038e-5 / 4.239e-6 (the mixed mode on the same inputs:
# 8.7e-4 ... 1.8e-3 and 2.0e-3 ... 2.2e-3)
DEC_PINS = {'tiny_8x8': 3.1e-6, 'small_16x16': 4.8e-6, 'sd_8x8': 1.06e-5, 'sd_16x24': 1.41e-5, 'sd_32x32': 1.13e-5,
            'wide192_8x8': 3.7e-6}
ENC_PINS = {'tiny_32x32': 4.9e-6, 'sd_64x64': 1.30e-5, 'wide192_32x32': 5.3e-6}
# the VQ stages against the committed fp32 goldens: hard bar = a tenth of the mixed pins (tests/test_cin_gpu.py, tests/test_inpaint_gpu.py),
# pin = 1.25 x measured: cin h 1.019e-5, dec_q 3.242e-5; inpaint h 1.022e-5, dec_q 2.933e-5, dec_nq 2.539e-5
VQ_HARD = {'cin': {'h': 2.0e-4, 'dec_q': 6.1e-4}, 'inpaint': {'h': 2.1e-4, 'dec_q': 5.0e-4, 'dec_nq': 5.0e-4}}
VQ_PINS = {'cin': {'h': 1.28e-5, 'dec_q': 4.06e-5}, 'inpaint': {'h': 1.28e-5, 'dec_q': 3.67e-5, 'dec_nq': 3.18e-5}}

_models, _refs = {}, {}


# ---- fp64 oracle: oracle.vae_ref's layers on a double state dict --------------------------------------------------------------
def _decode64(sd, ch_mult, nrb, z):
    h = vae_ref._conv(sd, 'post_quant_conv', z.double(), padding=0)
    h = vae_ref._conv(sd, 'decoder.conv_in', h)
    h = vae_ref._res(sd, 'decoder.mid.block_1', h)
    if 'decoder.mid.attn_1.q.weight' in sd:
        h = vae_ref._attn(sd, 'decoder.mid.attn_1', h)
    h = vae_ref._res(sd, 'decoder.mid.block_2', h)
    for lvl in reversed(range(len(ch_mult))):
        for i in range(nrb + 1):
            h = vae_ref._res(sd, f'decoder.up.{lvl}.block.{i}', h)
        if lvl != 0:
            h = F.interpolate(h, scale_factor=2.0, mode='nearest')
            h = vae_ref._conv(sd, f'decoder.up.{lvl}.upsample.conv', h)
    return vae_ref._conv(sd, 'decoder.conv_out', vae_ref._swish(vae_ref._gn(sd, 'decoder.norm_out', h)))


def _encode64(sd, ch_mult, nrb, x):
    n = len(ch_mult)
    h = vae_ref._conv(sd, 'encoder.conv_in', x.double())
    for lvl in range(n):
        for i in range(nrb):
            h = vae_ref._res(sd, f'encoder.down.{lvl}.block.{i}', h)
        if lvl != n - 1:
            h = F.pad(h, (0, 1, 0, 1), mode='constant', value=0)
            h = vae_ref._conv(sd, f'encoder.down.{lvl}.downsample.conv', h, stride=2, padding=0)
    h = vae_ref._res(sd, 'encoder.mid.block_1', h)
    if 'encoder.mid.attn_1.q.weight' in sd:
        h = vae_ref._attn(sd, 'encoder.mid.attn_1', h)
    h = vae_ref._res(sd, 'encoder.mid.block_2', h)
    h = vae_ref._conv(sd, 'encoder.conv_out', vae_ref._swish(vae_ref._gn(sd, 'encoder.norm_out', h)))
    return vae_ref._conv(sd, 'quant_conv', h, padding=0)


def _double(sd):
    return {k: v.double() for k, v in sd.items()}


@torch.no_grad()
def _ref64(kind, cfg_name, wseed, batch, h, w, iseed):
    """computed once per case and shared; returns (input fp32, fp64 result)"""
    key = (kind, cfg_name, wseed, batch, h, w, iseed)
    if key not in _refs:
        cfg = CFGS[cfg_name]
        sd = _double(make_vae_state_dict(cfg, wseed))
        if kind == 'dec':
            x = make_vae_inputs(cfg, batch, h, w, seed=iseed)
            _refs[key] = (x, _decode64(sd, cfg.ch_mult, cfg.num_res_blocks, x))
        else:
            g = torch.Generator().manual_seed(iseed)
            x = torch.rand(batch, cfg.in_channels, h, w, generator=g) * 2 - 1
            _refs[key] = (x, _encode64(sd, cfg.ch_mult, cfg.num_res_blocks, x))
    return _refs[key]


def _model(cfg_name, wseed, prec):
    key = (cfg_name, wseed, prec)
    if key not in _models:
        from stable_diffusion_amd import AutoencoderKLHIP
        cfg = CFGS[cfg_name]
        m = AutoencoderKLHIP(cfg.ddconfig(), {'target': 'torch.nn.Identity'}, cfg.embed_dim, hip_precision=prec)
        m.load_state_dict(make_vae_state_dict(cfg, wseed), strict=True)
        _models[key] = m.cuda().eval()
    return _models[key]


def _case(name, golden_dir, kind):
    """(cfg name, weight seed, batch, h, w, input seed, golden output or None)"""
    path = os.path.join(golden_dir, f'vae_{kind}_{name}.npz')
    if name.startswith('wide192'):
        h, w = (int(v) for v in name.split('_')[1].split('x'))
        return 'wide192', 0, 2, h, w, 1 if kind == 'dec' else 2, None
    z = np.load(path)
    gold = torch.from_numpy(z['out' if kind == 'dec' else 'moments'])
    return str(z['cfg']), int(z['weight_seed']), int(z['batch']), int(z['h']), int(z['w']), int(z['input_seed']), gold


def _report(tag, got, ref64, gold, pin, hard):
    err = (got.double() - ref64).abs()
    mx, rms = float(err.max()), float(err.pow(2).mean().sqrt())
    gerr = float((got - gold).abs().max()) if gold is not None else float('nan')
    print(f'[first stage full {tag}] vs fp64 max-abs {mx:.3e} rms {rms:.3e} | vs fp32 golden max-abs {gerr:.3e} | '
          f'|ref|max {float(ref64.abs().max()):.3f} (pin {pin:.2e}, hard bar {hard:.1e})', flush=True)
    assert bool(torch.isfinite(got).all())
    assert mx <= hard and mx <= min(pin, hard)
    if gold is not None:
        assert got.shape == gold.shape and gerr <= hard
    return mx


@pytest.mark.parametrize('case', ['tiny_8x8', 'small_16x16', 'sd_8x8', 'sd_16x24', 'sd_32x32', 'wide192_8x8'])
def test_full_decode_vs_fp64(case, golden_dir):
    """tiny / small: mid width 128, the narrow split-fp16 attention kernel; sd: 512, wide192: 192 -- the wide-head one"""
    cfg_name, wseed, batch, h, w, iseed, gold = _case(case, golden_dir, 'dec')
    lat, ref = _ref64('dec', cfg_name, wseed, batch, h, w, iseed)
    m = _model(cfg_name, wseed, 'full')
    assert m.hip_precision == 'full' and m._handle.lib.sdmi_vae_precision(m._handle.h) == 1
    img = m.decode(lat.cuda()).cpu()
    emix = float((_model(cfg_name, wseed, 'mixed').decode(lat.cuda()).cpu().double() - ref).abs().max())
    print(f'[first stage full decode {case}] mixed mode vs fp64 max-abs {emix:.3e}', flush=True)
    assert img.dtype == torch.float32
    _report(f'decode {case}', img, ref, gold, DEC_PINS[case], DEC_HARD)


@pytest.mark.parametrize('case', ['tiny_32x32', 'sd_64x64', 'wide192_32x32'])
def test_full_encode_vs_fp64(case, golden_dir):
    cfg_name, wseed, batch, h, w, iseed, gold = _case(case, golden_dir, 'enc')
    x, ref = _ref64('enc', cfg_name, wseed, batch, h, w, iseed)
    m = _model(cfg_name, wseed, 'full')
    mom = m.encode_moments(x.cuda()).cpu()
    emix = float((_model(cfg_name, wseed, 'mixed').encode_moments(x.cuda()).cpu().double() - ref).abs().max())
    print(f'[first stage full encode {case}] mixed mode vs fp64 max-abs {emix:.3e}', flush=True)
    _report(f'encode {case}', mom, ref, gold, ENC_PINS[case], ENC_HARD)


# ---- VQ first stages against the committed goldens ----------------------------------------------------------------------------
def _vq(tag, prec):
    key = ('vq', tag, prec)
    if key not in _models:
        from stable_diffusion_amd import VQModelInterfaceHIP
        kw = synthetic.CIN_VQ_KWARGS if tag == 'cin' else synthetic.INPAINT_VQ_KWARGS
        m = VQModelInterfaceHIP(**kw, hip_precision=prec)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models[key] = m.cuda()
    return _models[key]


def _vq_inputs(seed=1, img=128):                 # (tools/make_golden_cin.py / make_golden_inpaint.py vq_inputs)
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(2, 3, img // 8, img // 8, generator=g) * 2 - 1
    x = torch.nn.functional.interpolate(low, scale_factor=8, mode='bilinear', align_corners=False)
    x = (x + 0.1 * torch.randn(x.shape, generator=g)).clamp(-1, 1)
    return x, torch.randn(2, 3, img // 4, img // 4, generator=g)


@pytest.mark.parametrize('tag', ['cin', 'inpaint'])
def test_full_vq_first_stage_matches_reference(tag, golden_dir):
    """cin: mid-block attention on (width 512, the wide-head kernel); inpaint: attention off"""
    z = np.load(os.path.join(golden_dir, f'{tag}_vq_128.npz'))
    img, lat = _vq_inputs(seed=int(z['input_seed']), img=int(z['img']))
    m = _vq(tag, 'full')
    assert m.hip_precision == 'full'
    got = {'h': m.encode(img.cuda()).cpu(), 'dec_q': m.decode(lat.cuda()).cpu()}
    if tag == 'inpaint':
        got['dec_nq'] = m.decode(lat.cuda(), force_not_quantize=True).cpu()
    errs = {}
    for name, t in got.items():
        ref = torch.from_numpy(z[name])
        assert t.shape == ref.shape and bool(torch.isfinite(t).all())
        err = (t - ref).abs()
        errs[name] = float(err.max())
        print(f'[first stage full {tag} vq {name}] vs fp32 golden max-abs {err.max():.3e} rms {err.pow(2).mean().sqrt():.3e} '
              f'|ref|max {ref.abs().max():.3f} (pin {VQ_PINS[tag][name]:.2e}, hard bar {VQ_HARD[tag][name]:.1e})', flush=True)
    assert all(errs[k] <= VQ_HARD[tag][k] and errs[k] <= min(VQ_PINS[tag][k], VQ_HARD[tag][k]) for k in errs), errs


# ---- isolation ------------------------------------------------------------------------------------------------------------------
def test_mixed_keyword_equals_the_old_constructor():
    """hip_precision='mixed' and a handle from sdmi_vae_create (the entry point from before the keyword) give the same bits, with a
    full handle alive and used in the same process; both modes repeat bit for bit"""
    from stable_diffusion_amd import AutoencoderKLHIP, _lib
    cfg = SD_VAE
    lat = make_vae_inputs(cfg, 1, 16, 24, seed=1).cuda()
    mixed, full = _model('sd', 0, 'mixed'), _model('sd', 0, 'full')
    a = mixed.decode(lat)
    f1 = full.decode(lat)
    old = AutoencoderKLHIP(cfg.ddconfig(), {'target': 'torch.nn.Identity'}, cfg.embed_dim)
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.sdmi_vae_create(C.byref(old._cfg), 3, C.byref(h)))
    lib.sdmi_vae_destroy(old._handle.h)
    old._handle.h = h
    assert lib.sdmi_vae_precision(h) == 0
    old.load_state_dict(make_vae_state_dict(cfg, 0), strict=True)
    old = old.cuda().eval()
    b = old.decode(lat)
    a2, f2 = mixed.decode(lat), full.decode(lat)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, a2)
    assert torch.equal(f1, f2) and not torch.equal(f1, a)
    x = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    assert torch.equal(mixed.encode_moments(x), old.encode_moments(x))
    assert torch.equal(full.encode_moments(x), full.encode_moments(x))


def test_full_batches_are_independent_bit_for_bit():
    """the full mode pins split-K off, so an element's summation order does not depend on the batch: two latents decoded together
    equal the two decoded one by one, bit for bit"""
    m = _model('sd', 0, 'full')
    lat = make_vae_inputs(SD_VAE, 2, 8, 16, seed=9).cuda()
    both = m.decode(lat)
    for i in range(2):
        assert torch.equal(m.decode(lat[i:i + 1]), both[i:i + 1])


# ---- what the mode is for -------------------------------------------------------------------------------------------------------
def test_full_uint8_pixels_off_the_reference(golden_dir):
    """sd_32x32 through the reference's uint8 post-processing (scripts/txt2img.py:314-324): pixels that differ from the golden's.
    Measured on an MI355X: mixed 5603 of 196608, full 30."""
    from stable_diffusion_amd.postprocess import to_uint8_images
    z = np.load(os.path.join(golden_dir, 'vae_dec_sd_32x32.npz'))
    lat = make_vae_inputs(SD_VAE, int(z['batch']), int(z['h']), int(z['w']), seed=int(z['input_seed'])).cuda()
    gold = to_uint8_images(torch.from_numpy(z['out']).cuda())
    n = {prec: int((to_uint8_images(_model('sd', 0, prec).decode(lat)) != gold).sum()) for prec in ('mixed', 'full')}
    print(f'[first stage full uint8 sd_32x32] pixels (of {gold.numel()}) that differ from the reference image: mixed {n["mixed"]}, '
          f'full {n["full"]}', flush=True)
    assert n['full'] <= n['mixed']


@torch.no_grad()
def test_full_code_flips_off_the_fp64_encoder(golden_dir):
    """cin_vq_128: encode, then the nearest codebook row of every latent pixel against that of the fp64 oracle's encoding.
    Measured on an MI355X: mixed 2 of 2048 codes differ, full 0."""
    z = np.load(os.path.join(golden_dir, 'cin_vq_128.npz'))
    img, _ = _vq_inputs(seed=int(z['input_seed']), img=int(z['img']))
    dd = synthetic.CIN_VQ_KWARGS['ddconfig']
    sd = _double({k: v.detach().cpu() for k, v in _vq('cin', 'full').state_dict().items()})
    e = sd['quantize.embedding.weight']
    h64 = _encode64(sd, dd['ch_mult'], dd['num_res_blocks'], img)

    def codes(h):
        return torch.argmin(vq_ref.distances(h.double(), e), dim=1)
    want = codes(h64)
    flips = {}
    for prec in ('mixed', 'full'):
        h = _vq('cin', prec).encode(img.cuda()).cpu()
        flips[prec] = int((codes(h) != want).sum())
        print(f'[first stage full code flips cin_vq_128 {prec}] h vs fp64 max-abs {float((h.double() - h64).abs().max()):.3e}, '
              f'{flips[prec]} of {want.numel()} codes differ from the fp64 encoder\'s', flush=True)
    assert flips['full'] <= flips['mixed']
