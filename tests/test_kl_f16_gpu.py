"""The KL-f16 first stage of the retrieval-augmented model (AutoencoderKLHIP with attn_resolutions: AttnBlocks after every ResBlock of a
level, 16 latent channels) on the MI355X against goldens of the reference's own Encoder / Decoder (tools/make_golden_kl_f16.py, fp32, CPU);
weights and inputs are regenerated here from the fixtures' seeds.

Latents: 6 x 10 (60 tokens: below one key tile of the flash kernels; W % 4 != 0, the one-pixel conv_out form), 8 x 8 (exactly one tile;
the 4-pixel form) and 10 x 12 (one tile and a partial one), on the real widths (ch 128, d = 512; B = 1, and B = 2 on 8 x 8), on
kl_f16_thin (ch 64, d = 256; and B = 10 on 8 x 8: two library calls) and, as 16 x 16 and 16 x 24 images, on kl_narrow (d = 128 on the lower
level) and kl_two_levels (d = 64 at the full image resolution too).

Mixed precision: the project's first-stage bars (tests/test_vae_gpu.py: decode 3.0e-3, moments 3.5e-3 -- half an 8-bit level); every case
prints its error beside the fixture's fp16-operand floor (the reference arithmetic at fp16 operands against itself unrounded).  A case
measured above its bar is listed in FLOOR_CASES and held to 1.25 x its floor instead (README's rule of the outlier family); the bar is
not raised.  With these weights the decodes of the five-level configurations have floors of 4.7e-3 .. 9.4e-3, i.e. the reference's own
arithmetic at fp16 operands does not meet 3.0e-3 there (kl_f16_floors_above_bar.json).  Measured on an MI355X: see FLOOR_CASES and
profiles/kl_f16_parity.txt.
Full precision: the hard bars of tests/test_first_stage_full_gpu.py, decode 3.0e-4 and moments 3.5e-4, against the same goldens."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import synthetic  # noqa: E402

DEC_TOL, ENC_TOL = 3.0e-3, 3.5e-3            # tests/test_vae_gpu.py
DEC_HARD, ENC_HARD = 3.0e-4, 3.5e-4          # tests/test_first_stage_full_gpu.py
CASES = {'kl_f16': ['6x10_b1', '8x8_b1', '8x8_b2', '10x12_b1'], 'kl_f16_thin': ['6x10_b1', '8x8_b1', '10x12_b1', '8x8_b10'],
         'kl_narrow': ['8x8_b2', '8x12_b2'], 'kl_two_levels': ['8x8_b2', '8x12_b2']}
ALL = [(t, c) for t, cs in CASES.items() for c in cs]
# (tag, kind, case) measured above the bar in mixed precision on an MI355X, held to 1.25 x the fixture's floor: the eight decodes of the
# five-level configurations, whose floors are themselves above the bar.  Measured max-abs | floor (rms 6.1e-4 .. 6.8e-4 on images of
# |x| <= 3.4): kl_f16 6.30e-3 | 6.10e-3, 4.09e-3 | 5.31e-3, 4.56e-3 | 4.73e-3, 4.85e-3 | 4.92e-3; kl_f16_thin 5.64e-3 | 7.02e-3,
# 5.73e-3 | 5.92e-3, 8.01e-3 | 9.36e-3, 7.02e-3 | 8.80e-3 -- 0.77 .. 1.03 x the floor.  Every other case is inside its bar: the two-level
# decodes 8.3e-4 .. 9.7e-4 (floors 9.5e-4 .. 1.31e-3), all moments 7.4e-4 .. 1.78e-3 (floors 8.9e-4 .. 1.93e-3).
FLOOR_CASES = (('kl_f16', 'dec', '6x10_b1'), ('kl_f16', 'dec', '8x8_b1'), ('kl_f16', 'dec', '8x8_b2'), ('kl_f16', 'dec', '10x12_b1'),
               ('kl_f16_thin', 'dec', '6x10_b1'), ('kl_f16_thin', 'dec', '8x8_b1'), ('kl_f16_thin', 'dec', '10x12_b1'),
               ('kl_f16_thin', 'dec', '8x8_b10'))
_models = {}


def _model(tag, prec='mixed'):
    key = (tag, prec)
    if key not in _models:
        from stable_diffusion_amd import AutoencoderKLHIP
        kw = synthetic.KL_F16_STANDINS[tag]
        m = AutoencoderKLHIP(kw['ddconfig'], {'target': 'torch.nn.Identity'}, kw['embed_dim'], hip_precision=prec)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models[key] = m.cuda().eval()
    return _models[key]


def _dec_case(golden_dir, tag, case):
    z = np.load(os.path.join(golden_dir, f'{tag}_dec_{case}.npz'))
    ed = synthetic.KL_F16_STANDINS[tag]['embed_dim']
    g = torch.Generator().manual_seed(int(z['input_seed']))
    lat = torch.randn(int(z['batch']), ed, int(z['h']), int(z['w']), generator=g) / float(z['scale_factor'])
    return lat, torch.from_numpy(z['out']), [int(i) for i in z['samples']], float(z['floor_maxabs'])


def _enc_case(golden_dir, tag, case):
    z = np.load(os.path.join(golden_dir, f'{tag}_enc_{case}.npz'))
    g = torch.Generator().manual_seed(int(z['input_seed']))
    x = torch.rand(int(z['batch']), 3, int(z['h']), int(z['w']), generator=g) * 2 - 1
    return x, torch.from_numpy(z['moments']), float(z['floor_maxabs'])


def _hold(tag, kind, case, err, bar, floor):
    mx = float(err.max())
    listed = (tag, kind, case) in FLOOR_CASES
    print(f'[kl_f16 {kind} {tag} {case}] HIP-vs-reference(fp32) max-abs {mx:.3e} rms {float(err.pow(2).mean().sqrt()):.3e} | fp16-operand floor '
          f'{floor:.3e} | bar {bar:.1e}' + (f' (listed: held to 1.25 x floor = {1.25 * floor:.3e})' if listed else ''), flush=True)
    assert mx <= (1.25 * floor if listed else bar), (tag, kind, case, mx, floor)


@pytest.mark.parametrize('tag,case', ALL)
def test_decode_matches_reference_golden(tag, case, golden_dir):
    lat, ref, keep, floor = _dec_case(golden_dir, tag, case)
    img = _model(tag).decode(lat.cuda()).cpu()
    assert img.dtype == torch.float32 and img[keep].shape == ref.shape and bool(torch.isfinite(img).all())
    _hold(tag, 'dec', case, (img[keep] - ref).abs(), DEC_TOL, floor)


@pytest.mark.parametrize('tag,case', ALL)
def test_encode_matches_reference_golden(tag, case, golden_dir):
    x, ref, floor = _enc_case(golden_dir, tag, case)
    m = _model(tag)
    mom = m.encode_moments(x.cuda())
    assert mom.shape == ref.shape and bool(torch.isfinite(mom).all())
    _hold(tag, 'enc', case, (mom.cpu() - ref).abs(), ENC_TOL, floor)
    post = m.encode(x.cuda())                    # the posterior: mode() is the first embed_dim channels of the moments
    assert torch.equal(post.mode(), mom[:, :m.embed_dim])
    assert torch.allclose(post.std, torch.exp(0.5 * mom[:, m.embed_dim:].clamp(-30.0, 20.0)))


@pytest.mark.parametrize('tag,case', [('kl_f16', '6x10_b1'), ('kl_f16', '8x8_b2'), ('kl_f16', '10x12_b1'), ('kl_f16_thin', '6x10_b1'),
                                      ('kl_narrow', '8x12_b2'), ('kl_two_levels', '8x8_b2')])
def test_full_precision_matches_reference_golden(tag, case, golden_dir):
    """hip_precision='full' on handles with level attention: attn_block_full at d = 512 / 256 (the wide split-fp16 kernel), 128 and 64.
    Measured on an MI355X (profiles/kl_f16_parity.txt): decode 2.28e-5 .. 3.52e-5 on the five-level configurations and 3.3e-6 .. 3.5e-6 on
    the two-level ones, moments 2.4e-6 .. 9.1e-6 -- a tenth of the hard bars and less; no per-case pins are added."""
    m = _model(tag, 'full')
    assert m._handle.lib.sdmi_vae_precision(m._handle.h) == 1
    lat, ref, keep, _ = _dec_case(golden_dir, tag, case)
    err = (m.decode(lat.cuda()).cpu()[keep] - ref).abs()
    x, mref, _ = _enc_case(golden_dir, tag, case)
    merr = (m.encode_moments(x.cuda()).cpu() - mref).abs()
    print(f'[kl_f16 full {tag} {case}] decode max-abs {float(err.max()):.3e} (hard bar {DEC_HARD:.1e}) moments max-abs {float(merr.max()):.3e} '
          f'(hard bar {ENC_HARD:.1e})', flush=True)
    assert float(err.max()) <= DEC_HARD and float(merr.max()) <= ENC_HARD


def test_decode_is_repeatable_and_scaled(golden_dir):
    """bit-identical run to run; decode_first_stage's 1 / scale_factor equals decoding the pre-scaled latent"""
    m = _model('kl_f16')
    lat, _, _, floor = _dec_case(golden_dir, 'kl_f16', '10x12_b1')
    lat = lat.cuda()
    a, b = m.decode(lat), m.decode(lat)
    assert torch.equal(a, b)
    sf = synthetic.KL_F16_SCALE_FACTOR
    c = m.decode_first_stage(lat * sf, scale_factor=sf)
    assert torch.equal(c, m.decode(lat * sf, z_scale=1.0 / sf))      # the scale_factor keyword IS the pre-scale, bit for bit
    # ... and (z s) / s differs from z by an fp32 rounding, which flips fp16 operand roundings downstream: two mixed decodes of one image,
    # each within this (listed) case's bound of the reference, are within twice that bound of each other
    diff = float((a - c).abs().max())
    print(f'[kl_f16 decode_first_stage kl_f16 10x12_b1] max-abs against the decode of the unscaled latent {diff:.3e} (bound {2 * 1.25 * floor:.3e})',
          flush=True)
    assert diff <= 2 * 1.25 * floor
    e = m.encode_moments(torch.zeros(1, 3, 96, 160, device='cuda'))
    assert torch.equal(e, m.encode_moments(torch.zeros(1, 3, 96, 160, device='cuda')))


def test_mask_zero_is_the_old_entry_bit_for_bit():
    """a handle without level attention created through sdmi_vae_create_attn(mask 0) gives the bits of sdmi_vae_create_precision's"""
    from oracle.vae_ref import TINY_VAE, make_vae_inputs, make_vae_state_dict
    from stable_diffusion_amd import AutoencoderKLHIP, _lib
    lib = _lib.load()
    out = []
    for new_entry in (False, True):
        m = AutoencoderKLHIP(TINY_VAE.ddconfig(), {'target': 'torch.nn.Identity'}, TINY_VAE.embed_dim)
        if new_entry:
            h = C.c_void_p()
            _lib.check(lib.sdmi_vae_create_attn(C.byref(m._cfg), None, 3, 0, 0, C.byref(h)))
            lib.sdmi_vae_destroy(m._handle.h)
            m._handle.h = h
        m.load_state_dict(make_vae_state_dict(TINY_VAE, 0), strict=True)
        m = m.cuda().eval()
        lat = make_vae_inputs(TINY_VAE, 2, 8, 8, seed=1).cuda()
        x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda() * 2 - 1
        out.append((m.decode(lat), m.encode_moments(x)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
