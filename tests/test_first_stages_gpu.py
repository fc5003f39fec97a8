"""The rest of the first-stage zoo on the MI355X -- KL-f32 (six levels, attention on the 16 x 16 and 8 x 8 levels, 64 latent channels: the
wide fp32 ends), KL-f4, VQ-f8 / VQ-f8-n256 / VQ-f16 (level attention on a codebook first stage) and their stand-ins at ch 64 -- against
goldens of the reference's own Encoder / Decoder (tools/make_golden_first_stages.py, fp32, CPU); weights and inputs are regenerated here
from the fixtures' seeds.

KL-f32 latents (f = 32): 2 x 3 (6 / 24 tokens at the two attention levels, W % 4 != 0: the one-pixel conv_out form), 4 x 4 (16 / 64 tokens,
exactly one key tile at the upper level; the 4-pixel form), 3 x 5 (15 / 60 tokens); on kl_f32_thin also 4 x 8 at B = 2, 2 x 2 at B = 10
(two library calls) and 1 x 2 (a 32 x 64 image: one pixel row and two tokens at the lowest level -- it runs and meets the same bars).
VQ latents: 6 x 10, 8 x 8 (B = 1 and 2), 10 x 12; encode (h), decode with and without quantization, the quantizer's codes.
KL-f4 latents 8 x 8 and 6 x 10 at f = 4.

Mixed precision: the project's first-stage bars (tests/test_vae_gpu.py: decode 3.0e-3, moments / h 3.5e-3); every case prints its error
beside the fixture's fp16-operand floor (the reference arithmetic at fp16 operands against itself unrounded).  A case measured above its
bar on the MI355X is listed in FLOOR_CASES and held to 1.25 x its floor instead; the bar is not raised, and only cases that
first_stages_floors_above_bar.json names -- where the reference's own fp16-operand arithmetic misses the bar too -- may be listed
(test_floor_cases_are_named_by_the_tool).  With these weights that is every decode of this file: the floors are 3.1e-3 (KL-f4), 4.9e-3 ..
7.4e-3 (VQ-f8), 9.0e-3 .. 1.5e-2 (VQ-f16, KL-f32: five and six levels of 3x3 convs behind unit-variance latents); every moments / h floor
is inside its bar.  Measured values: the comment on FLOOR_CASES and profiles/first_stages_parity.txt.
Full precision: the hard bars of tests/test_first_stage_full_gpu.py, decode 3.0e-4 and moments / h 3.5e-4, against the same goldens."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vq_ref  # noqa: E402
from stable_diffusion_amd import synthetic  # noqa: E402

DEC_TOL, ENC_TOL = 3.0e-3, 3.5e-3            # tests/test_vae_gpu.py
DEC_HARD, ENC_HARD = 3.0e-4, 3.5e-4          # tests/test_first_stage_full_gpu.py
KL_F32 = ['2x3_b1', '4x4_b1', '3x5_b1']
VQ = ['6x10_b1', '8x8_b1', '8x8_b2', '10x12_b1']
KL_CASES = {'kl_f32': KL_F32, 'kl_f32_thin': KL_F32 + ['4x8_b2', '2x2_b10', '1x2_b1'], 'kl_f4': ['8x8_b1', '6x10_b1']}
VQ_CASES = {'vq_f8': VQ, 'vq_f8_thin': VQ, 'vq_f16_thin': VQ, 'vq_f16': ['8x8_b1'], 'vq_f8_n256_thin': ['8x8_b1']}
KL_ALL = [(t, c) for t, cs in KL_CASES.items() for c in cs]
VQ_ALL = [(t, c) for t, cs in VQ_CASES.items() for c in cs]
# (tag, kind, case) measured above the bar in mixed precision on an MI355X, held to 1.25 x the fixture's floor: every decode of this file, whose
# floors are themselves above the bar.  Measured max-abs (and its share of the floor; per case in profiles/first_stages_parity.txt):
#   kl_f32 / kl_f32_thin decode  4.60e-03 .. 8.50e-03 (0.44 .. 0.78 x floor)  rms 7.0e-4 .. 8.3e-4
#   kl_f4 decode                 3.02e-03 .. 3.04e-03 (0.94 .. 0.97 x floor)
#   vq_f8 / _thin / n256 decode  3.68e-03 .. 7.15e-03 (0.59 .. 1.24 x floor)  rms 6.2e-4 .. 7.9e-4
#   vq_f16 / vq_f16_thin decode  7.02e-03 .. 1.08e-02 (0.64 .. 0.96 x floor)  rms 8.4e-4 .. 9.8e-4
# The closest is vq_f8_thin dec_nq 8x8_b2 at 6.149e-3 against 1.25 x 4.975e-3 = 6.219e-3.  Every moments / h case is inside its bar:
# 7.01e-04 .. 1.83e-03 against 3.5e-3.
# KL-f32 before its decoder's deep levels took split-fp16 operands (csrc/vae.cpp, Vae::build): 8.5e-3 .. 1.83e-2, three of the nine above
# 1.25 x their floor at an rms no larger than the floor's own (1.1e-3 .. 1.3e-3).
FLOOR_CASES = (
    ('kl_f32', 'dec', '2x3_b1'), ('kl_f32', 'dec', '4x4_b1'), ('kl_f32', 'dec', '3x5_b1'),
    ('kl_f32_thin', 'dec', '2x3_b1'), ('kl_f32_thin', 'dec', '4x4_b1'), ('kl_f32_thin', 'dec', '3x5_b1'), ('kl_f32_thin', 'dec', '4x8_b2'),
    ('kl_f32_thin', 'dec', '2x2_b10'), ('kl_f32_thin', 'dec', '1x2_b1'),
    ('kl_f4', 'dec', '8x8_b1'), ('kl_f4', 'dec', '6x10_b1'),
    ('vq_f8', 'dec_q', '6x10_b1'), ('vq_f8', 'dec_nq', '6x10_b1'), ('vq_f8', 'dec_q', '8x8_b1'), ('vq_f8', 'dec_nq', '8x8_b1'), ('vq_f8', 'dec_q',
    '8x8_b2'), ('vq_f8', 'dec_nq', '8x8_b2'), ('vq_f8', 'dec_q', '10x12_b1'), ('vq_f8', 'dec_nq', '10x12_b1'),
    ('vq_f8_thin', 'dec_q', '6x10_b1'), ('vq_f8_thin', 'dec_nq', '6x10_b1'), ('vq_f8_thin', 'dec_q', '8x8_b1'), ('vq_f8_thin', 'dec_nq', '8x8_b1'),
    ('vq_f8_thin', 'dec_q', '8x8_b2'), ('vq_f8_thin', 'dec_nq', '8x8_b2'), ('vq_f8_thin', 'dec_q', '10x12_b1'), ('vq_f8_thin', 'dec_nq', '10x12_b1'),
    ('vq_f16_thin', 'dec_q', '6x10_b1'), ('vq_f16_thin', 'dec_nq', '6x10_b1'), ('vq_f16_thin', 'dec_q', '8x8_b1'), ('vq_f16_thin', 'dec_nq',
    '8x8_b1'), ('vq_f16_thin', 'dec_q', '8x8_b2'), ('vq_f16_thin', 'dec_nq', '8x8_b2'), ('vq_f16_thin', 'dec_q', '10x12_b1'), ('vq_f16_thin',
    'dec_nq', '10x12_b1'),
    ('vq_f16', 'dec_q', '8x8_b1'), ('vq_f16', 'dec_nq', '8x8_b1'),
    ('vq_f8_n256_thin', 'dec_q', '8x8_b1'), ('vq_f8_n256_thin', 'dec_nq', '8x8_b1'),
)
_models = {}


def _model(tag, prec='mixed'):
    key = (tag, prec)
    if key not in _models:
        if len(_models) >= 4:                      # (the full-width models are 270 .. 420 MB of fp32 parameters each)
            _models.clear()
            torch.cuda.empty_cache()
        m = synthetic.make_first_stage(synthetic.FIRST_STAGES[tag], prec)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models[key] = m.cuda().eval()
    return _models[key]


def _pick(img, z):
    """the elements of a library output that the fixture holds: the kept batch samples, and of those the sampled elements where it is large"""
    kept = img[[int(i) for i in z['samples']]]
    assert tuple(kept.shape) == tuple(int(s) for s in z['full_shape'])
    elems = torch.from_numpy(z['elems'])
    return kept.reshape(-1)[elems] if elems.numel() else kept


def _dec_case(golden_dir, tag, case, kind='dec'):
    z = np.load(os.path.join(golden_dir, f'{tag}_{kind}_{case}.npz'))
    ed = synthetic.FIRST_STAGES[tag]['embed_dim']
    g = torch.Generator().manual_seed(int(z['input_seed']))
    lat = torch.randn(int(z['batch']), ed, int(z['h']), int(z['w']), generator=g)
    return lat, torch.from_numpy(z['out']), z, float(z['floor_maxabs'])


def _enc_case(golden_dir, tag, case):
    z = np.load(os.path.join(golden_dir, f'{tag}_enc_{case}.npz'))
    g = torch.Generator().manual_seed(int(z['input_seed']))
    x = torch.rand(int(z['batch']), 3, int(z['h']), int(z['w']), generator=g) * 2 - 1
    return x, torch.from_numpy(z['moments']), float(z['floor_maxabs'])


def _hold(tag, kind, case, err, bar, floor):
    mx = float(err.max())
    listed = (tag, kind, case) in FLOOR_CASES
    print(f'[first_stages {kind} {tag} {case}] HIP-vs-reference(fp32) max-abs {mx:.3e} rms {float(err.pow(2).mean().sqrt()):.3e} | fp16-operand '
          f'floor {floor:.3e} | bar {bar:.1e}' + (f' (listed: held to 1.25 x floor = {1.25 * floor:.3e})' if listed else ''), flush=True)
    return mx <= (1.25 * floor if listed else bar)


def test_floor_cases_are_named_by_the_tool(golden_dir):
    with open(os.path.join(golden_dir, 'first_stages_floors_above_bar.json')) as f:
        named = {(t, k, c) for t, k, c, _ in json.load(f)['above_bar_over_1.25']}
    assert set(FLOOR_CASES) <= named, sorted(set(FLOOR_CASES) - named)
    assert len(set(FLOOR_CASES)) == len(FLOOR_CASES)


# ---- KL-f32, KL-f4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,case', KL_ALL)
def test_kl_decode_matches_reference_golden(tag, case, golden_dir):
    """kl_f4 constructs on the parent commit too, and at the 8 x 8 latent it launches there what it launches here (three levels, no level
    attention, 3 latent channels: nothing of it is new) -- 3.018e-3, a hair above the 3.0e-3 bar under a floor of 3.13e-3, hence listed.
    Its 6 x 10 latent is refused on the parent in mixed precision (60 tokens: the GEMM-form mid attention needs H W % 64 == 0) and takes
    the flash form here.  kl_f32 and kl_f32_thin fail on the parent in the constructor (z_channels 64)."""
    lat, ref, z, floor = _dec_case(golden_dir, tag, case)
    img = _model(tag).decode(lat.cuda()).cpu()
    assert img.dtype == torch.float32 and bool(torch.isfinite(img).all())
    assert _hold(tag, 'dec', case, (_pick(img, z) - ref).abs(), DEC_TOL, floor)


@pytest.mark.parametrize('tag,case', KL_ALL)
def test_kl_encode_matches_reference_golden(tag, case, golden_dir):
    x, ref, floor = _enc_case(golden_dir, tag, case)
    m = _model(tag)
    mom = m.encode_moments(x.cuda())
    assert mom.shape == ref.shape and bool(torch.isfinite(mom).all())
    assert _hold(tag, 'enc', case, (mom.cpu() - ref).abs(), ENC_TOL, floor)
    post = m.encode(x.cuda())                    # the posterior: mode() is the first embed_dim channels of the moments
    assert torch.equal(post.mode(), mom[:, :m.embed_dim])
    assert torch.allclose(post.std, torch.exp(0.5 * mom[:, m.embed_dim:].clamp(-30.0, 20.0)))


@pytest.mark.parametrize('tag,case', [('kl_f32', '2x3_b1'), ('kl_f32_thin', '4x4_b1'), ('kl_f32_thin', '3x5_b1'), ('kl_f4', '6x10_b1')])
def test_kl_full_precision_matches_reference_golden(tag, case, golden_dir):
    m = _model(tag, 'full')
    assert m._handle.lib.sdmi_vae_precision(m._handle.h) == 1
    lat, ref, z, _ = _dec_case(golden_dir, tag, case)
    err = (_pick(m.decode(lat.cuda()).cpu(), z) - ref).abs()
    x, mref, _ = _enc_case(golden_dir, tag, case)
    merr = (m.encode_moments(x.cuda()).cpu() - mref).abs()
    print(f'[first_stages full {tag} {case}] decode max-abs {float(err.max()):.3e} (hard bar {DEC_HARD:.1e}) moments max-abs '
          f'{float(merr.max()):.3e} (hard bar {ENC_HARD:.1e})', flush=True)
    assert float(err.max()) <= DEC_HARD and float(merr.max()) <= ENC_HARD


# ---- VQ-f8, VQ-f8-n256, VQ-f16 ------------------------------------------------------------------------------------------------------------
def _codes_match(m, lat, z):
    """the quantizer's codes against the reference's wherever the fp64 distance gap is clear -- and the fixture's input is one where it is
    clear at every pixel (the tool advanced the seed until it was)"""
    codes = m.quantize(lat.cuda())[2][2].cpu()
    e = dict(m.named_parameters())['quantize.embedding.weight'].detach().cpu()
    ref_idx = torch.from_numpy(z['idx']).long()
    assert torch.equal(vq_ref.quantize(lat, e)[1], ref_idx)                  # (the regenerated codebook and latent are the tool's)
    d = vq_ref.distances(lat.double(), e.double())
    best = d.gather(1, ref_idx.view(-1, 1)).squeeze(1)
    second = d.scatter(1, ref_idx.view(-1, 1), float('inf')).min(1).values
    clear = (second - best) > 1e-5 * best.abs().clamp_min(1e-30)
    assert float(clear.double().mean()) == 1.0 and float(z['clear_share']) == 1.0
    assert torch.equal(codes[clear], ref_idx.view(-1)[clear])


@pytest.mark.parametrize('tag,case', VQ_ALL)
def test_vq_matches_reference_golden(tag, case, golden_dir):
    m = _model(tag)
    assert m.attn_level_mask != 0
    x, href, hfloor = _enc_case(golden_dir, tag, case)
    h = m.encode(x.cuda())
    assert h.shape == href.shape and bool(torch.isfinite(h).all())
    ok = [_hold(tag, 'enc', case, (h.cpu() - href).abs(), ENC_TOL, hfloor)]
    lat, ref_q, zq, floor_q = _dec_case(golden_dir, tag, case, 'dec_q')
    _, ref_nq, znq, floor_nq = _dec_case(golden_dir, tag, case, 'dec_nq')
    _codes_match(m, lat, zq)
    dec_q, dec_nq = m.decode(lat.cuda()).cpu(), m.decode(lat.cuda(), force_not_quantize=True).cpu()
    assert bool(torch.isfinite(dec_q).all()) and bool(torch.isfinite(dec_nq).all())
    ok.append(_hold(tag, 'dec_q', case, (_pick(dec_q, zq) - ref_q).abs(), DEC_TOL, floor_q))
    ok.append(_hold(tag, 'dec_nq', case, (_pick(dec_nq, znq) - ref_nq).abs(), DEC_TOL, floor_nq))
    assert all(ok), (tag, case, ok)           # (every figure is printed before the first one is judged)


@pytest.mark.parametrize('tag,case', [('vq_f8', '6x10_b1'), ('vq_f16_thin', '8x8_b2')])
def test_vq_full_precision_matches_reference_golden(tag, case, golden_dir):
    m = _model(tag, 'full')
    assert m._handle.lib.sdmi_vae_precision(m._handle.h) == 1
    x, href, _ = _enc_case(golden_dir, tag, case)
    herr = float((m.encode(x.cuda()).cpu() - href).abs().max())
    lat, ref_q, zq, _ = _dec_case(golden_dir, tag, case, 'dec_q')
    _, ref_nq, znq, _ = _dec_case(golden_dir, tag, case, 'dec_nq')
    eq = float((_pick(m.decode(lat.cuda()).cpu(), zq) - ref_q).abs().max())
    enq = float((_pick(m.decode(lat.cuda(), force_not_quantize=True).cpu(), znq) - ref_nq).abs().max())
    print(f'[first_stages full {tag} {case}] decode max-abs {eq:.3e} (quantized) {enq:.3e} (not quantized) (hard bar {DEC_HARD:.1e}) h max-abs '
          f'{herr:.3e} (hard bar {ENC_HARD:.1e})', flush=True)
    assert eq <= DEC_HARD and enq <= DEC_HARD and herr <= ENC_HARD


# ---- repeatability, the scale keyword, the create entries ----------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,case,kind', [('kl_f32_thin', '3x5_b1', 'dec'), ('vq_f8_thin', '6x10_b1', 'dec_q')])
def test_repeatable_and_scaled(tag, case, kind, golden_dir):
    """two decodes and two encodes of one input are bit-equal; decode_first_stage's scale_factor IS decode's z_scale = 1 / scale_factor"""
    m = _model(tag)
    lat, _, _, _ = _dec_case(golden_dir, tag, case, kind)
    x, _, _ = _enc_case(golden_dir, tag, case)
    lat, x = lat.cuda(), x.cuda()
    assert torch.equal(m.decode(lat), m.decode(lat))
    assert torch.equal(m.encode_moments(x), m.encode_moments(x))
    s = 0.22765929
    assert torch.equal(m.decode_first_stage(lat, scale_factor=s), m.decode(lat, z_scale=1.0 / s))


def test_vq_mask_zero_is_the_old_entry_bit_for_bit():
    """a codebook handle without level attention created through sdmi_vae_create_attn(ext, mask 0) gives the bits of
    sdmi_vae_create_precision's"""
    from stable_diffusion_amd import VQModelInterfaceHIP, _lib
    lib = _lib.load()
    kw = dict(embed_dim=3, n_embed=512, ddconfig=dict(synthetic.CIN_VQ_DDCONFIG, ch=64))
    out = []
    for new_entry in (False, True):
        m = VQModelInterfaceHIP(**kw)
        assert m.attn_level_mask == 0
        if new_entry:
            ext = _lib.VaeExt()
            ext.double_z, ext.mid_attn, ext.n_embed = 0, 1, 512
            h = C.c_void_p()
            _lib.check(lib.sdmi_vae_create_attn(C.byref(m._cfg), C.byref(ext), 3, 0, 0, C.byref(h)))
            lib.sdmi_vae_destroy(m._handle.h)
            m._handle.h = h
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        m = m.cuda().eval()
        lat = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1)).cuda()
        x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda() * 2 - 1
        out.append((m.decode(lat), m.decode(lat, force_not_quantize=True), m.encode(x)))
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[1]))
