"""The older class-conditional ImageNet model (models/ldm/cin256/config.yaml) on the MI355X: its UNet at the yaml's widths
(model_channels 256, channel_mult [1, 2, 4]; SpatialTransformers with 8 / 16 / 32 heads of 32 channels on every level) against goldens of
the reference's own UNetModel (tools/make_golden_cin256_old.py; weights regenerated from the seeded per-key generator), with the one-token
contexts [B, 1, 512] of ClassEmbedder -- the only configuration that combines many heads of 32 channels with the ctx1_broadcast path.

Latents 8 x 8 and 16 x 16 at B = 2 and 32 x 32 at B = 1, t = (1, 741).  Bars: 1e-3 in mixed precision and 2e-5 in full, the bars of
tests/test_rdm_gpu.py, with its fp16-operand floor rule: every case prints its error beside the fixture's floor (computed from the
reference); a mixed case measured above 1e-3 would go into FLOOR_CASES and be held to 1.25 x its floor -- the list is empty (floors
5.1e-4 .. 5.7e-4).  The one-token shortcut equals the general attention path (SDMI_CTX1=0, the switch of tests/test_cin_gpu.py) bit for
bit.  Its first stage, VQ-f8, is tested in tests/test_first_stages_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import synthetic  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MIXED_TOL, FULL_TOL = 1e-3, 2e-5           # tests/test_rdm_gpu.py
UNET_CASES = ['8x8_b2', '16x16_b2', '32x32_b1']
FLOOR_CASES = ()        # cases measured above MIXED_TOL in mixed precision: none
_models = {}


def _unet(prec='mixed'):
    if ('unet', prec) not in _models:
        torch.cuda.empty_cache()
        from stable_diffusion_amd import UNetModelHIP
        m = UNetModelHIP(**synthetic.CIN256_OLD_UNET_KWARGS, hip_precision=prec)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models[('unet', prec)] = m.cuda().eval()
    return _models[('unet', prec)]


def _embedder():
    if 'emb' not in _models:
        from stable_diffusion_amd import ClassEmbedderHIP
        m = ClassEmbedderHIP(**synthetic.CIN256_OLD_CLASS_KWARGS)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models['emb'] = m.cuda().eval()
    return _models['emb']


def _case(name):
    z = np.load(os.path.join(GOLD, f'cin256_old_unet_{name}.npz'))
    g = torch.Generator().manual_seed(int(z['input_seed']))
    x = torch.randn(int(z['batch']), 4, int(z['h']), int(z['w']), generator=g).cuda()
    t = torch.tensor([int(v) for v in z['t']], dtype=torch.int64).cuda()
    with torch.no_grad():
        ctx = _embedder()({'class_label': torch.as_tensor(z['classes'], dtype=torch.int64).cuda()})
    assert ctx.shape == (x.shape[0], 1, 512)
    return z, x, t, ctx


@pytest.mark.parametrize('prec', ['mixed', 'full'])
@pytest.mark.parametrize('case', UNET_CASES)
def test_cin256_old_unet_matches_reference(case, prec, monkeypatch):
    monkeypatch.delenv('SDMI_CTX1', raising=False)
    z, x, t, ctx = _case(case)
    eps = _unet(prec)(x, t, context=ctx)
    torch.cuda.synchronize()
    ref = torch.from_numpy(z['eps'])
    err = (eps.float().cpu() - ref).abs()
    mx, floor = float(err.max()), float(z['floor_maxabs'])
    tol = FULL_TOL if prec == 'full' else (max(MIXED_TOL, 1.25 * floor) if case in FLOOR_CASES else MIXED_TOL)
    print(f'[cin256_old unet {case} {prec}] max-abs {mx:.3e} rms {float(err.pow(2).mean().sqrt()):.3e} |eps|max {float(ref.abs().max()):.3f} '
          f'(tol {tol:.2e}; fp16-operand floor {floor:.2e})', flush=True)
    assert eps.shape == ref.shape and bool(torch.isfinite(eps).all())
    assert mx <= tol


def test_cin256_old_one_token_shortcut_is_the_general_path_bit_for_bit(monkeypatch):
    """many heads of 32 channels over one key: ctx1_broadcast's copy of V against the attention kernels at nkv = 1 (softmax exactly 1)"""
    z, x, t, ctx = _case('16x16_b2')
    m = _unet('mixed')
    monkeypatch.delenv('SDMI_CTX1', raising=False)
    eps1 = m(x, t, context=ctx).clone()
    monkeypatch.setenv('SDMI_CTX1', '0')
    eps0 = m(x, t, context=ctx.clone()).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eps1).all()) and torch.equal(eps1, eps0)
