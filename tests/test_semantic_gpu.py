"""The semantic-synthesis models on the device against the reference goldens of tools/make_golden_semantic.py:

* the UNet (model_channels 128, channel_mult [1, 4, 8], legacy AttentionBlock in the middle block only, plain Downsample / Upsample
  convolutions, six input channels) in both precisions at the project's bars, 1e-3 mixed and 2e-5 full, each printed beside the case's
  stored fp16-operand floor; a case the golden tool lists in semantic_floors_above_bar.json (floor above 1e-3 / 1.25) is held to
  1.25 x its floor in mixed precision -- the project's outlier rule; the bar itself is not raised;
* SpatialRescalerHIP.encode against the reference module's fp32 at twice the fp64 bar of tests/test_rescale_kernels_gpu.py (both are
  within one bar of fp64), encode_labels bit-equal to encode(one_hot);
* the pipeline: labels 64 x 64, B = 2, 10 DDIM steps at eta 0 against the reference DDIMSampler over the reference modules at the
  fixture's bar (the divergence of the reference's own second run with every eps moved by 1e-3 sign(randn)), and decode_first_stage of
  the golden's samples at the un-tiled VQ-f4 pin of tests/test_faces_gpu.py;
* synthesize: one step at 64 x 128 from labels and from the one-hot tensor with one x_T gives the same image bit for bit."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import test_rescale_kernels_gpu as TRK  # noqa: E402  (the fp64 reference and bar of the rescale kernels)
from test_faces_gpu import VQ_DEC_PIN  # noqa: E402
from stable_diffusion_amd import synthetic  # noqa: E402

DEV = 'cuda'
MIXED_TOL, FULL_TOL = 1e-3, 2e-5
UNET_CASES = ['8x8_b2', '16x24_b1', '32x32_b1', '8x8_b10']
RESCALER_CASES = ['yaml_16x24_randn', 'yaml_16x24_onehot', 'yaml_13x19_bias', 'c5_6x10_n1', 'c7_12x20_nomap']
_models = {}


def _pipeline(prec):
    """one SemanticSynthesisHIP per precision for the module (seeded weights under the reference's key names)"""
    if prec not in _models:
        _models.clear()
        torch.cuda.empty_cache()
        from stable_diffusion_amd import SemanticSynthesisHIP
        _models[prec] = SemanticSynthesisHIP(hip_precision=prec).load_synthetic(0).cuda()
    return _models[prec]


def _unet_inputs(batch, channels, h, w, ts, seed=1):       # (tools/make_golden_semantic.py unet_inputs)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, channels, h, w, generator=g), torch.tensor(ts, dtype=torch.int64)


def _rescaler_input(kind, batch, channels, h, w, seed=2):   # (tools/make_golden_semantic.py rescaler_input)
    g = torch.Generator().manual_seed(seed)
    if kind == 'randn':
        return 3.0 * torch.randn(batch, channels, h, w, generator=g)
    return F.one_hot(torch.randint(0, channels, (batch, h, w), generator=g), channels).permute(0, 3, 1, 2).float().contiguous()


@pytest.mark.parametrize('case', UNET_CASES)
@pytest.mark.parametrize('prec', ['full', 'mixed'])      # (outermost: one model per precision, 'mixed' stays for the tests below)
def test_unet_matches_reference(prec, case, golden_dir):
    """8x8_b2: the smallest legal latent (the middle block sees 2 x 2 pixels); 16x24_b1: non-square; 32x32_b1; 8x8_b10: chunked 8 + 2"""
    z = np.load(os.path.join(golden_dir, f'semantic_unet_{case}.npz'))
    with open(os.path.join(golden_dir, 'semantic_floors_above_bar.json')) as f:
        above = {e['case']: float(e['floor_maxabs']) for e in json.load(f)}
    assert int(z['weight_seed']) == 0
    floor = float(z['floor_maxabs'])
    assert (case in above) == (floor > MIXED_TOL / 1.25) and above.get(case, floor) == floor
    x, t = _unet_inputs(int(z['batch']), 6, int(z['h']), int(z['w']), tuple(int(v) for v in z['t']), seed=int(z['input_seed']))
    ref = torch.from_numpy(z['eps'])
    eps = _pipeline(prec).model.diffusion_model(x.cuda(), t.cuda())
    torch.cuda.synchronize()
    err = (eps.float().cpu() - ref).abs()
    mx, rms = float(err.max()), float(err.pow(2).mean().sqrt())
    tol = FULL_TOL if prec == 'full' else (1.25 * floor if case in above else MIXED_TOL)
    print(f'[semantic unet {case} {prec}] max-abs {mx:.3e} rms {rms:.3e} |eps|max {ref.abs().max():.3f} (tol {tol:.3e}, fp16-operand floor '
          f'{floor:.3e})', flush=True)
    assert eps.shape == ref.shape and bool(torch.isfinite(eps).all())
    assert mx <= tol


@pytest.mark.parametrize('case', RESCALER_CASES)
def test_rescaler_matches_reference_module(case, golden_dir):
    from stable_diffusion_amd import SpatialRescalerHIP
    z = np.load(os.path.join(golden_dir, f'semantic_rescaler_{case}.npz'))
    kwargs = json.loads(str(z['kwargs']))
    r = SpatialRescalerHIP(**kwargs)
    r.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in r.state_dict().items()], int(z['weight_seed'])), strict=True)
    r = r.cuda()
    x = _rescaler_input(str(z['kind']), int(z['batch']), kwargs['in_channels'], int(z['h']), int(z['w']), seed=int(z['input_seed'])).cuda()
    out = r.encode(x)
    torch.cuda.synchronize()
    ref = torch.from_numpy(z['out']).cuda()
    w = r.channel_mapper.weight.detach().flatten(1) if r.remap_output else None
    b = r.channel_mapper.bias.detach() if r.remap_output and r.channel_mapper.bias is not None else None
    _, bound = TRK._ref_and_bound(x, w, b, r.n_stages)
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    err = (out.double() - ref.double()).abs()
    ratio = float((err / (2 * bound).clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
    print(f'[semantic rescaler {case}] max-abs vs the reference module {float(err.max()):.3e}, worst err / (2 x fp64 bar) {ratio:.4f}', flush=True)
    assert ratio <= 1.0
    if str(z['kind']) == 'onehot':
        labels = x.argmax(dim=1)
        for dt in (torch.uint8, torch.int32, torch.int64):
            assert torch.equal(r.encode_labels(labels.to(dt)), out), dt
        with pytest.raises(ValueError, match=r'\[0, 182\)'):
            r.encode_labels(labels.to(torch.int64) + 100)


def test_pipeline_matches_reference_loop(golden_dir):
    from stable_diffusion_amd import DDIMSamplerHIP
    z = np.load(os.path.join(golden_dir, 'semantic_pipeline_16x16.npz'))
    steps, b, h, w = int(z['steps']), int(z['batch']), int(z['h']), int(z['w'])
    assert float(z['perturb']) == MIXED_TOL and int(z['weight_seed']) == 0 and float(z['eta']) == 0.0
    m = _pipeline('mixed')
    x_T = torch.randn(b, 3, h // 4, w // 4, generator=torch.Generator().manual_seed(int(z['input_seed'])))
    labels = torch.randint(0, 182, (b, h, w), generator=torch.Generator().manual_seed(int(z['label_seed'])))     # (the tool's pipeline_inputs)
    c = m.cond_stage_model.encode_labels(labels.cuda())
    assert torch.equal(c, m.get_learned_conditioning(F.one_hot(labels, 182).permute(0, 3, 1, 2).float().contiguous().cuda()))
    e_c = float((c.cpu() - torch.from_numpy(z['c'])).abs().max())
    with contextlib.redirect_stdout(io.StringIO()):
        samples, _ = DDIMSamplerHIP(m).sample(steps, batch_size=b, shape=(3, h // 4, w // 4), conditioning=c, eta=0.0, verbose=False,
                                              x_T=x_T.cuda())
    e = m.first_stage_model.state_dict()['quantize.embedding.weight']
    zq = e[torch.from_numpy(z['idx']).long().to(e.device)].permute(0, 3, 1, 2).contiguous()      # the golden's own quantized latent
    x_dec = m.decode_first_stage(zq, force_not_quantize=True)     # (at the golden's codes: a code flip near a cell boundary is not the UNet's)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(samples).all()) and bool(torch.isfinite(x_dec).all())
    e_s = float((samples.cpu() - torch.from_numpy(z['samples'])).abs().max())
    e_x = float((x_dec.cpu() - torch.from_numpy(z['x_dec'])).abs().max())
    bar_s = float(z['bar_samples'])
    print(f'[semantic pipeline] c max-abs {e_c:.3e}; samples max-abs {e_s:.3e} (bar {bar_s:.3e}); decode of the golden latent max-abs {e_x:.3e} '
          f'(pin {VQ_DEC_PIN:.1e})', flush=True)
    assert tuple(x_dec.shape) == (b, 3, h, w)
    assert e_s <= bar_s and e_x <= VQ_DEC_PIN, (e_s, bar_s, e_x)


def test_synthesize_from_labels_equals_from_one_hot():
    m = _pipeline('mixed')
    labels = torch.randint(0, 182, (1, 64, 128), generator=torch.Generator().manual_seed(11))
    x_T = torch.randn(1, 3, 16, 32, generator=torch.Generator().manual_seed(12)).cuda()
    with contextlib.redirect_stdout(io.StringIO()):
        a = m.synthesize(labels=labels.cuda(), steps=1, eta=0.0, x_T=x_T)
        b = m.synthesize(segmentation=F.one_hot(labels, 182).permute(0, 3, 1, 2).float().contiguous().cuda(), steps=1, eta=0.0, x_T=x_T)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (1, 3, 64, 128) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    with pytest.raises(ValueError, match='multiples of 16'):
        m.synthesize(labels=labels[:, :40].cuda(), steps=1)
