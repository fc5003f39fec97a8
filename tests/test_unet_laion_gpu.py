"""UNetModelHIP at the LAION-400M model's context width (txt2img-1p4B-eval.yaml: context_dim 1280, everything else as SD v1)
against goldens of the reference UNetModel (tools/make_golden_laion.py); weights and inputs regenerated from the goldens'
seeds (oracle.weights), as tests/test_unet_gpu.py does.

Mixed mode: the SD-v1 benign-family bar, 1e-3 max-abs.  Full mode: per-case (max-abs, rms) pins, ~1.25 x what an MI355X
measured, in the form of tests/test_unet_full_precision_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.plan import UNetConfig  # noqa: E402
from oracle.weights import make_inputs, make_state_dict  # noqa: E402

LAION = UNetConfig(context_dim=1280)
TOL = 1e-3
FULL_PINS = {            # (max-abs, rms), ~1.25 x measured in full mode (LAION-400M UNet)
    'laion_16x16': (8.2e-06, 1.77e-06),      # measured 6.56e-6, 1.42e-6
    'laion_64x64': (9.5e-06, 1.89e-06),      # measured 7.63e-6, 1.51e-6
}
_models = {}


def _model(prec):
    if prec not in _models:
        torch.cuda.empty_cache()
        from stable_diffusion_amd import UNetModelHIP
        m = UNetModelHIP(**LAION.ref_kwargs(), hip_precision=prec)
        m.load_state_dict(make_state_dict(LAION, 0), strict=True)
        _models[prec] = m.cuda()
    return _models[prec]


def _case(golden_dir, case):
    z = np.load(os.path.join(golden_dir, f'unet_{case}.npz'))
    assert int(z['context_dim']) == 1280 and int(z['weight_seed']) == 0
    x, t, ctx = make_inputs(LAION, int(z['batch']), int(z['h']), int(z['w']), seed=int(z['input_seed']), ctx_len=int(z['ctx_len']))
    assert torch.equal(t, torch.from_numpy(z['t']))
    return x, t, ctx, torch.from_numpy(z['eps'])


@pytest.mark.parametrize('case', list(FULL_PINS))
def test_unet_ctx1280_mixed_matches_reference(case, golden_dir):
    x, t, ctx, ref = _case(golden_dir, case)
    eps = _model('mixed')(x.cuda(), t.cuda(), context=ctx.cuda())
    torch.cuda.synchronize()
    err = (eps.float().cpu() - ref).abs()
    print(f'[unet {case} mixed] max-abs {err.max():.3e} rms {err.pow(2).mean().sqrt():.3e} |eps|max {ref.abs().max():.3f}', flush=True)
    assert eps.shape == ref.shape and bool(torch.isfinite(eps).all())
    assert float(err.max()) <= TOL


@pytest.mark.parametrize('case', list(FULL_PINS))
def test_unet_ctx1280_full_matches_reference(case, golden_dir):
    x, t, ctx, ref = _case(golden_dir, case)
    eps = _model('full')(x.cuda(), t.cuda(), context=ctx.cuda())
    torch.cuda.synchronize()
    err = (eps.float().cpu() - ref).abs()
    mx, rms = float(err.max()), float(err.pow(2).mean().sqrt())
    pin_max, pin_rms = FULL_PINS[case]
    print(f'[unet {case} full] max-abs {mx:.3e} rms {rms:.3e} (pins {pin_max:.2e}, {pin_rms:.2e})', flush=True)
    assert mx <= pin_max and rms <= pin_rms


def test_unet_ctx1280_context_cache_and_timestep_table_bit_identical():
    """At ctx 1280: a second call on the cached cross-attention K/V, and a call whose timestep rows come from the table, give
    the same bits as a plain call; a changed context changes eps."""
    m = _model('mixed')
    x, t, ctx = make_inputs(LAION, 2, 16, 16, seed=12)
    x, ctx = x.cuda(), ctx.cuda()
    tt = torch.full((2,), 481, dtype=torch.long, device='cuda')
    plain = m(x, tt, context=ctx).clone()
    assert torch.equal(plain, m(x, tt, context=ctx))                 # cached K/V
    assert not torch.equal(plain, m(x, tt, context=ctx * 1.5))
    assert torch.equal(plain, m(x, tt, context=ctx.clone()))          # recomputed K/V
    m.cache_timesteps([981, 481, 1])
    try:
        for tv in (481, 1, 7):                                           # 7 is not in the table
            t2 = torch.full((2,), tv, dtype=torch.long, device='cuda')
            want = m(x, t2, context=ctx).clone()
            m.hint_timestep(tv)
            got = m(x, t2, context=ctx).clone()
            assert torch.equal(want, got), (tv, float((want - got).abs().max()))
    finally:
        m.cache_timesteps([])
