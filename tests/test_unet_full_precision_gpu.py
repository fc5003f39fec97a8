"""The full-precision UNet mode (UNetModelHIP(..., hip_precision='full'): every MFMA operand split-fp16) against the committed
reference goldens, and its isolation from the default mode.

Weights and inputs are regenerated from the goldens' seeds (oracle.weights), as tests/test_unet_gpu.py does.  Hard bar: max-abs
<= 2e-4 on every case, the outlier family included (north_star is 1e-3; emulating split-fp16 on every operand class of
oracle/fp16_floor.py gives 5e-6 .. 1.1e-5)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.plan import SD_V1, SMALL40, TINY  # noqa: E402
from oracle.weights import make_inputs, make_state_dict  # noqa: E402

HARD_MAX = 2e-4
CFGS = {'tiny': TINY, 'small40': SMALL40, 'sdv1': SD_V1}
# the 23 cases of tests/test_unet_gpu.py
CASES = ['tiny_16x16', 'tiny_8x24', 'tiny_b1_8x8', 'tiny_b10_8x8', 'tiny_real_16x16', 'small40_16x16',
         'sdv1_8x8', 'sdv1_16x16', 'sdv1_32x32', 'sdv1_64x64', 'sdv1_96x96', 'sdv1_t1_741_16x16', 'sdv1_b6_16x16',
         'sdv1_w1_16x16', 'sdv1_w1_32x32', 'sdv1_w1_64x64', 'sdv1_w2_16x16', 'sdv1_w2_32x32', 'sdv1_w2_64x64',
         'sdv1_real_16x16', 'sdv1_real_32x32', 'sdv1_real_64x64', 'sdv1_real1_16x16']
# per case (max-abs, rms) bars: ~1.25x what the full mode measured on an MI355X (profiles/full_precision_r07.txt), never above HARD_MAX
PINS = {
    'tiny_16x16': (4.06e-06, 9.73e-07),
    'tiny_8x24': (3.80e-06, 9.21e-07),
    'tiny_b1_8x8': (2.91e-06, 9.17e-07),
    'tiny_b10_8x8': (3.72e-06, 8.84e-07),
    'tiny_real_16x16': (7.60e-06, 1.59e-06),
    'small40_16x16': (8.79e-06, 1.87e-06),
    'sdv1_8x8': (5.72e-06, 1.66e-06),
    'sdv1_16x16': (7.15e-06, 1.80e-06),
    'sdv1_32x32': (8.06e-06, 1.80e-06),
    'sdv1_64x64': (9.05e-06, 1.82e-06),
    'sdv1_96x96': (9.01e-06, 1.82e-06),
    'sdv1_t1_741_16x16': (7.82e-06, 1.73e-06),
    'sdv1_b6_16x16': (8.72e-06, 1.79e-06),
    'sdv1_w1_16x16': (7.79e-06, 1.82e-06),
    'sdv1_w1_32x32': (7.82e-06, 1.84e-06),
    'sdv1_w1_64x64': (8.51e-06, 1.91e-06),
    'sdv1_w2_16x16': (7.82e-06, 1.78e-06),
    'sdv1_w2_32x32': (7.84e-06, 1.83e-06),
    'sdv1_w2_64x64': (8.72e-06, 1.88e-06),
    'sdv1_real_16x16': (6.86e-06, 1.90e-06),
    'sdv1_real_32x32': (8.01e-06, 2.10e-06),
    'sdv1_real_64x64': (1.28e-05, 2.55e-06),
    'sdv1_real1_16x16': (7.26e-06, 1.37e-06),
}
_models = {}


def _style(z):
    return str(z['style']) if 'style' in z.files else 'uniform'


def _models_for(cfg_name, wseed, style):
    """(mixed, full) UNetModelHIP pair on one state dict"""
    key = (cfg_name, wseed, style)
    if key not in _models:
        _models.clear()
        torch.cuda.empty_cache()
        from stable_diffusion_amd import UNetModelHIP
        cfg = CFGS[cfg_name]
        sd = make_state_dict(cfg, wseed, style=style)
        pair = []
        for prec in ('mixed', 'full'):
            m = UNetModelHIP(**cfg.ref_kwargs(), hip_precision=prec)
            m.load_state_dict(sd, strict=True)
            pair.append(m.cuda().eval())
        _models[key] = tuple(pair)
    return _models[key]


def _inputs(cfg, z):
    return make_inputs(cfg, int(z['batch']), int(z['h']), int(z['w']), seed=int(z['input_seed']), ctx_len=int(z['ctx_len']),
                       timesteps=tuple(int(v) for v in z['t']), style=_style(z))


@pytest.mark.parametrize('case', CASES)
def test_full_precision_eps_matches_reference_golden(case, golden_dir):
    z = np.load(os.path.join(golden_dir, f'unet_{case}.npz'))
    cfg_name = case.split('_')[0]
    cfg = CFGS[cfg_name]
    mixed, full = _models_for(cfg_name, int(z['weight_seed']), _style(z))
    assert full.hip_precision == 'full' and mixed.hip_precision == 'mixed'
    x, t, ctx = _inputs(cfg, z)
    ref = torch.from_numpy(z['eps'])
    eps = full(x.cuda(), t.cuda(), context=ctx.cuda()).float().cpu()
    eps_mixed = mixed(x.cuda(), t.cuda(), context=ctx.cuda()).float().cpu()
    err, err_m = (eps - ref).abs(), (eps_mixed - ref).abs()
    mx, rms = float(err.max()), float(err.pow(2).mean().sqrt())
    print(f'[unet full {case}] max-abs {mx:.3e} rms {rms:.3e} | mixed max-abs {float(err_m.max()):.3e} rms '
          f'{float(err_m.pow(2).mean().sqrt()):.3e} | ratio {float(err_m.max()) / max(mx, 1e-30):.0f}x', flush=True)
    assert eps.shape == ref.shape and bool(torch.isfinite(eps).all())
    assert mx <= HARD_MAX
    if case in PINS:
        bar_max, bar_rms = PINS[case]
        assert mx <= min(bar_max, HARD_MAX) and rms <= bar_rms


def test_mixed_mode_unchanged_by_a_full_handle():
    """A mixed handle gives the same bits before and after a full handle was created and ran in the same process (tuning table,
    static environment caches, launch tapes)."""
    from stable_diffusion_amd import UNetModelHIP
    sd = make_state_dict(TINY, 0)
    x, t, ctx = make_inputs(TINY, 2, 16, 16, seed=3)
    x, t, ctx = x.cuda(), t.cuda(), ctx.cuda()
    mixed = UNetModelHIP(**TINY.ref_kwargs())
    mixed.load_state_dict(sd, strict=True)
    mixed = mixed.cuda().eval()
    before = [mixed(x, t, context=ctx).clone() for _ in range(2)]       # (the second call replays a launch tape)
    full = UNetModelHIP(**TINY.ref_kwargs(), hip_precision='full')
    full.load_state_dict(sd, strict=True)
    full = full.cuda().eval()
    eps_full = full(x, t, context=ctx)
    eps_full2 = full(x, t, context=ctx)
    after = [mixed(x, t, context=ctx).clone() for _ in range(2)]
    fresh = UNetModelHIP(**TINY.ref_kwargs())
    fresh.load_state_dict(sd, strict=True)
    fresh = fresh.cuda().eval()
    eps_fresh = fresh(x, t, context=ctx)
    torch.cuda.synchronize()
    assert torch.equal(before[0], before[1]) and torch.equal(after[0], before[0]) and torch.equal(after[1], before[0])
    assert torch.equal(eps_fresh, before[0])
    assert torch.equal(eps_full, eps_full2) and not torch.equal(eps_full, before[0])


def test_packed_blob_is_tied_to_the_precision(tmp_path):
    """save_packed / load_packed round-trip within a mode (same eps); a blob of the other mode is refused with a message naming it"""
    from stable_diffusion_amd import UNetModelHIP
    from stable_diffusion_amd._lib import SdmiError
    sd = make_state_dict(TINY, 0)
    x, t, ctx = make_inputs(TINY, 2, 8, 8, seed=4)
    x, t, ctx = x.cuda(), t.cuda(), ctx.cuda()
    blobs, eps = {}, {}
    for prec in ('mixed', 'full'):
        m = UNetModelHIP(**TINY.ref_kwargs(), hip_precision=prec)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        eps[prec] = m(x, t, context=ctx).clone()
        blobs[prec] = str(tmp_path / f'{prec}.sdmipk')
        m.save_packed(blobs[prec])
    for prec, other in (('mixed', 'full'), ('full', 'mixed')):
        m = UNetModelHIP(**TINY.ref_kwargs(), hip_precision=prec).cuda().eval()
        m.load_packed(blobs[prec])
        assert torch.equal(m(x, t, context=ctx), eps[prec])
        m2 = UNetModelHIP(**TINY.ref_kwargs(), hip_precision=prec).cuda().eval()
        with pytest.raises(SdmiError, match=f'{other}-precision UNet handle'):
            m2.load_packed(blobs[other])
