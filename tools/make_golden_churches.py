"""Generate the unconditional LSUN-Churches model's fixtures under tests/golden/ from the reference code (build container only).

    PYTHONPATH=. python tools/make_golden_churches.py

UNet: the reference `UNetModel` (ldm/modules/diffusionmodules/openaimodel.py) at models/ldm/lsun_churches256/config.yaml's
unet_config (use_scale_shift_norm, resblock_updown, five levels, AttentionBlocks down to the full latent resolution), weights from
`stable_diffusion_amd.synthetic.synthetic_named_state_dict` over its own key list (seeded per key, so the GPU tests regenerate
the same tensors from the HIP module's key list), fp32 on the CPU.
Pipeline: the body of scripts/sample_diffusion.py's make_convolutional_sample -- the reference DDIMSampler at eta 1.0 with no
conditioning, then the reference `Decoder` behind post_quant_conv (AutoencoderKL.decode) on samples / scale_factor.  The per-step
noise is handed out from a seeded sequence, which the GPU test regenerates.  The loop runs a second time with every eps moved by
1e-3 * sign(randn) on every element at every step -- a UNet sitting exactly on the mixed-precision bar everywhere; the max-abs
divergence of `samples` and of `x_dec` from the first run is stored as the bars of the pipeline test.
Also written: the names / shapes of the UNet's state_dict and the parsed yaml.  The fixtures hold outputs and seeds, never weights.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import REF  # noqa: E402  (the reference checkout: $SD_REFERENCE)
OUT = os.path.join(ROOT, 'tests', 'golden')
YAML = os.path.join('models', 'ldm', 'lsun_churches256', 'config.yaml')
YAML_TRAIN = os.path.join('configs', 'latent-diffusion', 'lsun_churches-ldm-kl-8.yaml')

# name, batch, h, w, timesteps
UNET_CASES = [('16x16_b2', 2, 16, 16, (981, 1)), ('32x32_b1', 1, 32, 32, (500,)), ('32x32_b2', 2, 32, 32, (1, 981)),
              ('48x48_b1', 1, 48, 48, (981,)), ('16x16_b10', 10, 16, 16, (981, 881, 781, 681, 581, 481, 381, 281, 181, 1))]
N_KEYS, N_PARAMS = 520, 294966916
PIPE = dict(steps=10, batch=2, h=16, w=16, eta=1.0, scale_factor=0.37, input_seed=3, noise_seed=4, perturb_seed=5, perturb=1e-3)


def unet_inputs(batch, h, w, timesteps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 4, h, w, generator=g), torch.tensor(timesteps, dtype=torch.int64)


def pipeline_noise(seed, steps, shape):
    """x_T and the noise of every DDIM step (ddim.py:200 draws on every step), in the order the sampler asks for them"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), [torch.randn(shape, generator=g) for _ in range(steps)]


def vae_specs(ddconfig, embed_dim):
    """names / shapes of the decode half of AutoencoderKL (decoder.*, post_quant_conv.*) from the reference modules"""
    from ldm.modules.diffusionmodules.model import Decoder
    dec = Decoder(**ddconfig).eval()
    pqc = torch.nn.Conv2d(embed_dim, ddconfig['z_channels'], 1)
    return dec, pqc, ([('decoder.' + k, tuple(v.shape)) for k, v in dec.state_dict().items()] +
                      [('post_quant_conv.' + k, tuple(v.shape)) for k, v in pqc.state_dict().items()])


def main():
    import yaml
    from oracle.make_golden import _import_reference
    from stable_diffusion_amd.synthetic import CHURCHES_SCHEDULE, CHURCHES_UNET_KWARGS, CHURCHES_VAE_DDCONFIG, synthetic_named_state_dict
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with open(os.path.join(REF, YAML)) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(REF, YAML_TRAIN)) as f:
        assert yaml.safe_load(f)['model']['params']['unet_config'] == cfg['model']['params']['unet_config']
    with open(os.path.join(OUT, 'lsun_churches256_config.json'), 'w') as f:
        json.dump(cfg, f, indent=1)
    p = cfg['model']['params']
    assert dict(p['unet_config']['params']) == CHURCHES_UNET_KWARGS
    assert dict(p['first_stage_config']['params']['ddconfig']) == CHURCHES_VAE_DDCONFIG
    assert (p['timesteps'], p['linear_start'], p['linear_end']) == tuple(CHURCHES_SCHEDULE[k] for k in ('timesteps', 'linear_start', 'linear_end'))
    assert p['cond_stage_config'] == '__is_unconditional__' and CHURCHES_SCHEDULE['conditioning_key'] is None
    UNetModel = _import_reference()[0]

    # ---- UNet ----
    m = UNetModel(**p['unet_config']['params']).eval()
    specs = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert len(specs) == N_KEYS and sum(int(np.prod(s)) for _, s in specs) == N_PARAMS, (len(specs), sum(int(np.prod(s)) for _, s in specs))
    with open(os.path.join(OUT, 'churches_unet_state_dict_keys.json'), 'w') as f:
        json.dump({'module': 'UNetModel(**lsun_churches256 unet_config.params)', 'keys': [[k, list(s)] for k, s in specs]}, f, indent=0)
    m.load_state_dict(synthetic_named_state_dict(specs, 0), strict=True)
    for name, b, h, w, ts in UNET_CASES:
        x, t = unet_inputs(b, h, w, ts)
        with torch.no_grad():
            eps = m(x, t)
        print(f'[unet {name}] |eps| max {eps.abs().max():.3f} rms {eps.pow(2).mean().sqrt():.3f}', flush=True)
        assert bool(torch.isfinite(eps).all())
        np.savez_compressed(os.path.join(OUT, f'churches_unet_{name}.npz'), eps=eps.numpy().astype(np.float32), weight_seed=0,
                            input_seed=1, batch=b, h=h, w=w, t=t.numpy())

    # ---- pipeline: scripts/sample_diffusion.py:69-75,95-103 on reference modules (the reference DDIMSampler, CPU) ----
    import ldm.models.diffusion.ddim as ref_ddim
    from ldm.modules.diffusionmodules.util import make_beta_schedule

    class CpuDDIM(ref_ddim.DDIMSampler):
        def register_buffer(self, name, attr):            # (the reference moves its tables to cuda)
            setattr(self, name, attr)

    fs = p['first_stage_config']['params']
    dec, pqc, vspecs = vae_specs(fs['ddconfig'], fs['embed_dim'])
    vsd = synthetic_named_state_dict(vspecs, 0)
    dec.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith('decoder.')}, strict=True)
    pqc.load_state_dict({k[16:]: v for k, v in vsd.items() if k.startswith('post_quant_conv.')}, strict=True)

    class Model:                                           # what DDIMSampler reads on LatentDiffusion (ddpm.py:117-169,986-992,1408-1409)
        def __init__(self, perturb_seed=None):
            betas = make_beta_schedule('linear', p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'])
            ac = np.cumprod(1. - betas, axis=0)
            self.num_timesteps, self.device = int(p['timesteps']), torch.device('cpu')
            self.betas = torch.tensor(betas, dtype=torch.float32)
            self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
            self.alphas_cumprod_prev = torch.tensor(np.append(1., ac[:-1]), dtype=torch.float32)
            self.g = None if perturb_seed is None else torch.Generator().manual_seed(perturb_seed)

        def apply_model(self, x, t, c):
            assert c is None
            eps = m(x, t)
            if self.g is not None:
                eps = eps + PIPE['perturb'] * torch.sign(torch.randn(eps.shape, generator=self.g))
            return eps

    shape = (PIPE['batch'], 4, PIPE['h'], PIPE['w'])

    def run(perturb_seed):
        x_T, noises = pipeline_noise(PIPE['noise_seed'], PIPE['steps'], shape)
        seq = list(noises)
        ref_ddim.noise_like = lambda shp, device, repeat=False: seq.pop(0)
        with torch.no_grad():
            samples, _ = CpuDDIM(Model(perturb_seed)).sample(PIPE['steps'], batch_size=shape[0], shape=shape[1:], eta=PIPE['eta'],
                                                             verbose=False, x_T=x_T)
            x_dec = dec(pqc(samples / PIPE['scale_factor']))          # decode_first_stage: z = 1 / scale_factor * z (ddpm.py:713)
        assert not seq
        return samples, x_dec
    keep = ref_ddim.noise_like
    try:
        samples, x_dec = run(None)
        samples_p, x_dec_p = run(PIPE['perturb_seed'])
    finally:
        ref_ddim.noise_like = keep
    bar_s, bar_x = float((samples_p - samples).abs().max()), float((x_dec_p - x_dec).abs().max())
    print(f'[pipeline] |samples| max {samples.abs().max():.3f}; |x_dec| max {x_dec.abs().max():.3f}; bars from eps + {PIPE["perturb"]:g} sign: '
          f'samples {bar_s:.3e}, x_dec {bar_x:.3e}', flush=True)
    np.savez_compressed(os.path.join(OUT, 'churches_pipeline_16.npz'), samples=samples.numpy().astype(np.float32),
                        x_dec=x_dec.numpy().astype(np.float32), bar_samples=bar_s, bar_x_dec=bar_x, weight_seed=0,
                        **{k: v for k, v in PIPE.items()})
    print('LSUN-Churches fixtures written to', OUT)


if __name__ == '__main__':
    main()
