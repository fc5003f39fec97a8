"""Generate the fixtures of the face / bedroom LDMs and of bsr_sr's UNet under tests/golden/ from the reference code (build container only).

    PYTHONPATH=. python tools/make_golden_faces.py

UNets: the reference `UNetModel` (ldm/modules/diffusionmodules/openaimodel.py) at the unet_config that models/ldm/celeba256, ffhq256 and
lsun_beds256 share (model_channels 224, num_head_channels 32: AttentionBlocks of 14 / 21 / 28 heads, plain Downsample / Upsample
convolutions) and at models/ldm/bsr_sr's (160, six input channels, 20 heads), weights from
`stable_diffusion_amd.synthetic.synthetic_named_state_dict` over the module's own key list (seeded per key, so the GPU tests regenerate
the same tensors from the HIP module's key list), fp32 on the CPU.
Pipeline (faces): the body of scripts/sample_diffusion.py's make_convolutional_sample -- the reference DDIMSampler at eta 1.0 with no
conditioning, then VQModelInterface.decode (quantize -> post_quant_conv -> Decoder; the quantizer restated in tests/vq_ref.py) on the
samples.  The per-step noise is handed out from a seeded sequence, which the GPU test regenerates.  The loop runs a second time with every
eps moved by 1e-3 * sign(randn) on every element at every step -- a UNet sitting exactly on the mixed-precision bar everywhere; the
max-abs divergence of `samples` from the first run is stored as the bar of the pipeline test.  The decode is compared on the golden's OWN
latent (the stored code indices included), so a code flip next to a cell boundary is not charged to the UNet.
Also written: the names / shapes of both UNets' state_dicts and the four parsed yamls.  The fixtures hold outputs and seeds, never weights.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.make_golden import REF  # noqa: E402  (the reference checkout: $SD_REFERENCE)
OUT = os.path.join(ROOT, 'tests', 'golden')
FACE_MODELS = ('celeba256', 'ffhq256', 'lsun_beds256')

# name, batch, h, w, timesteps
FACES_CASES = [('8x8_b2', 2, 8, 8, (981, 1)), ('16x16_b2', 2, 16, 16, (1, 981)), ('32x32_b1', 1, 32, 32, (500,)),
               ('64x64_b1', 1, 64, 64, (981,)), ('16x16_b10', 10, 16, 16, (981, 881, 781, 681, 581, 481, 381, 281, 181, 1))]
BSR_CASES = [('16x16_b2', 2, 16, 16, (981, 1)), ('32x32_b1', 1, 32, 32, (500,))]
FACES_KEYS, FACES_PARAMS = 368, 274056163
BSR_KEYS, BSR_PARAMS = 306, 113622563
PIPE = dict(steps=10, batch=2, h=16, w=16, eta=1.0, input_seed=3, noise_seed=4, perturb_seed=5, perturb=1e-3)


def unet_inputs(batch, channels, h, w, timesteps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, channels, h, w, generator=g), torch.tensor(timesteps, dtype=torch.int64)


def pipeline_noise(seed, steps, shape):
    """x_T and the noise of every DDIM step (ddim.py:200 draws on every step), in the order the sampler asks for them"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), [torch.randn(shape, generator=g) for _ in range(steps)]


def vq_decode_specs(fp):
    """names / shapes of the decode half of VQModelInterface (decoder.*, quantize.embedding, post_quant_conv.*) from the reference modules"""
    from ldm.modules.diffusionmodules.model import Decoder
    dec = Decoder(**fp['ddconfig']).eval()
    pqc = torch.nn.Conv2d(fp['embed_dim'], fp['ddconfig']['z_channels'], 1)
    return dec, pqc, ([('decoder.' + k, tuple(v.shape)) for k, v in dec.state_dict().items()] +
                      [('quantize.embedding.weight', (fp['n_embed'], fp['embed_dim']))] +
                      [('post_quant_conv.' + k, tuple(v.shape)) for k, v in pqc.state_dict().items()])


def main():
    import yaml
    import vq_ref
    from oracle.make_golden import _import_reference
    from stable_diffusion_amd.synthetic import (BSR_SCHEDULE, BSR_UNET_KWARGS, FACES_SCHEDULE, FACES_UNET_KWARGS, FACES_VQ_KWARGS,
                                                synthetic_named_state_dict)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfgs = {}
    for name in FACE_MODELS + ('bsr_sr',):
        with open(os.path.join(REF, 'models', 'ldm', name, 'config.yaml')) as f:
            cfgs[name] = yaml.safe_load(f)
        with open(os.path.join(OUT, f'{name}_config.json'), 'w') as f:
            json.dump(cfgs[name], f)
    p = cfgs['celeba256']['model']['params']
    for name in FACE_MODELS:
        q = cfgs[name]['model']['params']
        assert q['unet_config'] == p['unet_config'], name
        assert dict(q['unet_config']['params']) == FACES_UNET_KWARGS, name
        fq = q['first_stage_config']['params']
        assert dict(embed_dim=fq['embed_dim'], n_embed=fq['n_embed'], ddconfig=dict(fq['ddconfig'])) == FACES_VQ_KWARGS, name
        assert (q['timesteps'], q['linear_start'], q['linear_end']) == tuple(FACES_SCHEDULE[k] for k in ('timesteps', 'linear_start', 'linear_end'))
        assert q['cond_stage_config'] == '__is_unconditional__' and FACES_SCHEDULE['conditioning_key'] is None
    pb = cfgs['bsr_sr']['model']['params']
    assert dict(pb['unet_config']['params']) == BSR_UNET_KWARGS
    assert (pb['timesteps'], pb['linear_start'], pb['linear_end']) == tuple(BSR_SCHEDULE[k] for k in ('timesteps', 'linear_start', 'linear_end'))
    assert pb['concat_mode'] is True and BSR_SCHEDULE['conditioning_key'] == 'concat'
    UNetModel = _import_reference()[0]

    # ---- UNets ----
    def unet_fixtures(tag, params, cases, n_keys, n_params, label):
        m = UNetModel(**params).eval()
        specs = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        assert len(specs) == n_keys and sum(int(np.prod(s)) for _, s in specs) == n_params, (len(specs), sum(int(np.prod(s)) for _, s in specs))
        with open(os.path.join(OUT, f'{tag}_unet_state_dict_keys.json'), 'w') as f:
            json.dump({'module': label, 'keys': [[k, list(s)] for k, s in specs]}, f)
        m.load_state_dict(synthetic_named_state_dict(specs, 0), strict=True)
        for name, b, h, w, ts in cases:
            x, t = unet_inputs(b, params['in_channels'], h, w, ts)
            with torch.no_grad():
                eps = m(x, t)
            print(f'[{tag} unet {name}] |eps| max {eps.abs().max():.3f} rms {eps.pow(2).mean().sqrt():.3f}', flush=True)
            assert bool(torch.isfinite(eps).all())
            np.savez_compressed(os.path.join(OUT, f'{tag}_unet_{name}.npz'), eps=eps.numpy().astype(np.float32), weight_seed=0,
                                input_seed=1, batch=b, h=h, w=w, t=t.numpy())
        return m

    m = unet_fixtures('faces', p['unet_config']['params'], FACES_CASES, FACES_KEYS, FACES_PARAMS,
                      'UNetModel(**celeba256 / ffhq256 / lsun_beds256 unet_config.params)')
    unet_fixtures('bsr', pb['unet_config']['params'], BSR_CASES, BSR_KEYS, BSR_PARAMS, 'UNetModel(**bsr_sr unet_config.params)')

    # ---- pipeline: scripts/sample_diffusion.py:69-75,95-103 on reference modules (the reference DDIMSampler, CPU) ----
    import ldm.models.diffusion.ddim as ref_ddim
    from ldm.modules.diffusionmodules.util import make_beta_schedule

    class CpuDDIM(ref_ddim.DDIMSampler):
        def register_buffer(self, name, attr):            # (the reference moves its tables to cuda)
            setattr(self, name, attr)

    fs = p['first_stage_config']['params']
    dec, pqc, vspecs = vq_decode_specs(fs)
    vsd = synthetic_named_state_dict(vspecs, 0)
    dec.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith('decoder.')}, strict=True)
    pqc.load_state_dict({k[16:]: v for k, v in vsd.items() if k.startswith('post_quant_conv.')}, strict=True)
    e = vsd['quantize.embedding.weight']

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

    shape = (PIPE['batch'], 3, PIPE['h'], PIPE['w'])

    def run(perturb_seed):
        x_T, noises = pipeline_noise(PIPE['noise_seed'], PIPE['steps'], shape)
        seq = list(noises)
        ref_ddim.noise_like = lambda shp, device, repeat=False: seq.pop(0)
        with torch.no_grad():
            samples, _ = CpuDDIM(Model(perturb_seed)).sample(PIPE['steps'], batch_size=shape[0], shape=shape[1:], eta=PIPE['eta'],
                                                             verbose=False, x_T=x_T)
        assert not seq
        return samples
    keep = ref_ddim.noise_like
    try:
        samples = run(None)
        samples_p = run(PIPE['perturb_seed'])
    finally:
        ref_ddim.noise_like = keep
    with torch.no_grad():
        zq, idx = vq_ref.quantize(samples, e)               # decode_first_stage: scale_factor 1.0 (no scale_factor in these yamls)
        x_dec = dec(pqc(zq))
    bar_s = float((samples_p - samples).abs().max())
    print(f'[pipeline] |samples| max {samples.abs().max():.3f}; |x_dec| max {x_dec.abs().max():.3f}; bar from eps + {PIPE["perturb"]:g} sign: '
          f'samples {bar_s:.3e}', flush=True)
    np.savez_compressed(os.path.join(OUT, 'faces_pipeline_16.npz'), samples=samples.numpy().astype(np.float32),
                        x_dec=x_dec.numpy().astype(np.float32), idx=idx.numpy().astype(np.int32), bar_samples=bar_s, weight_seed=0,
                        **{k: v for k, v in PIPE.items()})
    print('face / bedroom / bsr_sr fixtures written to', OUT)


if __name__ == '__main__':
    main()
