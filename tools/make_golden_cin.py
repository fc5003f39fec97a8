"""Generate the class-conditional ImageNet model's fixtures under tests/golden/ from the reference code (build container only).

    PYTHONPATH=. python tools/make_golden_cin.py

UNet: the reference `UNetModel` (ldm/modules/diffusionmodules/openaimodel.py) at configs/latent-diffusion/cin256-v2.yaml's
unet_config, weights from `stable_diffusion_amd.synthetic.synthetic_named_state_dict` over its own key list (seeded per key, so
the GPU tests regenerate the same tensors from the HIP module's key list), fp32 on the CPU.  The context is the reference
`ClassEmbedder`'s output for the case's class ids ([B, 1, 512]; class 1000 = the unconditional label), one case takes a random
context of four tokens instead.
First stage: the reference `Encoder` / `Decoder` (ldm/modules/diffusionmodules/model.py) at the yaml's ddconfig (mid-block
attention on), quant_conv / post_quant_conv as in VQModel.__init__, the quantizer restated in tests/vq_ref.py.
Pipeline: the cell of scripts/latent_imagenet_diffusion.ipynb (classifier-free guidance against class 1000, DDIM, eta 0) on the
reference modules with the reference DDIMSampler.
Also written: the names / shapes of the UNet's state_dict, the parsed yaml and the schedule `register_schedule` derives from it.
The fixtures hold outputs, seeds and class ids, never weights.
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.make_golden import REF  # noqa: E402  (the reference checkout: $SD_REFERENCE)
OUT = os.path.join(ROOT, 'tests', 'golden')
YAML = os.path.join('configs', 'latent-diffusion', 'cin256-v2.yaml')

# name, h, w, timesteps, class ids (one per row)
UNET_CASES = [('64x64_b1', 64, 64, (981,), (25,)), ('64x64_b2', 64, 64, (1, 981), (25, 992)), ('32x32_b2', 32, 32, (981, 1), (7, 1000)),
              ('96x96_b1', 96, 96, (981,), (992,)), ('16x16_b2', 16, 16, (500, 981), (0, 999)),
              ('64x64_b6', 64, 64, (981,) * 6, (1000, 25, 1000, 992, 25, 1000))]
CTX4_CASE = ('32x32_b2_ctx4', 32, 32, (981, 1))           # a context of four tokens: the general cross-attention at d_head = C
IMG = 128            # first-stage case: 2 images of 128 x 128 -> 32 x 32 latents
PIPE = dict(classes=(25, 992), n_samples_per_class=2, steps=10, scale=3.0, eta=0.0, h=24, w=24, seed=2)     # 96 x 96 images


def unet_inputs(batch, h, w, timesteps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 3, h, w, generator=g), torch.tensor(timesteps, dtype=torch.int64)


def ctx4_inputs(batch, seed=3):
    return torch.randn(batch, 4, 512, generator=torch.Generator().manual_seed(seed))


def vq_inputs(seed=1):
    """images in [-1, 1] (smooth + noise) and latents"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(2, 3, IMG // 8, IMG // 8, generator=g) * 2 - 1
    img = torch.nn.functional.interpolate(low, scale_factor=8, mode='bilinear', align_corners=False)
    img = (img + 0.1 * torch.randn(img.shape, generator=g)).clamp(-1, 1)
    z = torch.randn(2, 3, IMG // 4, IMG // 4, generator=g)
    return img, z


def _reference():
    from oracle.make_golden import _import_reference
    UNetModel, _, DDIMSampler, _ = _import_reference()
    for missing in ('clip', 'kornia'):           # imported at the top of ldm.modules.encoders.modules, not used by ClassEmbedder
        sys.modules.setdefault(missing, types.ModuleType(missing))
    from ldm.modules.diffusionmodules.model import Decoder, Encoder
    from ldm.modules.encoders.modules import ClassEmbedder
    return UNetModel, Encoder, Decoder, ClassEmbedder, DDIMSampler


def main():
    import yaml
    from stable_diffusion_amd.synthetic import CIN_CLASS_KWARGS, CIN_SCHEDULE, CIN_UNET_KWARGS, CIN_VQ_KWARGS, synthetic_named_state_dict
    import vq_ref
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with open(os.path.join(REF, YAML)) as f:
        cfg = yaml.safe_load(f)
    p = cfg['model']['params']
    assert p['unet_config']['params'] == CIN_UNET_KWARGS
    assert p['cond_stage_config']['params'] == CIN_CLASS_KWARGS
    assert (p['timesteps'], p['linear_start'], p['linear_end']) == tuple(CIN_SCHEDULE[k] for k in ('timesteps', 'linear_start', 'linear_end'))
    UNetModel, Encoder, Decoder, ClassEmbedder, DDIMSampler = _reference()
    from ldm.modules.diffusionmodules.util import make_beta_schedule

    # ---- schedule (ddpm.py register_schedule) ----
    betas = make_beta_schedule('linear', p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'])
    ac = np.cumprod(1. - betas, axis=0)
    with open(os.path.join(OUT, 'cin256_v2_config.json'), 'w') as f:
        json.dump(cfg, f, indent=1)
    np.savez_compressed(os.path.join(OUT, 'cin_schedule.npz'), betas=betas.astype(np.float32), alphas_cumprod=ac.astype(np.float32),
                        alphas_cumprod_prev=np.append(1., ac[:-1]).astype(np.float32))

    # ---- conditioner + UNet ----
    emb = ClassEmbedder(**p['cond_stage_config']['params']).eval()
    emb.load_state_dict(synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in emb.state_dict().items()], 0), strict=True)
    m = UNetModel(**p['unet_config']['params']).eval()
    specs = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    with open(os.path.join(OUT, 'cin_unet_state_dict_keys.json'), 'w') as f:
        json.dump({'module': 'UNetModel(**cin256-v2 unet_config.params)', 'keys': [[k, list(s)] for k, s in specs]}, f, indent=0)
    print(f'[unet] {len(specs)} keys, {sum(int(np.prod(s)) for _, s in specs) / 1e6:.1f} M parameters', flush=True)
    m.load_state_dict(synthetic_named_state_dict(specs, 0), strict=True)
    for name, h, w, ts, classes in UNET_CASES:
        x, t = unet_inputs(len(ts), h, w, ts)
        with torch.no_grad():
            c = emb({'class_label': torch.tensor(classes)})
            eps = m(x, t, context=c)
        assert c.shape == (len(ts), 1, 512)
        print(f'[unet {name}] |eps| max {eps.abs().max():.3f} rms {eps.pow(2).mean().sqrt():.3f}', flush=True)
        np.savez_compressed(os.path.join(OUT, f'cin_unet_{name}.npz'), eps=eps.numpy().astype(np.float32), weight_seed=0, input_seed=1,
                            batch=len(ts), h=h, w=w, t=t.numpy(), classes=np.array(classes, dtype=np.int64))
    name, h, w, ts = CTX4_CASE
    x, t = unet_inputs(len(ts), h, w, ts)
    with torch.no_grad():
        eps = m(x, t, context=ctx4_inputs(len(ts)))
    print(f'[unet {name}] |eps| max {eps.abs().max():.3f} rms {eps.pow(2).mean().sqrt():.3f}', flush=True)
    np.savez_compressed(os.path.join(OUT, f'cin_unet_{name}.npz'), eps=eps.numpy().astype(np.float32), weight_seed=0, input_seed=1,
                        ctx_seed=3, batch=len(ts), h=h, w=w, t=t.numpy())

    # ---- VQ first stage (mid-block attention on) ----
    fp = p['first_stage_config']['params']
    dd = fp['ddconfig']
    assert {k: fp[k] for k in ('embed_dim', 'n_embed', 'ddconfig')} == CIN_VQ_KWARGS
    enc, dec = Encoder(**dd).eval(), Decoder(**dd).eval()
    ed, zc = fp['embed_dim'], dd['z_channels']
    quant_conv, post_quant_conv = torch.nn.Conv2d(zc, ed, 1), torch.nn.Conv2d(ed, zc, 1)
    keys = ([('encoder.' + k, tuple(v.shape)) for k, v in enc.state_dict().items()] +
            [('decoder.' + k, tuple(v.shape)) for k, v in dec.state_dict().items()] +
            [('quantize.embedding.weight', (fp['n_embed'], ed))] +
            [('quant_conv.' + k, tuple(v.shape)) for k, v in quant_conv.state_dict().items()] +
            [('post_quant_conv.' + k, tuple(v.shape)) for k, v in post_quant_conv.state_dict().items()])
    with open(os.path.join(OUT, 'cin_vq_state_dict_keys.json'), 'w') as f:
        json.dump({'module': 'VQModelInterface(**cin256-v2 first_stage_config.params) without loss.*',
                   'keys': [[k, list(s)] for k, s in keys]}, f, indent=0)
    vsd = synthetic_named_state_dict(keys, 0)
    enc.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith('encoder.')}, strict=True)
    dec.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith('decoder.')}, strict=True)
    quant_conv.load_state_dict({k[11:]: v for k, v in vsd.items() if k.startswith('quant_conv.')}, strict=True)
    post_quant_conv.load_state_dict({k[16:]: v for k, v in vsd.items() if k.startswith('post_quant_conv.')}, strict=True)
    e = vsd['quantize.embedding.weight']
    img, z = vq_inputs()
    with torch.no_grad():
        h = quant_conv(enc(img))                                   # VQModelInterface.encode
        zq, idx = vq_ref.quantize(z, e)
        dec_q = dec(post_quant_conv(zq))                           # decode(z)
    print(f'[vq] |h| max {h.abs().max():.3f} rms {h.pow(2).mean().sqrt():.3f}; |img| max {dec_q.abs().max():.3f}', flush=True)
    np.savez_compressed(os.path.join(OUT, 'cin_vq_128.npz'), h=h.numpy().astype(np.float32), dec_q=dec_q.numpy().astype(np.float32),
                        idx=idx.numpy().astype(np.int32), weight_seed=0, input_seed=1, img=IMG)

    # ---- pipeline: the notebook's cell on reference modules (the reference DDIMSampler, CPU) ----
    class CpuDDIM(DDIMSampler):
        def register_buffer(self, name, attr):            # (the reference moves its tables to cuda)
            setattr(self, name, attr)

    class Model:                                           # what DDIMSampler reads on LatentDiffusion (ddpm.py:117-169,986-992,1408-1410)
        def __init__(self):
            self.num_timesteps, self.device = int(p['timesteps']), torch.device('cpu')
            self.betas = torch.tensor(betas, dtype=torch.float32)
            self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
            self.alphas_cumprod_prev = torch.tensor(np.append(1., ac[:-1]), dtype=torch.float32)

        def apply_model(self, x, t, c):
            return m(x, t, context=c)

    n = PIPE['n_samples_per_class']
    g = torch.Generator().manual_seed(PIPE['seed'])
    conds, lats = [], []
    with torch.no_grad():
        uc = emb({'class_label': torch.tensor(n * [1000])})
        for cls in PIPE['classes']:
            x_T = torch.randn(n, 3, PIPE['h'], PIPE['w'], generator=g)
            c = emb({'class_label': torch.tensor(n * [cls])})
            s, _ = CpuDDIM(Model()).sample(S=PIPE['steps'], conditioning=c, batch_size=n, shape=[3, PIPE['h'], PIPE['w']], verbose=False,
                                           x_T=x_T, unconditional_guidance_scale=PIPE['scale'], unconditional_conditioning=uc,
                                           eta=PIPE['eta'])
            conds.append(c)
            lats.append(s)
        samples = torch.cat(lats)
        x_dec = dec(post_quant_conv(vq_ref.quantize(samples, e)[0]))   # model.decode_first_stage(samples)
    print(f'[pipeline] |samples| max {samples.abs().max():.3f}; |x_dec| max {x_dec.abs().max():.3f}', flush=True)
    np.savez_compressed(os.path.join(OUT, 'cin_pipeline_96.npz'), cond=torch.cat(conds).numpy().astype(np.float32),
                        uc=uc.numpy().astype(np.float32), samples=samples.numpy().astype(np.float32),
                        x_dec=x_dec.numpy().astype(np.float32), weight_seed=0, input_seed=PIPE['seed'],
                        classes=np.array(PIPE['classes'], dtype=np.int64), n_samples_per_class=n, steps=PIPE['steps'],
                        scale=PIPE['scale'], eta=PIPE['eta'])
    print('class-conditional fixtures written to', OUT)


if __name__ == '__main__':
    main()
