"""Generate the fixtures of the semantic-synthesis models under tests/golden/ from the reference code (build container only).

    PYTHONPATH=. python tools/make_golden_semantic.py

UNet: the reference `UNetModel` at models/ldm/semantic_synthesis512's unet_config (semantic_synthesis256's differs in image_size only:
asserted), weights from `synthetic_named_state_dict` over the module's own key list, fp32 on the CPU.  Every case also stores its
fp16-operand floor through tools/make_golden_rdm.py's hook (`floor_maxabs`: the reference arithmetic with the operands of the classes
oracle/fp16_floor.py names rounded to fp16 once).  The floor comes from the reference, never from the library.  A case whose floor
exceeds 1e-3 / 1.25 is listed in semantic_floors_above_bar.json (the project's outlier rule: held to 1.25 x its floor).
Rescaler: the reference `SpatialRescaler` (bilinear, multiplier 0.5) in fp32 on 3 * randn and one-hot maps drawn from the stored seeds.
Pipeline: labels 64 x 64 -> one-hot -> the reference cond stage -> the reference DDIMSampler (10 steps, eta 0) over the reference UNet
behind cat([x, c], 1) -> the VQ-f4 decode of the reference Decoder on the golden's own codes.  The loop runs a second time with every eps
moved by 1e-3 * sign(randn); the max-abs divergence of `samples` is the bar of the test.
Also written: both parsed yamls and the names / shapes of the UNet's state_dict.  The fixtures hold outputs and seeds, never weights.
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle.make_golden import REF  # noqa: E402  (the reference checkout: $SD_REFERENCE)
OUT = os.path.join(ROOT, 'tests', 'golden')

# name, batch, h, w, timesteps
UNET_CASES = [('8x8_b2', 2, 8, 8, (981, 1)), ('16x24_b1', 1, 16, 24, (500,)), ('32x32_b1', 1, 32, 32, (500,)),
              ('8x8_b10', 10, 8, 8, (981, 881, 781, 681, 581, 481, 381, 281, 181, 1))]
UNET_KEYS, UNET_PARAMS = 216, 215229315
# name, kwargs of SpatialRescaler, batch, h, w, input kind ('randn': 3 * randn, 'onehot': one_hot(randint))
RESCALER_CASES = [('yaml_16x24_randn', dict(n_stages=2, in_channels=182, out_channels=3), 2, 16, 24, 'randn'),
                  ('yaml_16x24_onehot', dict(n_stages=2, in_channels=182, out_channels=3), 2, 16, 24, 'onehot'),
                  ('yaml_13x19_bias', dict(n_stages=2, in_channels=182, out_channels=3, bias=True), 1, 13, 19, 'randn'),
                  ('c5_6x10_n1', dict(n_stages=1, in_channels=5, out_channels=8, bias=True), 2, 6, 10, 'randn'),
                  ('c7_12x20_nomap', dict(n_stages=2, in_channels=7), 1, 12, 20, 'randn')]
PIPE = dict(steps=10, batch=2, h=64, w=64, eta=0.0, input_seed=3, label_seed=4, perturb_seed=5, perturb=1e-3)
MIXED_TOL = 1e-3


def unet_inputs(batch, channels, h, w, timesteps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, channels, h, w, generator=g), torch.tensor(timesteps, dtype=torch.int64)


def rescaler_input(kind, batch, channels, h, w, seed=2):
    g = torch.Generator().manual_seed(seed)
    if kind == 'randn':
        return 3.0 * torch.randn(batch, channels, h, w, generator=g)
    return F.one_hot(torch.randint(0, channels, (batch, h, w), generator=g), channels).permute(0, 3, 1, 2).float().contiguous()


def pipeline_inputs(batch, classes, h, w, input_seed, label_seed):
    """x_T over the latent h/4 x w/4 and the label map"""
    x_T = torch.randn(batch, 3, h // 4, w // 4, generator=torch.Generator().manual_seed(input_seed))
    return x_T, torch.randint(0, classes, (batch, h, w), generator=torch.Generator().manual_seed(label_seed))


def main():
    import yaml
    import vq_ref
    from make_golden_faces import vq_decode_specs
    from make_golden_rdm import install_fp16_floor, remove_fp16_floor
    from oracle.make_golden import _import_reference
    from stable_diffusion_amd.synthetic import (FACES_VQ_KWARGS, SEMANTIC_RESCALER_KWARGS, SEMANTIC_SCHEDULE, SEMANTIC_UNET_KWARGS,
                                                synthetic_named_state_dict)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfgs = {}
    for name in ('semantic_synthesis256', 'semantic_synthesis512'):
        with open(os.path.join(REF, 'models', 'ldm', name, 'config.yaml')) as f:
            cfgs[name] = yaml.safe_load(f)
        with open(os.path.join(OUT, f'{name}_config.json'), 'w') as f:
            json.dump(cfgs[name], f)
    p = cfgs['semantic_synthesis512']['model']['params']
    assert dict(p['unet_config']['params']) == SEMANTIC_UNET_KWARGS
    assert dict(cfgs['semantic_synthesis256']['model']['params']['unet_config']['params'], image_size=128) == SEMANTIC_UNET_KWARGS
    for q in (c['model']['params'] for c in cfgs.values()):
        fq = q['first_stage_config']['params']
        assert dict(embed_dim=fq['embed_dim'], n_embed=fq['n_embed'], ddconfig=dict(fq['ddconfig'])) == FACES_VQ_KWARGS
        assert dict(q['cond_stage_config']['params']) == SEMANTIC_RESCALER_KWARGS
        assert (q['timesteps'], q['linear_start'], q['linear_end']) == tuple(SEMANTIC_SCHEDULE[k] for k in ('timesteps', 'linear_start', 'linear_end'))
        assert q['concat_mode'] is True and q['cond_stage_key'] == 'segmentation' and SEMANTIC_SCHEDULE['conditioning_key'] == 'concat'
    UNetModel = _import_reference()[0]
    for missing in ('clip', 'kornia'):           # imported at the top of ldm.modules.encoders.modules, not used by SpatialRescaler
        sys.modules.setdefault(missing, types.ModuleType(missing))
    from ldm.modules.encoders.modules import SpatialRescaler

    # ---- UNet ----
    m = UNetModel(**SEMANTIC_UNET_KWARGS).eval()
    specs = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    n_params = sum(int(np.prod(s)) for _, s in specs)
    print(f'[semantic unet] {len(specs)} keys, {n_params} parameters', flush=True)
    assert (len(specs), n_params) == (UNET_KEYS, UNET_PARAMS), (len(specs), n_params)
    with open(os.path.join(OUT, 'semantic_unet_state_dict_keys.json'), 'w') as f:
        json.dump({'module': 'UNetModel(**semantic_synthesis512 unet_config.params)', 'n_params': n_params,
                   'keys': [[k, list(s)] for k, s in specs]}, f)
    m.load_state_dict(synthetic_named_state_dict(specs, 0), strict=True)
    above = []
    for name, b, h, w, ts in UNET_CASES:
        x, t = unet_inputs(b, SEMANTIC_UNET_KWARGS['in_channels'], h, w, ts)
        with torch.no_grad():
            eps = m(x, t)
            undo = install_fp16_floor(m)
            try:
                floor = float((m(x, t) - eps).abs().max())
            finally:
                remove_fp16_floor(undo)
            assert torch.equal(m(x, t), eps)                      # (the rounding is gone again)
        print(f'[semantic unet {name}] |eps| max {eps.abs().max():.3f} rms {eps.pow(2).mean().sqrt():.3f} floor {floor:.3e}', flush=True)
        assert bool(torch.isfinite(eps).all())
        if floor > MIXED_TOL / 1.25:
            above.append({'case': name, 'floor_maxabs': floor})
        np.savez_compressed(os.path.join(OUT, f'semantic_unet_{name}.npz'), eps=eps.numpy().astype(np.float32), weight_seed=0, input_seed=1,
                            batch=b, h=h, w=w, t=t.numpy(), floor_maxabs=floor)
    with open(os.path.join(OUT, 'semantic_floors_above_bar.json'), 'w') as f:
        json.dump(above, f)
    print(f'[semantic unet] floors above {MIXED_TOL / 1.25:.1e}: {above}', flush=True)

    # ---- the cond stage ----
    def rescaler(kwargs):
        r = SpatialRescaler(**kwargs).eval()
        r.load_state_dict(synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in r.state_dict().items()], 0), strict=True)
        return r
    for name, kwargs, b, h, w, kind in RESCALER_CASES:
        x = rescaler_input(kind, b, kwargs['in_channels'], h, w)
        with torch.no_grad():
            out = rescaler(kwargs)(x)
        print(f'[semantic rescaler {name}] {tuple(x.shape)} -> {tuple(out.shape)} |out| max {out.abs().max():.3f}', flush=True)
        np.savez_compressed(os.path.join(OUT, f'semantic_rescaler_{name}.npz'), out=out.numpy().astype(np.float32), weight_seed=0, input_seed=2,
                            kind=kind, batch=b, h=h, w=w, kwargs=json.dumps(kwargs))

    # ---- pipeline: labels -> cond stage -> the reference DDIMSampler over cat([x, c], 1) -> VQ-f4 decode ----
    import ldm.models.diffusion.ddim as ref_ddim
    from ldm.modules.diffusionmodules.util import make_beta_schedule

    class CpuDDIM(ref_ddim.DDIMSampler):
        def register_buffer(self, name, attr):            # (the reference moves its tables to cuda)
            setattr(self, name, attr)

    class Model:                                           # what DDIMSampler reads on LatentDiffusion (ddpm.py:117-169,986-992,1411-1413)
        def __init__(self, perturb_seed=None):
            betas = make_beta_schedule('linear', p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'])
            ac = np.cumprod(1. - betas, axis=0)
            self.num_timesteps, self.device = int(p['timesteps']), torch.device('cpu')
            self.betas = torch.tensor(betas, dtype=torch.float32)
            self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
            self.alphas_cumprod_prev = torch.tensor(np.append(1., ac[:-1]), dtype=torch.float32)
            self.g = None if perturb_seed is None else torch.Generator().manual_seed(perturb_seed)

        def apply_model(self, x, t, c):
            eps = m(torch.cat([x, c], dim=1), t)
            if self.g is not None:
                eps = eps + PIPE['perturb'] * torch.sign(torch.randn(eps.shape, generator=self.g))
            return eps

    classes = SEMANTIC_RESCALER_KWARGS['in_channels']
    x_T, labels = pipeline_inputs(PIPE['batch'], classes, PIPE['h'], PIPE['w'], PIPE['input_seed'], PIPE['label_seed'])
    with torch.no_grad():
        c = rescaler(SEMANTIC_RESCALER_KWARGS).encode(F.one_hot(labels, classes).permute(0, 3, 1, 2).float().contiguous())
    assert tuple(c.shape) == tuple(x_T.shape)

    def run(perturb_seed):
        with torch.no_grad():
            s, _ = CpuDDIM(Model(perturb_seed)).sample(S=PIPE['steps'], conditioning=c, batch_size=c.shape[0], shape=list(x_T.shape[1:]),
                                                       verbose=False, x_T=x_T, eta=PIPE['eta'])
        return s
    samples = run(None)
    bar_s = float((run(PIPE['perturb_seed']) - samples).abs().max())
    fs = p['first_stage_config']['params']
    dec, pqc, vspecs = vq_decode_specs(fs)
    vsd = synthetic_named_state_dict(vspecs, 0)
    dec.load_state_dict({k[8:]: v for k, v in vsd.items() if k.startswith('decoder.')}, strict=True)
    pqc.load_state_dict({k[16:]: v for k, v in vsd.items() if k.startswith('post_quant_conv.')}, strict=True)
    with torch.no_grad():
        zq, idx = vq_ref.quantize(samples, vsd['quantize.embedding.weight'])     # decode_first_stage: scale_factor 1.0 (none in these yamls)
        x_dec = dec(pqc(zq))
    print(f'[pipeline] |c| max {c.abs().max():.3f}; |samples| max {samples.abs().max():.3f}; |x_dec| max {x_dec.abs().max():.3f} '
          f'{tuple(x_dec.shape)}; bar from eps + {PIPE["perturb"]:g} sign: samples {bar_s:.3e}', flush=True)
    assert bool(torch.isfinite(samples).all()) and bool(torch.isfinite(x_dec).all())
    np.savez_compressed(os.path.join(OUT, 'semantic_pipeline_16x16.npz'), c=c.numpy().astype(np.float32), samples=samples.numpy().astype(np.float32),
                        x_dec=x_dec.numpy().astype(np.float32), idx=idx.numpy().astype(np.int32), bar_samples=bar_s, weight_seed=0,
                        **{k: v for k, v in PIPE.items()})
    print('semantic-synthesis fixtures written to', OUT)


if __name__ == '__main__':
    main()
