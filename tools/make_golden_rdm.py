"""Generate the fixtures of the retrieval-augmented UNet and of layout-to-image's under tests/golden/ from the reference code (build container only).

    PYTHONPATH=. python tools/make_golden_rdm.py [--no-full]

UNets: the reference `UNetModel` (ldm/modules/diffusionmodules/openaimodel.py) at configs/retrieval-augmented-diffusion/768x768.yaml's
unet_config (model_channels 448, num_head_channels 32 with SpatialTransformers: 14 / 28 / 42 / 56 heads; 16 latent channels), at
models/ldm/layout2img-openimages256's (128, transformer_depth 3, 92 context tokens) and at the two stand-ins of
`stable_diffusion_amd.synthetic` (RDM64: the yaml at model_channels 64; RDM448X2: the real width over two levels; RDM320X1: one level
of 320 channels, the width of the row-strip chain launches, with 10 heads of 32), weights from
`synthetic_named_state_dict` over the module's own key list (seeded per key, so the GPU tests regenerate the same tensors from the HIP
module's key list), fp32 on the CPU.  The context is N(0, 1) of 1 / 11 / 21 tokens (knn2img.py --knn 0 / 10 / 20: the text embedding
and its neighbours), 92 for layout-to-image, or all zeros (the script's unconditional context).
legacy: the module is built with legacy True and False; both must give one key list and, on RDM64, one output (openaimodel.py:542-549).
Every pytest case also stores its fp16-operand floor -- the reference arithmetic with every conv / linear / attention operand of the
classes oracle/fp16_floor.py names rounded to fp16 once -- as `floor_maxabs`: reported beside the measured error (every case is held to
the 1e-3 bar; a case measured above it would be listed by name in the test and held to 1.25 x its floor, README's rule of the outlier
family -- there is none).  The floor comes from the reference, never from the library.
Pipeline (RDM64): the body of scripts/knn2img.py:357-377 up to samples_ddim -- c = cat([text, nn]) of unit-norm rows, uc = zeros_like(c),
the reference DDIMSampler at the script's default --scale 5.0 and eta 0.0, 10 steps on 16 x 16.  The loop runs a second time with every eps
moved by 1e-3 * sign(randn) on every element at every step; the max-abs divergence of `samples` from the first run is the bar of the test.
Also written: the names / shapes of the two real UNets' state_dicts and the two parsed yamls.  The fixtures hold outputs and seeds, never weights.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.make_golden import REF  # noqa: E402  (the reference checkout: $SD_REFERENCE)
OUT = os.path.join(ROOT, 'tests', 'golden')
RDM_YAML = os.path.join('configs', 'retrieval-augmented-diffusion', '768x768.yaml')
LAYOUT_YAML = os.path.join('models', 'ldm', 'layout2img-openimages256', 'config.yaml')

# name, batch, h, w, timesteps, context tokens, context kind ('randn' / 'zero')
RDM64_CASES = [('8x8_b2', 2, 8, 8, (981, 1), 11, 'randn'), ('48x48_b1', 1, 48, 48, (500,), 11, 'randn'),
               ('16x16_b10', 10, 16, 16, (981, 881, 781, 681, 581, 481, 381, 281, 181, 1), 21, 'randn'),
               ('16x16_b2_ctx1', 2, 16, 16, (981, 1), 1, 'randn'), ('16x16_b2_ctx0', 2, 16, 16, (981, 1), 11, 'zero')]
RDM320X1_CASES = [('16x16_b2', 2, 16, 16, (981, 1), 11, 'randn')]        # (512 token rows: the LayerNorm fold and the row-strip chains are on)
RDM448X2_CASES = [('8x8_b2', 2, 8, 8, (981, 1), 11, 'randn'), ('24x24_b1', 1, 24, 24, (500,), 11, 'randn')]
LAYOUT_CASES = [('8x8_b2', 2, 8, 8, (981, 1), 92, 'randn'), ('32x32_b1', 1, 32, 32, (500,), 92, 'randn')]
RDM_FULL_CASES = [('8x8_b2', 2, 8, 8, (981, 1), 11, 'randn')]          # (tools/bench_rdm.py's parity line, not a pytest case)
RDM_KEYS, RDM_PARAMS = 688, 1335480400
PIPE = dict(steps=10, batch=2, h=16, w=16, eta=0.0, scale=5.0, knn=10, input_seed=3, ctx_seed=4, perturb_seed=5, perturb=1e-3)


def unet_inputs(batch, channels, h, w, timesteps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, channels, h, w, generator=g), torch.tensor(timesteps, dtype=torch.int64)


def context_inputs(batch, tokens, dim, kind='randn', seed=2):
    if kind == 'zero':
        return torch.zeros(batch, tokens, dim)
    return torch.randn(batch, tokens, dim, generator=torch.Generator().manual_seed(seed))


def pipeline_inputs(batch, channels, h, w, tokens, dim, input_seed, ctx_seed):
    """x_T and c = cat([text, nn], 1): rows of unit norm, as FrozenCLIPTextEmbedder and the retrieval database give them"""
    x_T = torch.randn(batch, channels, h, w, generator=torch.Generator().manual_seed(input_seed))
    c = torch.randn(batch, tokens, dim, generator=torch.Generator().manual_seed(ctx_seed))
    return x_T, c / c.norm(dim=-1, keepdim=True)


def install_fp16_floor(m):
    """oracle/fp16_floor.py's rounding on the reference module: the operands of the classes it names (3x3 convs, resampling convs, the
    transformer linears, q k^T and p v) rounded to fp16 once, fp32 accumulation, everything else untouched.  Returns the undo list."""
    from oracle.fp16_floor import CLASSES, Emul, r16
    from ldm.modules.attention import CrossAttention
    on = [c for c in CLASSES if c not in ('gn_silu_act', 'ln_act')]
    e = Emul(on)
    undo = []

    def conv_forward(mod):
        return lambda x: F.conv2d(r16(x), r16(mod.weight), mod.bias, mod.stride, mod.padding)

    def lin_forward(mod):
        return lambda x: F.linear(r16(x), r16(mod.weight), mod.bias)

    def attn_forward(mod):
        def forward(x, context=None, mask=None):
            assert mask is None
            h = mod.heads
            ctx = x if context is None else context
            q, k, v = mod.to_q(x), mod.to_k(ctx), mod.to_v(ctx)
            b, n, c = q.shape
            d = c // h

            def split(t):
                return t.reshape(b, t.shape[1], h, d).permute(0, 2, 1, 3).reshape(b * h, t.shape[1], d)
            q, k, v = r16(split(q)), r16(split(k)), r16(split(v))
            sim = torch.bmm(q, k.transpose(1, 2)) * mod.scale
            p16 = r16(torch.exp(sim - sim.amax(dim=-1, keepdim=True)))
            out = torch.bmm(p16, v) / p16.sum(dim=-1, keepdim=True)
            out = out.reshape(b, h, n, d).permute(0, 2, 1, 3).reshape(b, n, c)
            return mod.to_out(out)
        return forward

    for name, mod in m.named_modules():
        new = None
        if isinstance(mod, CrossAttention):
            new = attn_forward(mod)
        elif isinstance(mod, torch.nn.Conv2d) and e.cls_of(name) in on:
            new = conv_forward(mod)
        elif isinstance(mod, torch.nn.Linear) and e.cls_of(name) in on:
            new = lin_forward(mod)
        if new is not None:
            undo.append(mod)
            mod.forward = new
    return undo


def remove_fp16_floor(undo):
    for mod in undo:
        del mod.forward


def main():
    import yaml
    from oracle.make_golden import _import_reference
    from stable_diffusion_amd.synthetic import (LAYOUT_UNET_KWARGS, RDM320X1_UNET_KWARGS, RDM448X2_UNET_KWARGS, RDM64_UNET_KWARGS, RDM_SCHEDULE,
                                                RDM_UNET_KWARGS, synthetic_named_state_dict)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with_full = '--no-full' not in sys.argv
    cfgs = {}
    for tag, path in (('rdm768', RDM_YAML), ('layout2img', LAYOUT_YAML)):
        with open(os.path.join(REF, path)) as f:
            cfgs[tag] = yaml.safe_load(f)
        with open(os.path.join(OUT, f'{tag}_config.json'), 'w') as f:
            json.dump(cfgs[tag], f)
    p = cfgs['rdm768']['model']['params']
    pl = cfgs['layout2img']['model']['params']
    assert dict(p['unet_config']['params']) == RDM_UNET_KWARGS and dict(pl['unet_config']['params']) == LAYOUT_UNET_KWARGS
    assert (p['timesteps'], p['linear_start'], p['linear_end'], p['conditioning_key']) == \
        tuple(RDM_SCHEDULE[k] for k in ('timesteps', 'linear_start', 'linear_end', 'conditioning_key'))
    UNetModel = _import_reference()[0]

    def specs_of(m):
        return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]

    def meta_specs(params):
        with torch.device('meta'):
            return {flag: specs_of(UNetModel(**dict(params, legacy=flag))) for flag in (True, False)}

    # ---- key lists of the two real configurations; legacy True / False build the same module ----
    for tag, params, label in (('rdm', RDM_UNET_KWARGS, 'UNetModel(**retrieval-augmented-diffusion/768x768.yaml unet_config.params)'),
                               ('layout', LAYOUT_UNET_KWARGS, 'UNetModel(**layout2img-openimages256 unet_config.params)')):
        by_flag = meta_specs(params)
        assert by_flag[True] == by_flag[False], tag
        specs = by_flag[True]
        n_params = sum(int(np.prod(s)) for _, s in specs)
        print(f'[{tag}] {len(specs)} keys, {n_params} parameters', flush=True)
        if tag == 'rdm':
            assert (len(specs), n_params) == (RDM_KEYS, RDM_PARAMS), (len(specs), n_params)
        with open(os.path.join(OUT, f'{tag}_unet_state_dict_keys.json'), 'w') as f:
            json.dump({'module': label, 'n_params': n_params, 'keys': [[k, list(s)] for k, s in specs]}, f)

    def unet_fixtures(tag, params, cases, floor=True, check_legacy=False):
        m = UNetModel(**params).eval()
        specs = specs_of(m)
        sd = synthetic_named_state_dict(specs, 0)
        m.load_state_dict(sd, strict=True)
        other = None
        if check_legacy:
            other = UNetModel(**dict(params, legacy=False)).eval()
            other.load_state_dict(sd, strict=True)
        del sd
        for name, b, h, w, ts, tokens, kind in cases:
            x, t = unet_inputs(b, params['in_channels'], h, w, ts)
            c = context_inputs(b, tokens, params['context_dim'], kind)
            with torch.no_grad():
                eps = m(x, t, context=c)
                extra = {}
                if floor:
                    undo = install_fp16_floor(m)
                    try:
                        extra['floor_maxabs'] = float((m(x, t, context=c) - eps).abs().max())
                    finally:
                        remove_fp16_floor(undo)
                    assert torch.equal(m(x, t, context=c), eps)           # (the rounding is gone again)
                if other is not None:
                    assert torch.equal(other(x, t, context=c), eps), 'legacy=False computes something else'
            print(f'[{tag} unet {name}] |eps| max {eps.abs().max():.3f} rms {eps.pow(2).mean().sqrt():.3f} {extra}', flush=True)
            assert bool(torch.isfinite(eps).all())
            np.savez_compressed(os.path.join(OUT, f'{tag}_unet_{name}.npz'), eps=eps.numpy().astype(np.float32), weight_seed=0, input_seed=1,
                                ctx_seed=2, ctx_tokens=tokens, ctx_kind=kind, batch=b, h=h, w=w, t=t.numpy(), **extra)
        return m

    m64 = unet_fixtures('rdm64', RDM64_UNET_KWARGS, RDM64_CASES, check_legacy=True)
    unet_fixtures('rdm448x2', RDM448X2_UNET_KWARGS, RDM448X2_CASES)
    unet_fixtures('rdm320x1', RDM320X1_UNET_KWARGS, RDM320X1_CASES)
    unet_fixtures('layout', LAYOUT_UNET_KWARGS, LAYOUT_CASES)
    if with_full:
        unet_fixtures('rdm', RDM_UNET_KWARGS, RDM_FULL_CASES, floor=False)

    # ---- pipeline: scripts/knn2img.py:357-377 on reference modules (the reference DDIMSampler, CPU) ----
    import ldm.models.diffusion.ddim as ref_ddim
    from ldm.modules.diffusionmodules.util import make_beta_schedule

    class CpuDDIM(ref_ddim.DDIMSampler):
        def register_buffer(self, name, attr):            # (the reference moves its tables to cuda)
            setattr(self, name, attr)

    class Model:                                           # what DDIMSampler reads on LatentDiffusion (ddpm.py:117-169,986-992,1408-1410)
        def __init__(self, perturb_seed=None):
            betas = make_beta_schedule('linear', p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'])
            ac = np.cumprod(1. - betas, axis=0)
            self.num_timesteps, self.device = int(p['timesteps']), torch.device('cpu')
            self.betas = torch.tensor(betas, dtype=torch.float32)
            self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
            self.alphas_cumprod_prev = torch.tensor(np.append(1., ac[:-1]), dtype=torch.float32)
            self.g = None if perturb_seed is None else torch.Generator().manual_seed(perturb_seed)

        def apply_model(self, x, t, c):
            eps = m64(x, t, context=c)
            if self.g is not None:
                eps = eps + PIPE['perturb'] * torch.sign(torch.randn(eps.shape, generator=self.g))
            return eps

    kw = RDM64_UNET_KWARGS
    x_T, c = pipeline_inputs(PIPE['batch'], kw['in_channels'], PIPE['h'], PIPE['w'], 1 + PIPE['knn'], kw['context_dim'], PIPE['input_seed'],
                             PIPE['ctx_seed'])
    uc = torch.zeros_like(c)

    def run(perturb_seed):
        with torch.no_grad():
            s, _ = CpuDDIM(Model(perturb_seed)).sample(S=PIPE['steps'], conditioning=c, batch_size=c.shape[0],
                                                       shape=[kw['in_channels'], PIPE['h'], PIPE['w']], verbose=False, x_T=x_T,
                                                       unconditional_guidance_scale=PIPE['scale'], unconditional_conditioning=uc,
                                                       eta=PIPE['eta'])
        return s
    samples = run(None)
    bar_s = float((run(PIPE['perturb_seed']) - samples).abs().max())
    print(f'[pipeline] |samples| max {samples.abs().max():.3f}; bar from eps + {PIPE["perturb"]:g} sign: samples {bar_s:.3e}', flush=True)
    assert bool(torch.isfinite(samples).all())
    np.savez_compressed(os.path.join(OUT, 'rdm64_pipeline_16.npz'), samples=samples.numpy().astype(np.float32), bar_samples=bar_s,
                        weight_seed=0, **{k: v for k, v in PIPE.items()})
    print('retrieval-augmented / layout-to-image fixtures written to', OUT)


if __name__ == '__main__':
    main()
