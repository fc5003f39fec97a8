"""Generate the fixtures of the older class-conditional ImageNet model (models/ldm/cin256/config.yaml) under tests/golden/ from the
reference code (build container only).

    PYTHONPATH=. python tools/make_golden_cin256_old.py

UNet: the reference `UNetModel` (ldm/modules/diffusionmodules/openaimodel.py) at the yaml's unet_config -- model_channels 256,
channel_mult [1, 2, 4], SpatialTransformers with num_head_channels 32 (8 / 16 / 32 heads) on every level, context_dim 512 -- weights
from `synthetic_named_state_dict` over the module's own key list, seed 0, fp32 on the CPU.  The context is the reference `ClassEmbedder`'s
output for the case's class ids ([B, 1, 512]: ONE token; the yaml gives no n_classes, so the table has the default 1000 rows).
Every case stores its fp16-operand floor by tools/make_golden_rdm.py's rule (`install_fp16_floor`: the operands of the classes
oracle/fp16_floor.py names rounded to fp16 once); it comes from the reference, never from the library.
Also written: the key / shape lists of the UNet and the class embedder, and the parsed yaml (its first stage is VQ-f8:
tools/make_golden_first_stages.py).  The fixtures hold outputs, seeds and class ids, never weights.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle.make_golden import REF  # noqa: E402  (the reference checkout: $SD_REFERENCE)
from make_golden_rdm import install_fp16_floor, remove_fp16_floor  # noqa: E402
OUT = os.path.join(ROOT, 'tests', 'golden')
YAML = os.path.join('models', 'ldm', 'cin256', 'config.yaml')

# name, h, w, timesteps, class ids (one per row)
UNET_CASES = [('8x8_b2', 8, 8, (1, 741), (25, 992)), ('16x16_b2', 16, 16, (1, 741), (7, 999)), ('32x32_b1', 32, 32, (741,), (0,))]


def unet_inputs(batch, channels, h, w, timesteps, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, channels, h, w, generator=g), torch.tensor(timesteps, dtype=torch.int64)


def main():
    import yaml
    from oracle.make_golden import _import_reference
    from stable_diffusion_amd.synthetic import (CIN256_OLD_CLASS_KWARGS, CIN256_OLD_SCHEDULE, CIN256_OLD_UNET_KWARGS, CIN256_OLD_VQ_KWARGS,
                                                synthetic_named_state_dict)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with open(os.path.join(REF, YAML)) as f:
        cfg = yaml.safe_load(f)
    p = cfg['model']['params']
    fs = p['first_stage_config']['params']
    assert dict(p['unet_config']['params']) == CIN256_OLD_UNET_KWARGS and dict(p['cond_stage_config']['params']) == CIN256_OLD_CLASS_KWARGS
    assert {k: fs[k] for k in ('embed_dim', 'n_embed', 'ddconfig')} == CIN256_OLD_VQ_KWARGS
    assert p['first_stage_config']['target'] == 'ldm.models.autoencoder.VQModelInterface'
    assert (p['timesteps'], p['linear_start'], p['linear_end'], p['conditioning_key']) == \
        tuple(CIN256_OLD_SCHEDULE[k] for k in ('timesteps', 'linear_start', 'linear_end', 'conditioning_key'))
    with open(os.path.join(OUT, 'cin256_old_config.json'), 'w') as f:
        json.dump(cfg, f)
    UNetModel = _import_reference()[0]
    for missing in ('clip', 'kornia'):           # imported at the top of ldm.modules.encoders.modules, not used by ClassEmbedder
        sys.modules.setdefault(missing, types.ModuleType(missing))
    from ldm.modules.encoders.modules import ClassEmbedder

    emb = ClassEmbedder(**CIN256_OLD_CLASS_KWARGS).eval()
    emb_specs = [(k, tuple(v.shape)) for k, v in emb.state_dict().items()]
    emb.load_state_dict(synthetic_named_state_dict(emb_specs, 0), strict=True)
    m = UNetModel(**CIN256_OLD_UNET_KWARGS).eval()
    specs = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    n_params = sum(int(np.prod(s)) for _, s in specs)
    print(f'[cin256_old] {len(specs)} keys, {n_params} parameters', flush=True)
    with open(os.path.join(OUT, 'cin256_old_state_dict_keys.json'), 'w') as f:
        json.dump({'module': 'UNetModel(**models/ldm/cin256 unet_config.params)', 'n_params': n_params, 'keys': [[k, list(s)] for k, s in specs],
                   'class_embedder_keys': [[k, list(s)] for k, s in emb_specs]}, f)
    m.load_state_dict(synthetic_named_state_dict(specs, 0), strict=True)
    for name, h, w, ts, classes in UNET_CASES:
        x, t = unet_inputs(len(ts), CIN256_OLD_UNET_KWARGS['in_channels'], h, w, ts)
        with torch.no_grad():
            c = emb({'class_label': torch.tensor(classes)})
            assert c.shape == (len(ts), 1, 512)
            eps = m(x, t, context=c)
            undo = install_fp16_floor(m)
            try:
                floor = float((m(x, t, context=c) - eps).abs().max())
            finally:
                remove_fp16_floor(undo)
            assert torch.equal(m(x, t, context=c), eps)           # (the rounding is gone again)
        print(f'[cin256_old unet {name}] |eps| max {eps.abs().max():.3f} rms {eps.pow(2).mean().sqrt():.3f} floor {floor:.3e}', flush=True)
        assert bool(torch.isfinite(eps).all())
        np.savez_compressed(os.path.join(OUT, f'cin256_old_unet_{name}.npz'), eps=eps.numpy().astype(np.float32), weight_seed=0, input_seed=1,
                            batch=len(ts), h=h, w=w, t=t.numpy(), classes=np.array(classes, dtype=np.int64), floor_maxabs=floor)
    print('cin256 (old) fixtures written to', OUT)


if __name__ == '__main__':
    main()
