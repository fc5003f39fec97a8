"""Generate the CLIP vision tower's fixtures under tests/golden/ with the installed `transformers` on the CPU (no network, no checkpoint).

    PYTHONPATH=. python tools/make_golden_vit.py

`CLIPVisionModelWithProjection` is instantiated from a config (quick_gelu, eager attention), loaded with
stable_diffusion_amd.synthetic.synthetic_vision_state_dict and run in fp32.  The fixtures hold seeds and outputs, never weights or pixels:

vit_tiny_b3.npz         VIT_TINY, B = 3:      image_embeds, pooled_output, last_hidden_state (all 5 rows), fp16_floor
vit_l14thin_b2.npz      VIT_L14_THIN, B = 2:  image_embeds, pooled_output, last_hidden_state rows {0, 1, 128, 256}, fp16_floor
vit_state_dict_keys.json  key -> shape of CLIPVisionModelWithProjection at VIT_TINY ('vision') and of the safety checker around it
                        ('safety_checker': the tower one level deeper, the projection, 17 concept and 3 special-care vectors and thresholds)

fp16_floor (the idea of oracle/fp16_floor.py applied to this model): the max-abs deviation, over the three outputs, from the fp32 run of the
SAME model with every nn.Linear input and weight, both operands of the patch convolution and the q / k / v outputs rounded to fp16 once --
the roundings the mixed HIP walk performs by design.  It does not model fp16 attention probabilities or a different accumulation order; the
tests allow 2 x the floor for those.  The per-output floors are stored beside it (floor_image_embeds, floor_pooled_output, floor_hidden).
"""
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stable_diffusion_amd import synthetic  # noqa: E402
OUT = os.path.join(ROOT, 'tests', 'golden')

WEIGHT_SEED, PIXEL_SEED = 0, 1234
CASES = [('vit_tiny_b3', synthetic.VIT_TINY, 3, None), ('vit_l14thin_b2', synthetic.VIT_L14_THIN, 2, [0, 1, 128, 256])]


def pixel_values(B, S, seed=PIXEL_SEED):
    """what the tests regenerate: N(0, 1), about the spread of CLIP-normalised images"""
    return torch.randn((B, 3, S, S), generator=torch.Generator().manual_seed(seed))


def reference_model(cfg, seed=WEIGHT_SEED):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    hc = CLIPVisionConfig(hidden_size=cfg['hidden_size'], intermediate_size=cfg['intermediate_size'], projection_dim=cfg['projection_dim'],
                          num_hidden_layers=cfg['num_hidden_layers'], num_attention_heads=cfg['num_attention_heads'],
                          image_size=cfg['image_size'], patch_size=cfg['patch_size'], hidden_act='quick_gelu', layer_norm_eps=1e-5,
                          attention_dropout=0.0)
    hc._attn_implementation = 'eager'
    m = CLIPVisionModelWithProjection(hc).float().eval()
    sd = synthetic.synthetic_vision_state_dict(cfg, seed)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith('position_ids') for k in missing), (missing, unexpected)
    return m


def r16(t):
    return t.half().float()


def fp16_operand_model(m):
    """a copy of `m` whose Linear / patch-conv operands and q / k / v outputs are rounded to fp16 once"""
    e = copy.deepcopy(m)
    for name, mod in e.named_modules():
        if isinstance(mod, (nn.Linear, nn.Conv2d)):
            mod.weight.data = r16(mod.weight.data)
            mod.register_forward_pre_hook(lambda _m, args: (r16(args[0]),) + tuple(args[1:]))
        if name.endswith(('.q_proj', '.k_proj', '.v_proj')):
            mod.register_forward_hook(lambda _m, _a, out: r16(out))
    return e


@torch.no_grad()
def run(m, px):
    o = m(pixel_values=px)
    return dict(image_embeds=o.image_embeds, pooled_output=m.vision_model.post_layernorm(o.last_hidden_state[:, 0]),
                last_hidden_state=o.last_hidden_state)


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, cfg, B, rows in CASES:
        m = reference_model(cfg)
        px = pixel_values(B, cfg['image_size'])
        ref, emu = run(m, px), run(fp16_operand_model(m), px)
        T = ref['last_hidden_state'].shape[1]
        rows = list(range(T)) if rows is None else rows
        floors = {k: float((emu[k] - ref[k]).abs().max()) for k in ref}
        hid = ref['last_hidden_state'][:, rows]
        floors['last_hidden_state'] = float((emu['last_hidden_state'][:, rows] - hid).abs().max())
        floor = max(floors.values())
        np.savez_compressed(os.path.join(OUT, name + '.npz'), weight_seed=np.int64(WEIGHT_SEED), pixel_seed=np.int64(PIXEL_SEED), batch=np.int64(B),
                            image_embeds=ref['image_embeds'].numpy(), pooled_output=ref['pooled_output'].numpy(),
                            hidden_rows=np.asarray(rows, dtype=np.int64), last_hidden_state=hid.numpy(), fp16_floor=np.float64(floor),
                            floor_image_embeds=np.float64(floors['image_embeds']), floor_pooled_output=np.float64(floors['pooled_output']),
                            floor_hidden=np.float64(floors['last_hidden_state']))
        rms = {k: float(v.pow(2).mean().sqrt()) for k, v in ref.items()}
        print(f'{name}: T = {T}, fp16_floor = {floor:.3e}, per output {floors}, output rms {rms}')
    m = reference_model(synthetic.VIT_TINY)
    vision = {k: list(v.shape) for k, v in m.state_dict().items() if not k.endswith('position_ids')}
    Pd = synthetic.VIT_TINY['projection_dim']
    checker = {('vision_model.' + k if k.startswith('vision_model.') else k): s for k, s in vision.items()}
    checker.update(concept_embeds=[17, Pd], special_care_embeds=[3, Pd], concept_embeds_weights=[17], special_care_embeds_weights=[3])
    with open(os.path.join(OUT, 'vit_state_dict_keys.json'), 'w') as f:
        json.dump(dict(config=synthetic.VIT_TINY, vision=vision, safety_checker=checker), f, indent=1, sort_keys=True)
    print(f'vit_state_dict_keys.json: {len(vision)} + {len(checker)} keys')


if __name__ == '__main__':
    main()
