"""Generate the LAION-400M model's fixtures under tests/golden/ from the reference code (build container only).

    PYTHONPATH=. python tools/make_golden_laion.py

Text encoder: imports ldm/modules/x_transformer.py of the reference checkout (by file: ldm.modules.encoders.modules imports
clip and kornia at the top), builds BERTEmbedder's `TransformerWrapper(num_tokens, max_seq_len, attn_layers=Encoder(dim,
depth))` (modules.py:80-91), loads `tests/bert_ref.make_bert_state_dict` into it (strict=True), asserts the CPU restatement
`tests/bert_ref.bert_forward` equals it to 5e-5 and stores `forward(ids, return_embeddings=True)`.
UNet: the reference `UNetModel` at the 1p4B config (oracle.plan.UNetConfig(context_dim=1280)) with oracle.weights weights,
checked against oracle.unet_ref the same way.  Also: the names / shapes of the depth-32 state_dict and the parsed 1p4B yaml.
The fixtures hold outputs and seeds, never weights: the tests regenerate the weights from the seeds.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
REF = os.environ.get('SD_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden')
YAML_1P4B = os.path.join('configs', 'latent-diffusion', 'txt2img-1p4B-eval.yaml')

# name, config, weight seed, batch, L
BERT_CASES = [('tiny_b2', 'tiny', 0, 2, 77), ('tiny_b3_L40', 'tiny', 1, 3, 40), ('laion_d2_b2', 'laion_d2', 0, 2, 77),
              ('laion_b2', 'laion', 0, 2, 77)]
UNET_CASES = [('laion_16x16', 16, 16), ('laion_64x64', 64, 64)]


def _x_transformer():
    spec = importlib.util.spec_from_file_location('ref_x_transformer', os.path.join(REF, 'ldm', 'modules', 'x_transformer.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def bert_goldens():
    import bert_ref
    xt = _x_transformer()
    for name, cfg_name, seed, b, L in BERT_CASES:
        cfg = bert_ref.CFGS[cfg_name]
        m = xt.TransformerWrapper(num_tokens=cfg.vocab_size, max_seq_len=cfg.max_seq_len,
                                  attn_layers=xt.Encoder(dim=cfg.dim, depth=cfg.depth), emb_dropout=0.0).eval()
        sd = bert_ref.make_bert_state_dict(cfg, seed)
        m.load_state_dict(sd, strict=True)
        if cfg_name == 'laion':
            keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
            with open(os.path.join(OUT, 'bert_state_dict_keys.json'), 'w') as f:
                json.dump({'module': 'TransformerWrapper(num_tokens=30522, max_seq_len=77, attn_layers=Encoder(dim=1280, depth=32))',
                           'keys': keys}, f, indent=0)
        ids = bert_ref.make_bert_ids(cfg, b, L, seed=1)
        with torch.no_grad():
            ref = m(ids, return_embeddings=True)
            orc = bert_ref.bert_forward(sd, cfg, ids)
        err = (ref - orc).abs().max().item()
        print(f'[bert {name}] out {tuple(ref.shape)} |x| max {ref.abs().max():.3f} rms {ref.pow(2).mean().sqrt():.3f} '
              f'restatement-vs-reference {err:.3e}', flush=True)
        assert err < 5e-5, err
        np.savez_compressed(os.path.join(OUT, f'bert_{name}.npz'), out=ref.numpy().astype(np.float32), cfg=cfg_name,
                            weight_seed=seed, input_seed=1, batch=b, L=L, restatement_vs_reference=err)
        del m, sd


def unet_goldens():
    from oracle import unet_ref
    from oracle.make_golden import _import_reference
    from oracle.plan import UNetConfig
    from oracle.weights import make_inputs, make_state_dict
    UNetModel = _import_reference()[0]
    cfg = UNetConfig(context_dim=1280)
    sd = make_state_dict(cfg, 0)
    m = UNetModel(**cfg.ref_kwargs()).eval()
    m.load_state_dict(sd, strict=True)
    for name, h, w in UNET_CASES:
        x, t, ctx = make_inputs(cfg, 2, h, w, seed=1, ctx_len=77)
        with torch.no_grad():
            ref = m(x, t, context=ctx)
            orc = unet_ref.unet_forward(sd, cfg, x, t, ctx)
        err = (ref - orc).abs().max().item()
        print(f'[unet {name}] |eps| max {ref.abs().max():.3f} oracle-vs-reference {err:.3e}', flush=True)
        assert err < 5e-5, err
        np.savez_compressed(os.path.join(OUT, f'unet_{name}.npz'), eps=ref.numpy().astype(np.float32), weight_seed=0,
                            input_seed=1, batch=2, h=h, w=w, ctx_len=77, context_dim=1280, t=t.numpy(),
                            eps_absmax=float(ref.abs().max()), oracle_vs_reference=err)


def config_fixture():
    import yaml
    with open(os.path.join(REF, YAML_1P4B)) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(OUT, 'txt2img_1p4B_eval.json'), 'w') as f:
        json.dump(cfg, f, indent=1)
    print('parsed', YAML_1P4B)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    config_fixture()
    bert_goldens()
    unet_goldens()
    print('LAION-400M fixtures written to', OUT)


if __name__ == '__main__':
    main()
