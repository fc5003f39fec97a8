"""Host-side checks of the LAION-400M model's text encoder and its plumbing (no GPU): parameter names and shapes against the
reference module's state_dict, the CPU restatement against the reference goldens, the patched 1p4B config of the launcher,
the synthetic LAION checkpoint's keys, and the library's refusal of configurations its kernels cannot run."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import yaml

import bert_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launcher():
    spec = importlib.util.spec_from_file_location('run_reference_script', os.path.join(ROOT, 'tools', 'run_reference_script.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_registered_parameters_equal_reference_state_dict(golden_dir):
    from stable_diffusion_amd import BERTEmbedderHIP
    want = json.load(open(os.path.join(golden_dir, 'bert_state_dict_keys.json')))['keys']
    m = BERTEmbedderHIP(n_embed=1280, n_layer=32, use_tokenizer=False)
    got = [[k[len('transformer.'):], list(v.shape)] for k, v in m.state_dict().items()]
    assert got == want
    assert [[k, list(s)] for k, s, _ in bert_ref.bert_param_specs(bert_ref.LAION_BERT)] == want


@pytest.mark.parametrize('case', ['tiny_b2', 'tiny_b3_L40', 'laion_d2_b2'])
def test_restatement_reproduces_reference_golden(case, golden_dir):
    z = np.load(os.path.join(golden_dir, f'bert_{case}.npz'))
    cfg = bert_ref.CFGS[str(z['cfg'])]
    sd = bert_ref.make_bert_state_dict(cfg, int(z['weight_seed']))
    ids = bert_ref.make_bert_ids(cfg, int(z['batch']), int(z['L']), seed=int(z['input_seed']))
    out = bert_ref.bert_forward(sd, cfg, ids)
    err = (out - torch.from_numpy(z['out'])).abs().max().item()
    assert out.shape == tuple(z['out'].shape) and err <= 5e-5, err


def _diff(a, b, path=''):
    if isinstance(a, dict) and isinstance(b, dict):
        out = []
        for k in sorted(set(a) | set(b)):
            out += _diff(a.get(k), b.get(k), f'{path}.{k}' if path else k)
        return out
    return [] if a == b else [(path, a, b)]


def test_patched_1p4B_config_changes_exactly_the_three_targets(golden_dir):
    fixture = json.load(open(os.path.join(golden_dir, 'txt2img_1p4B_eval.json')))
    patched = yaml.safe_load(_launcher().laion_hip_yaml_text('/nonexistent-reference'))
    p = 'model.params.'
    assert sorted(_diff(fixture, patched)) == sorted([
        (p + 'cond_stage_config.target', 'ldm.modules.encoders.modules.BERTEmbedder', 'stable_diffusion_amd.bert.BERTEmbedderHIP'),
        (p + 'first_stage_config.target', 'ldm.models.autoencoder.AutoencoderKL', 'stable_diffusion_amd.vae.AutoencoderKLHIP'),
        (p + 'unet_config.target', 'ldm.modules.diffusionmodules.openaimodel.UNetModel', 'stable_diffusion_amd.unet.UNetModelHIP')])
    assert fixture['model']['params']['unet_config']['params']['context_dim'] == 1280
    assert fixture['model']['params']['cond_stage_config']['params'] == {'n_embed': 1280, 'n_layer': 32}


def test_synthetic_laion_checkpoint_keys_are_what_the_hip_modules_expect(golden_dir):
    from stable_diffusion_amd import AutoencoderKLHIP, BERTEmbedderHIP, UNetModelHIP
    cfg = json.load(open(os.path.join(golden_dir, 'txt2img_1p4B_eval.json')))['model']['params']
    sd = _launcher().synthetic_laion_state_dict(0)
    unet = UNetModelHIP(**cfg['unet_config']['params'])
    fs = cfg['first_stage_config']['params']
    vae = AutoencoderKLHIP(fs['ddconfig'], None, fs['embed_dim'])
    bert = BERTEmbedderHIP(**cfg['cond_stage_config']['params'], use_tokenizer=False)
    want = {}
    for prefix, mod in (('model.diffusion_model.', unet), ('first_stage_model.', vae), ('cond_stage_model.', bert)):
        want.update({prefix + k: tuple(v.shape) for k, v in mod.state_dict().items()})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sd['model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight'].shape == (320, 1280)


@pytest.mark.parametrize('field,value,msg', [('dim', 1000, 'multiple of 64'), ('ff_inner', 100, 'multiple of 64'),
                                             ('dim_head', 48, 'dim_head'), ('depth', 0, 'bad BERT config')])
def test_bert_create_refuses_bad_config(field, value, msg):
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.bert import make_bert_cfg
    lib = _lib.load()
    cfg = make_bert_cfg(1280, 2)
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.sdmi_bert_create(C.byref(cfg), C.byref(h)) != 0
    assert msg in lib.sdmi_last_error().decode()


def test_bert_workspace_refuses_long_sequences_and_big_batches():
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.bert import _BertHandle, make_bert_cfg
    hd = _BertHandle(make_bert_cfg(128, 2, vocab_size=1000))
    lib = hd.lib
    assert lib.sdmi_bert_workspace_bytes(hd.h, 2, 77) > 0
    assert lib.sdmi_bert_workspace_bytes(hd.h, 2, 78) == 0
    assert 'max_seq_len' in lib.sdmi_last_error().decode()
    assert lib.sdmi_bert_workspace_bytes(hd.h, 65, 77) == 0
    assert 'batch' in lib.sdmi_last_error().decode()
    assert lib.sdmi_bert_finalize(hd.h) != 0 and 'weight not set' in lib.sdmi_last_error().decode()
    _ = _lib
