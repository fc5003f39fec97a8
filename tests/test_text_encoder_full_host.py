"""Host-side pieces of the full-precision text encoders (no GPU needed): the hip_precision keyword of FrozenCLIPEmbedderHIP /
BERTEmbedderHIP, the C ABI additions (sdmi_clip_create_precision, sdmi_clip_precision, sdmi_bert_create_precision, sdmi_bert_precision
and the kernel entry points), the larger workspace, the refusal of a head dim without a causal split-fp16 kernel, and the yaml route."""
import ctypes as C
import importlib
import os

import pytest
import torch

import bert_ref
from oracle import clip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text_config(cfg):
    return dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads, max_position_embeddings=cfg.max_positions)


def _clip(cfg, **kw):
    from stable_diffusion_amd import FrozenCLIPEmbedderHIP
    return FrozenCLIPEmbedderHIP(text_config=_text_config(cfg), tokenizer=object(), **kw)


def _bert(cfg, **kw):
    from stable_diffusion_amd import BERTEmbedderHIP
    return BERTEmbedderHIP(**cfg.embedder_kwargs(), use_tokenizer=False, **kw)


MAKERS = [pytest.param(lambda **kw: _clip(clip_ref.TINY_CLIP, **kw), 'sdmi_clip_precision', id='clip'),
          pytest.param(lambda **kw: _bert(bert_ref.TINY_BERT, **kw), 'sdmi_bert_precision', id='bert')]


@pytest.mark.parametrize('make,getter', MAKERS)
def test_hip_precision_keyword(make, getter):
    mixed, default, full = make(hip_precision='mixed'), make(), make(hip_precision='full')
    assert mixed.hip_precision == 'mixed' and default.hip_precision == 'mixed' and full.hip_precision == 'full'
    lib = full._handle.lib
    assert [getattr(lib, getter)(m._handle.h) for m in (mixed, default, full)] == [0, 0, 1]
    # the same state_dict keys and shapes in both modes (only the packing inside the library differs)
    assert mixed._handle.weight_specs() == full._handle.weight_specs()
    assert [(k, tuple(v.shape)) for k, v in mixed.state_dict().items()] == [(k, tuple(v.shape)) for k, v in full.state_dict().items()]
    for bad in ('half', 'FULL', None, 1):
        with pytest.raises(ValueError, match='hip_precision must be one of'):
            make(hip_precision=bad)


def test_create_precision_abi():
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.bert import make_bert_cfg
    from stable_diffusion_amd.clip import make_clip_cfg
    lib = _lib.load()
    assert lib.sdmi_abi_version() == 17
    ccfg = make_clip_cfg(_text_config(clip_ref.SD_CLIP))
    bcfg = make_bert_cfg(**bert_ref.LAION_BERT.embedder_kwargs())
    for cfg, nm in ((ccfg, 'clip'), (bcfg, 'bert')):
        create, create_p = getattr(lib, f'sdmi_{nm}_create'), getattr(lib, f'sdmi_{nm}_create_precision')
        prec, destroy = getattr(lib, f'sdmi_{nm}_precision'), getattr(lib, f'sdmi_{nm}_destroy')
        h = C.c_void_p()
        for bad in (2, -1):
            assert create_p(C.byref(cfg), bad, C.byref(h)) != 0
            err = lib.sdmi_last_error()
            assert b'precision must be SDMI_PRECISION_MIXED (0) or SDMI_PRECISION_FULL (1)' in err and str(bad).encode() in err
        for p in (0, 1):
            assert create_p(C.byref(cfg), p, C.byref(h)) == 0
            assert prec(h) == p
            destroy(h)
        assert create(C.byref(cfg), C.byref(h)) == 0          # the entry point from before the keyword: mixed
        assert prec(h) == 0
        destroy(h)
        assert prec(None) == -1
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    for name in ('sdmi_clip_create_precision', 'sdmi_clip_precision', 'sdmi_bert_create_precision', 'sdmi_bert_precision',
                 'sdmi_k_attention_split16_causal', 'sdmi_k_quick_gelu_split', 'sdmi_k_gelu_erf_split', 'sdmi_k_quick_gelu'):
        assert name in _lib.exported_symbols() and name + '(' in hdr
    assert '#define SDMI_ABI_VERSION 17' in hdr


def test_full_handles_ask_for_more_workspace():
    """the dry pass runs the full walk: hi | lo of every operand and an fp32 q | k | v buffer"""
    for mixed, full, fn in ((_clip(clip_ref.SD_CLIP), _clip(clip_ref.SD_CLIP, hip_precision='full'), 'sdmi_clip_workspace_bytes'),
                            (_clip(clip_ref.TINY_CLIP), _clip(clip_ref.TINY_CLIP, hip_precision='full'), 'sdmi_clip_workspace_bytes'),
                            (_bert(bert_ref.LAION_BERT_D2), _bert(bert_ref.LAION_BERT_D2, hip_precision='full'), 'sdmi_bert_workspace_bytes'),
                            (_bert(bert_ref.TINY_BERT), _bert(bert_ref.TINY_BERT, hip_precision='full'), 'sdmi_bert_workspace_bytes')):
        f = getattr(full._handle.lib, fn)
        wm, wf = f(mixed._handle.h, 2, 77), f(full._handle.h, 2, 77)
        assert wm > 0 and wf > wm, (fn, wm, wf)
        assert f(full._handle.h, 2, 78) == 0                  # the same shape checks as the mixed walk


def test_full_clip_refuses_a_head_dim_without_a_causal_kernel():
    from stable_diffusion_amd import _lib
    cfg40 = clip_ref.CLIPTextCfg(vocab_size=1000, hidden_size=320, intermediate_size=1280, num_layers=1, num_heads=8)
    _clip(cfg40)                                              # mixed: the causal fp16 kernel has d = 40
    with pytest.raises(_lib.SdmiError, match='head dim 40'):
        _clip(cfg40, hip_precision='full')
    assert b'causal split-fp16 attention kernel (32, 64, 128)' in _lib.load().sdmi_last_error()
    for heads in (10, 5):                                     # d = 32 and 64 of the same width are created
        _clip(clip_ref.CLIPTextCfg(vocab_size=1000, hidden_size=320, intermediate_size=1280, num_layers=1, num_heads=heads),
              hip_precision='full')


_YAML = """model:
  target: ldm.models.diffusion.ddpm.LatentDiffusion
  params:
    unet_config:
      target: ldm.modules.diffusionmodules.openaimodel.UNetModel
      params:
        in_channels: 4

    first_stage_config:
      target: ldm.models.autoencoder.AutoencoderKL
      params:
        embed_dim: 4

    cond_stage_config:
      target: {target}
      params:
        hip_precision: full
{more}"""


def _instantiate_from_config(config):
    """ldm/util.py:78-93 restated: import `target`, call it with `params`"""
    module, cls = config['target'].rsplit('.', 1)
    return getattr(importlib.import_module(module), cls)(**config.get('params', dict()))


def test_yaml_hip_precision_reaches_both_encoders(monkeypatch):
    import yaml
    from stable_diffusion_amd import BERTEmbedderHIP, FrozenCLIPEmbedderHIP, clip
    monkeypatch.setattr(clip, 'CLIP_VIT_L14_TEXT', _text_config(clip_ref.TINY_CLIP))     # (the keyword route, not 123M zeros)
    import transformers
    monkeypatch.setattr(transformers.CLIPTokenizer, 'from_pretrained', classmethod(lambda cls, *a, **k: object()))
    text = _YAML.format(target='stable_diffusion_amd.clip.FrozenCLIPEmbedderHIP', more='')
    m = _instantiate_from_config(yaml.safe_load(text)['model']['params']['cond_stage_config'])
    assert isinstance(m, FrozenCLIPEmbedderHIP) and m.hip_precision == 'full' and m._handle.lib.sdmi_clip_precision(m._handle.h) == 1
    text = _YAML.format(target='stable_diffusion_amd.bert.BERTEmbedderHIP',
                        more='        n_embed: 128\n        n_layer: 2\n        use_tokenizer: false\n')
    m = _instantiate_from_config(yaml.safe_load(text)['model']['params']['cond_stage_config'])
    assert isinstance(m, BERTEmbedderHIP) and m.hip_precision == 'full' and m._handle.lib.sdmi_bert_precision(m._handle.h) == 1
    # without the key: mixed
    cfg = yaml.safe_load(text)['model']['params']['cond_stage_config']
    del cfg['params']['hip_precision']
    assert _instantiate_from_config(cfg).hip_precision == 'mixed'


def test_launcher_target_swap_keeps_the_key():
    """tools/run_reference_script.py swaps the three `target:` strings by plain text replacement: a `hip_precision: full` that the
    user's yaml carries under cond_stage_config.params stays where it is, and the UNet / first-stage switches do not touch it"""
    import yaml
    spec = importlib.util.spec_from_file_location('rrs', os.path.join(ROOT, 'tools', 'run_reference_script.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    src = open(os.path.join(ROOT, 'tools', 'run_reference_script.py')).read()
    assert "text = text.replace(old_clip, 'target: stable_diffusion_amd.clip.FrozenCLIPEmbedderHIP')" in src
    assert "text = text.replace(f'target: {old}\\n', f'target: {new}\\n')" in src
    assert m.HIP_TARGETS['ldm.modules.encoders.modules.BERTEmbedder'] == 'stable_diffusion_amd.bert.BERTEmbedderHIP'
    for ref_target, hip_target in (('ldm.modules.encoders.modules.FrozenCLIPEmbedder', 'stable_diffusion_amd.clip.FrozenCLIPEmbedderHIP'),
                                   ('ldm.modules.encoders.modules.BERTEmbedder', 'stable_diffusion_amd.bert.BERTEmbedderHIP')):
        text = _YAML.format(target=ref_target, more='        n_embed: 1280\n')
        for old, new in ((ref_target, hip_target), ('ldm.models.autoencoder.AutoencoderKL', 'stable_diffusion_amd.vae.AutoencoderKLHIP'),
                         ('ldm.modules.diffusionmodules.openaimodel.UNetModel', 'stable_diffusion_amd.unet.UNetModelHIP')):
            text = text.replace(f'target: {old}\n', f'target: {new}\n')
        text = m.add_first_stage_precision(m.add_hip_precision(text, 'mixed'), 'mixed')
        cfg = yaml.safe_load(text)['model']['params']
        assert cfg['cond_stage_config'] == {'target': hip_target, 'params': {'hip_precision': 'full', 'n_embed': 1280}}
        assert cfg['unet_config']['params']['hip_precision'] == 'mixed' and cfg['first_stage_config']['params']['hip_precision'] == 'mixed'
