"""The semantic-synthesis models, host side (no GPU): both parsed yamls (tests/golden/semantic_synthesis*_config.json,
tools/make_golden_semantic.py) build the UNet and the pipeline, the state-dict keys are the reference modules', every refusal of
SpatialRescalerHIP names its argument, the size rule of `synthesize` names the nearest sizes, and the header declares the two additive
entries at ABI 17."""
import json
import os
import re

import pytest
import torch

from stable_diffusion_amd import (SemanticSynthesisHIP, SpatialRescalerHIP, SuperResolutionHIP, UNetModelHIP, _lib, semantic,
                                  synthetic)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ('semantic_synthesis256', 'semantic_synthesis512')


def _config(golden_dir, name):
    with open(os.path.join(golden_dir, f'{name}_config.json')) as f:
        return json.load(f)


@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test"""
    def load():
        raise AssertionError('a refused call reached the library')
    monkeypatch.setattr(_lib, 'load', load)


@pytest.mark.parametrize('prec', ['mixed', 'full'])
@pytest.mark.parametrize('name', CONFIGS)
def test_unet_builds_from_the_yaml_with_the_reference_keys(name, prec, golden_dir):
    params = _config(golden_dir, name)['model']['params']['unet_config']['params']
    assert dict(params, image_size=128) == synthetic.SEMANTIC_UNET_KWARGS
    m = UNetModelHIP(**params, hip_precision=prec)
    with open(os.path.join(golden_dir, 'semantic_unet_state_dict_keys.json')) as f:
        ref = json.load(f)
    got = [(k, list(v.shape)) for k, v in m.state_dict().items()]
    assert len(got) == 216 and sum(v.numel() for v in m.state_dict().values()) == ref['n_params'] == 215229315
    assert sorted(got) == sorted((k, list(s)) for k, s in ref['keys'])


@pytest.mark.parametrize('name', CONFIGS)
def test_pipeline_builds_from_the_yaml(name, golden_dir):
    cfg = _config(golden_dir, name)
    fs = cfg['model']['params']['first_stage_config']['params']
    assert dict(embed_dim=fs['embed_dim'], n_embed=fs['n_embed'], ddconfig=dict(fs['ddconfig'])) == semantic.SEMANTIC_VQ_KWARGS == synthetic.FACES_VQ_KWARGS
    assert dict(cfg['model']['params']['cond_stage_config']['params']) == synthetic.SEMANTIC_RESCALER_KWARGS
    m = SemanticSynthesisHIP.from_config(cfg)
    assert m.model.conditioning_key == 'concat' and m.cond_stage_key == 'segmentation' and m.scale_factor == 1.0 and m.num_timesteps == 1000
    assert not hasattr(m, 'split_input_params')                       # (tiling is not built for this model)
    assert m.model.diffusion_model.in_channels == 6 and m.model.diffusion_model.out_channels == 3
    assert abs(float(m.betas[0]) - 0.0015) < 1e-9 and abs(float(m.betas[-1]) - 0.0205) < 1e-8
    assert (float(m.betas[0]), float(m.betas[-1])) == tuple(float(v) for v in SemanticSynthesisHIP().betas[[0, -1]])
    r = m.cond_stage_model
    assert isinstance(r, SpatialRescalerHIP) and (r.n_stages, r.in_channels, r.out_channels) == (2, 182, 3)
    sd = m.state_dict()
    assert [k for k in sd if k.startswith('cond_stage_model.')] == ['cond_stage_model.channel_mapper.weight']
    assert tuple(sd['cond_stage_model.channel_mapper.weight'].shape) == (3, 182, 1, 1)
    assert any(k.startswith('first_stage_model.decoder.') for k in sd) and any(k.startswith('model.diffusion_model.') for k in sd)


def test_rescaler_state_dict_keys():
    assert list(SpatialRescalerHIP(**synthetic.SEMANTIC_RESCALER_KWARGS).state_dict()) == ['channel_mapper.weight']
    sd = SpatialRescalerHIP(**synthetic.SEMANTIC_RESCALER_KWARGS, bias=True).state_dict()
    assert list(sd) == ['channel_mapper.weight', 'channel_mapper.bias'] and tuple(sd['channel_mapper.bias'].shape) == (3,)
    assert list(SpatialRescalerHIP(n_stages=2, in_channels=7).state_dict()) == []
    d = SpatialRescalerHIP()                                           # the reference's defaults
    assert (d.n_stages, d.method, d.multiplier, d.in_channels, d.out_channels, d.remap_output) == (1, 'bilinear', 0.5, 3, None, False)


@pytest.mark.parametrize('kwargs,arg', [(dict(method='nearest'), 'method'), (dict(method='area'), 'method'), (dict(multiplier=0.25), 'multiplier'),
                                        (dict(multiplier=2), 'multiplier'), (dict(n_stages=3), 'n_stages'),
                                        (dict(in_channels=182, out_channels=9), 'out_channels')])
def test_rescaler_refusals_name_their_argument(kwargs, arg, no_library):
    with pytest.raises(NotImplementedError, match=arg + '='):
        SpatialRescalerHIP(**kwargs)


def test_rescaler_refuses_cpu_tensors_and_bad_inputs(no_library):
    r = SpatialRescalerHIP(**synthetic.SEMANTIC_RESCALER_KWARGS)
    with pytest.raises(RuntimeError, match='device tensor only'):
        r.encode(torch.zeros(1, 182, 8, 8))
    with pytest.raises(RuntimeError, match='device tensor only'):
        r.encode_labels(torch.zeros(1, 8, 8, dtype=torch.int64))


def test_from_config_refuses_other_models(golden_dir):
    with open(os.path.join(golden_dir, 'bsr_sr_config.json')) as f:
        bsr = json.load(f)
    with pytest.raises(NotImplementedError, match='segmentation'):
        SemanticSynthesisHIP.from_config(bsr)
    cfg = _config(golden_dir, 'semantic_synthesis512')
    for edit in (lambda p: p.update(concat_mode=False), lambda p: p.update(cond_stage_key='LR_image'),
                 lambda p: p.update(cond_stage_config='__is_unconditional__'),
                 lambda p: p['cond_stage_config'].update(target='torch.nn.Identity')):
        c = json.loads(json.dumps(cfg))
        edit(c['model']['params'])
        with pytest.raises(NotImplementedError, match='SpatialRescaler'):
            SemanticSynthesisHIP.from_config(c)
    with pytest.raises(NotImplementedError, match='LR_image'):
        SuperResolutionHIP.from_config(cfg)                            # (and bsr_sr's class still refuses this one)


def test_synthesize_size_rule_names_the_nearest_sizes(monkeypatch):
    m = SemanticSynthesisHIP()

    def load():
        raise AssertionError('a refused size reached the library')
    monkeypatch.setattr(_lib, 'load', load)
    with pytest.raises(ValueError, match=r'height 192 or 208, width 304 or 320'):
        m.synthesize(labels=torch.zeros(1, 200, 310, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'height 16, width 256'):
        m.synthesize(segmentation=torch.zeros(1, 182, 8, 256))
    with pytest.raises(ValueError, match='exactly one'):
        m.synthesize()
    with pytest.raises(ValueError, match='exactly one'):
        m.synthesize(segmentation=torch.zeros(1, 182, 16, 16), labels=torch.zeros(1, 16, 16, dtype=torch.int64))
    assert semantic.nearest_valid_sizes(512) == (512, 512) and semantic.nearest_valid_sizes(513) == (512, 528)
    assert semantic.nearest_valid_sizes(8) == (None, 16)
    SemanticSynthesisHIP.check_size(512, 1024)


def test_header_declares_both_entries_at_abi_17():
    with open(os.path.join(ROOT, 'include', 'sdmi.h')) as f:
        h = f.read()
    assert re.search(r'#define SDMI_ABI_VERSION 17\b', h)
    flat = ' '.join(h.split())
    assert ('int sdmi_k_spatial_rescale(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, '
            'int n_stages, int Cout, void* stream);') in flat
    assert ('int sdmi_k_spatial_rescale_labels(const int32_t* labels, const float* w, const float* bias, float* out, int B, int Cin, int H, '
            'int W, int n_stages, int Cout, void* stream);') in flat
    assert {'sdmi_k_spatial_rescale', 'sdmi_k_spatial_rescale_labels'} <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert lib.sdmi_k_spatial_rescale and lib.sdmi_k_spatial_rescale_labels
