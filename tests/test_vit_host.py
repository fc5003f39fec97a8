"""CPU: host side of the CLIP image encoder -- the module mirrors' state-dict keys against transformers' own (tests/golden/vit_state_dict_keys.json,
tools/make_golden_vit.py), the OpenAI-`clip` naming converter, the refusals, the additive C ABI, the workspace query, and the fp64 statement of the
safety checker's concept head (tests/vit_ref.py) against hand-computed cases."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import vit_ref
from stable_diffusion_amd import _lib, synthetic, vision

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['sdmi_vit_create', 'sdmi_vit_destroy', 'sdmi_vit_num_weights', 'sdmi_vit_weight_info', 'sdmi_vit_set_weight', 'sdmi_vit_finalize',
               'sdmi_vit_workspace_bytes', 'sdmi_vit_forward', 'sdmi_k_vit_patchify', 'sdmi_k_vit_embed', 'sdmi_k_vit_preprocess',
               'sdmi_k_safety_head']


@pytest.fixture(scope='module')
def keys(golden_dir):
    with open(os.path.join(golden_dir, 'vit_state_dict_keys.json')) as f:
        return json.load(f)


def _shapes(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def test_vision_tower_state_dict_is_transformers(keys):
    assert keys['config'] == synthetic.VIT_TINY
    assert _shapes(vision.CLIPVisionHIP(synthetic.VIT_TINY)) == keys['vision']


def test_safety_checker_state_dict_is_the_shipped_checkers(keys):
    m = vision.StableDiffusionSafetyCheckerHIP(synthetic.VIT_TINY)
    assert _shapes(m) == keys['safety_checker']
    sd = {k: torch.full(tuple(s), 0.25) for k, s in keys['safety_checker'].items()}
    sd['vision_model.vision_model.embeddings.position_ids'] = torch.arange(5)[None]      # (older checkpoints carry the buffer)
    assert m.load_state_dict(sd, strict=True) is not None
    assert float(m.vision_model.vision_model.pre_layrnorm.weight[0]) == 0.25 and float(m.concept_embeds_weights[3]) == 0.25
    # the tower the forward runs sees the same tensors
    assert dict(m._tower[0].named_parameters())['vision_model.pre_layrnorm.weight'] is m.vision_model.vision_model.pre_layrnorm.weight


def test_full_size_defaults_are_vit_l14():
    specs = dict(vision._VitHandle(vision.make_vit_cfg(vision.CLIP_VIT_L14_VISION)).weight_specs())
    assert specs['vision_model.embeddings.patch_embedding.weight'] == (1024, 3, 14, 14)
    assert specs['vision_model.embeddings.position_embedding.weight'] == (257, 1024)
    assert specs['visual_projection.weight'] == (768, 1024)
    assert sum(k.startswith('vision_model.encoder.layers.') for k in specs) == 24 * 16
    assert sum(int(np.prod(s)) for s in specs.values()) == 303_179_776 + 768 * 1024        # CLIPVisionModel's parameters + the projection


def test_openai_naming_round_trips_keys_and_shapes(keys):
    hf = {k: torch.zeros(tuple(s)) for k, s in keys['vision'].items()}
    oa = vision.transformers_to_openai_clip(hf)
    C_, I, Pd = synthetic.VIT_TINY['hidden_size'], synthetic.VIT_TINY['intermediate_size'], synthetic.VIT_TINY['projection_dim']
    expect = {'visual.conv1.weight': (C_, 3, 14, 14), 'visual.class_embedding': (C_,), 'visual.positional_embedding': (5, C_),
              'visual.ln_pre.weight': (C_,), 'visual.ln_pre.bias': (C_,), 'visual.ln_post.weight': (C_,), 'visual.ln_post.bias': (C_,),
              'visual.proj': (C_, Pd)}
    for n in range(synthetic.VIT_TINY['num_hidden_layers']):
        p = f'visual.transformer.resblocks.{n}.'
        expect.update({p + 'attn.in_proj_weight': (3 * C_, C_), p + 'attn.in_proj_bias': (3 * C_,), p + 'attn.out_proj.weight': (C_, C_),
                       p + 'attn.out_proj.bias': (C_,), p + 'ln_1.weight': (C_,), p + 'ln_1.bias': (C_,), p + 'ln_2.weight': (C_,),
                       p + 'ln_2.bias': (C_,), p + 'mlp.c_fc.weight': (I, C_), p + 'mlp.c_fc.bias': (I,), p + 'mlp.c_proj.weight': (C_, I),
                       p + 'mlp.c_proj.bias': (C_,)})
    assert {k: tuple(v.shape) for k, v in oa.items()} == expect
    back = vision.openai_clip_to_transformers(dict(oa, **{'transformer.resblocks.0.ln_1.weight': torch.zeros(3), 'logit_scale': torch.zeros(())}))
    assert {k: list(v.shape) for k, v in back.items()} == keys['vision']
    # values: q | k | v are the thirds of in_proj in that order, the projection is transposed
    g = torch.Generator().manual_seed(0)
    oa = {k: torch.randn(v.shape, generator=g) for k, v in oa.items()}
    back = vision.openai_clip_to_transformers(oa)
    assert torch.equal(back['vision_model.encoder.layers.1.self_attn.k_proj.weight'], oa['visual.transformer.resblocks.1.attn.in_proj_weight'][C_:2 * C_])
    assert torch.equal(back['vision_model.encoder.layers.0.self_attn.v_proj.bias'], oa['visual.transformer.resblocks.0.attn.in_proj_bias'][2 * C_:])
    assert torch.equal(back['visual_projection.weight'], oa['visual.proj'].t())
    # the embedder takes either naming (and the reference module's own `model.visual.*`)
    emb = vision.FrozenClipImageEmbedderHIP(synthetic.VIT_TINY)
    emb.load_state_dict({'model.' + k: v for k, v in oa.items()}, strict=True)
    assert torch.equal(emb.model.visual_projection.weight, oa['visual.proj'].t())
    emb.load_state_dict({'model.' + k: v for k, v in back.items()}, strict=True)
    with pytest.raises(KeyError, match='unexpected OpenAI-clip key'):
        vision.openai_clip_to_transformers({'visual.transformer.resblocks.0.attn.bias_k': torch.zeros(1)})


def _create(**over):
    cfg = vision.make_vit_cfg(dict(synthetic.VIT_TINY, **over))
    h = C.c_void_p()
    lib = _lib.load()
    rc = lib.sdmi_vit_create(C.byref(cfg), C.byref(h))
    msg = lib.sdmi_last_error().decode()
    if rc == 0:
        lib.sdmi_vit_destroy(h)
    return rc, msg


REFUSALS = [(dict(hidden_size=96, num_attention_heads=3), 'hidden_size 96'), (dict(intermediate_size=160), 'intermediate_size 160'),
            (dict(hidden_size=192, num_attention_heads=8), 'head dim 24'), (dict(hidden_size=192, num_attention_heads=2), 'head dim 96'),
            (dict(image_size=30), r'image_size % patch_size != 0'), (dict(image_size=14 * 32), 'more than 1024 tokens')]


@pytest.mark.parametrize('over,name', REFUSALS, ids=[r[1].split(' ')[0] + str(i) for i, r in enumerate(REFUSALS)])
def test_refusals_at_creation_name_what_they_refuse(over, name):
    rc, msg = _create(**over)
    assert rc != 0 and re.search(name, msg), msg
    with pytest.raises(_lib.SdmiError, match=name):
        vision.CLIPVisionHIP(dict(synthetic.VIT_TINY, **over))


def test_accepted_edges_and_the_other_refusals():
    assert _create()[0] == 0
    assert _create(image_size=14 * 31)[0] == 0                                         # 962 tokens
    assert _create(hidden_size=128, num_attention_heads=2)[0] == 0                      # d = 64
    m = vision.CLIPVisionHIP(synthetic.VIT_TINY)
    lib = _lib.load()
    assert lib.sdmi_vit_workspace_bytes(m._handle.h, 65) == 0 and 'B > 64' in lib.sdmi_last_error().decode()
    assert lib.sdmi_vit_workspace_bytes(m._handle.h, 0) == 0
    for cls in (vision.CLIPVisionHIP, vision.StableDiffusionSafetyCheckerHIP):
        with pytest.raises(NotImplementedError, match="hip_precision='full'"):
            cls(synthetic.VIT_TINY, hip_precision='full')
    with pytest.raises(NotImplementedError, match="hip_precision='full'"):
        vision.FrozenClipImageEmbedderHIP(synthetic.VIT_TINY, hip_precision='full')
    with pytest.raises(NotImplementedError, match='antialias=True'):
        vision.FrozenClipImageEmbedderHIP(synthetic.VIT_TINY, antialias=True)
    with pytest.raises(NotImplementedError, match='quick_gelu'):
        vision.CLIPVisionHIP(dict(synthetic.VIT_TINY, hidden_act='gelu'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(torch.zeros(1, 3, 28, 28))
    with pytest.raises(FileNotFoundError, match='local'):
        vision.StableDiffusionSafetyCheckerHIP.from_pretrained('CompVis/stable-diffusion-safety-checker')


def test_abi_is_additive():
    lib = _lib.load()
    assert lib.sdmi_abi_version() == 17
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.exported_symbols() and name + '(' in hdr and hasattr(lib, name)
    assert C.sizeof(_lib.VitCfg) == 28 and [f[0] for f in _lib.VitCfg._fields_] == re.findall(
        r'int32_t (\w+);', hdr[hdr.index('typedef struct sdmi_vit_cfg'):hdr.index('} sdmi_vit_cfg;')])
    assert C.sizeof(_lib.ClipCfg) == 24 and C.sizeof(_lib.BertCfg) == 28
    assert lib.sdmi_k_vit_kpad(14) == 640 and lib.sdmi_k_vit_kpad(16) == 768 and lib.sdmi_k_vit_kpad(32) == 3072


def test_workspace_is_positive_and_monotone_in_batch():
    for cfg in (synthetic.VIT_TINY, synthetic.VIT_L14_THIN):
        m = vision.CLIPVisionHIP(cfg)
        need = [_lib.load().sdmi_vit_workspace_bytes(m._handle.h, B) for B in (1, 2, 3, 8, 64)]
        assert need[0] > 0 and all(a < b for a, b in zip(need, need[1:])), need


def test_from_pretrained_reads_a_local_directory_only(tmp_path):
    ref = vision.StableDiffusionSafetyCheckerHIP(synthetic.VIT_TINY)
    sd = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(i)) for i, (k, v) in enumerate(ref.state_dict().items())}
    torch.save(sd, tmp_path / 'pytorch_model.bin')
    vc = {k: v for k, v in synthetic.VIT_TINY.items() if k != 'projection_dim'}
    (tmp_path / 'config.json').write_text(json.dumps(dict(projection_dim=synthetic.VIT_TINY['projection_dim'], vision_config=vc)))
    m = vision.StableDiffusionSafetyCheckerHIP.from_pretrained(str(tmp_path))
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items()) and set(m.state_dict()) == set(sd)


# ---- the concept head, fp64 ------------------------------------------------------------------------------------------------------------------
def _unit(c):
    """a unit vector at cosine c to e0"""
    return np.array([c, np.sqrt(1.0 - c * c), 0.0, 0.0])


def test_round3_is_half_to_even():
    got = vit_ref.round3([0.0005, 0.0015, 0.0025, -0.0005, -0.0015, 0.00049, 0.00051, 0.0204, -0.0196])
    assert got.tolist() == [0.0, 0.002, 0.002, -0.0, -0.002, 0.0, 0.001, 0.02, -0.02]


def test_safety_head_reference_on_hand_computed_cases():
    img = np.array([[3.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0]])                       # (normalisation: lengths 3 and 2)
    # image 0 sees cosines 0.5, 0.3, 0.8; image 1 sees sqrt(0.75), sqrt(0.91), 0.6
    concepts = np.stack([_unit(0.5) * 7.0, _unit(0.3), _unit(0.8) * 0.1])
    thr = np.array([0.48, 0.3004, 0.9])
    has, cs, ss, raw_c, _ = vit_ref.safety_head(img, concepts, np.zeros((0, 4)), thr, np.zeros(0))
    assert np.allclose(raw_c[0], [0.02, -0.0004, -0.1], atol=1e-12)
    assert cs[0].tolist() == [0.02, -0.0, -0.1] and has.tolist() == [True, True]
    assert np.allclose(cs[1], [round(np.sqrt(0.75) - 0.48, 3), round(np.sqrt(0.91) - 0.3004, 3), -0.3], atol=1e-12)
    # +0.0003 rounds to 0 (not flagged), +0.0007 rounds to 0.001 (flagged)
    for off, flagged, score in ((0.0003, False, 0.0), (0.0007, True, 0.001), (-0.02, False, -0.02)):
        has, cs, _, _, _ = vit_ref.safety_head(img[:1], _unit(0.5)[None], np.zeros((0, 4)), [0.5 - off], [])
        assert has.tolist() == [flagged] and cs.tolist() == [[score]]
    # the adjustment: a special-care concept 0.02 over its threshold lifts a concept at -0.005 to +0.005
    special, sthr = np.stack([_unit(0.2), _unit(0.6)]), np.array([0.5, 0.58])
    has, cs, ss, raw_c, raw_s = vit_ref.safety_head(img[:1], _unit(0.5)[None], special, [0.505], sthr)
    assert ss.tolist() == [[-0.3, 0.02]] and cs.tolist() == [[0.005]] and has.tolist() == [True]
    assert np.allclose(raw_c, [[0.005]], atol=1e-12)
    has, cs, ss, _, _ = vit_ref.safety_head(img[:1], _unit(0.5)[None], special, [0.505], [0.5, 0.62])
    assert ss.tolist() == [[-0.3, -0.02]] and cs.tolist() == [[-0.005]] and has.tolist() == [False]
    # a raised adjustment also reaches the LATER special-care concepts, in index order
    has, cs, ss, _, _ = vit_ref.safety_head(img[:1], _unit(0.5)[None], special[::-1], [0.52], [0.58, 0.205])
    assert ss.tolist() == [[0.02, 0.005]] and cs.tolist() == [[-0.01]] and has.tolist() == [False]
    assert np.allclose(vit_ref.boundary_distance([0.0003, 0.0007, 0.02, -0.0196, 0.0005]), [0.0002, 0.0002, 0.0005, 0.0001, 0.0], atol=1e-12)
