"""The class-conditional ImageNet model (configs/latent-diffusion/cin256-v2.yaml) on the host: UNetModelHIP constructs from the
yaml's own parameters (num_heads=1, legacy left at True) and exposes exactly the reference UNetModel's state_dict keys and shapes
(fixtures of tools/make_golden_cin.py); the combinations outside the families are still refused by name; ClassEmbedderHIP; the
schedule; the C ABI did not move.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from stable_diffusion_amd import synthetic


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _params(golden_dir):
    return _load(golden_dir, 'cin256_v2_config.json')['model']['params']


def test_config_fixture_matches_the_constants(golden_dir):
    p = _params(golden_dir)
    assert p['unet_config']['params'] == synthetic.CIN_UNET_KWARGS
    assert 'legacy' not in p['unet_config']['params'] and p['unet_config']['params']['num_heads'] == 1
    fs = p['first_stage_config']['params']
    assert {k: fs[k] for k in ('embed_dim', 'n_embed', 'ddconfig')} == synthetic.CIN_VQ_KWARGS
    assert 'attn_type' not in fs['ddconfig']                      # mid-block attention on
    assert p['cond_stage_config']['params'] == synthetic.CIN_CLASS_KWARGS
    assert p['conditioning_key'] == 'crossattn'
    assert {k: p[k] for k in ('timesteps', 'linear_start', 'linear_end')} == synthetic.CIN_SCHEDULE
    assert (p['linear_start'], p['linear_end']) == (0.0015, 0.0195)


def test_cin_unet_state_dict_equals_reference(golden_dir):
    from stable_diffusion_amd import UNetModelHIP
    m = UNetModelHIP(**_params(golden_dir)['unet_config']['params'])
    mine = sorted((k, list(v.shape)) for k, v in m.state_dict().items())
    ref = sorted((k, list(s)) for k, s in _load(golden_dir, 'cin_unet_state_dict_keys.json')['keys'])
    assert mine == ref
    assert len(mine) == 688
    assert round(sum(v.numel() for v in m.state_dict().values()) / 1e6, 1) == 400.9
    # attn2.to_q / to_k are enumerated although a one-token context never reads them (the checkpoint has them)
    keys = dict(mine)
    assert keys['middle_block.1.transformer_blocks.0.attn2.to_q.weight'] == [960, 960]
    assert keys['middle_block.1.transformer_blocks.0.attn2.to_k.weight'] == [960, 512]
    assert m._handle.lib.sdmi_unet_workspace_bytes(m._handle.h, 8, 64, 64, 1) > 0


def test_cin_vq_constructs_with_mid_block_attention(golden_dir):
    from stable_diffusion_amd import VQModelInterfaceHIP
    m = VQModelInterfaceHIP(**synthetic.CIN_VQ_KWARGS)
    mine = sorted((k, list(v.shape)) for k, v in m.state_dict().items())
    ref = sorted((k, list(s)) for k, s in _load(golden_dir, 'cin_vq_state_dict_keys.json')['keys'])
    assert mine == ref
    assert any(k.startswith('decoder.mid.attn_1.') for k, _ in mine) and any(k.startswith('encoder.mid.attn_1.') for k, _ in mine)


@pytest.mark.parametrize('bad,name', [(dict(num_head_channels=64), 'num_head_channels'), (dict(num_heads=-1, num_head_channels=64), 'num_head_channels'),
                                      (dict(use_scale_shift_norm=True), 'scale-shift'), (dict(resblock_updown=True), 'resblock_updown'),
                                      (dict(num_classes=1000), 'class conditioning'), (dict(context_dim=None), 'context_dim'),
                                      (dict(dropout=0.1), 'dropout'), (dict(dims=1), 'dims'), (dict(num_heads_upsample=2), 'num_heads_upsample'),
                                      (dict(hip_precision='full'), '160')])
def test_cin_unet_still_refuses_by_name(bad, name):
    from stable_diffusion_amd import UNetModelHIP
    with pytest.raises(NotImplementedError, match=name):
        UNetModelHIP(**dict(synthetic.CIN_UNET_KWARGS, **bad))


def test_legacy_flag_is_accepted_either_way_for_num_heads():
    from oracle.plan import TINY
    from stable_diffusion_amd import UNetModelHIP
    a = UNetModelHIP(**dict(TINY.ref_kwargs(), legacy=True))
    b = UNetModelHIP(**dict(TINY.ref_kwargs(), legacy=False))
    assert [(k, v.shape) for k, v in a.state_dict().items()] == [(k, v.shape) for k, v in b.state_dict().items()]
    UNetModelHIP(**dict(TINY.ref_kwargs(), hip_precision='full'))          # (narrow heads: full precision as before)


def test_library_refuses_full_precision_wide_heads():
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.unet import PRECISIONS, make_cfg
    k = synthetic.CIN_UNET_KWARGS
    cfg = make_cfg(k['in_channels'], k['out_channels'], k['model_channels'], k['num_res_blocks'], k['channel_mult'],
                   k['attention_resolutions'], k['num_heads'], k['transformer_depth'], k['context_dim'])
    h = C.c_void_p()
    assert _lib.load().sdmi_unet_create_with_precision(C.byref(cfg), PRECISIONS['full'], C.byref(h)) != 0
    assert b'has no full-precision kernel' in _lib.load().sdmi_last_error()


def test_class_embedder_is_an_embedding_lookup():
    from stable_diffusion_amd import ClassEmbedderHIP
    m = ClassEmbedderHIP(**synthetic.CIN_CLASS_KWARGS)
    assert list(m.state_dict()) == ['embedding.weight'] and tuple(m.embedding.weight.shape) == (1001, 512)
    m.load_state_dict(synthetic.synthetic_named_state_dict([('embedding.weight', (1001, 512))], 0), strict=True)
    ids = torch.tensor([25, 992, 1000, 0])
    ref = torch.nn.Embedding(1001, 512)
    ref.load_state_dict(m.embedding.state_dict())
    with torch.no_grad():
        c = m({'class_label': ids})
        assert c.shape == (4, 1, 512)
        assert torch.equal(c, ref(ids)[:, None])
        assert torch.equal(m({'other': ids}, key='other'), c)
    assert ClassEmbedderHIP(8).key == 'class' and tuple(ClassEmbedderHIP(8).embedding.weight.shape) == (1000, 8)
    assert 0.9 < float(c.std()) < 1.1                               # the seeded table is N(0, 1) like nn.Embedding's own init


def test_schedule_equals_register_schedule(golden_dir):
    from stable_diffusion_amd import LatentDiffusionHIP
    ld = LatentDiffusionHIP(torch.nn.Identity(), **synthetic.CIN_SCHEDULE)
    z = np.load(os.path.join(golden_dir, 'cin_schedule.npz'))
    for k in ('betas', 'alphas_cumprod', 'alphas_cumprod_prev'):
        assert torch.equal(getattr(ld, k), torch.tensor(z[k])), k
    assert ld.model.conditioning_key == 'crossattn' and ld.num_timesteps == 1000


def test_abi_and_struct_layouts_unchanged():
    from stable_diffusion_amd import _lib
    assert _lib.load().sdmi_abi_version() == 17
    assert C.sizeof(_lib.UNetCfg) == 100 and C.sizeof(_lib.UNetExt) == 8 and C.sizeof(_lib.VaeCfg) == 60 and C.sizeof(_lib.VaeExt) == 12
    assert _lib._SIGS['sdmi_k_attention'][1] == [_lib.c_ptr] * 4 + [C.c_int] * 6 + [C.c_float, _lib.c_ptr]
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sdmi.h')) as f:
        assert '#define SDMI_ABI_VERSION 17' in f.read()
