"""The face / bedroom LDMs (models/ldm/celeba256, ffhq256, lsun_beds256: one unet_config, model_channels 224, num_head_channels 32) and
bsr_sr's UNet (160) on the host: the constants equal the yamls (fixtures of tools/make_golden_faces.py), UNetModelHIP constructs from the
yamls' own parameters through their `target:` strings and exposes exactly the reference modules' state_dict keys and shapes;
num_head_channels is admitted for the AttentionBlock family and no wider; widths that are no multiple of 32 and a 224-wide spatial
transformer stay refused; a packed blob of another num_head_channels is rejected by its header.  No GPU."""
import ctypes as C
import importlib
import json
import os
import struct

import pytest
import torch

from stable_diffusion_amd import synthetic

FACE_MODELS = ('celeba256', 'ffhq256', 'lsun_beds256')


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _params(golden_dir, model):
    return _load(golden_dir, f'{model}_config.json')['model']['params']


def test_config_fixtures_match_the_constants(golden_dir):
    first = _params(golden_dir, 'celeba256')
    for name in FACE_MODELS:
        p = _params(golden_dir, name)
        assert p['unet_config'] == first['unet_config']
        assert p['unet_config']['params'] == synthetic.FACES_UNET_KWARGS
        fs = p['first_stage_config']['params']
        assert dict(embed_dim=fs['embed_dim'], n_embed=fs['n_embed'], ddconfig=fs['ddconfig']) == synthetic.FACES_VQ_KWARGS
        assert p['cond_stage_config'] == '__is_unconditional__'
        assert synthetic.FACES_SCHEDULE == dict(timesteps=p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'],
                                                conditioning_key=None)
    assert (first['linear_start'], first['linear_end'], first['timesteps']) == (0.0015, 0.0195, 1000)
    b = _params(golden_dir, 'bsr_sr')
    assert b['unet_config']['params'] == synthetic.BSR_UNET_KWARGS and b['concat_mode'] is True
    assert synthetic.BSR_SCHEDULE == dict(timesteps=b['timesteps'], linear_start=b['linear_start'], linear_end=b['linear_end'],
                                          conditioning_key='concat')
    assert (b['linear_start'], b['linear_end']) == (0.0015, 0.0155)


def _instantiate(config, target):
    """instantiate_from_config (ldm/util.py:78-93) with the yaml's reference class swapped for this project's, as INTEGRATION.md does"""
    module, cls = target.rsplit('.', 1)
    return getattr(importlib.import_module(module), cls)(**config.get('params', dict()))


@pytest.mark.parametrize('model', FACE_MODELS + ('bsr_sr',))
def test_yaml_instantiates_through_its_target_strings(golden_dir, model):
    p = _params(golden_dir, model)
    assert p['unet_config']['target'] == 'ldm.modules.diffusionmodules.openaimodel.UNetModel'
    assert p['first_stage_config']['target'] == 'ldm.models.autoencoder.VQModelInterface'
    unet = _instantiate(p['unet_config'], 'stable_diffusion_amd.unet.UNetModelHIP')
    ref = _load(golden_dir, ('bsr' if model == 'bsr_sr' else 'faces') + '_unet_state_dict_keys.json')['keys']
    assert [(k, list(v.shape)) for k, v in sorted(unet.state_dict().items())] == sorted((k, list(s)) for k, s in ref)
    vq = _instantiate(p['first_stage_config'], 'stable_diffusion_amd.vae.VQModelInterfaceHIP')
    assert any(k.startswith('decoder.mid.attn_1.') for k in vq.state_dict())          # (no attn_type in these yamls: mid-block attention on)
    from stable_diffusion_amd import LatentDiffusionHIP
    sched = synthetic.BSR_SCHEDULE if model == 'bsr_sr' else synthetic.FACES_SCHEDULE
    assert LatentDiffusionHIP(unet, **sched).model.conditioning_key == sched['conditioning_key']


@pytest.mark.parametrize('precision', ['mixed', 'full'])
@pytest.mark.parametrize('tag,kwargs,n_keys,n_params', [('faces', 'FACES_UNET_KWARGS', 368, 274056163), ('bsr', 'BSR_UNET_KWARGS', 306, 113622563)])
def test_unet_state_dict_equals_reference(golden_dir, precision, tag, kwargs, n_keys, n_params):
    from stable_diffusion_amd import UNetModelHIP
    m = UNetModelHIP(**getattr(synthetic, kwargs), hip_precision=precision)
    sd = m.state_dict()
    ref = [tuple(kv) for kv in _load(golden_dir, f'{tag}_unet_state_dict_keys.json')['keys']]
    assert sorted((k, list(v.shape)) for k, v in sd.items()) == sorted((k, list(s)) for k, s in ref)      # name for name, shape for shape
    assert len(sd) == n_keys and sum(v.numel() for v in sd.values()) == n_params
    # plain Downsample / Upsample convolutions, AttentionBlocks with a conv1d qkv, no scale-shift norm
    assert any(k.endswith('.op.weight') for k in sd) and any(k.endswith('.conv.weight') for k in sd)
    mc = m.model_channels
    assert tuple(sd['middle_block.1.qkv.weight'].shape) == (3 * 4 * mc, 4 * mc, 1)
    assert tuple(sd['input_blocks.1.0.emb_layers.1.weight'].shape) == (mc, 4 * mc)
    assert m.num_head_channels == 32 and m.num_heads == -1 and m.hip_precision == precision
    assert m._handle.lib.sdmi_unet_workspace_bytes(m._handle.h, 8, 64, 64, 0) > 0


@pytest.mark.parametrize('bad,name', [
    (dict(use_spatial_transformer=True, context_dim=512, legacy=False), 'spatial transformer'),     # a spatial transformer + num_head_channels
    (dict(use_spatial_transformer=True, context_dim=512, legacy=False, num_heads=8, num_head_channels=-1), 'multiple of 64'),   # 224 wide
    (dict(model_channels=208), 'multiple of 64'),                                                    # not a multiple of 32
    (dict(num_head_channels=48), 'num_head_channels=48'),                                            # 448 % 48 != 0
    (dict(num_heads=8), 'num_heads == -1'),                                                          # both given
    (dict(use_scale_shift_norm=True), 'scale-shift'), (dict(use_new_attention_order=True), 'use_new_attention_order'),
    (dict(num_classes=10), 'class conditioning'), (dict(context_dim=768), 'context_dim')])
def test_refusals_still_fire(bad, name):
    from stable_diffusion_amd import UNetModelHIP
    with pytest.raises(NotImplementedError, match=name):
        UNetModelHIP(**dict(synthetic.FACES_UNET_KWARGS, **bad))


def _create(kw, attention_block, nhc, num_heads=-1, context_dim=0):
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.unet import make_cfg, unet_num_head_channels_flag
    lib = _lib.load()
    cfg = make_cfg(kw['in_channels'], kw['out_channels'], kw['model_channels'], kw['num_res_blocks'], kw['channel_mult'],
                   kw['attention_resolutions'], num_heads, 1, context_dim)
    ext = _lib.UNetExt()
    ext.attention_block, ext.resblock_updown = attention_block, 0
    h = C.c_void_p()
    rc = lib.sdmi_unet_create_flags(C.byref(cfg), C.byref(ext), unet_num_head_channels_flag(nhc) if nhc else 0, 0, C.byref(h))
    return lib, cfg, h, rc


def test_library_refusals():
    """the C ABI refuses what the Python class refuses: num_head_channels on a SpatialTransformer handle, widths off the 32 grid,
    224 with a SpatialTransformer, a num_head_channels that does not divide a level"""
    kw = synthetic.FACES_UNET_KWARGS
    lib, _, h, rc = _create(kw, 1, 32)
    assert rc == 0
    lib.sdmi_unet_destroy(h)
    lib, _, h, rc = _create(kw, 0, 32, num_heads=8, context_dim=512)
    assert rc != 0 and b'num_head_channels' in lib.sdmi_last_error()
    lib, _, h, rc = _create(dict(kw, model_channels=208), 1, 16)
    assert rc != 0 and b'multiple of 32' in lib.sdmi_last_error()
    lib, _, h, rc = _create(kw, 0, 0, num_heads=8, context_dim=512)
    assert rc != 0 and b'multiple of 64' in lib.sdmi_last_error()
    lib, _, h, rc = _create(kw, 1, 48)
    assert rc != 0 and b'not divisible by num_head_channels' in lib.sdmi_last_error()
    lib, _, h, rc = _create(kw, 1, 56)                       # divides 448 / 672 / 896, but no attention kernel of head dim 56
    assert rc != 0 and b'not instantiated' in lib.sdmi_last_error()


def test_heads_follow_num_head_channels():
    """without the flag the same widths are divided by num_heads: 448 / 8 = 56 channels per head, which no attention kernel is
    instantiated for -- the handle is refused by head dim; with num_head_channels = 32 every level has 32-channel heads and is accepted
    (test_library_refusals)"""
    kw = synthetic.FACES_UNET_KWARGS
    lib, _, h, rc = _create(kw, 1, 0, num_heads=8)
    assert rc != 0 and b'56' in lib.sdmi_last_error()


def test_packed_blob_of_another_num_head_channels_is_rejected():
    """the blob header records num_head_channels (the qkv rows are permuted per head): a header written for 64-channel heads is
    refused by a handle of 32-channel heads before any byte is copied"""
    kw = synthetic.FACES_UNET_KWARGS
    lib, cfg, h, rc = _create(kw, 1, 32)
    assert rc == 0
    total = int(lib.sdmi_unet_packed_bytes(h))
    assert total > 0

    def header(nhc, max_ds=4):
        # PackedHeader (csrc/unet.cpp): magic, abi, precise_1x1, n_buffers, reserved, sdmi_unet_cfg, total_bytes
        reserved = 1 | 2 | (max_ds << 8) | (1 << 4) | (nhc << 16)
        raw = b'SDMIPK01' + struct.pack('<4i', lib.sdmi_abi_version(), 1, 0, reserved) + bytes(cfg)
        raw += b'\0' * (-len(raw) % 8) + struct.pack('<q', total)
        return raw + b'\0' * 512
    for nhc, msg in ((64, b'num_head_channels 64'), (0, b'num_head_channels 0')):
        buf = header(nhc)
        assert lib.sdmi_unet_import_packed(h, buf, len(buf), None) != 0
        assert msg in lib.sdmi_last_error(), lib.sdmi_last_error()
    buf = header(32)                                          # the right family gets past the header and fails on the (absent) buffers
    assert lib.sdmi_unet_import_packed(h, buf, len(buf), None) != 0
    assert b'truncated or inconsistent' in lib.sdmi_last_error(), lib.sdmi_last_error()
    lib.sdmi_unet_destroy(h)


def test_source_split_packer_is_exported():
    from stable_diffusion_amd import _lib
    assert _lib.load().sdmi_k_pack_conv_weight_src is not None


def test_synthetic_state_dicts_are_seeded():
    sd = synthetic.synthetic_faces_unet_state_dict(0)
    assert len(sd) == 368 and tuple(sd['output_blocks.11.0.in_layers.2.weight'].shape) == (224, 448, 3, 3)
    assert float(sd['middle_block.1.proj_out.weight'].abs().max()) > 0 and float(sd['out.2.weight'].abs().max()) > 0
    again = synthetic.synthetic_named_state_dict([('out.2.weight', (3, 224, 3, 3))], 0)
    assert torch.equal(again['out.2.weight'], sd['out.2.weight'])
    bsr = synthetic.synthetic_faces_unet_state_dict(0, synthetic.BSR_UNET_KWARGS)
    assert len(bsr) == 306 and tuple(bsr['input_blocks.0.0.weight'].shape) == (160, 6, 3, 3)
