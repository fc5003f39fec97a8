"""The retrieval-augmented UNet (configs/retrieval-augmented-diffusion/768x768.yaml: model_channels 448, num_head_channels 32 with
SpatialTransformers, 16 latent channels) and layout-to-image's (models/ldm/layout2img-openimages256: 128, transformer_depth 3) on the
host: the constants equal the yamls (fixtures of tools/make_golden_rdm.py), UNetModelHIP constructs from the yamls' own parameters and
from the two stand-ins and exposes exactly the reference module's state_dict keys and shapes (688 keys, 1 335 480 400 parameters),
whatever `legacy` says; what stays refused still raises and names its reason; the creation flag word and the packed-blob header carry
num_head_channels.  No GPU."""
import ctypes as C
import json
import os
import struct

import pytest
import torch

from stable_diffusion_amd import synthetic

_cache = {}


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _unet(name, **kw):
    from stable_diffusion_amd import UNetModelHIP
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = UNetModelHIP(**dict(synthetic.RDM_STANDINS[name], **kw))
    return _cache[key]


def test_config_fixtures_match_the_constants(golden_dir):
    p = _load(golden_dir, 'rdm768_config.json')['model']['params']
    assert p['unet_config']['params'] == synthetic.RDM_UNET_KWARGS
    assert p['unet_config']['target'] == 'ldm.modules.diffusionmodules.openaimodel.UNetModel'
    assert synthetic.RDM_SCHEDULE == dict(timesteps=p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'],
                                          conditioning_key=p['conditioning_key'])
    assert (p['linear_start'], p['linear_end'], p['conditioning_key'], p['channels'], p['image_size']) == (0.0015, 0.015, 'crossattn', 16, 48)
    q = _load(golden_dir, 'layout2img_config.json')['model']['params']
    assert q['unet_config']['params'] == synthetic.LAYOUT_UNET_KWARGS
    assert q['cond_stage_config']['params']['max_seq_len'] == 92 and q['cond_stage_config']['params']['n_embed'] == 512
    assert synthetic.RDM64_UNET_KWARGS == dict(synthetic.RDM_UNET_KWARGS, model_channels=64)
    assert synthetic.RDM448X2_UNET_KWARGS == dict(synthetic.RDM_UNET_KWARGS, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=1)


@pytest.mark.parametrize('precision', ['mixed', 'full'])
@pytest.mark.parametrize('name,fixture,n_keys,n_params', [('rdm', 'rdm_unet_state_dict_keys.json', 688, 1335480400),
                                                          ('layout', 'layout_unet_state_dict_keys.json', 1328, 246277379)])
def test_weight_specs_equal_the_reference_key_list(golden_dir, name, fixture, n_keys, n_params, precision):
    """name for name, shape for shape, in both precisions (the handle's weight_specs: what pack() hands to the library)"""
    from stable_diffusion_amd import UNetModelHIP
    with torch.device('meta'):          # (688 / 1328 zero parameters of up to 5.3 GB: names and shapes are all this test reads)
        m = UNetModelHIP(**synthetic.RDM_STANDINS[name], hip_precision=precision)
    doc = _load(golden_dir, fixture)
    ref = sorted((k, tuple(s)) for k, s in doc['keys'])
    assert sorted(m._handle.weight_specs()) == ref
    total = 0
    for _, s in m._specs:
        n = 1
        for v in s:
            n *= v
        total += n
    assert (len(m._specs), total) == (n_keys, n_params) and doc['n_params'] == n_params
    assert sorted((k, tuple(v.shape)) for k, v in m.state_dict().items()) == ref
    assert m.num_head_channels == 32 and m.num_heads == -1 and m.use_spatial_transformer
    # 16 latent channels in and out; the workspace of the native 48 x 48 latent is sized in 64-bit
    if name == 'rdm':
        assert dict(m._specs)['out.2.weight'] == (16, 448, 3, 3) and dict(m._specs)['input_blocks.0.0.weight'] == (448, 16, 3, 3)
        assert dict(m._specs)['middle_block.1.transformer_blocks.0.ff.net.0.proj.weight'] == (14336, 1792)
        assert dict(m._specs)['middle_block.1.transformer_blocks.0.attn2.to_k.weight'] == (1792, 768)
        assert m._handle.lib.sdmi_unet_workspace_bytes(m._handle.h, 8, 48, 48, 21) > 0


@pytest.mark.parametrize('legacy', [True, False])
@pytest.mark.parametrize('name,n_keys', [('rdm64', 688), ('rdm448x2', 286)])
def test_standins_construct_with_either_legacy_flag(name, n_keys, legacy):
    """openaimodel.py:542-549: with num_head_channels dividing ch, legacy True and False build the same SpatialTransformers"""
    m = _unet(name, legacy=legacy)
    keys = [k for k, _ in m._specs]
    assert len(keys) == n_keys and sorted(keys) == sorted(k for k, _ in _unet(name)._specs)
    mc = m.model_channels
    assert dict(m._specs)['input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight'] == (mc, mc)
    assert m._handle.lib.sdmi_unet_workspace_bytes(m._handle.h, 2, 16, 16, 11) > 0


def test_rdm64_has_the_yamls_key_names(golden_dir):
    ref = sorted(k for k, _ in _load(golden_dir, 'rdm_unet_state_dict_keys.json')['keys'])
    assert sorted(k for k, _ in _unet('rdm64')._specs) == ref
    n = sum(v.numel() for v in _unet('rdm64').state_dict().values())
    assert 30.1e6 < n < 30.3e6


RDM64 = synthetic.RDM64_UNET_KWARGS


@pytest.mark.parametrize('bad,name', [
    (dict(num_heads=8), 'num_heads == -1'),                                          # both given
    (dict(num_head_channels=64), 'num_head_channels=64'),                            # divides 64 .. 256, but not a head dim the tests run
    (dict(num_head_channels=48), 'num_head_channels=48'),                            # 64 % 48 != 0
    (dict(model_channels=96), 'multiple of 64'),                                     # off the 64 grid
    (dict(use_scale_shift_norm=True), 'scale-shift'),
    (dict(resblock_updown=True), 'resblock_updown'),
    (dict(num_head_channels=-1), 'num_heads or num_head_channels'),                  # neither given
    (dict(context_dim=None), 'context_dim')])
def test_refusals_still_fire(bad, name):
    from stable_diffusion_amd import UNetModelHIP
    with pytest.raises(NotImplementedError, match=name):
        UNetModelHIP(**dict(RDM64, **bad))


def test_full_precision_head_dim_guard_reads_num_head_channels():
    """hip_precision='full' is limited by the split-fp16 attention kernel's head dim: with num_head_channels set that is the head dim
    (the guard used to divide by num_heads == -1)"""
    from stable_diffusion_amd import UNetModelHIP
    with pytest.raises(NotImplementedError, match=r"head dims up to 160; this configuration has d_head = 192 \(num_head_channels=192\)"):
        UNetModelHIP(**dict(RDM64, model_channels=192, num_head_channels=192, hip_precision='full'))
    assert _unet('rdm64', hip_precision='full').hip_precision == 'full'              # d = 32 is inside the limit
    # ... and a num_heads configuration keeps its own guard
    with pytest.raises(NotImplementedError, match='d_head = 960'):
        UNetModelHIP(**dict(synthetic.CIN_UNET_KWARGS, hip_precision='full'))


def _create(kw, nhc, num_heads=-1, attention_block=0, precision=0):
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.unet import make_cfg, unet_num_head_channels_flag
    lib = _lib.load()
    cfg = make_cfg(kw['in_channels'], kw['out_channels'], kw['model_channels'], kw['num_res_blocks'], kw['channel_mult'],
                   kw['attention_resolutions'], num_heads, kw['transformer_depth'], kw['context_dim'])
    ext = _lib.UNetExt()
    ext.attention_block, ext.resblock_updown = attention_block, 0
    h = C.c_void_p()
    rc = lib.sdmi_unet_create_flags(C.byref(cfg), C.byref(ext), unet_num_head_channels_flag(nhc) if nhc else 0, precision, C.byref(h))
    return lib, cfg, h, rc


def test_flag_word_round_trips_num_head_channels():
    from stable_diffusion_amd.unet import unet_num_head_channels_flag
    for n in (1, 32, 160, 4095):
        f = unet_num_head_channels_flag(n)
        assert (f & 0x0fff0000) >> 16 == n and f & ~0x0fff0000 == 0
    for n in (0, 4096, -1):
        with pytest.raises(ValueError):
            unet_num_head_channels_flag(n)
    m = _unet('rdm64')
    assert m.num_head_channels == 32 and m._cfg.num_heads == -1


def test_library_admits_and_refuses_what_the_class_does():
    """the C ABI: num_head_channels on a SpatialTransformer handle is accepted with num_heads = -1, refused together with num_heads and for every value other than the tested 32 -- whether or not an attention kernel of that head dim exists"""
    lib, _, h, rc = _create(RDM64, 32)
    assert rc == 0
    n = lib.sdmi_unet_num_weights(h)
    lib.sdmi_unet_destroy(h)
    assert n == 688
    lib, _, h, rc = _create(RDM64, 32, num_heads=8)
    assert rc != 0 and b'num_head_channels together with num_heads' in lib.sdmi_last_error()
    for nhc, mc in ((64, 64), (56, 448), (40, 320), (192, 192), (48, 64)):      # (the first four divide every level; 64 / 40 have attention kernels)
        lib, _, h, rc = _create(dict(RDM64, model_channels=mc), nhc)
        assert rc != 0 and f'num_head_channels {nhc} on a SpatialTransformer handle'.encode() in lib.sdmi_last_error(), lib.sdmi_last_error()
    lib, _, h, rc = _create(dict(RDM64, model_channels=192), 192, precision=1)
    assert rc != 0 and b'num_head_channels 192' in lib.sdmi_last_error()
    lib, _, h, rc = _create(dict(RDM64, model_channels=96), 32)
    assert rc != 0 and b'multiple of 64' in lib.sdmi_last_error()


def test_packed_blob_of_a_num_heads_handle_is_rejected():
    """the blob header records num_head_channels: a header a num_heads handle of equal shapes would write (num_heads 2 in the
    configuration, 0 in the num_head_channels field) is refused before any byte is copied, as is one of another num_head_channels"""
    kw = dict(RDM64, channel_mult=[1], attention_resolutions=[1])        # one level of 64 channels: 2 heads either way
    lib, cfg, h, rc = _create(kw, 32)
    assert rc == 0
    total = int(lib.sdmi_unet_packed_bytes(h))
    assert total > 0

    def header(cfg_bytes, nhc, max_ds=4):
        # PackedHeader (csrc/unet.cpp): magic, abi, precise_1x1, n_buffers, reserved, sdmi_unet_cfg, total_bytes
        reserved = 1 | 2 | (max_ds << 8) | (nhc << 16)
        raw = b'SDMIPK01' + struct.pack('<4i', lib.sdmi_abi_version(), 1, 0, reserved) + cfg_bytes
        raw += b'\0' * (-len(raw) % 8) + struct.pack('<q', total)
        return raw + b'\0' * 512
    lib2, cfg_heads, h2, rc2 = _create(kw, 0, num_heads=2)
    assert rc2 == 0
    assert int(lib.sdmi_unet_packed_bytes(h2)) == total                   # equal shapes: the same buffers, byte for byte
    lib.sdmi_unet_destroy(h2)
    buf = header(bytes(cfg_heads), 0)
    assert lib.sdmi_unet_import_packed(h, buf, len(buf), None) != 0
    assert b'different UNet configuration' in lib.sdmi_last_error(), lib.sdmi_last_error()
    for nhc, msg in ((0, b'num_head_channels 0'), (64, b'num_head_channels 64')):
        buf = header(bytes(cfg), nhc)
        assert lib.sdmi_unet_import_packed(h, buf, len(buf), None) != 0
        assert msg in lib.sdmi_last_error(), lib.sdmi_last_error()
    buf = header(bytes(cfg), 32)                                          # the right family gets past the header and fails on the (absent) buffers
    assert lib.sdmi_unet_import_packed(h, buf, len(buf), None) != 0
    assert b'truncated or inconsistent' in lib.sdmi_last_error(), lib.sdmi_last_error()
    lib.sdmi_unet_destroy(h)
