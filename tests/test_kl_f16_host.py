"""The KL-f16 first stage of the retrieval-augmented model (configs/retrieval-augmented-diffusion/768x768.yaml first_stage_config: ch 128,
ch_mult [1,1,2,2,4], z_channels 16, embed_dim 16, attn_resolutions [16]) on the host: the constants equal the yaml (the committed
rdm768_config.json and the fixture of tools/make_golden_kl_f16.py), AutoencoderKLHIP constructs from the yaml's own parameters and from the
three stand-ins and exposes exactly the reference module's state_dict keys and shapes in both precisions and per part, attn_resolutions
resolve to the levels the reference constructors give them, what stays refused raises and names its reason, and the C ABI grew by one
create call without moving a struct.  No GPU."""
import ctypes as C
import json
import os
import subprocess

import pytest

from stable_diffusion_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _kl(kw, **extra):
    from stable_diffusion_amd import AutoencoderKLHIP
    return AutoencoderKLHIP(kw['ddconfig'], None, kw['embed_dim'], **extra)


def test_yaml_equals_the_constants(golden_dir):
    p = _load(golden_dir, 'rdm768_config.json')['model']['params']
    fs = p['first_stage_config']
    assert fs['target'] == 'ldm.models.autoencoder.AutoencoderKL'
    assert fs['params']['ddconfig'] == synthetic.KL_F16_DDCONFIG and fs['params']['embed_dim'] == synthetic.KL_F16_KWARGS['embed_dim'] == 16
    assert p['scale_factor'] == synthetic.KL_F16_SCALE_FACTOR == 0.22765929
    doc = _load(golden_dir, 'kl_f16_state_dict_keys.json')
    assert doc['first_stage_params'] == synthetic.KL_F16_KWARGS and doc['narrow_ddconfig'] == synthetic.KL_NARROW_DDCONFIG
    assert synthetic.KL_F16_THIN_DDCONFIG == dict(synthetic.KL_F16_DDCONFIG, ch=64)
    assert synthetic.KL_TWO_LEVELS_DDCONFIG == dict(synthetic.KL_NARROW_DDCONFIG, attn_resolutions=[32, 16])


@pytest.mark.parametrize('precision', ['mixed', 'full'])
def test_weight_specs_equal_the_reference_key_list(golden_dir, precision):
    m = _kl(synthetic.KL_F16_KWARGS, hip_precision=precision)
    doc = _load(golden_dir, 'kl_f16_state_dict_keys.json')
    ref = sorted((k, tuple(s)) for k, s in doc['keys'])
    assert sorted(m._handle.weight_specs()) == ref
    assert sorted((k, tuple(v.shape)) for k, v in m.state_dict().items()) == ref
    assert sum(p.numel() for p in m.parameters()) == doc['n_params']
    assert m.factor == 16 and m.attn_level_mask == 1 << 4 == doc['attn_level_masks']['kl_f16']
    sp = dict(m._specs)
    assert sp['encoder.conv_out.weight'] == (32, 512, 3, 3) and sp['quant_conv.weight'] == (32, 32, 1, 1)
    assert sp['post_quant_conv.weight'] == (16, 16, 1, 1) and sp['decoder.conv_in.weight'] == (512, 16, 3, 3)
    # AttnBlocks after every ResBlock of level 4: two in the encoder, three in the decoder, d = 512; none on any other level
    attn = sorted({k.rsplit('.', 2)[0] for k in sp if '.attn.' in k})
    assert attn == ['decoder.up.4.attn.0', 'decoder.up.4.attn.1', 'decoder.up.4.attn.2', 'encoder.down.4.attn.0', 'encoder.down.4.attn.1']
    assert all(sp[a + '.q.weight'] == (512, 512, 1, 1) and sp[a + '.norm.bias'] == (512,) for a in attn)


def test_parts_give_the_decoder_the_encoder_and_both(golden_dir):
    ref = {k: tuple(s) for k, s in _load(golden_dir, 'kl_f16_state_dict_keys.json')['keys']}
    dec = {k: s for k, s in ref.items() if k.startswith(('decoder.', 'post_quant_conv.'))}
    enc = {k: s for k, s in ref.items() if k.startswith(('encoder.', 'quant_conv.'))}
    assert dec and enc and len(dec) + len(enc) == len(ref)
    for parts, want in ((1, dec), (2, enc), (3, ref)):
        assert dict(_kl(synthetic.KL_F16_KWARGS, parts=parts)._specs) == want, parts


@pytest.mark.parametrize('name,factor,mask,n_attn', [('kl_f16_thin', 16, 16, 5), ('kl_narrow', 2, 2, 5), ('kl_two_levels', 2, 3, 10)])
@pytest.mark.parametrize('precision', ['mixed', 'full'])
def test_stand_ins_construct(name, factor, mask, n_attn, precision):
    m = _kl(synthetic.KL_F16_STANDINS[name], hip_precision=precision)
    assert (m.factor, m.attn_level_mask) == (factor, mask)
    assert len({k.rsplit('.', 2)[0] for k, _ in m._specs if '.attn.' in k}) == n_attn
    lib = m._handle.lib
    # any latent / image whose sides the resampling chain admits is sized: the flash attention has no token-count rule
    assert lib.sdmi_vae_decode_workspace_bytes(m._handle.h, 1, 6, 10) > 0 and lib.sdmi_vae_decode_workspace_bytes(m._handle.h, 2, 3, 5) > 0
    assert lib.sdmi_vae_encode_workspace_bytes(m._handle.h, 1, 6 * factor, 10 * factor) > 0


def test_mask_derivation_matches_the_reference(golden_dir):
    from stable_diffusion_amd.vae import attn_level_mask
    masks = _load(golden_dir, 'kl_f16_state_dict_keys.json')['attn_level_masks']
    for res in ([16], [32, 16], []):
        assert attn_level_mask(dict(synthetic.KL_NARROW_DDCONFIG, attn_resolutions=res)) == masks[json.dumps(res)], res
    assert (masks['[16]'], masks['[32, 16]'], masks['[]']) == (2, 3, 0)
    assert attn_level_mask(synthetic.KL_F16_DDCONFIG) == masks['kl_f16'] == 16
    assert attn_level_mask(synthetic.SD_V1_VAE_DDCONFIG) == 0


def test_refusals_name_their_reason():
    from stable_diffusion_amd import AutoencoderKLHIP, VQModelInterfaceHIP, _lib
    # an entry that names no level: the narrow stand-in runs at 32 and 16
    with pytest.raises(NotImplementedError, match=r'attn_resolutions entry 8 names no level.*\[32, 16\]'):
        AutoencoderKLHIP(dict(synthetic.KL_NARROW_DDCONFIG, attn_resolutions=[16, 8]), None, 4)
    # a level width without an attention kernel: 64 x 17 = 1088 on level 0 (the mid block, at 64, has one), in each mode, by level
    wide = dict(synthetic.KL_NARROW_DDCONFIG, ch_mult=[17, 1], attn_resolutions=[32], num_res_blocks=1)
    with pytest.raises(_lib.SdmiError, match=r'level 0 attention width 1088 has no attention kernel'):
        AutoencoderKLHIP(wide, None, 4)
    with pytest.raises(_lib.SdmiError, match=r'level 0 attention width 1088 has no split-fp16 attention kernel'):
        AutoencoderKLHIP(wide, None, 4, hip_precision='full')
    AutoencoderKLHIP(dict(wide, attn_resolutions=[]), None, 4)                  # (without the level attention the width is built)
    # ... and the mid width of a handle with level attention, which runs the flash form too
    with pytest.raises(_lib.SdmiError, match=r'mid-block attention width 1088 has no attention kernel'):
        AutoencoderKLHIP(dict(wide, ch_mult=[1, 17]), None, 4)
    with pytest.raises(_lib.SdmiError, match=r'z_channels <= 16'):
        AutoencoderKLHIP(dict(synthetic.KL_F16_DDCONFIG, z_channels=17), None, 16)
    with pytest.raises(_lib.SdmiError, match=r'embed_dim <= 16'):
        AutoencoderKLHIP(synthetic.KL_F16_DDCONFIG, None, 17)
    with pytest.raises(NotImplementedError, match='attn_resolutions'):
        VQModelInterfaceHIP(embed_dim=3, n_embed=64, ddconfig=dict(synthetic.INPAINT_VQ_DDCONFIG, resolution=64, attn_resolutions=[16]))


def test_abi_is_additive():
    """version 17, one more create call, sdmi_vae_cfg / sdmi_vae_ext where they were; mask 0 is the older call, a mask past the levels is refused"""
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.vae import make_vae_cfg
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    assert '#define SDMI_ABI_VERSION 17' in hdr and lib.sdmi_abi_version() == 17
    for name in ('sdmi_vae_create_attn', 'sdmi_k_conv_out32'):
        assert name in _lib.exported_symbols() and name + '(' in hdr and hasattr(lib, name)
    assert C.sizeof(_lib.VaeCfg) == 15 * 4 and _lib.VaeCfg.embed_dim.offset == 14 * 4 and C.sizeof(_lib.VaeExt) == 3 * 4
    src = '#include <stdio.h>\n#include "sdmi.h"\nint main(){ printf("%zu %zu\\n", sizeof(sdmi_vae_cfg), sizeof(sdmi_vae_ext)); }\n'
    d = os.path.join(ROOT, 'stable-diffusion_amd', 'build')
    os.makedirs(d, exist_ok=True)
    c, exe = os.path.join(d, 'abi_probe_kl_f16.c'), os.path.join(d, 'abi_probe_kl_f16')
    open(c, 'w').write(src)
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ['60', '12']
    cfg = make_vae_cfg(synthetic.KL_NARROW_DDCONFIG, 4)
    h = C.c_void_p()
    for mask, n_attn in ((0, 0), (2, 5), (3, 10)):
        assert lib.sdmi_vae_create_attn(C.byref(cfg), None, 3, 0, mask, C.byref(h)) == 0
        n = lib.sdmi_vae_num_weights(h)
        lib.sdmi_vae_destroy(h)
        assert lib.sdmi_vae_create_precision(C.byref(cfg), None, 3, 0, C.byref(h)) == 0
        assert n == lib.sdmi_vae_num_weights(h) + 10 * n_attn
        lib.sdmi_vae_destroy(h)
    assert lib.sdmi_vae_create_attn(C.byref(cfg), None, 3, 0, 4, C.byref(h)) != 0
    assert b'names a level past the last one' in lib.sdmi_last_error()
