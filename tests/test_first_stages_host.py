"""The rest of the first-stage zoo (models/first_stage_models/kl-f32, kl-f4, vq-f8, vq-f8-n256, vq-f16 and configs/autoencoder/*) and the
older class-conditional model (models/ldm/cin256) on the host: the constants equal the parsed yamls (the committed json of
tools/make_golden_first_stages.py / make_golden_cin256_old.py), every configuration constructs in both precisions and exposes exactly the
reference module's state_dict keys and shapes, attn_resolutions resolve to the levels the reference constructors give them, what stays
refused raises and names its reason, and the C ABI grew by three kernel entries without moving a struct.  No GPU."""
import ctypes as C
import json
import os
import subprocess

import pytest

from stable_diffusion_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = ['kl_f32', 'kl_f4', 'vq_f8', 'vq_f8_n256', 'vq_f16']
MASKS = {'kl_f32': 48, 'kl_f32_thin': 48, 'kl_f4': 0, 'vq_f8': 8, 'vq_f8_thin': 8, 'vq_f8_n256': 8, 'vq_f8_n256_thin': 8, 'vq_f16': 16,
         'vq_f16_thin': 16}


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def test_yamls_equal_the_constants(golden_dir):
    doc = _load(golden_dir, 'first_stages_configs.json')
    assert set(doc) == set(synthetic.FIRST_STAGES) == set(MASKS)
    for tag in REAL:
        p, kw = doc[tag]['params'], synthetic.FIRST_STAGES[tag]
        vq = 'n_embed' in kw
        assert p['target'] == ('ldm.models.autoencoder.VQModel' if vq else 'ldm.models.autoencoder.AutoencoderKL')
        assert {k: p[k] for k in p if k != 'target'} == kw, tag
    assert doc['kl_f32']['same_as'] == 'configs/autoencoder/autoencoder_kl_8x8x64.yaml'
    assert doc['kl_f4']['same_as'] == 'configs/autoencoder/autoencoder_kl_64x64x3.yaml'
    assert synthetic.KL_F32_KWARGS == dict(embed_dim=64, ddconfig=synthetic.KL_F32_DDCONFIG) and synthetic.KL_F32_DDCONFIG['z_channels'] == 64
    assert synthetic.KL_F4_KWARGS['embed_dim'] == 3 and synthetic.KL_F4_DDCONFIG['attn_resolutions'] == []
    assert (synthetic.VQ_F8_KWARGS['n_embed'], synthetic.VQ_F8_N256_KWARGS['n_embed'], synthetic.VQ_F16_KWARGS['n_embed']) == (16384, 256, 16384)
    assert (synthetic.VQ_F8_KWARGS['embed_dim'], synthetic.VQ_F16_KWARGS['embed_dim']) == (4, 8)
    for tag in ('kl_f32', 'vq_f8', 'vq_f8_n256', 'vq_f16'):                       # the stand-ins are the yamls at ch 64
        thin, real = synthetic.FIRST_STAGES[tag + '_thin'], synthetic.FIRST_STAGES[tag]
        assert thin == dict(real, ddconfig=dict(real['ddconfig'], ch=64))
        assert doc[tag + '_thin']['kwargs'] == thin


@pytest.mark.parametrize('precision', ['mixed', 'full'])
@pytest.mark.parametrize('tag', sorted(MASKS))
def test_weight_specs_equal_the_reference_key_list(golden_dir, tag, precision):
    doc = _load(golden_dir, 'first_stages_configs.json')[tag]
    m = synthetic.make_first_stage(synthetic.FIRST_STAGES[tag], precision)
    ref = sorted((k, tuple(s)) for k, s in doc['keys'])
    assert sorted(m._handle.weight_specs()) == ref
    assert sorted((k, tuple(v.shape)) for k, v in m.state_dict().items()) == ref
    assert sum(p.numel() for p in m.parameters()) == doc['n_params']
    assert m.attn_level_mask == doc['attn_level_mask'] == MASKS[tag]
    assert m.factor == 2 ** (len(synthetic.FIRST_STAGES[tag]['ddconfig']['ch_mult']) - 1)
    lib = m._handle.lib
    # (a handle with level attention runs the flash form, which has no token-count rule; KL-f4's mid block keeps the GEMM form's H W % 64 == 0)
    h, w = (3, 5) if m.attn_level_mask else (8, 8)
    assert lib.sdmi_vae_decode_workspace_bytes(m._handle.h, 1, h, w) > 0
    assert lib.sdmi_vae_encode_workspace_bytes(m._handle.h, 2, h * m.factor, w * m.factor) > 0


def test_kl_f32_has_the_wide_ends_and_two_attention_levels():
    m = synthetic.make_first_stage(synthetic.KL_F32_KWARGS)
    sp = dict(m._specs)
    assert sp['decoder.conv_in.weight'] == (512, 64, 3, 3) and sp['encoder.conv_out.weight'] == (128, 512, 3, 3)
    assert sp['quant_conv.weight'] == (128, 128, 1, 1) and sp['post_quant_conv.weight'] == (64, 64, 1, 1)
    attn = sorted({k.rsplit('.', 2)[0] for k in sp if '.attn.' in k})
    assert attn == [f'decoder.up.{l}.attn.{i}' for l in (4, 5) for i in range(3)] + [f'encoder.down.{l}.attn.{i}' for l in (4, 5) for i in range(2)]
    assert all(sp[a + '.q.weight'] == (512, 512, 1, 1) for a in attn)
    assert m.factor == 32 and m.attn_level_mask == 0b110000


def test_vq_level_attention_and_codebooks():
    from stable_diffusion_amd.vae import attn_level_mask
    for tag, lvl, n_embed, D in (('vq_f8', 3, 16384, 4), ('vq_f8_n256', 3, 256, 4), ('vq_f16', 4, 16384, 8)):
        m = synthetic.make_first_stage(synthetic.FIRST_STAGES[tag])
        sp = dict(m._specs)
        assert sp['quantize.embedding.weight'] == (n_embed, D) and sp['quant_conv.weight'] == (D, D, 1, 1)
        attn = sorted({k.rsplit('.', 2)[0] for k in sp if '.attn.' in k})
        assert attn == [f'decoder.up.{lvl}.attn.{i}' for i in range(3)] + [f'encoder.down.{lvl}.attn.{i}' for i in range(2)]
        assert 'decoder.mid.attn_1.q.weight' in sp and m.attn_level_mask == 1 << lvl == attn_level_mask(synthetic.FIRST_STAGES[tag]['ddconfig'])


def test_refusals_name_their_reason():
    from stable_diffusion_amd import AutoencoderKLHIP, VQModelInterfaceHIP, _lib
    for zc in (17, 48, 65):
        with pytest.raises(_lib.SdmiError, match=r'z_channels <= 16 \(or 32 / 64\)'):
            AutoencoderKLHIP(dict(synthetic.KL_F32_DDCONFIG, z_channels=zc), None, 64)
        with pytest.raises(_lib.SdmiError, match=r'embed_dim <= 16 \(or 32 / 64\)'):
            AutoencoderKLHIP(synthetic.KL_F32_DDCONFIG, None, zc)
    for zc in (32, 64):
        AutoencoderKLHIP(dict(synthetic.KL_F32_DDCONFIG, z_channels=zc, ch=64), None, zc)
    # a VQ attn_resolutions entry that names no level: VQ-f8 runs at 256, 128, 64, 32
    with pytest.raises(NotImplementedError, match=r'attn_resolutions entry 16 names no level.*\[256, 128, 64, 32\]'):
        VQModelInterfaceHIP(embed_dim=4, n_embed=256, ddconfig=dict(synthetic.VQ_F8_DDCONFIG, attn_resolutions=[32, 16]))
    # attn_type 'none' with attn_resolutions: the reference would silently build no attention there
    with pytest.raises(NotImplementedError, match='attn_resolutions'):
        VQModelInterfaceHIP(embed_dim=4, n_embed=256, ddconfig=dict(synthetic.VQ_F8_DDCONFIG, attn_type='none'))
    VQModelInterfaceHIP(embed_dim=4, n_embed=256, ddconfig=dict(synthetic.VQ_F8_DDCONFIG, ch=64, attn_type='none', attn_resolutions=[]))
    # a codebook of another width than the quantizer has
    with pytest.raises(_lib.SdmiError, match='embed_dim must be 1, 2, 3, 4 or 8'):
        VQModelInterfaceHIP(embed_dim=16, n_embed=256, ddconfig=dict(synthetic.VQ_F16_DDCONFIG, z_channels=16))


def test_abi_is_additive():
    """version 17, three more kernel entries, sdmi_vae_cfg / sdmi_vae_ext where they were; a codebook handle takes a level mask"""
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.vae import make_vae_cfg
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    assert '#define SDMI_ABI_VERSION 17' in hdr and lib.sdmi_abi_version() == 17
    for name in ('sdmi_k_conv_in64', 'sdmi_k_conv_out128', 'sdmi_k_pointwise_nchw128'):
        assert name in _lib.exported_symbols() and name + '(' in hdr and hasattr(lib, name)
    assert C.sizeof(_lib.VaeCfg) == 15 * 4 and _lib.VaeCfg.embed_dim.offset == 14 * 4 and C.sizeof(_lib.VaeExt) == 3 * 4
    src = '#include <stdio.h>\n#include "sdmi.h"\nint main(){ printf("%zu %zu\\n", sizeof(sdmi_vae_cfg), sizeof(sdmi_vae_ext)); }\n'
    d = os.path.join(ROOT, 'stable-diffusion_amd', 'build')
    os.makedirs(d, exist_ok=True)
    c, exe = os.path.join(d, 'abi_probe_first_stages.c'), os.path.join(d, 'abi_probe_first_stages')
    open(c, 'w').write(src)
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ['60', '12']
    cfg = make_vae_cfg(dict(synthetic.VQ_F8_DDCONFIG, ch=64), 4, vq=True)
    ext = _lib.VaeExt()
    ext.double_z, ext.mid_attn, ext.n_embed = 0, 1, 256
    h = C.c_void_p()
    assert lib.sdmi_vae_create_precision(C.byref(cfg), C.byref(ext), 3, 0, C.byref(h)) == 0
    n0 = lib.sdmi_vae_num_weights(h)
    lib.sdmi_vae_destroy(h)
    for mask, n_attn in ((0, 0), (8, 5), (12, 10)):
        assert lib.sdmi_vae_create_attn(C.byref(cfg), C.byref(ext), 3, 0, mask, C.byref(h)) == 0
        assert lib.sdmi_vae_num_weights(h) == n0 + 10 * n_attn
        lib.sdmi_vae_destroy(h)
    assert lib.sdmi_vae_create_attn(C.byref(cfg), C.byref(ext), 3, 0, 16, C.byref(h)) != 0
    assert b'names a level past the last one' in lib.sdmi_last_error()


def test_cin256_old_builds_with_the_reference_key_lists(golden_dir):
    from stable_diffusion_amd import ClassEmbedderHIP, UNetModelHIP, VQModelInterfaceHIP
    p = _load(golden_dir, 'cin256_old_config.json')['model']['params']
    assert p['unet_config']['params'] == synthetic.CIN256_OLD_UNET_KWARGS
    assert p['cond_stage_config']['params'] == synthetic.CIN256_OLD_CLASS_KWARGS
    fs = p['first_stage_config']['params']
    assert {k: fs[k] for k in ('embed_dim', 'n_embed', 'ddconfig')} == synthetic.CIN256_OLD_VQ_KWARGS == synthetic.VQ_F8_KWARGS
    assert {k: p[k] for k in ('timesteps', 'linear_start', 'linear_end', 'conditioning_key')} == synthetic.CIN256_OLD_SCHEDULE
    doc = _load(golden_dir, 'cin256_old_state_dict_keys.json')
    ref = sorted((k, tuple(s)) for k, s in doc['keys'])
    for precision in ('mixed', 'full'):
        m = UNetModelHIP(**p['unet_config']['params'], hip_precision=precision)
        assert sorted((k, tuple(v.shape)) for k, v in m.state_dict().items()) == ref
        assert sum(v.numel() for v in m.state_dict().values()) == doc['n_params']
    e = ClassEmbedderHIP(**p['cond_stage_config']['params'])
    assert [[k, list(v.shape)] for k, v in e.state_dict().items()] == doc['class_embedder_keys'] == [['embedding.weight', [1000, 512]]]
    vq = VQModelInterfaceHIP(embed_dim=fs['embed_dim'], n_embed=fs['n_embed'], ddconfig=fs['ddconfig'], lossconfig=fs['lossconfig'])
    want = sorted((k, tuple(s)) for k, s in _load(golden_dir, 'first_stages_configs.json')['vq_f8']['keys'])
    assert sorted((k, tuple(v.shape)) for k, v in vq.state_dict().items()) == want and vq.attn_level_mask == 8
