"""Host-side pieces of the full-precision first stage (no GPU needed): the hip_precision keyword of AutoencoderKLHIP /
VQModelInterfaceHIP, the C ABI additions (sdmi_vae_create_precision, sdmi_vae_precision), the refusal of a mid-block attention width
without a split-fp16 kernel, and the --hip-first-stage-precision switch of tools/run_reference_script.py."""
import ctypes as C
import importlib.util
import os

import pytest

from oracle.vae_ref import SD_VAE, TINY_VAE, VAEConfig
from stable_diffusion_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_KERNEL_VAE = VAEConfig(ch=64, ch_mult=(1, 17), num_res_blocks=1)       # mid width 1088: above both attention kernels' ranges


def _kl(cfg, **kw):
    from stable_diffusion_amd import AutoencoderKLHIP
    return AutoencoderKLHIP(cfg.ddconfig(), {'target': 'torch.nn.Identity'}, cfg.embed_dim, **kw)


def test_hip_precision_keyword():
    from stable_diffusion_amd import VQModelInterfaceHIP
    for make in (lambda **kw: _kl(TINY_VAE, **kw), lambda **kw: VQModelInterfaceHIP(**synthetic.CIN_VQ_KWARGS, **kw)):
        mixed, default, full = make(hip_precision='mixed'), make(), make(hip_precision='full')
        assert mixed.hip_precision == 'mixed' and default.hip_precision == 'mixed' and full.hip_precision == 'full'
        lib = full._handle.lib
        assert [lib.sdmi_vae_precision(m._handle.h) for m in (mixed, default, full)] == [0, 0, 1]
        # the same state_dict keys and shapes in both modes (only the packing inside the library differs)
        assert mixed._handle.weight_specs() == full._handle.weight_specs()
        assert list(mixed.state_dict().keys()) == list(full.state_dict().keys())
        for bad in ('half', 'FULL', None, 1):
            with pytest.raises(ValueError, match='hip_precision'):
                make(hip_precision=bad)


def test_create_precision_abi():
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.vae import make_vae_cfg
    lib = _lib.load()
    assert lib.sdmi_abi_version() == 17
    cfg = make_vae_cfg(SD_VAE.ddconfig(), SD_VAE.embed_dim)
    ext = _lib.VaeExt()
    ext.double_z, ext.mid_attn, ext.n_embed = 1, 1, 0
    h = C.c_void_p()
    assert lib.sdmi_vae_create_precision(C.byref(cfg), None, 3, 2, C.byref(h)) != 0
    assert b'precision' in lib.sdmi_last_error()
    for prec in (0, 1):
        for e in (None, C.byref(ext)):
            assert lib.sdmi_vae_create_precision(C.byref(cfg), e, 3, prec, C.byref(h)) == 0
            assert lib.sdmi_vae_precision(h) == prec
            lib.sdmi_vae_destroy(h)
    assert lib.sdmi_vae_create(C.byref(cfg), 3, C.byref(h)) == 0
    assert lib.sdmi_vae_precision(h) == 0
    lib.sdmi_vae_destroy(h)
    assert lib.sdmi_vae_create_ext(C.byref(cfg), C.byref(ext), 3, C.byref(h)) == 0
    assert lib.sdmi_vae_precision(h) == 0
    lib.sdmi_vae_destroy(h)
    assert lib.sdmi_vae_precision(None) == -1
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    for name in ('sdmi_vae_create_precision', 'sdmi_vae_precision'):
        assert name in _lib.exported_symbols() and name + '(' in hdr
    assert '#define SDMI_ABI_VERSION 17' in hdr
    assert '192 .. 1024 in steps of 64 (csrc/attn_wide_split16.hip' in hdr          # the widened range of sdmi_k_attention_split16


def test_full_workspace_is_at_least_the_mixed_one():
    """the two-pass arena sizing runs the full executor: hi | lo operands of every conv and fp32 q / k / v, but no S / P buffer.  On
    the shipped first stages (SD's KL-f8, the VQ-f4 with mid-block attention) at the sizes they run at, that is more than the mixed
    path needs.  (Not a law: where the mixed path's S / P chunk dominates -- the 64-channel test config encoding 64 x 64 pixels, 1024
    tokens at the mid block -- the full path needs less; it reports what it needs, as the last lines check.)"""
    from stable_diffusion_amd import VQModelInterfaceHIP
    pairs = [(_kl(SD_VAE), _kl(SD_VAE, hip_precision='full')),
             (VQModelInterfaceHIP(**synthetic.CIN_VQ_KWARGS), VQModelInterfaceHIP(**synthetic.CIN_VQ_KWARGS, hip_precision='full'))]
    for mixed, full in pairs:
        lib = full._handle.lib
        for fn, shape in ((lib.sdmi_vae_decode_workspace_bytes, (1, 64, 64)), (lib.sdmi_vae_decode_workspace_bytes, (2, 8, 8)),
                          (lib.sdmi_vae_decode_workspace_bytes, (1, 16, 24)), (lib.sdmi_vae_encode_workspace_bytes, (1, 512, 512)),
                          (lib.sdmi_vae_encode_workspace_bytes, (2, 64, 64))):
            wm, wf = fn(mixed._handle.h, *shape), fn(full._handle.h, *shape)
            assert wm > 0 and wf >= wm, (shape, wm, wf)
    mixed, full = _kl(TINY_VAE), _kl(TINY_VAE, hip_precision='full')
    wm, wf = (full._handle.lib.sdmi_vae_encode_workspace_bytes(m._handle.h, 1, 64, 64) for m in (mixed, full))
    assert 0 < wf < wm


def test_full_refuses_a_mid_width_without_a_kernel():
    from stable_diffusion_amd import VQModelInterfaceHIP, _lib
    _kl(NO_KERNEL_VAE)                                   # mixed: the GEMM-based attention takes any width
    with pytest.raises(_lib.SdmiError, match='1088'):
        _kl(NO_KERNEL_VAE, hip_precision='full')
    assert b'split-fp16 attention kernel' in _lib.load().sdmi_last_error()
    # ... and only where the mid block has attention: attn_type 'none' at the same width is created
    dd = dict(synthetic.INPAINT_VQ_DDCONFIG, ch=64, ch_mult=[1, 17], num_res_blocks=1)
    VQModelInterfaceHIP(embed_dim=3, n_embed=64, ddconfig=dd, hip_precision='full')
    with pytest.raises(_lib.SdmiError, match='1088'):
        VQModelInterfaceHIP(embed_dim=3, n_embed=64, ddconfig=dict(dd, attn_type='vanilla'), hip_precision='full')


def test_superres_config_forwards_the_first_stage_precision(golden_dir):
    import json
    from stable_diffusion_amd.superres import SuperResolutionHIP
    cfg = json.load(open(os.path.join(golden_dir, 'bsr_sr_config.json')))
    assert SuperResolutionHIP.from_config(cfg).first_stage_model.hip_precision == 'mixed'
    cfg['model']['params']['first_stage_config']['params']['hip_precision'] = 'full'
    sr = SuperResolutionHIP.from_config(cfg)
    assert sr.first_stage_model.hip_precision == 'full' and sr.model.diffusion_model.hip_precision == 'mixed'


_YAML = """model:
  target: ldm.models.diffusion.ddpm.LatentDiffusion
  params:
    unet_config:
      target: stable_diffusion_amd.unet.UNetModelHIP
      params:
        image_size: 32 # unused
        in_channels: 4
        legacy: False

    first_stage_config:
      target: stable_diffusion_amd.vae.AutoencoderKLHIP
      params:
        embed_dim: 4
        ddconfig:
          double_z: true

    cond_stage_config:
      target: stable_diffusion_amd.clip.FrozenCLIPEmbedderHIP
"""


def test_run_reference_script_first_stage_precision_yaml():
    """--hip-first-stage-precision full adds exactly one line, `hip_precision: full`, to first_stage_config.params; --hip-precision alone
    still leaves first_stage_config untouched"""
    import yaml
    spec = importlib.util.spec_from_file_location('rrs', os.path.join(ROOT, 'tools', 'run_reference_script.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.add_first_stage_precision(_YAML, 'full')
    a, b = _YAML.splitlines(), out.splitlines()
    assert len(b) == len(a) + 1 and [l for l in b if l not in a] == ['        hip_precision: full']
    assert b.index('        hip_precision: full') == a.index('      target: stable_diffusion_amd.vae.AutoencoderKLHIP') + 2
    cfg = yaml.safe_load(out)['model']['params']
    assert cfg['first_stage_config']['params'] == {'hip_precision': 'full', 'embed_dim': 4, 'ddconfig': {'double_z': True}}
    assert 'hip_precision' not in cfg['unet_config']['params'] and 'params' not in cfg['cond_stage_config']
    # the UNet switch alone: one line under unet_config, first_stage_config as it was
    unet_only = m.add_hip_precision(_YAML, 'full')
    c = yaml.safe_load(unet_only)['model']['params']
    assert c['unet_config']['params']['hip_precision'] == 'full'
    assert c['first_stage_config'] == yaml.safe_load(_YAML)['model']['params']['first_stage_config']
    # both switches: one line each
    both = yaml.safe_load(m.add_first_stage_precision(unet_only, 'full'))['model']['params']
    assert both['unet_config']['params']['hip_precision'] == 'full' and both['first_stage_config']['params']['hip_precision'] == 'full'
    # the VQ first stage, and the bundle's re-serialised yaml that lists params before target
    vq = _YAML.replace('vae.AutoencoderKLHIP', 'vae.VQModelInterfaceHIP')
    assert yaml.safe_load(m.add_first_stage_precision(vq, 'full'))['model']['params']['first_stage_config']['params']['hip_precision'] == 'full'
    swapped = _YAML.replace('      target: stable_diffusion_amd.vae.AutoencoderKLHIP\n      params:\n', '      params:\n')
    swapped = swapped.replace('          double_z: true\n', '          double_z: true\n      target: stable_diffusion_amd.vae.AutoencoderKLHIP\n')
    out2 = m.add_first_stage_precision(swapped, 'full')
    assert yaml.safe_load(out2)['model']['params']['first_stage_config']['params']['hip_precision'] == 'full'
    assert len(out2.splitlines()) == len(swapped.splitlines()) + 1
    # a first stage that is not a HIP one is refused, not patched
    with pytest.raises(ValueError):
        m.add_first_stage_precision(_YAML.replace('stable_diffusion_amd.vae.AutoencoderKLHIP', 'ldm.models.autoencoder.AutoencoderKL'), 'full')
    src = open(os.path.join(ROOT, 'tools', 'run_reference_script.py')).read()
    assert "if args.hip_first_stage_precision:\n            text = add_first_stage_precision(text, args.hip_first_stage_precision)" in src
    assert "'--hip-first-stage-precision'" in src
