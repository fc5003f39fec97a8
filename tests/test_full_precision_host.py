"""Host-side pieces of the full-precision UNet mode (no GPU needed): the hip_precision keyword, the C ABI additions and the
--hip-precision switch of tools/run_reference_script.py."""
import ctypes as C
import importlib.util
import os

import pytest

from oracle.plan import TINY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hip_precision_keyword():
    from stable_diffusion_amd import UNetModelHIP
    mixed = UNetModelHIP(**TINY.ref_kwargs())
    full = UNetModelHIP(**TINY.ref_kwargs(), hip_precision='full')
    assert mixed.hip_precision == 'mixed' and full.hip_precision == 'full'
    lib = full._handle.lib
    assert lib.sdmi_unet_precision(mixed._handle.h) == 0 and lib.sdmi_unet_precision(full._handle.h) == 1
    # the same state_dict keys and shapes in both modes (only the packing inside the library differs)
    assert mixed._handle.weight_specs() == full._handle.weight_specs()
    for bad in ('half', 'FULL', None, 1):
        with pytest.raises(ValueError, match='hip_precision'):
            UNetModelHIP(**TINY.ref_kwargs(), hip_precision=bad)


def test_create_with_precision_abi():
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.unet import make_cfg
    lib = _lib.load()
    assert lib.sdmi_abi_version() == 17
    k = TINY.ref_kwargs()
    cfg = make_cfg(k['in_channels'], k['out_channels'], k['model_channels'], k['num_res_blocks'], k['channel_mult'],
                   k['attention_resolutions'], k['num_heads'], k['transformer_depth'], k['context_dim'])
    h = C.c_void_p()
    assert lib.sdmi_unet_create_with_precision(C.byref(cfg), 2, C.byref(h)) != 0
    assert b'precision' in lib.sdmi_last_error()
    for prec in (0, 1):
        assert lib.sdmi_unet_create_with_precision(C.byref(cfg), prec, C.byref(h)) == 0
        assert lib.sdmi_unet_precision(h) == prec
        lib.sdmi_unet_destroy(h)
    assert lib.sdmi_unet_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.sdmi_unet_precision(h) == 0
    lib.sdmi_unet_destroy(h)
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    for name in ('sdmi_unet_create_with_precision', 'sdmi_unet_precision', 'sdmi_k_attention_split16', 'sdmi_k_split_heads',
                 'sdmi_k_geglu_split', 'sdmi_k_layernorm_split'):
        assert name in _lib.exported_symbols() and name + '(' in hdr
    assert '#define SDMI_PRECISION_MIXED 0' in hdr and '#define SDMI_PRECISION_FULL 1' in hdr


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
      target: ldm.models.autoencoder.AutoencoderKL
      params:
        embed_dim: 4
"""


def test_run_reference_script_hip_precision_yaml():
    """--hip-precision full adds exactly one line, `hip_precision: full`, to unet_config.params; without the flag the launcher does not
    touch the yaml (add_hip_precision is not called)"""
    import yaml
    spec = importlib.util.spec_from_file_location('rrs', os.path.join(ROOT, 'tools', 'run_reference_script.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.add_hip_precision(_YAML, 'full')
    a, b = _YAML.splitlines(), out.splitlines()
    assert len(b) == len(a) + 1 and [l for l in b if l not in a] == ['        hip_precision: full']
    cfg = yaml.safe_load(out)['model']['params']
    assert cfg['unet_config']['params']['hip_precision'] == 'full' and 'hip_precision' not in cfg['first_stage_config']['params']
    # the bundle's re-serialised yaml may list params before target
    swapped = _YAML.replace('      target: stable_diffusion_amd.unet.UNetModelHIP\n      params:\n', '      params:\n')
    swapped = swapped.replace('        legacy: False\n', '        legacy: False\n      target: stable_diffusion_amd.unet.UNetModelHIP\n')
    out2 = m.add_hip_precision(swapped, 'full')
    assert yaml.safe_load(out2)['model']['params']['unet_config']['params']['hip_precision'] == 'full'
    assert len(out2.splitlines()) == len(swapped.splitlines()) + 1
    src = open(os.path.join(ROOT, 'tools', 'run_reference_script.py')).read()
    assert 'if args.hip_precision:\n            text = add_hip_precision(text, args.hip_precision)' in src
