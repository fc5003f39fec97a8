"""The unconditional LSUN-Churches model (models/ldm/lsun_churches256/config.yaml) on the host: UNetModelHIP constructs from
the yaml's own parameters and exposes exactly the reference module's state_dict keys and shapes (fixtures of
tools/make_golden_churches.py); scale-shift norm is admitted for the unconditional family and no wider; the library sizes the
legal latents and refuses the others; conditioning_key None; the ABI stayed put.  No GPU."""
import ctypes as C
import json
import os

import pytest
import torch

from stable_diffusion_amd import synthetic


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _params(golden_dir):
    return _load(golden_dir, 'lsun_churches256_config.json')['model']['params']


def test_config_fixture_matches_the_constants(golden_dir):
    p = _params(golden_dir)
    assert p['unet_config']['params'] == synthetic.CHURCHES_UNET_KWARGS
    fs = p['first_stage_config']['params']
    assert fs['embed_dim'] == 4 and fs['ddconfig'] == synthetic.CHURCHES_VAE_DDCONFIG == synthetic.SD_V1_VAE_DDCONFIG
    assert p['cond_stage_config'] == '__is_unconditional__' and p['scale_by_std'] is True
    assert synthetic.CHURCHES_SCHEDULE == dict(timesteps=p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'],
                                               conditioning_key=None)
    assert (p['linear_start'], p['linear_end'], p['timesteps']) == (0.0015, 0.0155, 1000)


@pytest.mark.parametrize('precision', ['mixed', 'full'])
def test_churches_unet_state_dict_equals_reference(golden_dir, precision):
    from stable_diffusion_amd import UNetModelHIP
    m = UNetModelHIP(**_params(golden_dir)['unet_config']['params'], hip_precision=precision)
    sd = m.state_dict()
    mine = [(k, list(v.shape)) for k, v in sd.items()]
    ref = [tuple(kv) for kv in _load(golden_dir, 'churches_unet_state_dict_keys.json')['keys']]
    assert sorted(mine) == sorted((k, list(s)) for k, s in ref)
    assert len(mine) == 520
    assert sum(v.numel() for v in sd.values()) == 294966916
    # scale-shift: emb_layers is twice as wide as the block's output (openaimodel.py:218-224)
    emb = {k: tuple(v.shape) for k, v in sd.items() if k.endswith('emb_layers.1.weight')}
    assert emb and all(s == (2 * sd[k.replace('emb_layers.1.weight', 'out_layers.3.bias')].shape[0], 768) for k, s in emb.items())
    assert emb['input_blocks.1.0.emb_layers.1.weight'] == (384, 768) and emb['middle_block.0.emb_layers.1.weight'] == (1536, 768)
    assert m.use_scale_shift_norm and m.hip_precision == precision


@pytest.mark.parametrize('bad', [dict(use_spatial_transformer=True, context_dim=512), dict(resblock_updown=False),
                                 dict(num_heads=-1, num_head_channels=32), dict(num_head_channels=32), dict(in_channels=7)])
def test_scale_shift_norm_is_admitted_for_the_unconditional_family_only(bad):
    from stable_diffusion_amd import UNetModelHIP
    with pytest.raises(NotImplementedError, match='scale-shift'):
        UNetModelHIP(**dict(synthetic.CHURCHES_UNET_KWARGS, **bad))


def test_other_families_still_refuse_scale_shift_norm():
    from stable_diffusion_amd import UNetModelHIP
    for kw in (synthetic.INPAINT_UNET_KWARGS, synthetic.CIN_UNET_KWARGS, synthetic.SD_V1_UNET_KWARGS):
        with pytest.raises(NotImplementedError, match='scale-shift'):
            UNetModelHIP(**dict(kw, use_scale_shift_norm=True))


def test_library_sizes_latents_that_are_multiples_of_16():
    from stable_diffusion_amd import UNetModelHIP, _lib
    m = UNetModelHIP(**synthetic.CHURCHES_UNET_KWARGS)
    ws = m._handle.lib.sdmi_unet_workspace_bytes
    assert ws(m._handle.h, 2, 32, 32, 0) > 0 and ws(m._handle.h, 2, 16, 16, 0) > 0 and ws(m._handle.h, 8, 48, 48, 0) > 0
    assert ws(m._handle.h, 1, 24, 32, 0) == 0
    assert b'multiples of 16' in _lib.load().sdmi_last_error()


def test_creation_flags_entry_point():
    """sdmi_unet_create_flags: flags 0 is sdmi_unet_create_ext; the scale-shift flag needs the AttentionBlock / resampling family;
    an unknown flag is refused."""
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.unet import UNET_SCALE_SHIFT_NORM, make_cfg
    lib = _lib.load()
    kw = synthetic.CHURCHES_UNET_KWARGS
    cfg = make_cfg(kw['in_channels'], kw['out_channels'], kw['model_channels'], kw['num_res_blocks'], kw['channel_mult'],
                   kw['attention_resolutions'], kw['num_heads'], 1, 0)
    ext = _lib.UNetExt()
    ext.attention_block, ext.resblock_updown = 1, 1

    def n_floats(flags):
        h = C.c_void_p()
        _lib.check(lib.sdmi_unet_create_flags(C.byref(cfg), C.byref(ext), flags, 0, C.byref(h)))
        buf, shape, nd, total = C.create_string_buffer(256), (C.c_int64 * 4)(), C.c_int(), 0
        for i in range(lib.sdmi_unet_num_weights(h)):
            _lib.check(lib.sdmi_unet_weight_info(h, i, buf, 256, shape, C.byref(nd)))
            if buf.value.endswith(b'emb_layers.1.bias'):
                total += shape[0]
        lib.sdmi_unet_destroy(h)
        return total
    assert n_floats(UNET_SCALE_SHIFT_NORM) == 2 * n_floats(0) > 0
    h = C.c_void_p()
    assert lib.sdmi_unet_create_flags(C.byref(cfg), C.byref(ext), 2, 0, C.byref(h)) != 0
    assert b'flag' in lib.sdmi_last_error()
    ext.resblock_updown = 0
    assert lib.sdmi_unet_create_flags(C.byref(cfg), C.byref(ext), UNET_SCALE_SHIFT_NORM, 0, C.byref(h)) != 0
    assert b'SDMI_UNET_SCALE_SHIFT_NORM' in lib.sdmi_last_error()


def test_unconditional_wrapper():
    """DiffusionWrapper with conditioning_key None (ddpm.py:1408-1409): the UNet gets x and t, no context, nothing concatenated."""
    from stable_diffusion_amd import LatentDiffusionHIP
    seen = []

    class Probe(torch.nn.Module):
        def forward(self, x, t, context=None, **kw):
            assert context is None and not kw
            seen.append(tuple(x.shape))
            return x * 2 + t.view(-1, 1, 1, 1)

    ld = LatentDiffusionHIP(Probe(), **synthetic.CHURCHES_SCHEDULE)
    assert ld.model.conditioning_key is None
    x, t = torch.randn(2, 4, 16, 16), torch.tensor([3, 5])
    assert torch.equal(ld.apply_model(x, t, None), x * 2 + t.view(-1, 1, 1, 1)) and seen == [(2, 4, 16, 16)]
    import numpy as np
    betas = np.linspace(0.0015 ** 0.5, 0.0155 ** 0.5, 1000, dtype=np.float64) ** 2
    assert torch.equal(ld.betas, torch.tensor(betas, dtype=torch.float32))
    assert LatentDiffusionHIP(Probe()).model.conditioning_key == 'crossattn'
    with pytest.raises(NotImplementedError):
        LatentDiffusionHIP(Probe(), conditioning_key='hybrid')


def test_abi_version_and_struct_sizes_are_unchanged():
    from stable_diffusion_amd import _lib
    assert _lib.load().sdmi_abi_version() == 17
    assert C.sizeof(_lib.UNetCfg) == 100 and C.sizeof(_lib.UNetExt) == 8 and C.sizeof(_lib.IGemmDesc) == 408


def test_synthetic_churches_state_dict_is_seeded():
    sd = synthetic.synthetic_churches_unet_state_dict(0)
    assert len(sd) == 520 and tuple(sd['output_blocks.14.0.emb_layers.1.weight'].shape) == (384, 768)
    assert float(sd['middle_block.1.proj_out.weight'].abs().max()) > 0 and float(sd['out.2.weight'].abs().max()) > 0
    again = synthetic.synthetic_named_state_dict([('out.2.weight', (4, 192, 3, 3))], 0)
    assert torch.equal(again['out.2.weight'], sd['out.2.weight'])
