"""The latent-inpainting model (models/ldm/inpainting_big/config.yaml) on the host: UNetModelHIP and VQModelInterfaceHIP
construct from the yaml's own parameters and expose exactly the reference modules' state_dict keys and shapes (fixtures of
tools/make_golden_inpaint.py); the kwargs outside the two UNet families are still refused; the concat conditioning and the
seeded weight generator.  No GPU."""
import json
import os

import pytest
import torch

from stable_diffusion_amd import synthetic


def _load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _params(golden_dir):
    return _load(golden_dir, 'inpainting_big_config.json')['model']['params']


def test_config_fixture_matches_the_constants(golden_dir):
    p = _params(golden_dir)
    assert p['unet_config']['params'] == synthetic.INPAINT_UNET_KWARGS
    fs = p['first_stage_config']['params']
    assert fs['embed_dim'] == synthetic.INPAINT_VQ_KWARGS['embed_dim'] and fs['n_embed'] == synthetic.INPAINT_VQ_KWARGS['n_embed']
    assert {k: fs['ddconfig'][k] for k in synthetic.INPAINT_VQ_DDCONFIG} == synthetic.INPAINT_VQ_DDCONFIG
    assert p['cond_stage_config'] == '__is_first_stage__' and p['concat_mode'] is True
    assert (p['linear_start'], p['linear_end'], p['timesteps']) == (0.0015, 0.0205, 1000)


@pytest.mark.parametrize('precision', ['mixed', 'full'])
def test_inpaint_unet_state_dict_equals_reference(golden_dir, precision):
    from stable_diffusion_amd import UNetModelHIP
    m = UNetModelHIP(**_params(golden_dir)['unet_config']['params'], hip_precision=precision)
    mine = [(k, list(v.shape)) for k, v in m.state_dict().items()]
    ref = [tuple(kv) for kv in _load(golden_dir, 'inpaint_unet_state_dict_keys.json')['keys']]
    assert sorted(mine) == sorted((k, list(s)) for k, s in ref)
    assert len(mine) == 416
    assert sum(v.numel() for v in m.state_dict().values()) == 387245827


def test_inpaint_vq_state_dict_equals_reference(golden_dir):
    from stable_diffusion_amd import VQModelInterfaceHIP
    fs = _params(golden_dir)['first_stage_config']['params']
    m = VQModelInterfaceHIP(**{k: v for k, v in fs.items() if k not in ('lossconfig', 'monitor')}, lossconfig=fs['lossconfig'])
    mine = sorted((k, list(v.shape)) for k, v in m.state_dict().items())
    ref = sorted((k, list(s)) for k, s in _load(golden_dir, 'inpaint_vq_state_dict_keys.json')['keys'])
    assert mine == ref
    assert m.embed_dim == 3 and m.n_embed == 8192 and m.factor == 4
    assert isinstance(m.quantize, torch.nn.Module) and tuple(m.quantize.embedding.weight.shape) == (8192, 3)
    with pytest.raises(RuntimeError, match='no CPU'):
        m.decode(torch.zeros(1, 3, 8, 8))


@pytest.mark.parametrize('bad', [dict(use_scale_shift_norm=True), dict(num_head_channels=64), dict(use_new_attention_order=True),
                                 dict(num_classes=10), dict(dims=1), dict(conv_resample=False), dict(dropout=0.1),
                                 dict(legacy=False), dict(context_dim=768), dict(num_heads=-1)])
def test_inpaint_unet_refuses_the_rest(bad):
    from stable_diffusion_amd import UNetModelHIP
    with pytest.raises(NotImplementedError):
        UNetModelHIP(**dict(synthetic.INPAINT_UNET_KWARGS, **bad))


def test_spatial_transformer_family_still_refuses_resblock_updown():
    from oracle.plan import TINY
    from stable_diffusion_amd import UNetModelHIP
    with pytest.raises(NotImplementedError):
        UNetModelHIP(**dict(TINY.ref_kwargs(), resblock_updown=True))


def test_vq_refuses_kl_ddconfig_and_kl_refuses_vq_ddconfig():
    from stable_diffusion_amd import AutoencoderKLHIP, VQModelInterfaceHIP
    with pytest.raises(NotImplementedError):
        VQModelInterfaceHIP(embed_dim=4, n_embed=16, ddconfig=synthetic.SD_V1_VAE_DDCONFIG)
    with pytest.raises(NotImplementedError):
        AutoencoderKLHIP(synthetic.INPAINT_VQ_DDCONFIG, None, 3)
    with pytest.raises(NotImplementedError):
        VQModelInterfaceHIP(**synthetic.INPAINT_VQ_KWARGS, remap='x.npy')


def test_unet_without_context_refuses_a_context():
    from stable_diffusion_amd import UNetModelHIP
    m = UNetModelHIP(**synthetic.INPAINT_UNET_KWARGS)
    with pytest.raises(ValueError, match='no cross-attention'):
        m(torch.zeros(1, 7, 8, 8), torch.zeros(1, dtype=torch.long), context=torch.zeros(1, 77, 768))
    m.pin_context(torch.zeros(1, 4, 8, 8))          # (no-op: nothing to cache)


def test_library_refuses_latents_not_multiple_of_8():
    from stable_diffusion_amd import UNetModelHIP, _lib
    m = UNetModelHIP(**synthetic.INPAINT_UNET_KWARGS)
    assert m._handle.lib.sdmi_unet_workspace_bytes(m._handle.h, 1, 64, 64, 0) > 0
    assert m._handle.lib.sdmi_unet_workspace_bytes(m._handle.h, 1, 60, 64, 0) == 0
    assert b'multiples of 8' in _lib.load().sdmi_last_error()
    assert m._handle.lib.sdmi_unet_workspace_bytes(m._handle.h, 1, 64, 64, 77) == 0     # a context length: refused
    assert b'no cross-attention' in _lib.load().sdmi_last_error()


def test_concat_conditioning_wrapper():
    from stable_diffusion_amd import LatentDiffusionHIP

    class Probe(torch.nn.Module):
        def forward(self, x, t, context=None):
            assert context is None
            return x[:, :3] + x[:, 3:6] * x[:, 6:7] + t.view(-1, 1, 1, 1)

    ld = LatentDiffusionHIP(Probe(), **synthetic.INPAINT_SCHEDULE)
    x, c = torch.randn(2, 3, 4, 4), torch.randn(2, 4, 4, 4)
    t = torch.tensor([3, 5])
    out = ld.apply_model(x, t, c)
    assert torch.equal(out, x + c[:, :3] * c[:, 3:4] + t.view(-1, 1, 1, 1))
    import numpy as np
    betas = np.linspace(0.0015 ** 0.5, 0.0205 ** 0.5, 1000, dtype=np.float64) ** 2
    assert torch.equal(ld.betas, torch.tensor(betas, dtype=torch.float32))
    assert LatentDiffusionHIP(Probe()).model.conditioning_key == 'crossattn'
    with pytest.raises(NotImplementedError):
        LatentDiffusionHIP(Probe(), conditioning_key='hybrid')


def test_synthetic_generator_is_order_independent_and_seeded():
    specs = [('a.out_layers.3.weight', (4, 4, 3, 3)), ('a.norm.weight', (4,)), ('a.bias', (4,)), ('quantize.embedding.weight', (8, 3))]
    a = synthetic.synthetic_named_state_dict(specs, 0)
    b = synthetic.synthetic_named_state_dict(list(reversed(specs)), 0)
    c = synthetic.synthetic_named_state_dict(specs, 1)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(not torch.equal(a[k], c[k]) for k in a)
    assert float(a['a.out_layers.3.weight'].abs().max()) > 0        # zero_module tensors are drawn too
    sd = synthetic.synthetic_inpaint_unet_state_dict(0)
    assert float(sd['middle_block.1.proj_out.weight'].abs().max()) > 0 and float(sd['out.2.weight'].abs().max()) > 0
