"""bsr_sr's tiled image pipeline, host side (no GPU): the weighting restatement against the reference's get_fold_unfold
(tests/golden/superres_fold.npz, tools/make_golden_superres.py), window geometry, every refusal before any library call, the untouched
un-tiled path of LatentDiffusionHIP, and SuperResolutionHIP built from models/ldm/bsr_sr's parsed yaml."""
import json
import os

import numpy as np
import pytest
import torch

from stable_diffusion_amd import LatentDiffusionHIP, SuperResolutionHIP, _lib, ldm_shim, superres, synthetic

CLIPS = dict(clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
# name, (H, W), ks, stride, uf, df, tie_braker (tools/make_golden_superres.py FOLD_GEOMS)
FOLD_GEOMS = [('s1', (32, 32), (16, 16), (16, 16), 1, 1, False), ('s2', (24, 32), (16, 16), (8, 8), 1, 1, False),
              ('s4', (32, 32), (16, 16), (4, 4), 1, 1, False), ('s2_tie', (24, 32), (16, 16), (8, 8), 1, 1, True),
              ('s4_tie', (32, 32), (16, 16), (4, 4), 1, 1, True), ('uf4', (24, 32), (16, 16), (8, 8), 4, 1, False),
              ('uf4_tie', (24, 32), (16, 16), (8, 8), 4, 1, True), ('df4', (64, 96), (32, 32), (16, 16), 1, 4, False),
              ('rect', (24, 24), (16, 8), (8, 8), 1, 1, False), ('unaligned', (21, 27), (9, 11), (3, 4), 1, 1, False),
              ('unaligned_tie', (21, 27), (9, 11), (3, 4), 1, 1, True)]


def params(ks, stride, tie=False, **kw):
    return dict(ks=tuple(ks), stride=tuple(stride), vqf=4, patch_distributed_vq=True, tie_braker=tie, **CLIPS, **kw)


@pytest.fixture
def no_library(monkeypatch):
    """any library call fails the test"""
    def load():
        raise AssertionError('a refused geometry reached the library')
    monkeypatch.setattr(_lib, 'load', load)


@pytest.mark.parametrize('name,hw,ks,stride,uf,df,tie', FOLD_GEOMS, ids=[g[0] for g in FOLD_GEOMS])
def test_weighting_equals_reference_bit_for_bit(name, hw, ks, stride, uf, df, tie, golden_dir):
    z = np.load(os.path.join(golden_dir, 'superres_fold.npz'))
    Ly, Lx = ldm_shim.patch_grid(hw[0], hw[1], ks, stride)
    w = ldm_shim.patch_weighting(ks[0] * uf // df, ks[1] * uf // df, Ly, Lx, params(ks, stride, tie))
    ref = torch.from_numpy(z[f'{name}_weighting'])                   # (1, 1, kh', kw', L)
    assert w.dtype == torch.float32 and tuple(w.shape) == (Ly * Lx, ref.shape[2], ref.shape[3])
    assert torch.equal(w, ref[0, 0].permute(2, 0, 1))
    assert ldm_shim.patch_weighting(ks[0] * uf // df, ks[1] * uf // df, Ly, Lx, params(ks, stride, tie)) is w        # cached per geometry


def test_window_origins_and_counts():
    assert ldm_shim.patch_grid(24, 32, (16, 16), (8, 8)) == (2, 3)
    assert ldm_shim.window_origins(24, 32, (16, 16), (8, 8)) == [(0, 0), (0, 8), (0, 16), (8, 0), (8, 8), (8, 16)]
    assert ldm_shim.patch_grid(256, 256, (128, 128), (64, 64)) == (3, 3)
    assert ldm_shim.patch_grid(21, 27, (9, 11), (3, 4)) == (5, 5)
    assert ldm_shim.window_origins(21, 27, (9, 11), (3, 4))[-1] == (12, 16)
    assert ldm_shim.patch_grid(16, 16, (16, 16), (8, 8)) == (1, 1)
    # torch.nn.Unfold's own block order and count
    x = torch.arange(24 * 32, dtype=torch.float32).view(1, 1, 24, 32)
    cols = torch.nn.Unfold((16, 16), stride=(8, 8))(x)
    assert cols.shape[-1] == 6
    for l, (y0, x0) in enumerate(ldm_shim.window_origins(24, 32, (16, 16), (8, 8))):
        assert torch.equal(cols[0, :, l].view(16, 16), x[0, 0, y0:y0 + 16, x0:x0 + 16])


def test_chunks_are_whole_windows_of_at_most_eight_rows():
    ld = LatentDiffusionHIP(torch.nn.Identity(), conditioning_key='concat')
    ld.split_input_params = params((16, 16), (8, 8))
    assert ld._window_chunks(6, 2) == [(0, 4), (4, 2)]              # 8 + 4 rows
    assert ld._window_chunks(9, 1) == [(0, 8), (8, 1)]
    assert ld._window_chunks(3, 10) == [(0, 1), (1, 1), (2, 1)]     # a batch above 8 rows: one window per call, the UNet splits it


@pytest.mark.parametrize('hw,ks,stride', [((12, 32), (16, 16), (8, 8)), ((24, 12), (16, 16), (8, 8)),      # kh > H, kw > W
                                          ((28, 32), (16, 16), (8, 8)), ((24, 30), (16, 16), (8, 8))])     # off the grid
def test_bad_geometry_raises_value_error_before_the_library(hw, ks, stride, no_library):
    x = torch.zeros(1, 3, *hw)
    with pytest.raises(ValueError, match='split_input_params'):
        ldm_shim.patch_unfold(x, None, ks, stride, 0, 1)
    with pytest.raises(ValueError, match='split_input_params'):
        ldm_shim.patch_fold(x, x, 1, hw, ks, stride)
    ld = LatentDiffusionHIP(torch.nn.Identity(), conditioning_key='concat', cond_stage_key='LR_image')
    ld.split_input_params = params(ks, stride)
    with pytest.raises(ValueError, match='split_input_params'):
        ld.apply_model(x, torch.zeros(1, dtype=torch.long), x)


@pytest.mark.parametrize('hw,ks,stride,uf,df,what', [((32, 32), (16, 16), (8, 8), 4, 4, 'at most one'), ((32, 32), (16, 16), (8, 8), 0, 1, 'positive'),
                                                     ((24, 24), (16, 8), (8, 8), 4, 1, 'non-square'), ((24, 24), (16, 8), (8, 8), 1, 4, 'non-square'),
                                                     ((36, 36), (18, 18), (9, 9), 1, 4, 'must divide')])
def test_patch_fold_refuses_bad_scaling_before_the_library(hw, ks, stride, uf, df, what, no_library):
    o, w = torch.zeros(9, 2, 16, 16), torch.zeros(9, 16, 16)
    for norm_only in (False, True):
        with pytest.raises(ValueError, match=what):
            ldm_shim.patch_fold(o, w, 1, hw, ks, stride, uf=uf, df=df, norm_only=norm_only)


class _FirstStage(torch.nn.Module):
    def decode(self, z):
        return ('dec', z)

    def encode(self, x):
        return ('enc', x)


def test_first_stage_refusals_before_the_library(no_library):
    ld = LatentDiffusionHIP(torch.nn.Identity(), conditioning_key='concat', first_stage_model=_FirstStage())
    ld.split_input_params = params((16, 8), (8, 8))
    with pytest.raises(ValueError, match='non-square'):
        ld.decode_first_stage(torch.zeros(1, 3, 24, 24))
    with pytest.raises(ValueError, match='non-square'):
        ld.encode_first_stage(torch.zeros(1, 3, 24, 24))
    ld.split_input_params = params((18, 18), (9, 9))
    with pytest.raises(ValueError, match='must divide'):
        ld.encode_first_stage(torch.zeros(1, 3, 36, 36))
    with pytest.raises(NotImplementedError):
        ld.decode_first_stage(torch.zeros(1, 3, 36, 36), predict_cids=True)


def test_tie_braker_on_a_single_row_or_column_of_windows(no_library):
    for Ly, Lx in ((1, 3), (3, 1), (1, 1)):
        with pytest.raises(ValueError, match='tie_braker'):
            ldm_shim.patch_weighting(16, 16, Ly, Lx, params((16, 16), (8, 8), True))
    ld = LatentDiffusionHIP(torch.nn.Identity(), conditioning_key='concat', cond_stage_key='LR_image')
    ld.split_input_params = params((16, 16), (8, 8), True)
    x = torch.zeros(1, 3, 16, 32)                                    # the reference's weights are NaN here
    with pytest.raises(ValueError, match='tie_braker'):
        ld.apply_model(x, torch.zeros(1, dtype=torch.long), x)


def test_apply_model_asserts_and_coordinates_bbox(no_library):
    x, t = torch.zeros(1, 3, 24, 32), torch.zeros(1, dtype=torch.long)
    ld = LatentDiffusionHIP(torch.nn.Identity(), conditioning_key='crossattn', cond_stage_key='coordinates_bbox')
    ld.split_input_params = params((16, 16), (8, 8))
    with pytest.raises(NotImplementedError, match='coordinates_bbox'):
        ld.apply_model(x, t, torch.zeros(1, 4, 8))
    with pytest.raises(AssertionError):
        ld.apply_model(x, t, {'c_concat': [x], 'c_crossattn': [torch.zeros(1, 4, 8)]})         # len(cond) == 1
    with pytest.raises(AssertionError):
        ld.apply_model(x, t, torch.zeros(1, 4, 8), return_ids=True)


class _RecordingUNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x, t, context=None):
        self.calls.append((x, t, context))
        return x[:, :3] * 2


@pytest.mark.parametrize('key', ['concat', 'crossattn', None])
def test_without_split_input_params_forwards_exactly_as_before(key, no_library):
    unet = _RecordingUNet()
    ld = LatentDiffusionHIP(unet, conditioning_key=key)
    assert not hasattr(ld, 'split_input_params') and ld.first_stage_model is None and ld.scale_factor == 1.0 and ld.cond_stage_key is None
    assert sorted(ld.state_dict()) == ['alphas_cumprod', 'alphas_cumprod_prev', 'betas', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod']
    x, t = torch.randn(2, 3, 24, 32), torch.tensor([5, 7])
    c = {'concat': torch.randn(2, 3, 24, 32), 'crossattn': torch.randn(2, 4, 8), None: None}[key]
    out = ld.apply_model(x, t, c)
    (xa, ta, ctx), = unet.calls
    assert ta is t and torch.equal(out, xa[:, :3] * 2)
    if key == 'concat':
        assert torch.equal(xa, torch.cat([x, c], 1)) and ctx is None
    elif key == 'crossattn':
        assert xa is x and ctx is c
    else:
        assert xa is x and ctx is None


def test_plain_first_stage_calls_without_tiling(no_library):
    ld = LatentDiffusionHIP(torch.nn.Identity(), first_stage_model=_FirstStage(), scale_factor=0.5)
    z = torch.ones(1, 3, 4, 4)
    tag, got = ld.decode_first_stage(z)
    assert tag == 'dec' and torch.equal(got, 2 * z)                  # 1 / scale_factor * z
    assert ld.encode_first_stage(z)[1] is z
    ld.split_input_params = params((16, 16), (8, 8))
    ld.split_input_params['patch_distributed_vq'] = False
    assert ld.decode_first_stage(z)[0] == 'dec' and ld.encode_first_stage(z)[1] is z and 'original_image_size' not in ld.split_input_params


def test_superres_instantiates_from_the_reference_config(golden_dir):
    with open(os.path.join(golden_dir, 'bsr_sr_config.json')) as f:
        cfg = json.load(f)
    fs = cfg['model']['params']['first_stage_config']['params']
    assert dict(embed_dim=fs['embed_dim'], n_embed=fs['n_embed'], ddconfig=dict(fs['ddconfig'])) == superres.BSR_VQ_KWARGS == synthetic.FACES_VQ_KWARGS
    sr = SuperResolutionHIP.from_config(cfg)
    assert sr.model.conditioning_key == 'concat' and sr.cond_stage_key == 'LR_image' and sr.scale_factor == 1.0
    assert sr.model.diffusion_model.in_channels == 6 and sr.model.diffusion_model.out_channels == 3
    assert isinstance(sr.cond_stage_model, torch.nn.Identity) and sr.num_timesteps == 1000
    assert abs(float(sr.betas[0]) - 0.0015) < 1e-9 and abs(float(sr.betas[-1]) - 0.0155) < 1e-8
    with open(os.path.join(golden_dir, 'bsr_unet_state_dict_keys.json')) as f:
        keys = {k for k, _ in json.load(f)['keys']}
    assert {k[len('model.diffusion_model.'):] for k in sr.state_dict() if k.startswith('model.diffusion_model.')} == keys
    assert any(k.startswith('first_stage_model.decoder.') for k in sr.state_dict())
    p = sr.tile_params
    assert (p['ks'], p['stride'], p['vqf'], p['patch_distributed_vq'], p['tie_braker']) == ((128, 128), (64, 64), 4, True, False)
    assert (p['clip_min_weight'], p['clip_max_weight']) == (0.01, 0.5)


def test_superres_tiling_switch_and_off_grid_message():
    sr = SuperResolutionHIP()
    assert sr.configure_tiling(128, 96) is False and not hasattr(sr, 'split_input_params')
    assert sr.configure_tiling(256, 192) is True and sr.split_input_params['ks'] == (128, 128)
    assert sr.configure_tiling(64, 64) is False and not hasattr(sr, 'split_input_params')
    with pytest.raises(ValueError, match=r'height 192 or 256, width 256 or 320'):
        sr.configure_tiling(200, 300)
    with pytest.raises(ValueError, match=r'height 128, width 256'):
        sr.configure_tiling(100, 256)
    assert superres.nearest_valid_sizes(256, 128, 64) == (256, 256) and superres.nearest_valid_sizes(257, 128, 64) == (256, 320)
    with pytest.raises(ValueError, match='3, h, w'):
        sr.upscale(torch.zeros(1, 4, 8, 8))
