"""The safety checker's feature extractor, host side (no GPU): the numpy restatement of PIL's 8-bit bicubic resize (tests/pil_ref.py) against
PIL itself and against the committed fixtures (tools/make_golden_feature_extractor.py), the library's coefficient tables against the
restatement's, the output-size rule, CLIPFeatureExtractorHIP's constructor / from_pretrained / refusals, and the launcher's switch."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pil_ref
from stable_diffusion_amd import _lib, vision

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W) -> (rh, rw): the ten shapes the restatement was first held to PIL on
PIL_SHAPES = [((512, 512), (224, 224)), ((512, 768), (224, 336)), ((768, 512), (336, 224)), ((40, 56), (28, 39)), ((64, 48), (37, 28)),
              ((256, 256), (224, 224)), ((100, 100), (224, 224)), ((17, 31), (28, 51)), ((224, 224), (224, 224)), ((320, 704), (224, 492))]
FIXTURES = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'clip_fe_*.npz')))
# (in, out): the pairs of the shapes above, the degenerate ends, upscales, a prime pair, long reductions
PAIRS = [(512, 224), (768, 336), (704, 492), (56, 39), (64, 37), (17, 28), (31, 51), (100, 224), (2, 1), (1, 28), (1, 1), (28, 28), (3, 2),
         (2, 3), (1, 2), (1024, 1), (1023, 7), (997, 991), (224, 225), (225, 224), (640, 224), (768, 224), (48, 28), (40, 28), (5000, 3)]


@pytest.mark.parametrize('hw,rhw', PIL_SHAPES, ids=[f'{h}x{w}' for (h, w), _ in PIL_SHAPES])
def test_restatement_is_pil_resize_bit_for_bit(hw, rhw):
    Image = pytest.importorskip('PIL.Image')
    img = np.random.default_rng(hw[0] * 1000 + hw[1]).integers(0, 256, hw + (3,), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img).resize((rhw[1], rhw[0]), Image.BICUBIC))
    assert np.array_equal(pil_ref.resize_u8(img, *rhw), ref)
    assert pil_ref.output_size(hw[0], hw[1], min(rhw)) == rhw


def test_fixtures_are_complete():
    assert sorted(os.path.basename(f) for f in FIXTURES) == ['clip_fe_17x31.npz', 'clip_fe_28x28.npz', 'clip_fe_28x40.npz', 'clip_fe_40x56.npz',
                                                             'clip_fe_64x48.npz', 'clip_fe_blocks_64x48.npz']


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[8:-4] for f in FIXTURES])
def test_restatement_equals_the_fixtures(path):
    """the fixtures carry PIL's and transformers' results; with PIL here, PIL is asked again"""
    z = np.load(path)
    resized, cropped, pv = pil_ref.extract(z['input'], size=28, crop=28)
    assert np.array_equal(resized, z['resized']) and np.array_equal(cropped, z['cropped'])
    assert z['pixel_values'].dtype == np.float32 and np.abs(pv - z['pixel_values']).max() <= 2e-6
    if 'blocks' in path:                      # the ringing of the 0 / 255 edges clips at both ends
        assert z['resized'].min() == 0 and z['resized'].max() == 255
    if path.endswith('28x40.npz'):            # crop only: left = (40 - 28) // 2 = 6
        assert np.array_equal(z['cropped'], z['input'][:, 6:34])
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.fromarray(z['input']).resize(resized.shape[1::-1], Image.BICUBIC)), z['resized'])


@pytest.mark.parametrize('n_in,n_out', PAIRS)
def test_library_tables_equal_the_restatement(n_in, n_out, lib):
    ks, bounds, kk = pil_ref.coeffs(n_in, n_out)
    assert lib.sdmi_fe_ksize(n_in, n_out) == ks == pil_ref.ksize(n_in, n_out)
    got_b, got_k = np.full((n_out, 2), -7, np.int32), np.full((n_out, ks), -7, np.int32)
    assert lib.sdmi_fe_coeffs(n_in, n_out, got_b.ctypes.data, got_k.ctypes.data) == 0
    assert np.array_equal(got_b, bounds) and np.array_equal(got_k, kk)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= ks).all()


def test_library_tables_refuse_sizes_below_one(lib):
    buf = np.zeros(64, np.int32)
    for n_in, n_out in ((0, 4), (4, 0), (-1, 4)):
        assert lib.sdmi_fe_ksize(n_in, n_out) == -1 and 'sizes below 1' in lib.sdmi_last_error().decode()
        assert lib.sdmi_fe_coeffs(n_in, n_out, buf.ctypes.data, buf.ctypes.data) != 0 and 'sizes below 1' in lib.sdmi_last_error().decode()
    assert lib.sdmi_fe_coeffs(4, 4, None, buf.ctypes.data) != 0 and 'null table' in lib.sdmi_last_error().decode()


def test_output_size_rule():
    fe = vision.CLIPFeatureExtractorHIP()
    for (H, W), want in [((512, 512), (224, 224)), ((512, 768), (224, 336)), ((768, 512), (336, 224)), ((320, 704), (224, 492)),
                         ((100, 100), (224, 224)), ((333, 500), (224, 336)), ((500, 333), (336, 224)), ((1, 7), (224, 1568))]:
        assert fe.output_size(H, W) == want == pil_ref.output_size(H, W, 224)
    rng = np.random.default_rng(3)
    for H, W, size in rng.integers(1, 2000, (200, 3)).tolist():
        assert vision.CLIPFeatureExtractorHIP(size=size, crop_size=1).output_size(H, W) == pil_ref.output_size(H, W, size)


def test_host_tables_of_the_extractor():
    fe = vision.CLIPFeatureExtractorHIP(size=28, crop_size=28)
    t = fe.tables(40, 56)
    assert t['h'][0] == pil_ref.ksize(56, 39) and np.array_equal(t['h'][2], pil_ref.coeffs(56, 39)[2])
    assert t['v'][0] == pil_ref.ksize(40, 28) and np.array_equal(t['v'][1], pil_ref.coeffs(40, 28)[1])
    assert fe.tables(28, 40) == {'h': None, 'v': None}                  # no pass on an axis whose size does not change
    t = fe.tables(64, 48)                                               # -> 37 x 28
    assert t['h'][1].shape == (28, 2) and t['v'][1].shape == (37, 2)

def test_constructor_defaults_and_from_pretrained(tmp_path):
    fe = vision.CLIPFeatureExtractorHIP()
    assert (fe.size, fe.crop_size, fe.resample) == (224, 224, 3)
    assert fe.image_mean == pil_ref.CLIP_MEAN and fe.image_std == pil_ref.CLIP_STD
    # the shipped checker's preprocessor_config.json (reference era: plain ints) and a current one (dict sizes)
    old = dict(crop_size=224, do_center_crop=True, do_convert_rgb=True, do_normalize=True, do_resize=True, feature_extractor_type='CLIPFeatureExtractor',
               image_mean=[0.48145466, 0.4578275, 0.40821073], image_std=[0.26862954, 0.26130258, 0.27577711], resample=3, size=224)
    new = dict(old, size={'shortest_edge': 96}, crop_size={'height': 64, 'width': 64}, image_processor_type='CLIPImageProcessor',
               rescale_factor=1 / 255, do_rescale=True, image_mean=[0.5, 0.4, 0.3])
    for name, cfg, want in (('old', old, (224, 224, pil_ref.CLIP_MEAN)), ('new', new, (96, 64, (0.5, 0.4, 0.3)))):
        d = tmp_path / name
        d.mkdir()
        (d / 'preprocessor_config.json').write_text(json.dumps(cfg))
        fe = vision.CLIPFeatureExtractorHIP.from_pretrained(str(d))
        assert (fe.size, fe.crop_size, fe.image_mean) == want
    with pytest.raises(FileNotFoundError, match='local'):              # a hub id is not a local directory: nothing is fetched
        vision.CLIPFeatureExtractorHIP.from_pretrained('CompVis/stable-diffusion-safety-checker')
    with pytest.raises(FileNotFoundError, match='preprocessor_config.json'):
        vision.CLIPFeatureExtractorHIP.from_pretrained(str(tmp_path))
    (tmp_path / 'old' / 'preprocessor_config.json').write_text(json.dumps(dict(old, resample=2)))
    with pytest.raises(NotImplementedError, match='resample'):
        vision.CLIPFeatureExtractorHIP.from_pretrained(str(tmp_path / 'old'))


def test_refusals_by_name():
    import torch
    F = vision.CLIPFeatureExtractorHIP
    for resample in (0, 1, 2, 4, 5):
        with pytest.raises(NotImplementedError, match='resample'):
            F(resample=resample)
    for flag in ('do_resize', 'do_center_crop', 'do_normalize'):
        with pytest.raises(NotImplementedError, match=flag):
            F(**{flag: False})
    with pytest.raises(NotImplementedError, match='crop_size > size'):
        F(size=224, crop_size=256)
    with pytest.raises(NotImplementedError, match='crop_size'):
        F(crop_size={'height': 224, 'width': 200})
    fe = F()
    with pytest.raises(RuntimeError, match='no CPU fallback'):          # a CPU float tensor: there is no CPU path
        fe(torch.zeros(1, 64, 64, 3))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        fe(np.zeros((64, 64, 3), np.float32))
    with pytest.raises(NotImplementedError, match="'pt' only"):
        fe(np.zeros((64, 64, 3), np.uint8), return_tensors='np')
    with pytest.raises(NotImplementedError, match='RGB'):
        fe([np.zeros((64, 64, 4), np.uint8)])
    b = vision.FeatureBatch(pixel_values=1)
    assert b.pixel_values == 1 and b['pixel_values'] == 1 and not hasattr(b, 'other')


def test_launcher_switch_installs_the_hip_extractor(tmp_path):
    """tools/run_reference_script.py --hip-feature-extractor: the switch exists, and install_stubs with the keyword makes
    AutoFeatureExtractor.from_pretrained return the HIP class -- from the checker directory's preprocessor_config.json when there is one, with the
    defaults otherwise.  In a child process (install_stubs patches modules for good); nothing is launched."""
    pytest.importorskip('transformers')
    pytest.importorskip('yaml')
    (tmp_path / 'preprocessor_config.json').write_text(json.dumps(dict(size=96, crop_size=64, resample=3)))
    code = f'''
import importlib.util, inspect, io, contextlib, sys
sys.path.insert(0, {ROOT!r})
spec = importlib.util.spec_from_file_location('run_reference_script', {os.path.join(ROOT, 'tools', 'run_reference_script.py')!r})
m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
assert inspect.signature(m.install_stubs).parameters['hip_feature_extractor'].default is None
buf = io.StringIO()
sys.argv = ['run_reference_script.py', '--help']
with contextlib.redirect_stdout(buf):
    try:
        m.main()
    except SystemExit:
        pass
assert '--hip-feature-extractor' in buf.getvalue() and '--hip-safety-dir' in buf.getvalue()
from stable_diffusion_amd.vision import CLIPFeatureExtractorHIP
import transformers
m.install_stubs(False, offline_stubs=True, hip_feature_extractor={str(tmp_path)!r})
fe = transformers.AutoFeatureExtractor.from_pretrained('CompVis/stable-diffusion-safety-checker')
assert type(fe) is CLIPFeatureExtractorHIP and (fe.size, fe.crop_size) == (96, 64)
m.install_stubs(False, offline_stubs=True, hip_feature_extractor='default')
fe = transformers.AutoFeatureExtractor.from_pretrained('CompVis/stable-diffusion-safety-checker')
assert type(fe) is CLIPFeatureExtractorHIP and (fe.size, fe.crop_size) == (224, 224)
print('LAUNCHER-OK')
'''
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=str(tmp_path),
                       env=dict(os.environ, HF_HUB_OFFLINE='1', TRANSFORMERS_OFFLINE='1'))
    assert r.returncode == 0 and 'LAUNCHER-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
