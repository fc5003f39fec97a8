"""The safety checker's feature extractor on the MI355X (sdmi_k_clip_feature_extract, CLIPFeatureExtractorHIP, check_images, check_safety).

Kernels run in guarded buffers (tests/guard.py; guards checked after every call, the source compared with what was uploaded).  The resized and
cropped uint8 image must EQUAL PIL's: the committed fixtures carry PIL's own bytes (tools/make_golden_feature_extractor.py), the larger shapes
are held to the numpy restatement (tests/pil_ref.py) that tests/test_feature_extractor_host.py holds to PIL bit for bit.

pixel_values: 2e-6 max-abs against the fp64 restatement and against transformers' fp32 values in the fixtures.  The bound: three correctly
rounded fp32 operations on fp32 constants, u / 255 (|.| <= 1, 6e-8), - mean (6e-8), / std (std ~ 0.26 amplifies both by 3.8 and rounds a
|value| <= 2.3 once more: 2.4e-7 of its own, plus the constants' own rounding), 8.6e-7 worst case; the bar is that, doubled and rounded up.

Measured on an MI355X (max-abs | bar): every uint8 comparison equal; pixel_values against fp64 1.7e-7 ... 2.8e-7 on the fixtures and on the four
224 shapes, against transformers' fp32 values 0.0 on every fixture | 2e-6.  255 of 255 constructed n + 0.5 products exist in fp32.  The two
check_images pictures' embeddings sit at cosine 0.66, scores +0.02 / -0.02.  All 18 cases together take under 2 s.
"""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import pil_ref  # noqa: E402
from stable_diffusion_amd import _lib, postprocess, synthetic, vision  # noqa: E402

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'clip_fe_*.npz')))
U8, F_NHWC, F_NCHW, F_RAW = 0, 1, 2, 3
PV_TOL = 2e-6
_cache = {}


def _run(src, kind, size, crop, case, mean=pil_ref.CLIP_MEAN, std=pil_ref.CLIP_STD):
    """one call of the C entry on a host tensor, everything the kernels touch in guarded buffers -> (pixel_values, uint8 image) as numpy"""
    lib = _lib.load()
    B = src.shape[0]
    H, W = (src.shape[1], src.shape[2]) if kind in (U8, F_NHWC) else (src.shape[2], src.shape[3])
    P = guard.Pool(DEV)
    gsrc = P.put('source', src)
    t = vision.CLIPFeatureExtractorHIP(size=size, crop_size=crop).tables(H, W)
    dev = {}
    for ax in 'hv':
        ks, b, k = t[ax] or (0, None, None)
        dev[ax] = (ks, None if b is None else P.put(ax + '_bounds', torch.from_numpy(b)), None if k is None else P.put(ax + '_kk', torch.from_numpy(k)))
    need = lib.sdmi_fe_workspace_bytes(B, H, W, size, crop)
    assert need >= 0
    ws = P.new('workspace', (max(int(need), 1),), torch.uint8)
    pv = P.new('pixel_values', (B, 3, crop, crop), torch.float32)
    u8 = P.new('uint8 image', (B, crop, crop, 3), torch.uint8)
    import ctypes as C
    _lib.check(lib.sdmi_k_clip_feature_extract(gsrc.data_ptr(), kind, B, 3, H, W, size, crop, _lib.ptr(dev['h'][1]), _lib.ptr(dev['h'][2]), dev['h'][0],
                                               _lib.ptr(dev['v'][1]), _lib.ptr(dev['v'][2]), dev['v'][0], (C.c_float * 3)(*mean), (C.c_float * 3)(*std),
                                               ws.data_ptr(), int(need), pv.data_ptr(), u8.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    P.check(case)
    assert torch.equal(gsrc.cpu(), src), f'{case}: the source was written'
    return pv.cpu().numpy(), u8.cpu().numpy()


def _pv_err(pv, cropped_u8):
    return max(float(np.abs(pv[b].astype(np.float64) - pil_ref.pixel_values(cropped_u8[b])).max()) for b in range(pv.shape[0]))


# ---- uint8 source -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[8:-4] for f in FIXTURES])
def test_uint8_source_equals_the_pil_fixtures(path):
    z = np.load(path)
    pv, u8 = _run(torch.from_numpy(z['input'])[None], U8, 28, 28, os.path.basename(path))
    assert np.array_equal(u8[0], z['cropped'])
    e64, etr = _pv_err(pv, z['cropped'][None]), float(np.abs(pv[0] - z['pixel_values']).max())
    print(f'[feature extractor] {os.path.basename(path)}: pixel_values vs fp64 {e64:.3e}, vs transformers {etr:.3e} | {PV_TOL:.0e}', flush=True)
    assert e64 <= PV_TOL and etr <= PV_TOL


@pytest.mark.parametrize('B,H,W', [(2, 512, 512), (2, 512, 768), (1, 768, 512), (1, 320, 704)])
def test_uint8_source_equals_the_restatement_at_224(B, H, W):
    """the shapes a user runs: several column tiles and row groups, a crop window narrower (or shorter) than the resized image -- the guards
    show that restricting the passes to the window reads and writes nothing outside it"""
    img = np.random.default_rng(H * 7 + W).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    pv, u8 = _run(torch.from_numpy(img), U8, 224, 224, f'{B}x{H}x{W}')
    ref = np.stack([pil_ref.extract(img[b])[1] for b in range(B)])
    assert np.array_equal(u8, ref), f'{int((u8 != ref).sum())} bytes differ'
    err = _pv_err(pv, ref)
    print(f'[feature extractor] {B}x{H}x{W} -> 224: pixel_values vs fp64 {err:.3e} | {PV_TOL:.0e}', flush=True)
    assert err <= PV_TOL


def test_custom_mean_std_and_crop_smaller_than_size():
    """constants that are exact in fp32; |value| <= 7, so the bound is 8 x (6e-8 + 6e-8) through the division by 0.125 plus half an ulp of 7
    (2.4e-7): 1.2e-6, doubled and rounded up"""
    img = np.random.default_rng(5).integers(0, 256, (3, 50, 70, 3), dtype=np.uint8)
    mean, std = (0.5, 0.25, 0.125), (0.5, 0.25, 0.125)
    pv, u8 = _run(torch.from_numpy(img), U8, 36, 21, 'crop 21 of 36', mean, std)                   # 50 x 70 -> 36 x 50, top 7, left 14
    ref = [pil_ref.extract(img[b], 36, 21, mean, std) for b in range(3)]
    assert np.array_equal(u8, np.stack([r[1] for r in ref]))
    assert max(float(np.abs(pv[b] - ref[b][2]).max()) for b in range(3)) <= 3e-6


# ---- fp32 sources -----------------------------------------------------------------------------------------------------------------------
def _rounding_probe():
    """28 x 28 x 3 floats (nothing is resized at size 28: the uint8 output IS the conversion): every k / 255, values whose fp32 product with 255
    is exactly n + 0.5, the ends, values just outside [0, 1], random filler"""
    vals = [np.float32(k) / np.float32(255) for k in range(256)]
    halves = []
    for n in range(255):
        x = np.float32((n + 0.5) / 255)
        for cand in (x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-1))):
            if np.float32(cand) * np.float32(255) == np.float32(n + 0.5):
                halves.append(np.float32(cand))
                break
    assert len(halves) >= 64, len(halves)                       # ties exist in fp32, and both parities: half to even is told from half up
    assert {int(h * np.float32(255)) % 2 for h in halves} == {0, 1}
    ends = [0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(0), np.float32(-1)), -0.001, 1.001, -0.0, 0.5]
    flat = np.random.default_rng(9).random(28 * 28 * 3).astype(np.float32)
    head = np.asarray(vals + halves + ends, dtype=np.float32)
    flat[:head.size] = head
    return flat.reshape(1, 28, 28, 3), len(halves)


def test_float_conversion_is_numpy_to_pil_rounding():
    x, n_halves = _rounding_probe()
    want = (x * 255).round().astype(np.uint8)                   # numpy_to_pil's own expression (every product rounds inside 0 .. 255)
    assert ((x * 255).round() >= 0).all() and ((x * 255).round() <= 255).all()
    _, u8 = _run(torch.from_numpy(x), F_NHWC, 28, 28, 'rounding probe NHWC')
    assert np.array_equal(u8, want), np.argwhere(u8 != want)[:8]
    _, u8c = _run(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))), F_NCHW, 28, 28, 'rounding probe NCHW')
    assert np.array_equal(u8c, want)
    # far outside the range: clamped (numpy's cast is undefined there)
    far = np.full((1, 28, 28, 3), 7.5, np.float32)
    far[0, ::2] = -3.0
    _, u8f = _run(torch.from_numpy(far), F_NHWC, 28, 28, 'far outside')
    assert (u8f[0, 1::2] == 255).all() and (u8f[0, ::2] == 0).all()
    print(f'[feature extractor] rounding probe: {n_halves} exact n + 0.5 products', flush=True)


def test_float_layouts_and_the_raw_kind_give_the_same_bits():
    g = torch.Generator().manual_seed(17)
    x = torch.rand((2, 40, 56, 3), generator=g)
    ref = np.stack([pil_ref.extract(pil_ref.to_u8(x[b].numpy()), 28, 28)[1] for b in range(2)])
    pv_a, u8_a = _run(x, F_NHWC, 28, 28, 'float NHWC')
    pv_b, u8_b = _run(x.permute(0, 3, 1, 2).contiguous(), F_NCHW, 28, 28, 'float NCHW')
    assert np.array_equal(u8_a, ref) and np.array_equal(u8_b, ref)
    assert np.array_equal(pv_a.view(np.uint32), pv_b.view(np.uint32)) and _pv_err(pv_a, ref) <= PV_TOL
    raw = (torch.rand((2, 3, 40, 56), generator=g) * 2.6 - 1.3)                # beyond [-1, 1] on both sides: the clamp matters
    pv_r, u8_r = _run(raw, F_RAW, 28, 28, 'raw decoder output')
    clamped = torch.clamp((raw.to(DEV) + 1.0) / 2.0, min=0.0, max=1.0).cpu()   # txt2img.py:314 as torch runs it on the device
    pv_c, u8_c = _run(clamped, F_NCHW, 28, 28, 'clamped, then [0, 1]')
    assert np.array_equal(u8_r, u8_c) and np.array_equal(pv_r.view(np.uint32), pv_c.view(np.uint32))
    assert (clamped == 0).any() and (clamped == 1).any() and (raw.abs() > 1).any()


# ---- the Python class -------------------------------------------------------------------------------------------------------------------
def test_two_calls_same_bits_and_the_table_cache():
    fe = vision.CLIPFeatureExtractorHIP(size=28, crop_size=28)
    rng = np.random.default_rng(23)
    a = torch.from_numpy(rng.integers(0, 256, (2, 40, 56, 3), dtype=np.uint8)).to(DEV)
    b = torch.from_numpy(rng.integers(0, 256, (1, 64, 48, 3), dtype=np.uint8)).to(DEV)
    pv1, u1 = fe.extract(a, return_uint8=True)
    first = {k: tuple(t.clone() if torch.is_tensor(t) else t for t in v) for k, v in fe._tables[(40, 56, str(a.device))].items()}
    pvb = fe(b).pixel_values                                     # a second size in between
    pv2, u2 = fe.extract(a, return_uint8=True)
    assert torch.equal(pv1, pv2) and torch.equal(u1, u2) and len(fe._tables) == 2
    host = fe.tables(40, 56)
    for ax in 'hv':
        now = fe._tables[(40, 56, str(a.device))][ax]
        assert now[0] == host[ax][0] == first[ax][0]
        assert all(torch.equal(now[i], first[ax][i]) and np.array_equal(now[i].cpu().numpy(), host[ax][i]) for i in (1, 2))
    assert np.array_equal(u1.cpu().numpy(), np.stack([pil_ref.extract(a[i].cpu().numpy(), 28, 28)[1] for i in range(2)]))
    out = fe(b)
    assert out['pixel_values'] is out.pixel_values and out.pixel_values.is_cuda and out.pixel_values.dtype == torch.float32
    assert torch.equal(out.pixel_values, pvb) and tuple(pvb.shape) == (1, 3, 28, 28)


def test_host_images_numpy_and_lists_of_mixed_sizes():
    fe = vision.CLIPFeatureExtractorHIP(size=28, crop_size=28)
    rng = np.random.default_rng(29)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((40, 56), (64, 48), (40, 56), (28, 40))]
    want = np.stack([pil_ref.extract(im, 28, 28)[2] for im in imgs])
    got = fe(imgs, return_tensors='pt').pixel_values
    assert tuple(got.shape) == (4, 3, 28, 28) and np.abs(got.cpu().numpy() - want).max() <= PV_TOL
    assert torch.equal(fe(imgs[1]).pixel_values, got[1:2]) and torch.equal(fe(np.stack([imgs[0], imgs[2]])).pixel_values, got[[0, 2]])
    try:
        from PIL import Image
    except ImportError:
        return
    assert torch.equal(fe([Image.fromarray(im) for im in imgs]).pixel_values, got)


# ---- the safety check on device images ------------------------------------------------------------------------------------------------------
def _checker():
    """VIT_TINY-sized checker (image_size 28) on two synthetic decoder outputs; concept 5 is built from the tower's own embeddings of the two
    images so that image 0 scores +0.02 and image 1 -0.02 against it, every other score at most -0.02: far from a threshold"""
    if 'checker' in _cache:
        return _cache['checker']
    import vit_ref
    cfg = synthetic.VIT_TINY
    g = torch.Generator().manual_seed(41)
    xs = torch.randn((2, 3, 40, 56), generator=g) * 0.8
    xs[1] = -xs[1].flip(2) * 0.3 + torch.linspace(-1, 1, 56)[None, None, :]            # a different picture, not a second noise field
    xs = xs.to(DEV)
    x01 = torch.clamp((xs + 1.0) / 2.0, min=0.0, max=1.0)
    fe = vision.CLIPFeatureExtractorHIP(size=cfg['image_size'], crop_size=cfg['image_size'])
    checker = vision.StableDiffusionSafetyCheckerHIP(cfg)
    sd = synthetic.synthetic_vision_state_dict(cfg, 7)
    csd = {('vision_model.' + k if k.startswith('vision_model.') else k): v for k, v in sd.items()}
    Nc, Ns, E = 17, 3, cfg['projection_dim']
    csd.update(concept_embeds=torch.ones(Nc, E), special_care_embeds=torch.ones(Ns, E), concept_embeds_weights=torch.ones(Nc),
               special_care_embeds_weights=torch.ones(Ns))
    checker.load_state_dict(csd, strict=True)
    checker.to(DEV)
    emb = checker._tower[0](fe(x01, layout='NCHW').pixel_values)[0].cpu().numpy().astype(np.float64)
    u0, u1 = emb[0] / np.linalg.norm(emb[0]), emb[1] / np.linalg.norm(emb[1])
    c01 = float(u0 @ u1)
    s = np.sqrt(1.0 - c01 * c01)
    print(f'[check_images] cosine between the two images\' embeddings {c01:.4f}', flush=True)
    assert s > 0.08, c01                                                             # (the construction below needs |q| < 1)
    rng = np.random.default_rng(43)
    concepts, special = rng.standard_normal((Nc, E)), rng.standard_normal((Ns, E))
    e1 = (u1 - c01 * u0) / s
    w = concepts[5] - (concepts[5] @ u0) * u0
    w = w - (w @ e1) * e1
    p, q = 0.02, (-0.02 - 0.02 * c01) / s
    concepts[5] = 3.0 * (p * u0 + q * e1 + np.sqrt(1.0 - p * p - q * q) * w / np.linalg.norm(w))
    assert np.allclose(vit_ref.cosines(emb, concepts[5:6])[:, 0], [0.02, -0.02], atol=1e-12)
    thr_c, thr_s = vit_ref.cosines(emb, concepts).max(0) + 0.02, vit_ref.cosines(emb, special).max(0) + 0.02
    thr_c[5] = 0.0
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(DEV)       # noqa: E731
    checker.concept_embeds.data.copy_(f32(concepts)); checker.special_care_embeds.data.copy_(f32(special))
    checker.concept_embeds_weights.data.copy_(f32(thr_c)); checker.special_care_embeds_weights.data.copy_(f32(thr_s))
    _cache['checker'] = (checker, fe, xs, x01)
    return _cache['checker']


def test_check_images_is_the_extractor_then_forward():
    checker, fe, _, x01 = _checker()
    for layout, x in (('NCHW', x01), ('NHWC', x01.permute(0, 2, 3, 1).contiguous())):
        a, b = x.clone(), x.clone()
        out, has = checker.check_images(a, extractor=fe, layout=layout)
        scores = checker.last_scores['concept_scores'].clone()
        ref, ref_has = checker(clip_input=fe(b, layout=layout).pixel_values, images=b)
        assert has == ref_has == [True, False] and all(type(v) is bool for v in has)
        assert out.is_cuda and out.shape == x.shape and torch.equal(out, ref) and torch.equal(scores, checker.last_scores['concept_scores'])
        assert not out[0].any() and torch.equal(out[1].view(torch.int32), x[1].view(torch.int32))
        assert abs(float(scores[0, 5]) - 0.02) <= 1e-3 and float(scores[1].max()) <= -0.02 + 1e-3
    u8 = (x01.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous()          # the uint8 kind, and the checker's own default extractor
    out, has = checker.check_images(u8.clone())
    assert has == [True, False] and not out[0].any() and torch.equal(out[1], u8[1])
    with pytest.raises(ValueError, match='image_size'):
        checker.check_images(x01.clone(), extractor=vision.CLIPFeatureExtractorHIP(size=32, crop_size=32), layout='NCHW')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        checker.check_images(x01.cpu(), layout='NCHW')


def test_postprocess_check_safety_is_the_chain_of_its_parts():
    checker, fe, xs, x01 = _checker()
    keep = xs.clone()
    out, has = postprocess.check_safety(xs, checker, fe)
    assert torch.equal(xs, keep)                                                      # the decoder output itself is left alone
    ref, ref_has = checker(clip_input=fe(x01, layout='NCHW').pixel_values, images=x01.clone())
    assert has == ref_has == [True, False] and torch.equal(out, ref)
    assert tuple(out.shape) == (2, 3, 40, 56) and out.dtype == torch.float32 and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    # the raw-decoder kind on xs is the [0, 1] kind on the clamped image, bit for bit
    assert torch.equal(fe(xs, layout='NCHW', value_range=(-1, 1)).pixel_values, fe(x01, layout='NCHW').pixel_values)
    out2, has2 = postprocess.check_safety(xs, checker)                                # default extractor: the tower's image size
    assert has2 == has and torch.equal(out2, out)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_launcher_refusals_set_the_error_and_launch_nothing():
    import ctypes as C
    lib = _lib.load()
    P = guard.Pool(DEV)
    src = P.put('source', torch.zeros((1, 40, 56, 3), dtype=torch.uint8))
    t = vision.CLIPFeatureExtractorHIP(size=28, crop_size=28).tables(40, 56)
    hb, hk, vb, vk = (P.put(n, torch.from_numpy(a)) for n, a in (('hb', t['h'][1]), ('hk', t['h'][2]), ('vb', t['v'][1]), ('vk', t['v'][2])))
    ws = P.new('workspace', (1 << 16,), torch.uint8)
    pv = P.new('pixel_values', (1, 3, 32, 32), torch.float32)
    u8 = P.new('uint8 image', (1, 32, 32, 3), torch.uint8)
    mean, std = (C.c_float * 3)(*pil_ref.CLIP_MEAN), (C.c_float * 3)(*pil_ref.CLIP_STD)
    hks, vks = t['h'][0], t['v'][0]

    def call(kind=U8, B=1, Cc=3, H=40, W=56, size=28, crop=28, hks=hks, vks=vks, ws_bytes=1 << 16):
        return lib.sdmi_k_clip_feature_extract(src.data_ptr(), kind, B, Cc, H, W, size, crop, hb.data_ptr(), hk.data_ptr(), hks, vb.data_ptr(),
                                               vk.data_ptr(), vks, mean, std, ws.data_ptr(), ws_bytes, pv.data_ptr(), u8.data_ptr(),
                                               _lib.stream_ptr())
    for kw, name in ((dict(crop=32), 'crop_size > size'), (dict(Cc=4), 'channel count other than 3'), (dict(Cc=1), 'channel count other than 3'),
                     (dict(size=0), 'sizes below 1'), (dict(crop=0), 'sizes below 1'), (dict(H=0), 'sizes below 1'), (dict(B=0), 'sizes below 1'),
                     (dict(hks=hks + 2), "horizontal tables' ksize does not match"), (dict(vks=vks - 2), "vertical tables' ksize does not match"),
                     (dict(H=80, W=112), 'ksize does not match'), (dict(kind=4), 'unknown source kind'), (dict(ws_bytes=16), 'workspace too small')):
        assert call(**kw) != 0, kw
        assert name in lib.sdmi_last_error().decode(), (kw, lib.sdmi_last_error().decode())
    assert lib.sdmi_fe_workspace_bytes(1, 40, 56, 28, 32) == -1 and 'crop_size > size' in lib.sdmi_last_error().decode()
    torch.cuda.synchronize()
    P.check('refusals')
    assert (pv.view(torch.int32) == -1).all() and (u8 == 0xFF).all() and (ws == 0xFF).all()        # nothing was launched
    assert call() == 0                                                                            # ... and the same buffers do run
    torch.cuda.synchronize()
    P.check('after the refusals')
    assert torch.isfinite(pv.reshape(-1)[:3 * 28 * 28]).all()                                     # ([1, 3, 28, 28] at the head of the buffer)
