"""The CLIP image encoder on the MI355X: vision tower, safety checker, image embedder.

Kernels in guarded buffers (tests/guard.py; guard words checked after every launch): sdmi_k_vit_patchify bit-equal to a numpy unfold rounded to
fp16 with exactly-zero pad columns; sdmi_k_vit_embed bit-equal to the fp32 adds; sdmi_k_vit_preprocess against an fp64 restatement
(tests/vit_ref.py) at 4 x the error of torch's own fp32 bicubic at the same inputs (floor 1e-6: a different, equally valid fp32 order of the
16-tap sum); sdmi_k_safety_head's flags and rounded scores exactly equal to the fp64 statement on constructed scores that the test first shows
to lie >= 1e-4 from every rounding boundary.  Then CLIPVisionHIP against transformers' fp32 goldens (tools/make_golden_vit.py) at 2 x the
golden's own fp16-operand floor (the factor covers fp16 attention probabilities and accumulation order, which the floor does not model), the
safety checker end to end, and the image embedder.

Shapes: VIT_TINY (5 tokens padded to 8, d = 32, GEMM rows 15) and VIT_L14_THIN (257 tokens = eight 32-query slices plus one row, nkv_pad 264,
d = 64, GEMM rows 514); K = 588 zero-padded to 640 in both.

Measured on an MI355X (max-abs error | bar):
  vit_tiny_b3      image_embeds 2.78e-3, pooled_output 1.90e-3, hidden rows 3.45e-3 | 5.95e-3 (2 x floor 2.97e-3)
  vit_l14thin_b2   image_embeds 1.46e-3, pooled_output 1.50e-3, hidden rows 2.14e-3 | 4.26e-3 (2 x floor 2.13e-3)
  preprocess       16x24->28: 6.71e-6 (torch 6.71e-6), 40x56->28: 1.59e-5 (torch 1.63e-5), 64x48->224: 1.87e-5 (torch 1.87e-5) | 4 x torch
  safety checker   cosine error 2.9e-5 against scores 0.02 from zero; image embedder against the tower 1.1e-3 | 5.95e-3
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import vit_ref  # noqa: E402
from stable_diffusion_amd import _lib, synthetic, vision  # noqa: E402

DEV = 'cuda'
GOLDENS = {'vit_tiny_b3': synthetic.VIT_TINY, 'vit_l14thin_b2': synthetic.VIT_L14_THIN}
_cache = {}


def seeded(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _sync_check(pool, case):
    torch.cuda.synchronize()
    pool.check(case)


# ---- kernels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,B', [(28, 3), (224, 2)])
def test_patchify_is_bit_equal_to_unfold_and_pads_with_zeros(S, B):
    p, K, Kp = 14, 588, 640
    assert _lib.load().sdmi_k_vit_kpad(p) == Kp
    px = seeded((B, 3, S, S), 21 + S)
    P = guard.Pool(DEV)
    gpx = P.put('pixel_values', px)
    out = P.new('cols', (B * (S // p) ** 2, Kp), torch.float16)
    _lib.check(_lib.load().sdmi_k_vit_patchify(gpx.data_ptr(), out.data_ptr(), B, S, p, _lib.stream_ptr()))
    _sync_check(P, f'patchify S={S}')
    got = out.cpu().numpy()
    ref = vit_ref.patchify(px.numpy(), p, Kp)
    assert np.array_equal(got.view(np.uint16), ref.view(np.uint16))
    assert not got[:, K:].view(np.uint16).any() and got[:, :K].any()
    assert torch.equal(gpx.cpu(), px)


@pytest.mark.parametrize('B,T,C', [(3, 5, 64), (2, 257, 1024)])
def test_embed_is_bit_equal_to_the_fp32_adds(B, T, C):
    patch, cls, pos = seeded((B * (T - 1), C), 31), seeded((C,), 32, 0.5), seeded((T, C), 33, 0.5)
    P = guard.Pool(DEV)
    gp, gc, gq = P.put('patch', patch), P.put('class_embedding', cls), P.put('position_embedding', pos)
    out = P.new('tokens', (B, T, C), torch.float32)
    _lib.check(_lib.load().sdmi_k_vit_embed(gp.data_ptr(), gc.data_ptr(), gq.data_ptr(), out.data_ptr(), B, T, C, _lib.stream_ptr()))
    _sync_check(P, f'embed T={T}')
    ref = np.empty((B, T, C), dtype=np.float32)
    ref[:, 0] = cls.numpy() + pos.numpy()[0]
    ref[:, 1:] = patch.numpy().reshape(B, T - 1, C) + pos.numpy()[None, 1:]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def _torch_preprocess(x, S):
    y = torch.nn.functional.interpolate(x, size=(S, S), mode='bicubic', align_corners=True)
    mean, std = torch.tensor(vit_ref.CLIP_MEAN)[None, :, None, None], torch.tensor(vit_ref.CLIP_STD)[None, :, None, None]
    return ((y + 1.0) / 2.0 - mean) / std


@pytest.mark.parametrize('H,W,S', [(16, 24, 28), (40, 56, 28), (64, 48, 224)])
def test_preprocess_vs_fp64_at_the_error_of_torchs_own_fp32_bicubic(H, W, S):
    B = 2
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(H * W)) * 2.0 - 1.0
    x[:, :, 0, 0], x[:, :, -1, -1], x[0, 1, H // 2, W // 2], x[1, 2, 1, W - 2] = 1.0, -1.0, 1.0, -1.0       # values reaching +-1, corners included
    ref64 = vit_ref.preprocess(x.numpy(), S)
    err_torch = float(np.abs(_torch_preprocess(x, S).numpy().astype(np.float64) - ref64).max())
    P = guard.Pool(DEV)
    gx = P.put('x', x)
    out = P.new('out', (B, 3, S, S), torch.float32)
    _lib.check(_lib.load().sdmi_k_vit_preprocess(gx.data_ptr(), out.data_ptr(), B, H, W, S, _lib.stream_ptr()))
    _sync_check(P, f'preprocess {H}x{W}->{S}')
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref64).max())
    bound = max(4.0 * err_torch, 1e-6)
    print(f'[vit_preprocess] {H}x{W}->{S}: kernel {err:.3e}, torch fp32 {err_torch:.3e}, bound {bound:.3e}', flush=True)
    assert err <= bound
    if S == synthetic.VIT_TINY['image_size']:                                          # the module's preprocess is this launch
        assert torch.equal(vision.FrozenClipImageEmbedderHIP(synthetic.VIT_TINY).preprocess(x.to(DEV)).cpu(), out.cpu())


def _construct(images, offsets, thr, rng):
    """vectors whose cosine with image b is thr[j] + offsets[b][j]: a combination of the (orthonormalised) image directions and a unit vector
    orthogonal to all of them, at a random length"""
    B, E = images.shape
    q, _ = np.linalg.qr(np.concatenate([images.T, rng.standard_normal((E, len(thr)))], 1))        # columns: images' span first
    # images must already be orthogonal for cos(image_b, q_b) = 1: the caller builds them from q
    out = np.zeros((len(thr), E))
    for j in range(len(thr)):
        cos = np.array([thr[j] + offsets[b][j] for b in range(B)])
        assert (cos ** 2).sum() < 1.0
        sign = np.sign(images @ q[:, :B]).diagonal()
        out[j] = (q[:, :B] * sign * cos).sum(1) + np.sqrt(1.0 - (cos ** 2).sum()) * q[:, B + j]
        out[j] *= rng.uniform(0.5, 20.0)
    return out


def _run_safety_head(img, concepts, special, thr_c, thr_s, case):
    B, Nc, Ns = len(img), len(concepts), len(special)
    P = guard.Pool(DEV)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))     # noqa: E731
    gi, gc, gtc = P.put('image_embeds', t32(img)), P.put('concept_embeds', t32(concepts)), P.put('concept_thresholds', t32(thr_c))
    gs = P.put('special_care_embeds', t32(special)) if Ns else torch.empty((0, img.shape[1]), device=DEV)
    gts = P.put('special_care_thresholds', t32(thr_s)) if Ns else torch.empty((0,), device=DEV)
    has = P.new('has_nsfw', (B,), torch.int32)
    cs = P.new('concept_scores', (B, Nc), torch.float32)
    ss = P.new('special_scores', (B, Ns), torch.float32) if Ns else torch.empty((B, 0), device=DEV)
    vision.safety_head(gi, gc, gs, gtc, gts, out=(has, cs, ss))
    _sync_check(P, case)
    return has.cpu().numpy(), cs.cpu().numpy(), ss.cpu().numpy(), (gi, gc, gs, gtc, gts)


def test_safety_head_flags_and_rounded_scores_equal_fp64_exactly():
    B, Nc, Ns, E = 3, 17, 3, 768
    rng = np.random.default_rng(7)
    q, _ = np.linalg.qr(rng.standard_normal((E, B)))
    images = (q * rng.uniform(0.5, 30.0, B)).T                                       # orthogonal image vectors of different lengths
    thr_c, thr_s = rng.uniform(0.05, 0.25, Nc), rng.uniform(0.05, 0.25, Ns)
    # offsets above the threshold BEFORE the adjustment.  image 0: special-care concept 1 at +0.02 raises the adjustment, so concept 0 at -0.005
    # becomes +0.005 (flagged) and everything else moves from -0.03 to -0.02; image 1: no special-care concept fires, concept 0 at -0.005 stays
    # unflagged, concept 5 at +0.0003 rounds to 0 (not flagged); image 2: -0.02, +0.02, +0.0003, +0.0007 (rounds to 0.001: flagged) side by side
    off_s = [[-0.02, 0.02, -0.02], [-0.02, -0.02, -0.02], [-0.02, -0.02, -0.02]]
    off_c = [[-0.005] + [-0.03] * 16, [-0.005] + [-0.02] * 4 + [0.0003] + [-0.02] * 11, [-0.02, 0.02, 0.0003, 0.0007] + [-0.02] * 13]
    concepts, special = _construct(images, off_c, thr_c, rng), _construct(images, off_s, thr_s, rng)
    # the fp64 reference on the fp32 values the kernel reads
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                  # noqa: E731
    has_ref, cs_ref, ss_ref, raw_c, raw_s = vit_ref.safety_head(f32(images), f32(concepts), f32(special), f32(thr_c), f32(thr_s))
    assert np.allclose(raw_s, np.array(off_s) + np.array([[0, 0, 0.01], [0, 0, 0], [0, 0, 0]]), atol=2e-6)
    assert np.allclose(raw_c, np.array(off_c) + np.array([[0.01], [0.0], [0.0]]), atol=2e-6)
    assert min(vit_ref.boundary_distance(raw_c).min(), vit_ref.boundary_distance(raw_s).min()) >= 1e-4
    assert has_ref.tolist() == [True, False, True] and cs_ref[0, 0] == 0.005 and cs_ref[1, 0] == -0.005
    assert cs_ref[2, :4].tolist() == [-0.02, 0.02, 0.0, 0.001] and cs_ref[1, 5] == 0.0
    has, cs, ss, ops = _run_safety_head(images, concepts, special, thr_c, thr_s, 'safety_head 17/3/768')
    assert has.tolist() == [1, 0, 1]
    assert np.array_equal(cs, cs_ref.astype(np.float32)) and np.array_equal(ss, ss_ref.astype(np.float32))
    # without the special-care concepts nothing lifts image 0's concept 0
    has0, cs0, _, _ = _run_safety_head(images, concepts, np.zeros((0, E)), thr_c, np.zeros(0), 'safety_head 17/0/768')
    ref0 = vit_ref.safety_head(f32(images), f32(concepts), np.zeros((0, E)), f32(thr_c), [])
    assert has0.tolist() == [0, 0, 1] and np.array_equal(cs0, ref0[1].astype(np.float32)) and cs0[0, 0] == np.float32(-0.005)


def test_safety_head_smallest_shape():
    B, E = 2, 32
    rng = np.random.default_rng(9)
    q, _ = np.linalg.qr(rng.standard_normal((E, B)))
    images = (q * rng.uniform(0.5, 5.0, B)).T
    concepts = _construct(images, [[0.0007], [0.0003]], [0.3], rng)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                  # noqa: E731
    has_ref, cs_ref, _, raw_c, _ = vit_ref.safety_head(f32(images), f32(concepts), np.zeros((0, E)), f32([0.3]), [])
    assert vit_ref.boundary_distance(raw_c).min() >= 1e-4 and has_ref.tolist() == [True, False]
    has, cs, _, _ = _run_safety_head(images, concepts, np.zeros((0, E)), [0.3], np.zeros(0), 'safety_head 1/0/32')
    assert has.tolist() == [1, 0] and np.array_equal(cs, cs_ref.astype(np.float32)) and cs.tolist() == [[np.float32(0.001)], [0.0]]


def test_kernel_launchers_refuse_what_they_cannot_run():
    lib = _lib.load()
    z = torch.zeros(4096, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    s = _lib.stream_ptr()
    p = z.data_ptr()
    for call, name in ((lambda: lib.sdmi_k_safety_head(p, p, p, p, p, i.data_ptr(), p, p, 1, 65, 3, 32, s), 'Nc <= 64'),
                       (lambda: lib.sdmi_k_safety_head(p, p, p, p, p, i.data_ptr(), p, p, 1, 17, 3, 30, s), 'multiple of 4'),
                       (lambda: lib.sdmi_k_vit_patchify(p, p, 1, 30, 14, s), 'image_size % patch_size'),
                       (lambda: lib.sdmi_k_vit_embed(p, p, p, p, 1, 5, 6, s), 'C % 4')):
        assert call() != 0 and name in lib.sdmi_last_error().decode(), lib.sdmi_last_error().decode()


# ---- the tower ---------------------------------------------------------------------------------------------------------------------------
def _golden(golden_dir, name):
    if ('golden', name) not in _cache:
        _cache[('golden', name)] = dict(np.load(os.path.join(golden_dir, name + '.npz')))
    return _cache[('golden', name)]


def _pixels(z, cfg):
    return seeded((int(z['batch']), 3, cfg['image_size'], cfg['image_size']), int(z['pixel_seed']))


def _tower(golden_dir, name):
    """the tower with the golden's weights and its outputs on the golden's pixel values, computed once"""
    if ('tower', name) not in _cache:
        cfg, z = GOLDENS[name], _golden(golden_dir, name)
        sd = synthetic.synthetic_vision_state_dict(cfg, int(z['weight_seed']))
        m = vision.CLIPVisionHIP(cfg)
        m.load_state_dict(sd, strict=True)
        m.to(DEV)
        out = [t.clone() for t in m(_pixels(z, cfg).to(DEV))]
        again = m(_pixels(z, cfg).to(DEV))
        assert all(torch.equal(a, b) for a, b in zip(out, again))               # fixed summation order: the same bits
        _cache[('tower', name)] = (m, sd, [t.cpu().numpy() for t in out])
    return _cache[('tower', name)]


@pytest.mark.parametrize('name', list(GOLDENS))
def test_tower_vs_transformers_fp32_at_twice_the_fp16_operand_floor(name, golden_dir):
    z = _golden(golden_dir, name)
    _, _, (embeds, pooled, hidden) = _tower(golden_dir, name)
    floor = float(z['fp16_floor'])
    errs = dict(image_embeds=np.abs(embeds - z['image_embeds']).max(), pooled_output=np.abs(pooled - z['pooled_output']).max(),
                hidden_rows=np.abs(hidden[:, z['hidden_rows']] - z['last_hidden_state']).max())
    print(f'[vit parity] {name}: ' + ', '.join(f'{k} {v:.3e}' for k, v in errs.items()) + f' | floor {floor:.3e}, bound {2 * floor:.3e}', flush=True)
    assert np.isfinite(embeds).all() and np.isfinite(hidden).all()
    assert 1e-4 < floor < 1e-2                                                        # the golden's own floor is what the design predicts
    for k, v in errs.items():
        assert v <= 2.0 * floor, (k, v, floor)


def test_safety_checker_end_to_end(golden_dir):
    name = 'vit_l14thin_b2'
    cfg, z = GOLDENS[name], _golden(golden_dir, name)
    tower, sd, (embeds, _, _) = _tower(golden_dir, name)
    g = z['image_embeds'].astype(np.float64)
    rng = np.random.default_rng(11)
    Nc, Ns, E = 17, 3, g.shape[1]
    concepts, special = rng.standard_normal((Nc, E)), rng.standard_normal((Ns, E))
    # concept 5 at cosine 0.5 to image 0 and 0.4 to image 1 (the two embeddings of one random tower are nearly parallel, cosine 0.98: the
    # concept leans on the part of image 1 that image 0 does not have)
    u0, u1 = g[0] / np.linalg.norm(g[0]), g[1] / np.linalg.norm(g[1])
    c01 = float(u0 @ u1)
    e1 = (u1 - c01 * u0) / np.sqrt(1.0 - c01 * c01)
    w = concepts[5] - (concepts[5] @ u0) * u0
    w = w - (w @ e1) * e1
    beta = (0.4 - 0.5 * c01) / np.sqrt(1.0 - c01 * c01)
    concepts[5] = 3.0 * (0.5 * u0 + beta * e1 + np.sqrt(0.75 - beta * beta) * w / np.linalg.norm(w))
    assert np.allclose(vit_ref.cosines(g, concepts[5:6])[:, 0], [0.5, 0.4], atol=1e-12)
    # every threshold 0.02 above the larger of the two images' cosines, except concept 5's: image 0 sits 0.02 over it
    thr_c, thr_s = vit_ref.cosines(g, concepts).max(0) + 0.02, vit_ref.cosines(g, special).max(0) + 0.02
    thr_c[5] = 0.48
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                  # noqa: E731
    has_ref, cs_ref, ss_ref, raw_c, raw_s = vit_ref.safety_head(g, f32(concepts), f32(special), f32(thr_c), f32(thr_s))
    assert has_ref.tolist() == [True, False] and abs(raw_c[0, 5] - 0.02) < 1e-6 and raw_c[1].max() <= -0.02 + 1e-6 and raw_s.max() <= -0.02 + 1e-6
    cos_err = max(np.abs(vit_ref.cosines(embeds, m) - vit_ref.cosines(g, m)).max() for m in (concepts, special))
    print(f'[safety checker] measured cosine error {cos_err:.3e}; smallest |rounded score| {min(np.abs(cs_ref).min(), np.abs(ss_ref).min()):.3e}', flush=True)
    assert min(np.abs(cs_ref).min(), np.abs(ss_ref).min()) >= 4.0 * cos_err
    checker = vision.StableDiffusionSafetyCheckerHIP(cfg)
    csd = {('vision_model.' + k if k.startswith('vision_model.') else k): v for k, v in sd.items()}
    csd.update(concept_embeds=torch.from_numpy(f32(concepts)), special_care_embeds=torch.from_numpy(f32(special)),
               concept_embeds_weights=torch.from_numpy(f32(thr_c)), special_care_embeds_weights=torch.from_numpy(f32(thr_s)))
    checker.load_state_dict(csd, strict=True)
    checker.to(DEV)
    images = np.random.default_rng(12).random((2, 8, 8, 3)).astype(np.float32)
    keep = images.copy()
    out, has = checker(clip_input=_pixels(z, cfg), images=images)                     # (the feature extractor hands over a CPU tensor)
    assert has == [True, False] and all(type(v) is bool for v in has)
    assert out.shape == keep.shape and not out[0].any() and np.array_equal(out[1].view(np.uint32), keep[1].view(np.uint32))
    # (scores of the image that is further under a threshold may sit next to a rounding boundary: one rounding step, not equality)
    assert np.abs(checker.last_scores['concept_scores'].cpu().numpy() - cs_ref).max() <= 1e-3 + cos_err + 1e-6


def test_image_embedder_is_preprocess_then_the_tower(golden_dir):
    name = 'vit_tiny_b3'
    cfg, z = GOLDENS[name], _golden(golden_dir, name)
    tower, sd, _ = _tower(golden_dir, name)
    emb = vision.FrozenClipImageEmbedderHIP(cfg)
    emb.load_state_dict({'model.' + k: v for k, v in vision.transformers_to_openai_clip(sd).items()}, strict=True)     # (OpenAI naming in)
    emb.to(DEV)
    x = torch.rand((2, 3, 40, 56), generator=torch.Generator().manual_seed(5)) * 2.0 - 1.0
    got = emb(x.to(DEV))
    ref = tower(_torch_preprocess(x, cfg['image_size']).to(DEV))[0]
    err = float((got - ref).abs().max())
    print(f'[image embedder] vs the tower on the CPU-preprocessed input: {err:.3e} | bound {2 * float(z["fp16_floor"]):.3e}', flush=True)
    assert got.shape == (2, cfg['projection_dim']) and err <= 2.0 * float(z['fp16_floor'])
