"""Fixtures of the feature-extractor tests: PIL's and transformers' own results on small seeded images, so the GPU tests need neither.

    python tools/make_golden_feature_extractor.py        # needs Pillow and transformers; writes tests/golden/clip_fe_*.npz

Each file holds `input` (uint8 [H, W, 3]), `resized` (PIL's Image.resize(..., BICUBIC) of it, shortest side 28), `cropped` (its centre 28 x 28)
and `pixel_values` (CLIPImageProcessor(size=28, crop_size=28) on the PIL image, fp32 [3, 28, 28])."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = CROP = 28


def inputs():
    """name -> uint8 [H, W, 3]"""
    rng = np.random.default_rng(20240607)
    out = {f'{h}x{w}': rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
           for h, w in ((40, 56), (64, 48), (17, 31),       # down, down (portrait), an upscale whose windows are clipped at both borders
                        (28, 28), (28, 40))}                # nothing resized; crop only, odd remainder 12 -> left = 6
    yy, xx = np.mgrid[0:64, 0:48]
    blocks = (((yy // 8) + (xx // 8)) % 2 * 255).astype(np.uint8)           # 8 x 8 blocks of 0 and 255: the ringing clips at both ends
    out['blocks_64x48'] = np.ascontiguousarray(np.repeat(blocks[:, :, None], 3, axis=2))
    return out


def main():
    from PIL import Image
    # (by path: tests/ on sys.path would shadow packages transformers probes for, `kernels` among them)
    spec = importlib.util.spec_from_file_location('pil_ref', os.path.join(ROOT, 'tests', 'pil_ref.py'))
    pil_ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pil_ref)
    try:                                 # the PIL backend, which is what the reference-era CLIPFeatureExtractor is
        from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil as CLIPImageProcessor
    except ImportError:                  # older transformers: the one class resizes through PIL
        from transformers import CLIPImageProcessor
    proc = CLIPImageProcessor(size={'shortest_edge': SIZE}, crop_size={'height': CROP, 'width': CROP}, resample=Image.BICUBIC,
                              image_mean=list(pil_ref.CLIP_MEAN), image_std=list(pil_ref.CLIP_STD))
    gold = os.path.join(ROOT, 'tests', 'golden')
    for name, img in inputs().items():
        H, W = img.shape[:2]
        rh, rw = pil_ref.output_size(H, W, SIZE)
        pil = Image.fromarray(img)
        resized = np.asarray(pil.resize((rw, rh), Image.BICUBIC))
        top, left = (rh - CROP) // 2, (rw - CROP) // 2
        cropped = np.ascontiguousarray(resized[top:top + CROP, left:left + CROP])
        pv = proc(pil, return_tensors='np')['pixel_values'][0].astype(np.float32)
        assert pv.shape == (3, CROP, CROP)
        # transformers resizes through PIL as well: its values must be those of PIL's own cropped image
        assert np.abs(pv - pil_ref.pixel_values(cropped)).max() < 1e-6, name
        path = os.path.join(gold, f'clip_fe_{name}.npz')
        np.savez_compressed(path, input=img, resized=resized, cropped=cropped, pixel_values=pv)
        print(f'{path}: {H}x{W} -> {rh}x{rw} -> {CROP}x{CROP}, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
