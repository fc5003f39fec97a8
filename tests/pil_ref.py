"""PIL's 8-bit bicubic `Image.resize`, the centre crop and CLIP's normalisation, restated in numpy (no PIL import): the reference the HIP
feature extractor is tested against where PIL is not installed.  tests/test_feature_extractor_host.py holds it to PIL itself, bit for bit.

Pillow's Resample.c: precompute_coeffs + bicubic_filter in double, normalize_coeffs_8bpc to 22 fraction bits, then a horizontal pass that
stores uint8 and a vertical pass that reads it; an axis whose size does not change has no pass."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize(n_in, n_out):
    filterscale = max(n_in / n_out, 1.0)
    return int(math.ceil(2.0 * filterscale)) * 2 + 1


def coeffs(n_in, n_out):
    """-> (ksize, bounds int32 [n_out, 2] = (xmin, xmax), kk int32 [n_out, ksize])"""
    scale = filterscale = n_in / n_out
    filterscale = max(filterscale, 1.0)
    support = 2.0 * filterscale
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ks), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ks, bounds, kk


def _pass(img, n_out, axis):
    """one 8-bit pass along `axis` (0 rows, 1 columns) of img uint8 [H, W, C]"""
    _, bounds, kk = coeffs(img.shape[axis], n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx in range(n_out):
        xmin, xmax = (int(v) for v in bounds[xx])
        k = kk[xx, :xmax].astype(np.int64).reshape((xmax,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + xmax] * k).sum(0)
        assert np.abs(acc).max() < 2 ** 31
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_u8(img, rh, rw):
    """Image.fromarray(img).resize((rw, rh), BICUBIC) for img uint8 [H, W, C]"""
    if rw != img.shape[1]:
        img = _pass(img, rw, 1)
    if rh != img.shape[0]:
        img = _pass(img, rh, 0)
    return img


def output_size(H, W, size):
    """transformers' get_resize_output_image_size(..., default_to_square=False): (rh, rw)"""
    short, long = (H, W) if H <= W else (W, H)
    other = int(size * long / short)
    return (size, other) if H <= W else (other, size)


def center_crop(img, crop):
    top, left = (img.shape[0] - crop) // 2, (img.shape[1] - crop) // 2
    return img[top:top + crop, left:left + crop]


def to_u8(x):
    """numpy_to_pil's conversion of a float image in [0, 1]"""
    return (np.asarray(x, np.float32) * 255).round().astype(np.uint8)


def pixel_values(u8, mean=CLIP_MEAN, std=CLIP_STD):
    """cropped uint8 [crop, crop, 3] -> fp64 [3, crop, crop]"""
    x = u8.astype(np.float64) / 255.0
    x = (x - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def extract(img, size=224, crop=224, mean=CLIP_MEAN, std=CLIP_STD):
    """uint8 [H, W, 3] -> (resized uint8, cropped uint8, pixel_values fp64 [3, crop, crop])"""
    rh, rw = output_size(img.shape[0], img.shape[1], size)
    r = resize_u8(img, rh, rw)
    c = np.ascontiguousarray(center_crop(r, crop))
    return r, c, pixel_values(c, mean, std)
