"""Host post-processing of the reference scripts (scripts/txt2img.py:313-327, scripts/img2img.py:264-280), SURVEY.md 8 f-4:

    x = model.decode_first_stage(samples)               -> AutoencoderKLHIP.decode_first_stage
    x = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)  \\
    x = 255. * x.permute(0, 2, 3, 1)  ... astype(uint8)  } `to_uint8_images`: one device pass, same bytes
    Image.fromarray(x).save(path)                       -> `save_png`
    put_watermark(img, wm_encoder)                      -> `put_watermark` (needs the optional `imwatermark` package)

The safety checker is built as well: `stable_diffusion_amd.vision.StableDiffusionSafetyCheckerHIP` (its CLIP ViT-L/14 vision tower and the
concept head in libsdmi), and so is its feature extractor (`vision.CLIPFeatureExtractorHIP`: numpy_to_pil's uint8 conversion and PIL's
bicubic resize and crop, bit for bit, on the device).  `check_safety` below is txt2img.py:314-317 from the raw decode output to the checked images
and the flags, without the image leaving the GPU:

    x = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)  \\
    x = x.cpu().permute(0, 2, 3, 1).numpy()              } `check_safety`: the same clamp, then extractor -> tower -> head on the device;
    x_checked, has_nsfw = check_safety(x)               /  one small device-to-host copy (the flags)
"""
import numpy as np
import torch

from . import _lib


@torch.no_grad()
def to_uint8_images(x_samples):
    """decode_first_stage output [B, C, H, W] (cuda, any float dtype) -> uint8 [B, H, W, C] (cuda), bit-identical to
    `(255. * clamp((x + 1) / 2, 0, 1).permute(0, 2, 3, 1).numpy()).astype(np.uint8)` of scripts/txt2img.py:314-324."""
    if not x_samples.is_cuda:
        raise RuntimeError('to_uint8_images runs on MI355X device tensors only (no CPU fallback)')
    x = x_samples.detach().float().contiguous()
    B, C, H, W = x.shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().sdmi_image_to_uint8(x.data_ptr(), out.data_ptr(), B, C, H, W, _lib.stream_ptr()))
    return out


@torch.no_grad()
def check_safety(x_samples, checker, extractor=None):
    """scripts/txt2img.py:314-317 on the device.  `x_samples`: the raw decode_first_stage output [B, 3, H, W] (cuda); `checker`: a
    StableDiffusionSafetyCheckerHIP; `extractor`: a CLIPFeatureExtractorHIP (default: the checker's own, at the tower's image size).
    -> (images fp32 [B, 3, H, W] in [0, 1] with the flagged ones zeroed, has_nsfw_concepts): `images.permute(0, 2, 3, 1)` is the script's
    x_checked_image, still on the device (`to_uint8_images` itself takes the raw decode output: for the unflagged images its bytes are
    those of `(255. * images)` truncated, txt2img.py:323)."""
    if not x_samples.is_cuda:
        raise RuntimeError('check_safety runs on MI355X device tensors only (no CPU fallback)')
    x = torch.clamp((x_samples.detach().float() + 1.0) / 2.0, min=0.0, max=1.0)
    return checker.check_images(x, extractor=extractor, layout='NCHW', value_range=(0, 1))


def put_watermark(img, wm_encoder=None):
    """scripts/txt2img.py:41-46: dwtDct invisible watermark through `imwatermark`, when an encoder is given."""
    if wm_encoder is None:
        return img
    import cv2
    from PIL import Image
    arr = cv2.cvtColor(np.array(img), cv2.COLOR_RGB2BGR)
    arr = wm_encoder.encode(arr, 'dwtDct')
    return Image.fromarray(arr[:, :, ::-1])


def make_watermark_encoder(text='StableDiffusionV1'):
    """scripts/txt2img.py:261-264; returns None (no watermark) when `imwatermark` is not installed."""
    try:
        from imwatermark import WatermarkEncoder
    except ImportError:
        return None
    enc = WatermarkEncoder()
    enc.set_watermark('bytes', text.encode('utf-8'))
    return enc


def save_png(u8_hwc, path, wm_encoder=None):
    """One image (uint8 [H, W, C], any device) -> PNG file, as scripts/txt2img.py:324-326."""
    from PIL import Image
    arr = u8_hwc.cpu().numpy() if isinstance(u8_hwc, torch.Tensor) else np.asarray(u8_hwc)
    img = put_watermark(Image.fromarray(arr), wm_encoder)
    img.save(path)
    return path
