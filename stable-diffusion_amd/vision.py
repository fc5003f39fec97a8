"""The CLIP image encoder on MI355X: the vision tower, the NSFW safety checker and the image embedder.

    CLIPVisionHIP                   <- transformers.CLIPVisionModelWithProjection
    StableDiffusionSafetyCheckerHIP <- diffusers.pipelines.stable_diffusion.safety_checker.StableDiffusionSafetyChecker
                                       (scripts/txt2img.py:26-29, 88-95; scripts/img2img.py)
    FrozenClipImageEmbedderHIP      <- ldm.modules.encoders.modules.FrozenClipImageEmbedder (modules.py:197-228)

The tower (patch embedding, 24 pre-norm encoder layers, post-LayerNorm, projection) runs in libsdmi.so behind the `sdmi_vit_*` handle, the concept
head in `sdmi_k_safety_head`, the embedder's bicubic preprocess in `sdmi_k_vit_preprocess`.  Mixed precision only: fp16 MFMA operands, fp32
accumulation and residual stream.  No CPU / PyTorch fallback.

    CLIPFeatureExtractorHIP         <- transformers.CLIPFeatureExtractor as AutoFeatureExtractor builds it for the checker (scripts/txt2img.py:28)

The checker's feature extractor (numpy_to_pil's uint8 conversion, PIL's 8-bit bicubic resize, centre crop, / 255, mean / std) runs in
`sdmi_k_clip_feature_extract`, its uint8 stage bit-equal to PIL's; `StableDiffusionSafetyCheckerHIP.check_images` chains it with the tower and the
head on device images.
"""
import ctypes as C
import json
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .unet import _Node

CLIP_VIT_L14_VISION = dict(image_size=224, patch_size=14, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24,
                           num_attention_heads=16, projection_dim=768)
SAFETY_CONCEPTS, SAFETY_SPECIAL_CARE = 17, 3          # rows of concept_embeds / special_care_embeds in the shipped checker


def make_vit_cfg(vc):
    if vc.get('hidden_act', 'quick_gelu') != 'quick_gelu':
        raise NotImplementedError('CLIPVisionHIP implements the quick_gelu CLIP vision tower only')
    cfg = _lib.VitCfg()
    cfg.image_size, cfg.patch_size = int(vc['image_size']), int(vc['patch_size'])
    cfg.hidden_size, cfg.intermediate_size = int(vc['hidden_size']), int(vc['intermediate_size'])
    cfg.num_layers, cfg.num_heads, cfg.projection_dim = int(vc['num_hidden_layers']), int(vc['num_attention_heads']), int(vc['projection_dim'])
    return cfg


def _without_position_ids(sd):
    """older transformers keep `embeddings.position_ids` (arange) as a persistent buffer: present in the shipped checkpoints, never a weight"""
    return {k: v for k, v in sd.items() if not k.endswith('embeddings.position_ids')}


def _check_precision(hip_precision):
    if hip_precision != 'mixed':
        raise NotImplementedError(f"hip_precision={hip_precision!r}: the CLIP vision tower runs hip_precision='mixed' only "
                                  "(hip_precision='full' is not built for it)")


class _VitHandle:
    """Owns one sdmi_vit*."""

    def __init__(self, cfg):
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.sdmi_vit_create(C.byref(cfg), C.byref(h)))
        self.h = h

    def weight_specs(self):
        n = self.lib.sdmi_vit_num_weights(self.h)
        out = []
        buf = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(n):
            _lib.check(self.lib.sdmi_vit_weight_info(self.h, i, buf, 256, shape, C.byref(nd)))
            out.append((buf.value.decode(), tuple(shape[j] for j in range(nd.value))))
        return out

    def __del__(self):
        try:
            if self.h:
                self.lib.sdmi_vit_destroy(self.h)
                self.h = None
        except Exception:
            pass


class CLIPVisionHIP(nn.Module):
    """`forward(pixel_values)` -> (image_embeds [B, projection_dim], pooled_output [B, hidden], last_hidden_state [B, T, hidden]).
    Parameter names are CLIPVisionModelWithProjection's (`vision_model.*`, `visual_projection.weight`)."""
    MAX_BATCH = 64

    def __init__(self, vision_config=None, hip_precision='mixed'):
        super().__init__()
        _check_precision(hip_precision)
        self.hip_precision = hip_precision
        self.vision_config = dict(CLIP_VIT_L14_VISION if vision_config is None else vision_config)
        self._cfg = make_vit_cfg(self.vision_config)
        self._handle = _VitHandle(self._cfg)
        self._specs = self._handle.weight_specs()
        for key, shape in self._specs:
            *path, leaf = key.split('.')
            node = self
            for name in path:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            node.register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._packed_sig = None
        self._sentinels = None
        self._ws = None
        self.eval()

    @property
    def num_tokens(self):
        return 1 + (self._cfg.image_size // self._cfg.patch_size) ** 2

    # ---- weights -> library (same dirty tracking as FrozenCLIPEmbedderHIP) ----------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._packed_sig = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, *a, **k):
        self._packed_sig = None
        return super().load_state_dict(_without_position_ids(state_dict), *a, **k)

    def mark_dirty(self):
        self._packed_sig = None

    def _signature(self):
        if getattr(self, '_sentinels', None) is None:
            ps = dict(self.named_parameters())
            keys = [self._specs[0][0], self._specs[len(self._specs) // 2][0], self._specs[-1][0]]
            self._sentinels = [ps[k] for k in keys]
        return tuple((p.data_ptr(), p._version) for p in self._sentinels)

    def pack(self):
        lib = self._handle.lib
        stream = _lib.stream_ptr()
        ps = dict(self.named_parameters())
        for key, shape in self._specs:
            p = ps[key].detach()
            if not p.is_cuda:
                raise RuntimeError('CLIPVisionHIP parameters must live on the GPU (call model.cuda() first); there is no CPU implementation of this path')
            p = p.float().contiguous()
            shp = (C.c_int64 * len(shape))(*shape)
            _lib.check(lib.sdmi_vit_set_weight(self._handle.h, key.encode(), p.data_ptr(), shp, len(shape), stream))
        torch.cuda.current_stream().synchronize()
        _lib.check(lib.sdmi_vit_finalize(self._handle.h))
        self._sentinels = None
        self._packed_sig = self._signature()

    @torch.no_grad()
    def forward(self, pixel_values):
        S = self._cfg.image_size
        if not pixel_values.is_cuda:
            raise RuntimeError('CLIPVisionHIP runs on an MI355X device tensor only (no CPU fallback)')
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            raise ValueError(f'pixel_values must be [B, 3, {S}, {S}], got {tuple(pixel_values.shape)}')
        if self._packed_sig is None or self._packed_sig != self._signature():
            self.pack()
        px = pixel_values.detach().float().contiguous()
        B, T, Ch, Pd = px.shape[0], self.num_tokens, self._cfg.hidden_size, self._cfg.projection_dim
        embeds = torch.empty((B, Pd), dtype=torch.float32, device=px.device)
        pooled = torch.empty((B, Ch), dtype=torch.float32, device=px.device)
        hidden = torch.empty((B, T, Ch), dtype=torch.float32, device=px.device)
        lib = self._handle.lib
        for b0 in range(0, B, self.MAX_BATCH):
            nb = min(self.MAX_BATCH, B - b0)
            key = (nb, str(px.device))
            if self._ws is None or self._ws[0] != key:
                need = lib.sdmi_vit_workspace_bytes(self._handle.h, nb)
                if need <= 0:
                    _lib.check(-1)
                self._ws = (key, torch.empty(int(need), dtype=torch.uint8, device=px.device))
            ws = self._ws[1]
            _lib.check(lib.sdmi_vit_forward(self._handle.h, px[b0:b0 + nb].data_ptr(), hidden[b0:b0 + nb].data_ptr(), pooled[b0:b0 + nb].data_ptr(),
                                            embeds[b0:b0 + nb].data_ptr(), nb, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return embeds, pooled, hidden


@torch.no_grad()
def safety_head(image_embeds, concept_embeds, special_care_embeds, concept_thresholds, special_care_thresholds, out=None):
    """sdmi_k_safety_head on device tensors -> (has_nsfw int32 [B], concept_scores [B, Nc], special_scores [B, Ns]); `out` = the three
    preallocated outputs."""
    if not image_embeds.is_cuda:
        raise RuntimeError('safety_head runs on MI355X device tensors only (no CPU fallback)')
    B, E = image_embeds.shape
    Nc, Ns = concept_embeds.shape[0], special_care_embeds.shape[0]
    dev = image_embeds.device
    if out is None:
        out = (torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, Nc), dtype=torch.float32, device=dev),
               torch.empty((B, Ns), dtype=torch.float32, device=dev))
    for t in (image_embeds, concept_embeds, special_care_embeds, concept_thresholds, special_care_thresholds):
        assert t.dtype == torch.float32 and t.is_contiguous()
    has, cs, ss = out
    _lib.check(_lib.load().sdmi_k_safety_head(image_embeds.data_ptr(), concept_embeds.data_ptr(), special_care_embeds.data_ptr() if Ns else None,
                                              concept_thresholds.data_ptr(), special_care_thresholds.data_ptr() if Ns else None, has.data_ptr(),
                                              cs.data_ptr(), ss.data_ptr() if Ns else None, B, Nc, Ns, E, _lib.stream_ptr()))
    return has, cs, ss


CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)
PIL_BICUBIC = 3                                       # PIL.Image.BICUBIC, the `resample` of the shipped preprocessor_config.json
# (dtype is uint8, layout, value_range) -> SDMI_FE_SRC_*
_FE_KINDS = {(True, 'NHWC', None): 0, (False, 'NHWC', (0.0, 1.0)): 1, (False, 'NCHW', (0.0, 1.0)): 2, (False, 'NCHW', (-1.0, 1.0)): 3}


def _fe_int(v, keys, what):
    """`size` / `crop_size` as transformers writes them: an int, or a dict ({'shortest_edge': n} / {'height': n, 'width': n})"""
    if isinstance(v, dict):
        vals = {int(v[k]) for k in keys if k in v}
        if len(vals) != 1:
            raise NotImplementedError(f'CLIPFeatureExtractorHIP: {what}={v!r} is not supported (one number: {" / ".join(keys)})')
        return vals.pop()
    return int(v)


class FeatureBatch(dict):
    """What the extractor returns: `.pixel_values`, also by key (transformers' BatchFeature, as far as the scripts use it)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def to(self, *a, **k):
        return FeatureBatch({key: (v.to(*a, **k) if torch.is_tensor(v) else v) for key, v in self.items()})


class CLIPFeatureExtractorHIP:
    """transformers' CLIPFeatureExtractor / CLIPImageProcessor of the safety checker (scripts/txt2img.py:26-29, 88-90) on the MI355X: numpy_to_pil's
    uint8 conversion, PIL's bicubic resize of the shortest side to `size`, the centre crop to `crop_size`, / 255, mean / std -- two launches of
    `sdmi_k_clip_feature_extract`, the resized uint8 image bit-equal to PIL's.  `__call__(images, return_tensors='pt')` -> an object with
    `.pixel_values`, a device fp32 [B, 3, crop, crop] tensor.  `images`:

      * a device tensor, [B, ...] or one image: uint8 [H, W, 3]; or float, by `layout` ('NHWC', the default: the script's x_image; or 'NCHW')
        and `value_range` ((0, 1), the default; or (-1, 1) with 'NCHW': the raw decode_first_stage output, clamp((x + 1) / 2, 0, 1) applied
        inside).  Values outside the range are clamped.
      * a uint8 numpy array [H, W, 3] / [B, H, W, 3], or a list of PIL RGB images / uint8 arrays: uploaded as uint8 in one copy per image size.

    Bicubic, RGB and crop_size <= size only; everything else is refused by name.  A CPU float tensor is refused: there is no CPU path."""

    model_input_names = ['pixel_values']

    def __init__(self, size=224, crop_size=224, image_mean=CLIP_IMAGE_MEAN, image_std=CLIP_IMAGE_STD, resample=PIL_BICUBIC, do_resize=True,
                 do_center_crop=True, do_normalize=True, do_rescale=True, rescale_factor=1 / 255, device=None):
        if int(resample) != PIL_BICUBIC:
            raise NotImplementedError(f'CLIPFeatureExtractorHIP: resample={resample!r} is not built (bicubic, PIL.Image.BICUBIC = 3, only)')
        for name, v in (('do_resize', do_resize), ('do_center_crop', do_center_crop), ('do_normalize', do_normalize), ('do_rescale', do_rescale)):
            if not v:
                raise NotImplementedError(f'CLIPFeatureExtractorHIP: {name}=False is not built (resize, centre crop, / 255 and normalise always run)')
        if abs(float(rescale_factor) - 1 / 255) > 1e-12:
            raise NotImplementedError(f'CLIPFeatureExtractorHIP: rescale_factor={rescale_factor!r} is not built (1 / 255 only)')
        self.size = _fe_int(size, ('shortest_edge',), 'size')
        self.crop_size = _fe_int(crop_size, ('height', 'width'), 'crop_size')
        if self.size < 1 or self.crop_size < 1:
            raise ValueError('CLIPFeatureExtractorHIP: size and crop_size must be at least 1')
        if self.crop_size > self.size:
            raise NotImplementedError(f'CLIPFeatureExtractorHIP: crop_size > size ({self.crop_size} > {self.size}) is not built '
                                      '(the processor would pad the image)')
        self.image_mean, self.image_std = tuple(float(v) for v in image_mean), tuple(float(v) for v in image_std)
        if len(self.image_mean) != 3 or len(self.image_std) != 3:
            raise NotImplementedError('CLIPFeatureExtractorHIP: a channel count other than 3 (RGB images only)')
        self.resample = PIL_BICUBIC
        self.device = device
        self._mean = (C.c_float * 3)(*self.image_mean)
        self._std = (C.c_float * 3)(*self.image_std)
        self._tables = {}

    @classmethod
    def from_pretrained(cls, local_dir, **kwargs):
        """A LOCAL directory holding preprocessor_config.json; never reaches for a hub."""
        path = os.path.join(local_dir, 'preprocessor_config.json')
        if not os.path.isdir(local_dir) or not os.path.exists(path):
            raise FileNotFoundError(f'{local_dir!r}: no local preprocessor_config.json (CLIPFeatureExtractorHIP.from_pretrained loads local '
                                    'files only; nothing is downloaded)')
        with open(path) as f:
            cfg = json.load(f)
        known = ('size', 'crop_size', 'image_mean', 'image_std', 'resample', 'do_resize', 'do_center_crop', 'do_normalize', 'do_rescale',
                 'rescale_factor')
        args = {k: cfg[k] for k in known if cfg.get(k) is not None}
        args.update(kwargs)
        return cls(**args)

    def output_size(self, H, W):
        """(rh, rw) of the resize: the shortest side becomes `size`, the other int(size * long / short)"""
        rh, rw = C.c_int(), C.c_int()
        _lib.check(_lib.load().sdmi_fe_output_size(int(H), int(W), self.size, C.byref(rh), C.byref(rw)))
        return rh.value, rw.value

    def tables(self, H, W):
        """Host tables of an (H, W) image, numpy int32: {'h': (ksize, bounds [rw, 2], kk [rw, ksize]) or None, 'v': ... or None}; an axis
        that keeps its size has none.  No GPU involved."""
        lib = _lib.load()
        rh, rw = self.output_size(H, W)
        out = {}
        for name, n_in, n_out in (('h', W, rw), ('v', H, rh)):
            if n_in == n_out:
                out[name] = None
                continue
            ks = lib.sdmi_fe_ksize(n_in, n_out)
            if ks < 0:
                _lib.check(-1)
            bounds, kk = np.empty((n_out, 2), np.int32), np.empty((n_out, ks), np.int32)
            _lib.check(lib.sdmi_fe_coeffs(n_in, n_out, bounds.ctypes.data, kk.ctypes.data))
            out[name] = (ks, bounds, kk)
        return out

    def _device_tables(self, H, W, device):
        key = (H, W, str(device))
        t = self._tables.get(key)
        if t is None:               # one upload per image size and device; the entries are never written again
            t = {name: (None if v is None else (v[0], torch.from_numpy(v[1]).to(device), torch.from_numpy(v[2]).to(device)))
                 for name, v in self.tables(H, W).items()}
            self._tables[key] = t
        return t

    @torch.no_grad()
    def extract(self, x, layout='NHWC', value_range=(0, 1), return_uint8=False):
        """One device batch of equal-sized images -> pixel_values (and the resized, cropped uint8 image [B, crop, crop, 3])."""
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError('CLIPFeatureExtractorHIP runs on MI355X device tensors only (no CPU fallback)')
        is_u8 = x.dtype == torch.uint8
        if not is_u8 and not x.is_floating_point():
            raise TypeError(f'CLIPFeatureExtractorHIP: images must be uint8 or float, got {x.dtype}')
        kind = _FE_KINDS.get((is_u8, layout, None if is_u8 else tuple(float(v) for v in value_range)))
        if kind is None:
            raise NotImplementedError(f'CLIPFeatureExtractorHIP: dtype {x.dtype} with layout={layout!r}, value_range={value_range!r} is not a '
                                      "source kind (uint8 'NHWC'; float 'NHWC' (0, 1); float 'NCHW' (0, 1) or (-1, 1))")
        if x.dim() == 3:
            x = x[None]
        if x.dim() != 4:
            raise ValueError(f'CLIPFeatureExtractorHIP: images must be [B, H, W, 3] or [B, 3, H, W], got {tuple(x.shape)}')
        x = (x if is_u8 else x.detach().float()).contiguous()
        B, (H, W, Cc) = x.shape[0], ((x.shape[1], x.shape[2], x.shape[3]) if layout == 'NHWC' else (x.shape[2], x.shape[3], x.shape[1]))
        lib = _lib.load()
        S, Cr = self.size, self.crop_size
        t = self._device_tables(H, W, x.device) if Cc == 3 else {'h': None, 'v': None}       # (C != 3: the library refuses it by name)
        need = lib.sdmi_fe_workspace_bytes(B, H, W, S, Cr)
        if need < 0:
            _lib.check(-1)
        ws = torch.empty(max(int(need), 1), dtype=torch.uint8, device=x.device)
        pv = torch.empty((B, 3, Cr, Cr), dtype=torch.float32, device=x.device)
        u8 = torch.empty((B, Cr, Cr, 3), dtype=torch.uint8, device=x.device) if return_uint8 else None
        hks, hb, hk = t['h'] or (0, None, None)
        vks, vb, vk = t['v'] or (0, None, None)
        _lib.check(lib.sdmi_k_clip_feature_extract(x.data_ptr(), kind, B, Cc, H, W, S, Cr, _lib.ptr(hb), _lib.ptr(hk), hks, _lib.ptr(vb), _lib.ptr(vk),
                                                   vks, self._mean, self._std, ws.data_ptr(), ws.numel(), pv.data_ptr(), _lib.ptr(u8),
                                                   _lib.stream_ptr()))
        return (pv, u8) if return_uint8 else pv

    def _upload_groups(self, arrays):
        """uint8 host images -> [(indices, device batch)] with one upload per image size"""
        dev = self.device if self.device is not None else 'cuda'
        groups = {}
        for i, a in enumerate(arrays):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise NotImplementedError(f'CLIPFeatureExtractorHIP: host images must be uint8 RGB [H, W, 3], got {a.dtype} {a.shape}')
            groups.setdefault(a.shape, []).append(i)
        return [(idx, torch.from_numpy(np.stack([arrays[i] for i in idx])).to(dev)) for idx in groups.values()]

    def __call__(self, images, return_tensors='pt', layout='NHWC', value_range=(0, 1)):
        if return_tensors != 'pt':
            raise NotImplementedError(f"CLIPFeatureExtractorHIP: return_tensors={return_tensors!r} is not built ('pt' only)")
        if torch.is_tensor(images):
            return FeatureBatch(pixel_values=self.extract(images, layout, value_range))
        if isinstance(images, np.ndarray):
            if images.dtype != np.uint8:
                raise RuntimeError('CLIPFeatureExtractorHIP: a host float image has no path here (no CPU fallback); pass uint8, or a device tensor')
            arrays = [images] if images.ndim == 3 else list(images)
        else:
            arrays = []
            for im in (images if isinstance(images, (list, tuple)) else [images]):
                if torch.is_tensor(im):
                    raise NotImplementedError('CLIPFeatureExtractorHIP: a list of tensors is not a source kind (stack them into one device tensor)')
                if not isinstance(im, np.ndarray):          # a PIL image
                    if getattr(im, 'mode', 'RGB') != 'RGB':
                        raise NotImplementedError(f'CLIPFeatureExtractorHIP: image mode {im.mode!r} is not built (RGB only)')
                    im = np.asarray(im)
                arrays.append(im)
        if not arrays:
            raise ValueError('CLIPFeatureExtractorHIP: no images')
        groups = self._upload_groups(arrays)
        if len(groups) == 1:
            return FeatureBatch(pixel_values=self.extract(groups[0][1]))
        pv = torch.empty((len(arrays), 3, self.crop_size, self.crop_size), dtype=torch.float32, device=groups[0][1].device)
        for idx, batch in groups:
            pv[torch.tensor(idx, device=pv.device)] = self.extract(batch)
        return FeatureBatch(pixel_values=pv)


def _read_checkpoint(local_dir):
    """state dict of a local `model.safetensors` or `pytorch_model.bin`; local files only"""
    st = os.path.join(local_dir, 'model.safetensors')
    if os.path.exists(st):
        from safetensors.torch import load_file
        return load_file(st)
    pt = os.path.join(local_dir, 'pytorch_model.bin')
    if os.path.exists(pt):
        return torch.load(pt, map_location='cpu')
    raise FileNotFoundError(f'{local_dir}: neither model.safetensors nor pytorch_model.bin (local files only; nothing is downloaded)')


class StableDiffusionSafetyCheckerHIP(nn.Module):
    """`forward(clip_input, images)` -> (images, has_nsfw_concepts) as scripts/txt2img.py:check_safety uses them: flagged entries of the numpy
    `images` are replaced by zeros, `has_nsfw_concepts` is a list of bools.  Parameter names are the shipped checker's:
    `vision_model.vision_model.*`, `visual_projection.weight`, `concept_embeds`, `special_care_embeds`, `concept_embeds_weights`,
    `special_care_embeds_weights` (load_state_dict(strict=True) of its checkpoint)."""

    def __init__(self, vision_config=None, n_concepts=SAFETY_CONCEPTS, n_special_care=SAFETY_SPECIAL_CARE, hip_precision='mixed'):
        super().__init__()
        _check_precision(hip_precision)
        self._tower = [CLIPVisionHIP(vision_config, hip_precision)]          # (kept out of _modules: its parameters are mirrored below)
        tower = self._tower[0]
        # the checker nests CLIPVisionModel one level deeper and owns the projection itself
        self.add_module('vision_model', _Node())
        self.vision_model.add_module('vision_model', tower._modules['vision_model'])
        self.add_module('visual_projection', tower._modules['visual_projection'])
        Pd = tower._cfg.projection_dim
        self.concept_embeds = nn.Parameter(torch.ones(n_concepts, Pd), requires_grad=False)
        self.special_care_embeds = nn.Parameter(torch.ones(n_special_care, Pd), requires_grad=False)
        self.concept_embeds_weights = nn.Parameter(torch.ones(n_concepts), requires_grad=False)
        self.special_care_embeds_weights = nn.Parameter(torch.ones(n_special_care), requires_grad=False)
        self.last_scores = None
        self.eval()

    @classmethod
    def from_pretrained(cls, local_dir, **kwargs):
        """A LOCAL directory holding config.json and model.safetensors / pytorch_model.bin; never reaches for a hub."""
        if not os.path.isdir(local_dir):
            raise FileNotFoundError(f'{local_dir!r} is not a local directory (StableDiffusionSafetyCheckerHIP.from_pretrained loads local files only)')
        with open(os.path.join(local_dir, 'config.json')) as f:
            cfg = json.load(f)
        vc = dict(CLIP_VIT_L14_VISION)
        vc.update({k: v for k, v in (cfg.get('vision_config') or cfg.get('vision_config_dict') or {}).items() if k in vc or k == 'hidden_act'})
        vc['projection_dim'] = int(cfg.get('projection_dim', vc['projection_dim']))
        sd = _read_checkpoint(local_dir)
        sd = {k: v for k, v in sd.items() if not k.endswith('position_ids')}
        m = cls(vc, n_concepts=sd['concept_embeds'].shape[0], n_special_care=sd['special_care_embeds'].shape[0], **kwargs)
        m.load_state_dict(sd, strict=True)
        return m

    def _apply(self, fn, *a, **k):
        self._tower[0].mark_dirty()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, *a, **k):
        self._tower[0].mark_dirty()
        return super().load_state_dict(_without_position_ids(state_dict), *a, **k)

    @torch.no_grad()
    def forward(self, clip_input, images):
        dev = self.concept_embeds.device
        if dev.type != 'cuda':
            raise RuntimeError('StableDiffusionSafetyCheckerHIP parameters must live on the GPU (call .cuda() first); there is no CPU implementation')
        embeds = self._tower[0](clip_input.to(dev))[0]
        has, cs, ss = safety_head(embeds, self.concept_embeds.detach().float().contiguous(), self.special_care_embeds.detach().float().contiguous(),
                                  self.concept_embeds_weights.detach().float().contiguous(),
                                  self.special_care_embeds_weights.detach().float().contiguous())
        self.last_scores = dict(concept_scores=cs, special_scores=ss)
        has_nsfw_concepts = [bool(v) for v in has.cpu().tolist()]
        for i, flagged in enumerate(has_nsfw_concepts):
            if flagged:
                images[i] = torch.zeros_like(images[i]) if torch.is_tensor(images[i]) else np.zeros(images[i].shape)   # (the checker's black image)
        return images, has_nsfw_concepts

    @torch.no_grad()
    def check_images(self, x, extractor=None, layout='NHWC', value_range=(0, 1)):
        """scripts/txt2img.py:check_safety without the image leaving the GPU: device images of any source kind of CLIPFeatureExtractorHIP
        (`layout` / `value_range` as there) -> the extractor, the tower, the head.  Flagged images are zeroed in place on the device; returns
        (x, has_nsfw_concepts) as `forward(clip_input=extractor(x).pixel_values, images=x)` does -- the same launches -- with one small
        device-to-host copy, of the flags."""
        S = self._tower[0]._cfg.image_size
        if extractor is None:
            if getattr(self, '_extractor', None) is None:
                self._extractor = CLIPFeatureExtractorHIP(size=S, crop_size=S)
            extractor = self._extractor
        if extractor.crop_size != S:
            raise ValueError(f"check_images: the extractor's crop_size {extractor.crop_size} differs from the tower's image_size {S}")
        dev = self.concept_embeds.device
        if dev.type != 'cuda':
            raise RuntimeError('StableDiffusionSafetyCheckerHIP parameters must live on the GPU (call .cuda() first); there is no CPU implementation')
        if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 4:
            raise RuntimeError('check_images takes one device batch [B, H, W, 3] / [B, 3, H, W] (no CPU fallback)')
        embeds = self._tower[0](extractor.extract(x, layout, value_range))[0]
        has, cs, ss = safety_head(embeds, self.concept_embeds.detach().float().contiguous(), self.special_care_embeds.detach().float().contiguous(),
                                  self.concept_embeds_weights.detach().float().contiguous(),
                                  self.special_care_embeds_weights.detach().float().contiguous())
        self.last_scores = dict(concept_scores=cs, special_scores=ss)
        x.masked_fill_((has != 0).view(-1, 1, 1, 1), 0)               # (the checker's black image)
        return x, [bool(v) for v in has.cpu().tolist()]


# ---- OpenAI `clip` naming -> transformers naming ----------------------------------------------------------------------------------------
_OPENAI_LAYER = {'ln_1.weight': 'layer_norm1.weight', 'ln_1.bias': 'layer_norm1.bias', 'ln_2.weight': 'layer_norm2.weight',
                 'ln_2.bias': 'layer_norm2.bias', 'attn.out_proj.weight': 'self_attn.out_proj.weight',
                 'attn.out_proj.bias': 'self_attn.out_proj.bias', 'mlp.c_fc.weight': 'mlp.fc1.weight', 'mlp.c_fc.bias': 'mlp.fc1.bias',
                 'mlp.c_proj.weight': 'mlp.fc2.weight', 'mlp.c_proj.bias': 'mlp.fc2.bias'}
_OPENAI_TOP = {'visual.conv1.weight': 'vision_model.embeddings.patch_embedding.weight',
               'visual.class_embedding': 'vision_model.embeddings.class_embedding',
               'visual.positional_embedding': 'vision_model.embeddings.position_embedding.weight',
               'visual.ln_pre.weight': 'vision_model.pre_layrnorm.weight', 'visual.ln_pre.bias': 'vision_model.pre_layrnorm.bias',
               'visual.ln_post.weight': 'vision_model.post_layernorm.weight', 'visual.ln_post.bias': 'vision_model.post_layernorm.bias'}


def openai_clip_to_transformers(sd):
    """State dict of an OpenAI `clip` model (the `visual.*` entries; everything else is ignored) -> CLIPVisionModelWithProjection naming:
    `attn.in_proj_{weight, bias}` split into q | k | v, `visual.proj` ([width, out]) transposed into `visual_projection.weight`."""
    out = {}
    for k, v in sd.items():
        if not k.startswith('visual.'):
            continue
        if k in _OPENAI_TOP:
            out[_OPENAI_TOP[k]] = v
        elif k == 'visual.proj':
            out['visual_projection.weight'] = v.t().contiguous()
        elif k.startswith('visual.transformer.resblocks.'):
            n, rest = k[len('visual.transformer.resblocks.'):].split('.', 1)
            p = f'vision_model.encoder.layers.{n}.'
            if rest in ('attn.in_proj_weight', 'attn.in_proj_bias'):
                leaf = rest.rsplit('_', 1)[1]
                for name, part in zip(('q_proj', 'k_proj', 'v_proj'), v.chunk(3, dim=0)):
                    out[p + f'self_attn.{name}.{leaf}'] = part.contiguous()
            elif rest in _OPENAI_LAYER:
                out[p + _OPENAI_LAYER[rest]] = v
            else:
                raise KeyError(f'unexpected OpenAI-clip key {k!r}')
        else:
            raise KeyError(f'unexpected OpenAI-clip key {k!r}')
    return out


def transformers_to_openai_clip(sd):
    """The inverse of `openai_clip_to_transformers` (tests: the mapping round-trips keys and shapes)."""
    inv_top = {v: k for k, v in _OPENAI_TOP.items()}
    inv_layer = {v: k for k, v in _OPENAI_LAYER.items()}
    out, qkv = {}, {}
    for k, v in sd.items():
        if k in inv_top:
            out[inv_top[k]] = v
        elif k == 'visual_projection.weight':
            out['visual.proj'] = v.t().contiguous()
        else:
            n, rest = k[len('vision_model.encoder.layers.'):].split('.', 1)
            p = f'visual.transformer.resblocks.{n}.'
            if rest in inv_layer:
                out[p + inv_layer[rest]] = v
            else:
                _, name, leaf = rest.split('.')
                qkv.setdefault((p, leaf), {})[name] = v
    for (p, leaf), parts in qkv.items():
        out[p + f'attn.in_proj_{leaf}'] = torch.cat([parts['q_proj'], parts['k_proj'], parts['v_proj']], 0)
    return out


_OPENAI_TEXT_TOP = {'token_embedding.weight': 'text_model.embeddings.token_embedding.weight',
                    'positional_embedding': 'text_model.embeddings.position_embedding.weight',
                    'ln_final.weight': 'text_model.final_layer_norm.weight', 'ln_final.bias': 'text_model.final_layer_norm.bias'}
_OPENAI_NOT_TEXT = ('visual.', 'logit_scale', 'input_resolution', 'context_length', 'vocab_size')


def openai_clip_text_to_transformers(sd):
    """The text half of an OpenAI `clip` state dict (`visual.*`, `logit_scale` and the jit archive's scalars are ignored) ->
    CLIPTextModelWithProjection naming: `transformer.resblocks.N.attn.in_proj_{weight, bias}` split into q | k | v, `text_projection`
    ([width, embed]) transposed into `text_projection.weight`."""
    out = {}
    for k, v in sd.items():
        if k.startswith(_OPENAI_NOT_TEXT):
            continue
        if k in _OPENAI_TEXT_TOP:
            out[_OPENAI_TEXT_TOP[k]] = v
        elif k == 'text_projection':
            out['text_projection.weight'] = v.t().contiguous()
        elif k.startswith('transformer.resblocks.'):
            n, rest = k[len('transformer.resblocks.'):].split('.', 1)
            p = f'text_model.encoder.layers.{n}.'
            if rest in ('attn.in_proj_weight', 'attn.in_proj_bias'):
                leaf = rest.rsplit('_', 1)[1]
                for name, part in zip(('q_proj', 'k_proj', 'v_proj'), v.chunk(3, dim=0)):
                    out[p + f'self_attn.{name}.{leaf}'] = part.contiguous()
            elif rest in _OPENAI_LAYER:
                out[p + _OPENAI_LAYER[rest]] = v
            else:
                raise KeyError(f'unexpected OpenAI-clip key {k!r}')
        else:
            raise KeyError(f'unexpected OpenAI-clip key {k!r}')
    return out


def transformers_to_openai_clip_text(sd):
    """The inverse of `openai_clip_text_to_transformers` (`text_model.embeddings.position_ids` has no OpenAI counterpart and is dropped)."""
    inv_top = {v: k for k, v in _OPENAI_TEXT_TOP.items()}
    inv_layer = {v: k for k, v in _OPENAI_LAYER.items()}
    out, qkv = {}, {}
    for k, v in sd.items():
        if k in inv_top:
            out[inv_top[k]] = v
        elif k == 'text_projection.weight':
            out['text_projection'] = v.t().contiguous()
        elif k == 'text_model.embeddings.position_ids':
            continue
        elif k.startswith('text_model.encoder.layers.'):
            n, rest = k[len('text_model.encoder.layers.'):].split('.', 1)
            p = f'transformer.resblocks.{n}.'
            if rest in inv_layer:
                out[p + inv_layer[rest]] = v
            else:
                _, name, leaf = rest.split('.')
                qkv.setdefault((p, leaf), {})[name] = v
        else:
            raise KeyError(f'unexpected CLIPTextModelWithProjection key {k!r}')
    for (p, leaf), parts in qkv.items():
        out[p + f'attn.in_proj_{leaf}'] = torch.cat([parts['q_proj'], parts['k_proj'], parts['v_proj']], 0)
    return out


class FrozenClipImageEmbedderHIP(nn.Module):
    """modules.py:197-228: `preprocess` = bicubic resize to the tower's image size (align_corners=True), (x + 1) / 2, CLIP mean / std -- one launch
    of sdmi_k_vit_preprocess; `forward(x)` = image_embeds of the preprocessed images (`self.model.encode_image`).  Parameters live under
    `model.` in transformers naming; `load_state_dict` also takes OpenAI-`clip` naming (`visual.*`, or `model.visual.*` as the reference's own
    module names them) and converts it."""

    def __init__(self, vision_config=None, antialias=False, hip_precision='mixed'):
        super().__init__()
        if antialias:
            raise NotImplementedError('FrozenClipImageEmbedderHIP: antialias=True is not supported (the resize kernel does not antialias)')
        self.antialias = False
        self.add_module('model', CLIPVisionHIP(vision_config, hip_precision))
        self.eval()

    def load_state_dict(self, state_dict, *a, **k):
        sd = _without_position_ids(state_dict)
        self.model.mark_dirty()
        if any(key.startswith(('visual.', 'model.visual.')) for key in sd):
            sd = {'model.' + key: v for key, v in
                  openai_clip_to_transformers({(key[len('model.'):] if key.startswith('model.') else key): v for key, v in sd.items()}).items()}
        return super().load_state_dict(sd, *a, **k)

    @torch.no_grad()
    def preprocess(self, x):
        if not x.is_cuda:
            raise RuntimeError('FrozenClipImageEmbedderHIP runs on MI355X device tensors only (no CPU fallback)')
        x = x.detach().float().contiguous()
        B, Cc, H, W = x.shape
        if Cc != 3:
            raise ValueError('preprocess expects [B, 3, H, W] images in [-1, 1]')
        S = self.model._cfg.image_size
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().sdmi_k_vit_preprocess(x.data_ptr(), out.data_ptr(), B, H, W, S, _lib.stream_ptr()))
        return out

    def forward(self, x):
        return self.model(self.preprocess(x))[0]
