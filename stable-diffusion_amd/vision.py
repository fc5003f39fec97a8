"""The CLIP image encoder on MI355X: the vision tower, the NSFW safety checker and the image embedder.

    CLIPVisionHIP                   <- transformers.CLIPVisionModelWithProjection
    StableDiffusionSafetyCheckerHIP <- diffusers.pipelines.stable_diffusion.safety_checker.StableDiffusionSafetyChecker
                                       (scripts/txt2img.py:26-29, 88-95; scripts/img2img.py)
    FrozenClipImageEmbedderHIP      <- ldm.modules.encoders.modules.FrozenClipImageEmbedder (modules.py:197-228)

The tower (patch embedding, 24 pre-norm encoder layers, post-LayerNorm, projection) runs in libsdmi.so behind the `sdmi_vit_*` handle, the concept
head in `sdmi_k_safety_head`, the embedder's bicubic preprocess in `sdmi_k_vit_preprocess`.  Mixed precision only: fp16 MFMA operands, fp32
accumulation and residual stream.  The feature extractor (PIL resize and crop) stays the reference's host call, as the tokenizer does.  No CPU /
PyTorch fallback.
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
