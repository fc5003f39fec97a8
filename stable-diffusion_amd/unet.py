"""`UNetModelHIP` -- drop-in for `ldm.modules.diffusionmodules.openaimodel.UNetModel` on MI355X.

Plugged in through the reference's own plugin mechanism (`instantiate_from_config`, ldm/util.py:78-93):
a copy of configs/stable-diffusion/v1-inference.yaml with

    unet_config:
      target: stable_diffusion_amd.unet.UNetModelHIP

Same constructor keywords (openaimodel.py:443-470), same parameter names (so
`model.load_state_dict(sd, strict=False)` at scripts/txt2img.py:56 fills it), same call
`diffusion_model(x, t, context=cc)` (ldm/models/diffusion/ddpm.py:1410).  The latent-inpainting UNet
(models/ldm/inpainting_big/config.yaml: legacy AttentionBlocks, resblock_updown, no context) is the second family:
`diffusion_model(cat([x, c_concat], 1), t)` (ddpm.py:1411-1413).  The unconditional LSUN-Churches UNet
(models/ldm/lsun_churches256/config.yaml: the same blocks with use_scale_shift_norm, five levels, attention at the full
latent resolution) is the third: `diffusion_model(x, t)` (ddpm.py DiffusionWrapper, conditioning_key None).  The arithmetic runs in
libsdmi.so (hand-written gfx950 kernels); this class only owns the parameters, packs them into the
library on first use and hands raw device pointers across the C ABI.
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib


def make_cfg(in_channels, out_channels, model_channels, num_res_blocks, channel_mult, attention_resolutions,
             num_heads, transformer_depth, context_dim):
    cfg = _lib.UNetCfg()
    cfg.in_channels, cfg.out_channels, cfg.model_channels = in_channels, out_channels, model_channels
    cfg.num_res_blocks = num_res_blocks
    channel_mult = list(channel_mult)
    attention_resolutions = list(attention_resolutions)
    if len(channel_mult) > 8 or len(attention_resolutions) > 8:
        raise ValueError('at most 8 levels / attention resolutions')
    cfg.n_levels = len(channel_mult)
    for i, m in enumerate(channel_mult):
        cfg.channel_mult[i] = int(m)
    cfg.n_attention_resolutions = len(attention_resolutions)
    for i, a in enumerate(attention_resolutions):
        cfg.attention_resolutions[i] = int(a)
    cfg.num_heads, cfg.transformer_depth, cfg.context_dim = num_heads, transformer_depth, int(context_dim)
    return cfg


PRECISIONS = {'mixed': 0, 'full': 1}      # SDMI_PRECISION_MIXED / SDMI_PRECISION_FULL (include/sdmi.h)
UNET_SCALE_SHIFT_NORM = 1                 # SDMI_UNET_SCALE_SHIFT_NORM (sdmi_unet_create_flags)


def unet_num_head_channels_flag(n):
    """SDMI_UNET_NUM_HEAD_CHANNELS(n) (include/sdmi.h): num_head_channels rides in bits 16..27 of the creation flag word"""
    if not 0 < int(n) < 4096:
        raise ValueError(f'num_head_channels must be 1..4095, got {n}')
    return int(n) << 16


class _Handle:
    """Owns one sdmi_unet*."""

    def __init__(self, cfg, precision='mixed', ext=None, flags=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        if flags:
            _lib.check(self.lib.sdmi_unet_create_flags(C.byref(cfg), C.byref(ext), flags, PRECISIONS[precision], C.byref(h)))
        elif ext is None:
            _lib.check(self.lib.sdmi_unet_create_with_precision(C.byref(cfg), PRECISIONS[precision], C.byref(h)))
        else:
            _lib.check(self.lib.sdmi_unet_create_ext(C.byref(cfg), C.byref(ext), PRECISIONS[precision], C.byref(h)))
        self.h = h

    def weight_specs(self):
        n = self.lib.sdmi_unet_num_weights(self.h)
        out = []
        buf = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(n):
            _lib.check(self.lib.sdmi_unet_weight_info(self.h, i, buf, 256, shape, C.byref(nd)))
            out.append((buf.value.decode(), tuple(shape[j] for j in range(nd.value))))
        return out

    def __del__(self):
        try:
            if self.h:
                self.lib.sdmi_unet_destroy(self.h)
                self.h = None
        except Exception:
            pass


class _Node(nn.Module):
    """Name-only container so parameter paths equal the reference's (e.g. input_blocks.1.0.in_layers.0.weight)."""


class UNetModelHIP(nn.Module):
    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None,
                 use_checkpoint=False, use_fp16=False, num_heads=-1, num_head_channels=-1, num_heads_upsample=-1,
                 use_scale_shift_norm=False, resblock_updown=False, use_new_attention_order=False,
                 use_spatial_transformer=False, transformer_depth=1, context_dim=None, n_embed=None, legacy=True,
                 hip_precision='mixed'):
        """`hip_precision` (not a keyword of the reference UNetModel): 'mixed' (default) = fp16 MFMA operands with split-fp16 where the
        precision allocation puts it; 'full' = every MFMA operand split-fp16 (~22-bit operands, fp32 accumulation),
        slower.  Fixed for the module's lifetime; packed-weight blobs are tied to it."""
        super().__init__()
        if hip_precision not in PRECISIONS:
            raise ValueError(f"hip_precision must be one of {sorted(PRECISIONS)}, got {hip_precision!r}")
        self.hip_precision = hip_precision
        # three families, anything else is refused loudly:
        #   SD v1 (configs/stable-diffusion/v1-inference.yaml:29-44): SpatialTransformers with cross-attention, legacy=False; the
        #   class-conditional ImageNet model (configs/latent-diffusion/cin256-v2.yaml:19-39) is the same family with num_heads=1
        #   (d_head = C = 384 / 576 / 960) and legacy left at True -- with num_head_channels == -1 that flag changes nothing for a
        #   SpatialTransformer (openaimodel.py:542-549: dim_head = ch // num_heads either way)
        #   latent inpainting (models/ldm/inpainting_big/config.yaml:24-41): legacy AttentionBlocks (num_heads, no context),
        #   ResBlocks with resampling (resblock_updown)
        #   unconditional LSUN-Churches (models/ldm/lsun_churches256/config.yaml:33-52): the inpainting family's blocks with
        #   use_scale_shift_norm (openaimodel.py:267-271), nothing concatenated (in_channels == out_channels), five levels, attention
        #   at every resolution down to the full latent one (head dims 24 / 48 / 96)
        #   faces / bedrooms / super-resolution (models/ldm/celeba256, ffhq256, lsun_beds256: one unet_config, model_channels 224;
        #   models/ldm/bsr_sr: 160): legacy AttentionBlocks with num_head_channels=32 and num_heads left at -1 (openaimodel.py:561-563:
        #   heads = ch // 32 -> 14 / 21 / 28, 20), plain Downsample / Upsample convolutions, no scale-shift norm; widths that are
        #   multiples of 32, not of 64 (the GEMM kernels' half k-tile).
        #   retrieval-augmented diffusion / layout-to-image (configs/retrieval-augmented-diffusion/768x768.yaml:19-42,
        #   models/ldm/layout2img-openimages256/config.yaml:16-36): SD v1's SpatialTransformer blocks with num_head_channels=32 and
        #   num_heads left at -1, legacy at its default True.  openaimodel.py:542-549 gives num_heads = ch // num_head_channels and
        #   dim_head = num_head_channels with legacy False, and with legacy True recomputes dim_head = ch // num_heads -- the same
        #   number wherever num_head_channels divides ch (checked against the reference module: tools/make_golden_rdm.py builds it
        #   with either flag and gets one key list and one output).  Admitted for the head dims the tests run (ST_HEAD_CHANNELS).
        #   semantic synthesis (models/ldm/semantic_synthesis256 / 512 config.yaml:16-32): the inpainting family's legacy AttentionBlocks
        #   (num_heads=8) with the face family's plain Downsample / Upsample convolutions (resblock_updown=False), model_channels 128,
        #   channel_mult [1, 4, 8] (a 128 -> 512 ResBlock), six input channels.  attention_resolutions [32, 16, 8] names none of the
        #   three levels (ds 1 / 2 / 4), so the only attention is the middle block's: 8 heads of 128 at width 1024.
        self.use_spatial_transformer = bool(use_spatial_transformer)
        unsupported = []
        if use_spatial_transformer:
            if context_dim is None: unsupported.append('use_spatial_transformer=True with context_dim')
            if resblock_updown: unsupported.append('resblock_updown=False with a spatial transformer')
        else:
            if context_dim is not None: unsupported.append('context_dim=None without a spatial transformer')
            if not legacy: unsupported.append('legacy=True without a spatial transformer')
            if use_new_attention_order: unsupported.append('use_new_attention_order=False (QKVAttentionLegacy)')
        nhc = num_head_channels != -1
        if nhc:
            # the reference asserts exactly one of the two is set (openaimodel.py:489-493) and lets num_head_channels win where both are
            if num_heads != -1: unsupported.append('num_head_channels with num_heads == -1 (one of the two, as the shipped configs)')
            chans = [model_channels * m for i, m in enumerate(channel_mult) if 2 ** i in list(attention_resolutions)]
            chans.append(model_channels * list(channel_mult)[-1])       # (the middle block)
            if num_head_channels < 1 or any(c % num_head_channels for c in chans):
                unsupported.append(f'num_head_channels={num_head_channels} dividing every attention level ({sorted(set(chans))})')
            elif use_spatial_transformer and num_head_channels not in self.ST_HEAD_CHANNELS:
                unsupported.append(f'num_head_channels in {sorted(self.ST_HEAD_CHANNELS)} with a spatial transformer (the head dims this '
                                   f'family is tested at), got num_head_channels={num_head_channels}')
        elif num_heads == -1:
            unsupported.append('num_heads or num_head_channels')
        if model_channels % 32 or (use_spatial_transformer and model_channels % 64):
            unsupported.append('model_channels a multiple of 64 (of 32 without a spatial transformer), got %d' % model_channels)
        if num_heads_upsample not in (-1, num_heads): unsupported.append('num_heads_upsample == num_heads')
        if dims != 2 or not conv_resample: unsupported.append('dims=2, conv_resample')
        if use_scale_shift_norm:
            # admitted for the family it is validated on and no wider: the unconditional models
            rule = []
            if use_spatial_transformer: rule.append('no spatial transformer')
            if not resblock_updown: rule.append('resblock_updown=True')
            if num_heads == -1 or num_head_channels != -1: rule.append('num_heads (not num_head_channels)')
            if in_channels != out_channels: rule.append('in_channels == out_channels (nothing concatenated)')
            if rule:
                unsupported.append('scale-shift norm (use_scale_shift_norm=True) only for the unconditional family -- no spatial '
                                   'transformer, resblock_updown=True, num_heads given, in_channels == out_channels; this configuration '
                                   'lacks: ' + ', '.join(rule))
        if num_classes is not None or n_embed is not None: unsupported.append('no class conditioning / codebook head')
        if dropout != 0: unsupported.append('dropout=0')
        if use_spatial_transformer and hip_precision == 'full' and (nhc or num_heads > 0):
            # heads wider than 160 run on the wide-head kernel (csrc/attn_wide.hip), which has no split-fp16 form.  (In front of the other
            # refusals: with num_head_channels set the head dim is that number, and one above the limit is named as such.)
            levels = [model_channels * m for i, m in enumerate(channel_mult) if 2 ** i in list(attention_resolutions)]
            d_max = num_head_channels if nhc else max(levels + [model_channels * list(channel_mult)[-1]]) // num_heads
            if d_max > self.FULL_MAX_HEAD_DIM:
                how = f'num_head_channels={num_head_channels}' if nhc else f'num_heads={num_heads}'
                raise NotImplementedError(f"hip_precision='full' supports attention head dims up to {self.FULL_MAX_HEAD_DIM}; this "
                                          f'configuration has d_head = {d_max} ({how}): use hip_precision=\'mixed\'')
        if unsupported:
            raise NotImplementedError('UNetModelHIP supports the SD-v1, latent-inpainting, unconditional, semantic-synthesis and num_head_channels AttentionBlock / '
                                      'SpatialTransformer UNet families only; needs: ' +
                                      '; '.join(unsupported))
        if isinstance(context_dim, (list, tuple)) or type(context_dim).__name__ == 'ListConfig':
            context_dim = list(context_dim)[0]
        context_dim = 0 if context_dim is None else context_dim
        self.resblock_updown = bool(resblock_updown)
        self.use_scale_shift_norm = bool(use_scale_shift_norm)
        self.image_size = image_size
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = list(attention_resolutions)
        self.channel_mult = list(channel_mult)
        self.num_heads, self.transformer_depth, self.context_dim = num_heads, transformer_depth, int(context_dim)
        self.use_checkpoint = use_checkpoint      # accepted, meaningless at inference (util.py:102-128)
        self.dtype = torch.float32
        self._cfg = make_cfg(in_channels, out_channels, model_channels, num_res_blocks, self.channel_mult,
                             self.attention_resolutions, num_heads, transformer_depth, self.context_dim)
        ext = None
        if not use_spatial_transformer or resblock_updown or nhc:      # (the creation flag word travels with an ext struct)
            ext = _lib.UNetExt()
            ext.attention_block, ext.resblock_updown = int(not use_spatial_transformer), int(bool(resblock_updown))
        self.num_head_channels = num_head_channels
        flags = (UNET_SCALE_SHIFT_NORM if use_scale_shift_norm else 0) | (unet_num_head_channels_flag(num_head_channels) if nhc else 0)
        self._handle = _Handle(self._cfg, hip_precision, ext, flags)
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
        self._from_blob = False       # weights came from load_packed(): the nn.Parameters are NOT the weight source
        self._sentinels = None
        self._ws = None
        self._ctx_ref = None
        self._ctx_ver = None
        self._ctx_shape = None
        self._pinned = None
        self._pinned_ctx = None

    # ---- weights -> library ---------------------------------------------------------------------------
    # Re-pack whenever the parameters may have changed: device moves / dtype casts (_apply), load_state_dict,
    # or an explicit mark_dirty() after in-place edits.  A cheap per-call check of a few sentinel tensors catches
    # the common in-place cases without walking all 686 parameters on the hot path.
    # After load_packed() the library's packed buffers are the only weight source (the parameters stay at their zero
    # initialisation): a device move / dtype cast must then NOT trigger a repack from the parameters -- that would
    # silently replace the blob with all-zero weights.  load_state_dict() / mark_dirty() hand the role back to the parameters.
    def _apply(self, fn, *a, **k):
        if not self._from_blob:
            self._packed_sig = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed_sig = None
        self._from_blob = False
        return super().load_state_dict(*a, **k)

    def mark_dirty(self):
        self._packed_sig = None
        self._from_blob = False

    def _needs_pack(self):
        if self._from_blob:
            return False
        return self._packed_sig is None or self._packed_sig != self._signature()

    def _signature(self):
        if getattr(self, '_sentinels', None) is None:
            ps = dict(self.named_parameters())
            keys = [self._specs[0][0], self._specs[len(self._specs) // 2][0], self._specs[-1][0]]
            self._sentinels = [ps[k] for k in keys]
        return tuple((p.data_ptr(), p._version) for p in self._sentinels)

    def pack(self):
        """Hand every parameter to the library (repacked to fp16 [N][K] there). Called lazily by forward()."""
        lib = self._handle.lib
        stream = _lib.stream_ptr()
        ps = dict(self.named_parameters())
        for key, shape in self._specs:
            p = ps[key].detach()
            if not p.is_cuda:
                raise RuntimeError('UNetModelHIP parameters must live on the GPU (call model.cuda() first); '
                                   'there is no CPU implementation of this path')
            p = p.float().contiguous()
            shp = (C.c_int64 * len(shape))(*shape)
            _lib.check(lib.sdmi_unet_set_weight(self._handle.h, key.encode(), p.data_ptr(), shp, len(shape), stream))
        torch.cuda.current_stream().synchronize()
        _lib.check(lib.sdmi_unet_finalize(self._handle.h))
        self._sentinels = None
        self._packed_sig = self._signature()
        self._from_blob = False
        self._ctx_ref = None

    # ---- packed-weight blob --------------------------------------------------------------------------
    def save_packed(self, path):
        """Write the library's packed fp16 weights (after pack()) to `path`: header + buffers, mmap-able."""
        import numpy as np
        if self._needs_pack():
            self.pack()
        lib = self._handle.lib
        n = int(lib.sdmi_unet_packed_bytes(self._handle.h))
        buf = np.empty(n, dtype=np.uint8)
        _lib.check(lib.sdmi_unet_export_packed(self._handle.h, buf.ctypes.data, n, _lib.stream_ptr()))
        buf.tofile(path)
        return n

    def load_packed(self, path):
        """Load a blob written by save_packed() / tools/pack_checkpoint.py straight into the library (no fp32 state_dict,
        no repack).  The nn.Parameters of this module are left untouched (they are not used by forward())."""
        import numpy as np
        if not torch.cuda.is_available():
            raise RuntimeError('UNetModelHIP runs on an MI355X only (no CPU fallback)')
        blob = np.memmap(path, dtype=np.uint8, mode='r')
        _lib.check(self._handle.lib.sdmi_unet_import_packed(self._handle.h, blob.ctypes.data, int(blob.shape[0]),
                                                            _lib.stream_ptr()))
        self._sentinels = None
        self._packed_sig = self._signature()
        self._from_blob = True
        self._ctx_ref = None
        return self

    _WS_KEEP = 4      # workspaces kept per module: a chunked batch (8 + 2 rows) or txt2img + img2img shapes alternate between a few

    def _workspace(self, B, H, W, L, device):
        """Caller-owned scratch of sdmi_unet_forward for this shape.  A few shapes are kept (most recently used first), so
        a batch evaluated in chunks of different sizes does not re-size and re-allocate its workspace on every step."""
        key = (B, H, W, L, str(device))
        if self._ws is None:
            self._ws = []
        for i, (k, buf) in enumerate(self._ws):
            if k == key:
                if i:
                    self._ws.insert(0, self._ws.pop(i))
                return buf
        need = self._handle.lib.sdmi_unet_workspace_bytes(self._handle.h, B, H, W, L)
        if need <= 0:
            _lib.check(-1)
        buf = torch.empty(int(need), dtype=torch.uint8, device=device)
        self._ws.insert(0, (key, buf))
        del self._ws[self._WS_KEEP:]
        return buf

    def _reserve_context(self, B, L):
        """K / V^T cache capacity of the library (grow-only; sdmi_unet_forward itself never allocates)."""
        need = B * ((L + 7) // 8 * 8)
        if need > getattr(self, '_ctx_cap', 8 * 80):
            _lib.check(self._handle.lib.sdmi_unet_reserve_context(self._handle.h, B, L))
            self._ctx_cap = need

    # ---- context pinning (used by the HIP samplers) ------------------------------------------------------------
    def pin_context(self, context):
        """Compute the cross-attention K/V of every SpatialTransformer for `context` once (attention.py:174-176
        depend on the context only) and reuse them for every forward() until unpin_context().  A forward() that gets a
        different tensor object is compared with the pinned contents (one small device compare) and, if it differs,
        recomputes its K/V -- an img_callback or a second sampler sharing the UNet never sees stale K/V.
        A UNet without cross-attention (AttentionBlocks) has nothing to cache: a no-op."""
        if not getattr(self, 'use_spatial_transformer', True):
            return
        if not context.is_cuda:
            raise RuntimeError('UNetModelHIP runs on an MI355X device tensor only (no CPU fallback)')
        if self._needs_pack():
            self.pack()
        B, L, D = context.shape
        assert D == self.context_dim
        if B > self.MAX_ROWS:           # the library caches K/V for one call of <= 8 rows: chunked batches recompute them
            self._pinned = None
            return
        down = 2 ** (len(self.channel_mult) - 1)
        ws = self._workspace(B, down, down, L, context.device)
        self._reserve_context(B, L)
        ctx32 = context.detach().float().contiguous()
        _lib.check(self._handle.lib.sdmi_unet_cache_context(self._handle.h, ctx32.data_ptr(), B, L, ws.data_ptr(),
                                                            ws.numel(), _lib.stream_ptr()))
        self._pinned = (B, L)
        self._pinned_ctx = (context, context._version, ctx32.clone() if ctx32 is context else ctx32)
        self._ctx_ref = None

    def unpin_context(self):
        self._pinned = None
        self._pinned_ctx = None

    # ---- timestep table (used by the HIP samplers) ----------------------------------------------------------------
    def cache_timesteps(self, timesteps):
        """Compute the timestep path -- timestep_embedding -> time_embed -> the 22 emb_layers (openaimodel.py:723-724,
        218-224), which depends on the timestep only -- for a list of INTEGER timesteps in one batch
        (sdmi_unet_cache_timesteps).  A forward() announced by hint_timestep(t) then takes its rows from the table instead
        of re-reading the 103 MB of fp32 emb_layers weights; the values are bit-identical.  SDMI_T_TABLE=0 disables it."""
        if os.environ.get('SDMI_T_TABLE', '1') == '0':
            return
        if self._needs_pack():
            self.pack()
        ts = sorted({int(t) for t in timesteps})
        arr = (C.c_int64 * len(ts))(*ts)
        _lib.check(self._handle.lib.sdmi_unet_cache_timesteps(self._handle.h, arr, len(ts), _lib.stream_ptr()))

    def hint_timestep(self, t):
        """Every row of the NEXT forward()'s integer `timesteps` tensor equals t (the samplers build that tensor from this
        very int, plms.py:137, ddim.py:148): take the cached rows if cache_timesteps() covered t."""
        self._t_hint = int(t)

    def clear_timestep_hint(self):
        """Drop a hint that was not consumed (the samplers call this when apply_model raised before reaching forward())."""
        self._t_hint = None

    def _pinned_matches(self, context):
        ref, ver, saved = self._pinned_ctx
        if context is ref and context._version == ver:
            return True
        c = context.detach()
        return bool(torch.equal(c if c.dtype == torch.float32 else c.float(), saved))

    # ---- UNetModel.forward (openaimodel.py:710-742) ----------------------------------------------------------
    FULL_MAX_HEAD_DIM = 160       # widest head of the split-fp16 attention kernel (csrc/attn_split16.hip)
    ST_HEAD_CHANNELS = (32,)      # num_head_channels admitted with a spatial transformer: the head dims tests/test_rdm_gpu.py runs
    MAX_ROWS = 8      # rows per library call (sdmi_unet_forward); larger batches are split, rows are independent

    @torch.no_grad()
    def forward(self, x, timesteps=None, context=None, y=None, **kwargs):
        # one-shot: the hint describes THIS call; it is consumed before anything below can raise, so a failed call cannot
        # leave it behind for a later, unrelated forward
        t_hint, self._t_hint = getattr(self, '_t_hint', None), None
        assert y is None, 'must specify y if and only if the model is class-conditional'
        no_ctx = not getattr(self, 'use_spatial_transformer', True)
        if no_ctx and context is not None:
            raise ValueError('this UNet has no cross-attention (AttentionBlocks): context must be None')
        if not x.is_cuda:
            raise RuntimeError('UNetModelHIP runs on an MI355X device tensor only (no CPU fallback)')
        if no_ctx:
            if timesteps is None:
                raise ValueError('timesteps are required')
            return self._forward_no_context(x, timesteps, t_hint)
        if context is None or timesteps is None:
            raise ValueError('timesteps and context are required')
        if self._needs_pack():
            self.pack()
        B, Cin, H, W = x.shape
        assert Cin == self.in_channels
        assert timesteps.shape == (B,)
        if t_hint is not None and os.environ.get('SDMI_CHECK_T_HINT') == '1':
            # debug: the hint is the caller's assertion about a device tensor; this check costs a device round trip
            if not bool((timesteps == t_hint).all()):
                raise RuntimeError(f'hint_timestep({t_hint}) does not describe the timesteps tensor {timesteps.tolist()}')
        assert context.dim() == 3 and context.shape[0] == B and context.shape[2] == self.context_dim
        if B > self.MAX_ROWS:
            # e.g. `txt2img.py --n_samples 5` = CFG batch 10 (scripts/txt2img.py:110-114): the reference has no
            # cross-sample op (GroupNorm and attention are per sample), so the batch is evaluated in chunks of <= 8 rows
            outs = [self._forward_rows(x[i:i + self.MAX_ROWS], timesteps[i:i + self.MAX_ROWS],
                                       context[i:i + self.MAX_ROWS], allow_reuse=False, t_hint=t_hint)
                    for i in range(0, B, self.MAX_ROWS)]
            return torch.cat(outs, dim=0)
        return self._forward_rows(x, timesteps, context, allow_reuse=True, t_hint=t_hint)

    def _forward_no_context(self, x, timesteps, t_hint):
        """UNetModel.forward(x, timesteps) of the AttentionBlock family: sdmi_unet_forward with ctx = NULL, Lctx = 0."""
        if self._needs_pack():
            self.pack()
        B, Cin, H, W = x.shape
        assert Cin == self.in_channels
        assert timesteps.shape == (B,)
        down = 2 ** (len(self.channel_mult) - 1)
        if H % down or W % down:
            raise ValueError(f'latent H and W must be multiples of {down} for this UNet (got {H} x {W}): the down ResBlocks '
                             'average-pool 2 x 2 and round down')
        outs = []
        for i in range(0, B, self.MAX_ROWS):
            xi = x[i:i + self.MAX_ROWS].detach().float().contiguous()
            ti = timesteps[i:i + self.MAX_ROWS]
            if ti.dtype in (torch.int64, torch.int32, torch.int16, torch.uint8):
                t_i64, t_f32 = ti.detach().to(torch.int64).contiguous(), None
            else:
                t_i64, t_f32 = None, ti.detach().float().contiguous()
            b = xi.shape[0]
            ws = self._workspace(b, H, W, 0, x.device)
            out = torch.empty((b, self.out_channels, H, W), dtype=torch.float32, device=x.device)
            if t_hint is not None and t_i64 is not None:
                _lib.check(self._handle.lib.sdmi_unet_hint_timestep(self._handle.h, int(t_hint)))
            _lib.check(self._handle.lib.sdmi_unet_forward(
                self._handle.h, xi.data_ptr(), _lib.ptr(t_i64), _lib.ptr(t_f32), None, out.data_ptr(),
                b, H, W, 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
            outs.append(out)
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _forward_rows(self, x, timesteps, context, allow_reuse, t_hint=None):
        B, Cin, H, W = x.shape
        x32 = x.detach().float().contiguous()
        if timesteps.dtype in (torch.int64, torch.int32, torch.int16, torch.uint8):
            t_i64, t_f32 = timesteps.detach().to(torch.int64).contiguous(), None
        else:
            t_i64, t_f32 = None, timesteps.detach().float().contiguous()
        L = context.shape[1]
        ws = self._workspace(B, H, W, L, x.device)
        # cross-attention K/V depend on the context only: skip their recomputation while the context is pinned (and
        # still has the pinned contents) or the caller keeps passing the very same, unmodified tensor object
        reuse = False
        if allow_reuse:
            if self._pinned == (B, L):
                reuse = self._pinned_matches(context)
            else:
                reuse = (self._ctx_ref is context) and (self._ctx_ver == context._version) and self._ctx_shape == (B, L)
        ctx32 = None
        if not reuse:
            ctx32 = context.detach().float().contiguous()
            self._reserve_context(B, L)
        out = torch.empty((B, self.out_channels, H, W), dtype=torch.float32, device=x.device)
        if t_hint is not None and t_i64 is not None:
            _lib.check(self._handle.lib.sdmi_unet_hint_timestep(self._handle.h, int(t_hint)))
        _lib.check(self._handle.lib.sdmi_unet_forward(
            self._handle.h, x32.data_ptr(), _lib.ptr(t_i64), _lib.ptr(t_f32), _lib.ptr(ctx32), out.data_ptr(),
            B, H, W, L, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        if not reuse:
            # the library has ONE K/V cache and it now holds THIS context: any pin is void -- whatever its shape (a call with
            # another (B, L), or a chunk of a larger batch, displaced it too) -- and the identity shortcut only applies to
            # un-chunked calls.  The next pinned-shape forward then passes its context again instead of ctx = NULL.
            self._pinned, self._pinned_ctx = None, None
            if allow_reuse:
                self._ctx_ref, self._ctx_ver, self._ctx_shape = context, context._version, (B, L)
            else:
                self._ctx_ref = None
        return out
