"""`AutoencoderKLHIP` -- drop-in for `ldm.models.autoencoder.AutoencoderKL` (inference only) on MI355X.

Plugged in through the reference's plugin mechanism (`instantiate_from_config`, ldm/util.py:78-93;
`LatentDiffusion.instantiate_first_stage`, ldm/models/diffusion/ddpm.py:502-507): a copy of
configs/stable-diffusion/v1-inference.yaml with

    first_stage_config:
      target: stable_diffusion_amd.vae.AutoencoderKLHIP

Same constructor keywords (autoencoder.py:286-295), same parameter names (`encoder.*`, `decoder.*`, `quant_conv.*`,
`post_quant_conv.*`, so the `first_stage_model.*` part of an SD checkpoint loads), same calls:
`decode(z)` (autoencoder.py:330-333, reached from `decode_first_stage`, ddpm.py:705-763) and `encode(x)`
(autoencoder.py:324-328, reached from `encode_first_stage`, ddpm.py:825-863) which returns the reference's
`DiagonalGaussianDistribution` when `ldm` is importable (`get_first_stage_encoding` type-checks it, ddpm.py:542-549).
The arithmetic runs in libsdmi.so; there is no CPU / PyTorch fallback.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .unet import PRECISIONS, _Node


class DiagonalGaussianDistributionHIP:
    """ldm/modules/distributions/distributions.py:24-63 (the members the sampling scripts use)."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if self.deterministic:
            self.var = self.std = torch.zeros_like(self.mean)

    def sample(self):
        return self.mean + self.std * torch.randn(self.mean.shape).to(device=self.parameters.device)

    def mode(self):
        return self.mean


def _posterior(moments):
    try:        # inside the reference's LatentDiffusion the posterior must be the reference's own class
        from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
        return DiagonalGaussianDistribution(moments)
    except ImportError:
        return DiagonalGaussianDistributionHIP(moments)


def _check_precision(hip_precision):
    if hip_precision not in PRECISIONS:
        raise ValueError(f"hip_precision must be one of {sorted(PRECISIONS)}, got {hip_precision!r}")
    return hip_precision


def attn_level_mask(ddconfig):
    """`attn_resolutions` resolved to levels the way Encoder.__init__ / Decoder.__init__ do (model.py:389-411, 481-524): level l runs at
    curr_res = resolution // 2**l and gets an AttnBlock after every ResBlock when that value is in attn_resolutions.  Returns the bit mask
    (bit l = level l) sdmi_vae_create_attn takes.  An entry that names no level is refused, by name: the reference would silently build a
    model without that attention, and a config that means something else than it says is not run."""
    dd = dict(ddconfig)
    wanted = [int(r) for r in dd.get('attn_resolutions', [])]
    if not wanted:
        return 0
    n = len(list(dd.get('ch_mult', (1, 2, 4, 8))))
    res = int(dd['resolution'])
    enc = [res // 2 ** l for l in range(n)]                              # Encoder: curr_res //= 2 after every level but the last
    dec = [(res // 2 ** (n - 1)) * 2 ** (n - 1 - l) for l in range(n)]   # Decoder: from the lowest level up, curr_res *= 2
    missing = [r for r in wanted if r not in enc]
    if missing or enc != dec:
        raise NotImplementedError(
            f'attn_resolutions entry {missing[0] if missing else wanted[0]} names no level of this first stage: the levels run at '
            f'resolutions {enc}' + ('' if enc == dec else f' in the encoder and {dec} in the decoder') +
            ' (resolution // 2**level); AutoencoderKLHIP does not drop an attention the config asks for')
    return sum(1 << l for l in range(n) if enc[l] in wanted)


def make_vae_cfg(ddconfig, embed_dim, vq=False):
    """vq: the VQModelInterface family (double_z False, attn_type 'vanilla' or 'none'; attn_resolutions with 'vanilla' only: VQ-f8 [32],
    VQ-f16 [16]); else the AutoencoderKL one (SD-v1's KL-f8, and KL-f16 / KL-f32 with attention at resolution levels: attn_level_mask)."""
    dd = dict(ddconfig)
    unsupported = []
    if vq and list(dd.get('attn_resolutions', [])) and dd.get('attn_type', 'vanilla') == 'none':
        # (make_attn(.., 'none') is an Identity, model.py:205-216: the reference would silently build no attention at the levels named)
        unsupported.append("attn_resolutions=[] with attn_type='none' (level attention needs attn_type='vanilla')")
    else:
        attn_level_mask(dd)                  # (refuses an entry that names no level)
    if dd.get('dropout', 0.0) != 0: unsupported.append('dropout=0')
    if vq:
        if dd.get('double_z', True): unsupported.append('double_z=False')
        if dd.get('use_linear_attn', False) or dd.get('attn_type', 'vanilla') not in ('vanilla', 'none'):
            unsupported.append("attn_type='vanilla' or 'none'")
    else:
        if not dd.get('double_z', True): unsupported.append('double_z=True')
        if dd.get('use_linear_attn', False) or dd.get('attn_type', 'vanilla') != 'vanilla': unsupported.append("attn_type='vanilla'")
    if not dd.get('resamp_with_conv', True): unsupported.append('resamp_with_conv=True')
    if dd.get('tanh_out', False) or dd.get('give_pre_end', False): unsupported.append('tanh_out=False, give_pre_end=False')
    if unsupported:
        raise NotImplementedError(('VQModelInterfaceHIP supports the latent-inpainting first stage family only; needs: ' if vq else
                                   'AutoencoderKLHIP supports the SD-v1 first stage family only; needs: ') + '; '.join(unsupported))
    cfg = _lib.VaeCfg()
    ch_mult = list(dd.get('ch_mult', (1, 2, 4, 8)))
    if len(ch_mult) > 8:
        raise ValueError('at most 8 levels')
    cfg.ch, cfg.out_ch, cfg.n_levels = int(dd['ch']), int(dd['out_ch']), len(ch_mult)
    for i, m in enumerate(ch_mult):
        cfg.ch_mult[i] = int(m)
    cfg.num_res_blocks, cfg.in_channels = int(dd['num_res_blocks']), int(dd['in_channels'])
    cfg.z_channels, cfg.embed_dim = int(dd['z_channels']), int(embed_dim)
    return cfg


class _VaeHandle:
    """Owns one sdmi_vae*."""

    def __init__(self, cfg, parts, ext=None, precision='mixed', attn_mask=0):
        self.lib = _lib.load()
        self.h = None
        h = C.c_void_p()
        e = None if ext is None else C.byref(ext)
        if attn_mask:       # (a handle without level attention is created by the entry it always was)
            _lib.check(self.lib.sdmi_vae_create_attn(C.byref(cfg), e, parts, PRECISIONS[precision], attn_mask, C.byref(h)))
        else:
            _lib.check(self.lib.sdmi_vae_create_precision(C.byref(cfg), e, parts, PRECISIONS[precision], C.byref(h)))
        self.h = h

    def weight_specs(self):
        n = self.lib.sdmi_vae_num_weights(self.h)
        out = []
        buf = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(n):
            _lib.check(self.lib.sdmi_vae_weight_info(self.h, i, buf, 256, shape, C.byref(nd)))
            out.append((buf.value.decode(), tuple(shape[j] for j in range(nd.value))))
        return out

    def __del__(self):
        try:
            if self.h:
                self.lib.sdmi_vae_destroy(self.h)
                self.h = None
        except Exception:
            pass


class AutoencoderKLHIP(nn.Module):
    MAX_BATCH = 8     # images per library call (larger batches are looped)

    def __init__(self, ddconfig, lossconfig=None, embed_dim=4, ckpt_path=None, ignore_keys=[], image_key='image',
                 colorize_nlabels=None, monitor=None, parts=3, hip_precision='mixed'):
        """`hip_precision` (not a keyword of the reference AutoencoderKL): 'mixed' (default) = fp16 MFMA operands; 'full' = every MFMA
        operand of the ResBlocks, the resampling convs and the attention blocks is a split-fp16 pair (three MFMA passes), as in
        UNetModelHIP's full mode.  Fixed for the module's lifetime; the state_dict keys are the same in both modes.
        `ddconfig['attn_resolutions']` (KL-f16: [16], KL-f32: [16, 8]) puts an AttnBlock behind every ResBlock of the levels it names (attn_level_mask)."""
        super().__init__()
        self.hip_precision = _check_precision(hip_precision)
        self.image_key = image_key
        self.embed_dim = int(embed_dim)
        self.ddconfig = dict(ddconfig)
        self._cfg = make_vae_cfg(ddconfig, embed_dim)
        self._parts = parts
        self.attn_level_mask = attn_level_mask(ddconfig)      # attn_resolutions as levels (0: mid-block attention only)
        self._handle = _VaeHandle(self._cfg, parts, None, hip_precision, self.attn_level_mask)
        self._specs = self._handle.weight_specs()
        for key, shape in self._specs:
            *path, leaf = key.split('.')
            node = self
            for name in path:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            node.register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))
        if monitor is not None:
            self.monitor = monitor
        self._packed_sig = None
        self._sentinels = None
        self._ws = {}
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    @property
    def factor(self):
        return 2 ** (self._cfg.n_levels - 1)

    def init_from_ckpt(self, path, ignore_keys=list()):
        """autoencoder.py:312-321"""
        sd = torch.load(path, map_location='cpu')['state_dict']
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                del sd[k]
        self.load_state_dict(sd, strict=False)

    # ---- weights -> library (same dirty tracking as UNetModelHIP) --------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._packed_sig = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed_sig = None
        return super().load_state_dict(*a, **k)

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
                raise RuntimeError('AutoencoderKLHIP parameters must live on the GPU (call model.cuda() first); '
                                   'there is no CPU implementation of this path')
            p = p.float().contiguous()
            shp = (C.c_int64 * len(shape))(*shape)
            _lib.check(lib.sdmi_vae_set_weight(self._handle.h, key.encode(), p.data_ptr(), shp, len(shape), stream))
        torch.cuda.current_stream().synchronize()
        _lib.check(lib.sdmi_vae_finalize(self._handle.h))
        self._sentinels = None
        self._packed_sig = self._signature()

    def _ready(self, x):
        if not x.is_cuda:
            raise RuntimeError('AutoencoderKLHIP runs on an MI355X device tensor only (no CPU fallback)')
        if self._packed_sig is None or self._packed_sig != self._signature():
            self.pack()

    def _workspace(self, kind, B, H, W, device):
        key = (kind, B, H, W, str(device))
        if key not in self._ws:
            fn = self._handle.lib.sdmi_vae_decode_workspace_bytes if kind == 'dec' else \
                self._handle.lib.sdmi_vae_encode_workspace_bytes
            need = fn(self._handle.h, B, H, W)
            if need <= 0:
                _lib.check(-1)
            for k in [k for k in self._ws if k[0] == kind]:     # one live workspace per direction (img2img alternates
                del self._ws[k]                                  # encode and decode for every image)
            self._ws[key] = torch.empty(int(need), dtype=torch.uint8, device=device)
        return self._ws[key]

    # ---- AutoencoderKL.decode (autoencoder.py:330-333) ---------------------------------------------------------------
    @torch.no_grad()
    def decode(self, z, z_scale=1.0):
        """z [B, embed_dim, h, w] -> image [B, out_ch, h*f, w*f] fp32.  `z_scale` multiplies z first (the 1/scale_factor
        of decode_first_stage, ddpm.py:713, folded into the first kernel)."""
        self._ready(z)
        B, Cz, H, W = z.shape
        assert Cz == self.embed_dim
        z32 = z.detach().float().contiguous()
        f = self.factor
        out = torch.empty((B, self._cfg.out_ch, H * f, W * f), dtype=torch.float32, device=z.device)
        for b0 in range(0, B, self.MAX_BATCH):
            nb = min(self.MAX_BATCH, B - b0)
            ws = self._workspace('dec', nb, H, W, z.device)
            _lib.check(self._handle.lib.sdmi_vae_decode(self._handle.h, z32[b0:b0 + nb].data_ptr(), float(z_scale),
                                                        out[b0:b0 + nb].data_ptr(), nb, H, W, ws.data_ptr(), ws.numel(),
                                                        _lib.stream_ptr()))
        return out

    # ---- AutoencoderKL.encode (autoencoder.py:324-328) ---------------------------------------------------------------
    @torch.no_grad()
    def encode_moments(self, x):
        self._ready(x)
        B, Cin, H, W = x.shape
        assert Cin == self._cfg.in_channels
        f = self.factor
        if H % f or W % f:
            raise ValueError(f'image sides must be multiples of {f}')
        x32 = x.detach().float().contiguous()
        out = torch.empty((B, 2 * self.embed_dim, H // f, W // f), dtype=torch.float32, device=x.device)
        for b0 in range(0, B, self.MAX_BATCH):
            nb = min(self.MAX_BATCH, B - b0)
            ws = self._workspace('enc', nb, H, W, x.device)
            _lib.check(self._handle.lib.sdmi_vae_encode(self._handle.h, x32[b0:b0 + nb].data_ptr(),
                                                        out[b0:b0 + nb].data_ptr(), nb, H, W, ws.data_ptr(), ws.numel(),
                                                        _lib.stream_ptr()))
        return out

    def encode(self, x):
        return _posterior(self.encode_moments(x))

    def forward(self, input, sample_posterior=True):
        """autoencoder.py:335-342"""
        posterior = self.encode(input)
        z = posterior.sample() if sample_posterior else posterior.mode()
        return self.decode(z), posterior

    # ---- LatentDiffusion.decode_first_stage / encode_first_stage for callers without the reference's LatentDiffusion ---
    def decode_first_stage(self, z, scale_factor=0.18215):
        return self.decode(z, z_scale=1.0 / scale_factor)

    def encode_first_stage(self, x, scale_factor=0.18215, sample=True):
        p = self.encode(x)
        return scale_factor * (p.sample() if sample else p.mode())


class _QuantizerHIP(nn.Module):
    """`quantize` of VQModelInterface (taming's VectorQuantizer2): holds `embedding.weight`; calling it returns the reference's
    (z_q, emb_loss, (perplexity, min_encodings, indices)) with the loss terms None (inference)."""

    def __init__(self, run):
        super().__init__()
        self._run = run          # (a plain function, not a module: no parameter cycle)

    def forward(self, h):
        zq, idx = self._run(h, True)
        return zq, None, (None, None, idx.reshape(-1))


class VQModelInterfaceHIP(AutoencoderKLHIP):
    """`VQModelInterfaceHIP` -- drop-in for `ldm.models.autoencoder.VQModelInterface` (inference only), the first stage and
    the `__is_first_stage__` cond stage of the latent-inpainting model (models/ldm/inpainting_big/config.yaml:42-64):

        first_stage_config:
          target: stable_diffusion_amd.vae.VQModelInterfaceHIP

    encode(x) = quant_conv(encoder(x)) with no quantization (autoencoder.py:269-272); decode(h, force_not_quantize=False) =
    decoder(post_quant_conv(quantize(h))) (:274-283), the quantizer being taming's VectorQuantizer2 in its legacy form: the
    nearest codebook row by sum(z^2) + sum(e^2) - 2 z.e, first index on ties, z_q = z + (e[idx] - z) in fp32 (HIP kernel).
    Parameter names: encoder.*, decoder.*, quant_conv.*, post_quant_conv.*, quantize.embedding.weight.
    `ddconfig['attn_resolutions']` (models/first_stage_models/vq-f8: [32], vq-f16: [16]; attn_type 'vanilla') puts an AttnBlock behind
    every ResBlock of the levels it names, as for AutoencoderKLHIP (attn_level_mask)."""

    def __init__(self, embed_dim, ddconfig=None, n_embed=None, lossconfig=None, ckpt_path=None, ignore_keys=[],
                 image_key='image', colorize_nlabels=None, monitor=None, batch_resize_range=None, scheduler_config=None,
                 lr_g_factor=1.0, remap=None, sane_index_shape=False, use_ema=False, hip_precision='mixed'):
        if ddconfig is None or n_embed is None:
            raise TypeError('VQModelInterfaceHIP needs ddconfig and n_embed')
        unsupported = []
        if remap is not None: unsupported.append('remap=None')
        if use_ema: unsupported.append('use_ema=False')
        if unsupported:
            raise NotImplementedError('VQModelInterfaceHIP supports the latent-inpainting first stage family only; needs: ' +
                                      '; '.join(unsupported))
        self.n_embed = int(n_embed)
        nn.Module.__init__(self)
        self.hip_precision = _check_precision(hip_precision)      # (as AutoencoderKLHIP's)
        self.image_key = image_key
        self.embed_dim = int(embed_dim)
        self.ddconfig = dict(ddconfig)
        self._cfg = make_vae_cfg(ddconfig, embed_dim, vq=True)
        ext = _lib.VaeExt()
        ext.double_z, ext.mid_attn, ext.n_embed = 0, int(self.ddconfig.get('attn_type', 'vanilla') != 'none'), self.n_embed
        self._parts = 3
        self.attn_level_mask = attn_level_mask(ddconfig)      # attn_resolutions as levels (0: mid-block attention only)
        self._handle = _VaeHandle(self._cfg, 3, ext, hip_precision, self.attn_level_mask)
        self._specs = self._handle.weight_specs()
        self.add_module('quantize', _QuantizerHIP(self._quantize))
        for key, shape in self._specs:
            *path, leaf = key.split('.')
            node = self
            for name in path:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            node.register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))
        if monitor is not None:
            self.monitor = monitor
        self._packed_sig = None
        self._sentinels = None
        self._ws = {}
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    @torch.no_grad()
    def encode(self, x):
        """autoencoder.py:269-272: h = quant_conv(encoder(x)) [B, embed_dim, H/f, W/f] (the library's encode writes h, not moments)."""
        return self.encode_moments(x)

    @torch.no_grad()
    def encode_moments(self, x):
        self._ready(x)
        B, Cin, H, W = x.shape
        assert Cin == self._cfg.in_channels
        f = self.factor
        if H % f or W % f:
            raise ValueError(f'image sides must be multiples of {f}')
        x32 = x.detach().float().contiguous()
        out = torch.empty((B, self.embed_dim, H // f, W // f), dtype=torch.float32, device=x.device)
        for b0 in range(0, B, self.MAX_BATCH):
            nb = min(self.MAX_BATCH, B - b0)
            ws = self._workspace('enc', nb, H, W, x.device)
            _lib.check(self._handle.lib.sdmi_vae_encode(self._handle.h, x32[b0:b0 + nb].data_ptr(),
                                                        out[b0:b0 + nb].data_ptr(), nb, H, W, ws.data_ptr(), ws.numel(),
                                                        _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def decode(self, h, force_not_quantize=False, z_scale=1.0):
        """autoencoder.py:274-283.  `z_scale` multiplies h first (the 1/scale_factor of decode_first_stage, ddpm.py:713)."""
        self._ready(h)
        B, Cz, H, W = h.shape
        assert Cz == self.embed_dim
        z32 = h.detach().float().contiguous()
        f = self.factor
        out = torch.empty((B, self._cfg.out_ch, H * f, W * f), dtype=torch.float32, device=h.device)
        for b0 in range(0, B, self.MAX_BATCH):
            nb = min(self.MAX_BATCH, B - b0)
            ws = self._workspace('dec', nb, H, W, h.device)
            _lib.check(self._handle.lib.sdmi_vae_decode_vq(self._handle.h, z32[b0:b0 + nb].data_ptr(), float(z_scale),
                                                           0 if force_not_quantize else 1, out[b0:b0 + nb].data_ptr(), nb, H,
                                                           W, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def _quantize(self, h, return_indices=False):
        """The quantizer alone (self.quantize(h) calls it): z_q [B, embed_dim, H, W] (and the int64 indices [B, H, W])."""
        self._ready(h)
        B, Cz, H, W = h.shape
        assert Cz == self.embed_dim
        z32 = h.detach().float().contiguous()
        zq = torch.empty_like(z32)
        idx = torch.empty((B, H, W), dtype=torch.int32, device=h.device)
        norms = torch.empty(self.n_embed, dtype=torch.float32, device=h.device)
        cb = dict(self.named_parameters())['quantize.embedding.weight'].detach().float().contiguous()
        _lib.check(self._handle.lib.sdmi_k_vq_quantize(z32.data_ptr(), 1.0, cb.data_ptr(), norms.data_ptr(), self.n_embed,
                                                       self.embed_dim, zq.data_ptr(), idx.data_ptr(), B, H * W,
                                                       _lib.stream_ptr()))
        return (zq, idx.long()) if return_indices else zq

    def forward(self, input, return_pred_indices=False):
        """autoencoder.py:94-100 (eval): decode(encode(x)) through the quantizer."""
        return self.decode(self.encode(input))

    def decode_first_stage(self, z, scale_factor=1.0, force_not_quantize=False):
        return self.decode(z, force_not_quantize=force_not_quantize, z_scale=1.0 / scale_factor)

    def encode_first_stage(self, x, scale_factor=1.0):
        return scale_factor * self.encode(x)
