"""The two thin wrappers between the samplers and the UNet, restated so the hot path can be driven without
pytorch_lightning: `LatentDiffusion.apply_model` (ldm/models/diffusion/ddpm.py:891-900,986-992) and
`DiffusionWrapper.forward` (ddpm.py:1402-1421, conditioning_key 'crossattn', 'concat' for the latent-inpainting
model: the UNet reads cat([x, c_concat], 1) and no context, or None for the unconditional models: the UNet reads x and t
alone), plus the schedule buffers
`DDPM.register_schedule` registers (ddpm.py:117-169) that the samplers read.

With the real `ldm` package installed the reference's own LatentDiffusion does this job;
this module exists for bench.py / tests / multi-GPU sampling where only the UNet path is needed.

With an attribute `split_input_params` (the reference tests `hasattr`, ddpm.py:715,827,902) apply_model, decode_first_stage and
encode_first_stage run over sliding windows as the reference's do (ddpm.py:564-651, 715-752, 826-858, 902-984), restated for the
executor: the windows of all samples are rows of UNet / first-stage calls of up to MAX_ROWS rows, gathered by sdmi_k_patch_unfold (the
concat of the conditioning image included) and stitched by sdmi_k_patch_fold (csrc/patch.hip); nothing goes through torch Unfold / Fold.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib

MAX_ROWS = 8       # rows per tiled UNet / first-stage call (UNetModelHIP.MAX_ROWS, AutoencoderKLHIP.MAX_BATCH)
PATCH_COND_KEYS = ('image', 'LR_image', 'segmentation', 'bbox_img')      # ddpm.py:917-918: conditionings that are cut into windows too


def make_beta_schedule_linear(n_timestep=1000, linear_start=0.00085, linear_end=0.0120):
    """util.py:21-25 with the SD-v1 yaml values (v1-inference.yaml:5-6,9)."""
    return np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=np.float64) ** 2


# ---- sliding windows (LatentDiffusion.split_input_params) -----------------------------------------------------------------------
def patch_grid(h, w, ks, stride):
    """(Ly, Lx) of ddpm.py:609-610.  ValueError where the windows do not tile the input: a window larger than a side (torch's Unfold
    raises), or a side off the ks + n * stride grid (the reference leaves pixels uncovered: fold(weighting) is 0 there, its output NaN)."""
    (kh, kw), (sy, sx) = (int(v) for v in ks), (int(v) for v in stride)
    if kh < 1 or kw < 1 or sy < 1 or sx < 1:
        raise ValueError(f'split_input_params: ks {tuple(ks)} and stride {tuple(stride)} must be positive')
    if kh > h or kw > w:
        raise ValueError(f'split_input_params: window {kh} x {kw} is larger than the input {h} x {w}')
    if (h - kh) % sy or (w - kw) % sx:
        raise ValueError(f'split_input_params: input {h} x {w} is not window {kh} x {kw} plus a multiple of stride {sy} x {sx}: '
                         'the reference leaves the remainder uncovered (0 / 0)')
    return (h - kh) // sy + 1, (w - kw) // sx + 1


def window_origins(h, w, ks, stride):
    """(y0, x0) of window l = ly * Lx + lx, in l order (torch.nn.Unfold's block order)"""
    Ly, Lx = patch_grid(h, w, ks, stride)
    return [(ly * int(stride[0]), lx * int(stride[1])) for ly in range(Ly) for lx in range(Lx)]


def _delta_border(h, w):
    """ddpm.py:564-583, op for op (int64 meshgrid / int64 corner -> fp32; min over the four normalised border distances)"""
    y = torch.arange(0, h).view(h, 1, 1).repeat(1, w, 1)
    x = torch.arange(0, w).view(1, w, 1).repeat(h, 1, 1)
    arr = torch.cat([y, x], dim=-1) / torch.tensor([h - 1, w - 1]).view(1, 1, 2)
    dist_left_up = torch.min(arr, dim=-1, keepdim=True)[0]
    dist_right_down = torch.min(1 - arr, dim=-1, keepdim=True)[0]
    return torch.min(torch.cat([dist_left_up, dist_right_down], dim=-1), dim=-1)[0]


_weighting_cache = {}


def _weighting_key(kh, kw, Ly, Lx, params):
    """what the weighting depends on: the window, the grid and the clips (the tie-breaker's only when it is on)"""
    tie = bool(params.get('tie_braker', False))
    return (int(kh), int(kw), int(Ly), int(Lx), float(params['clip_min_weight']), float(params['clip_max_weight']),
            (float(params['clip_min_tie_weight']), float(params['clip_max_tie_weight'])) if tie else None)


def patch_weighting(kh, kw, Ly, Lx, params):
    """get_weighting(kh, kw, Ly, Lx) (ddpm.py:585-599) on the host, as [Ly * Lx, kh, kw] fp32 (the reference's [1, kh * kw, L], transposed):
    the border distance of a window element, clipped, times -- with `tie_braker` -- the clipped border distance of the window in the grid."""
    key = _weighting_key(kh, kw, Ly, Lx, params)
    tie = key[6] is not None
    if key not in _weighting_cache:
        kh, kw, Ly, Lx = key[:4]
        if kh < 2 or kw < 2:
            raise ValueError(f'split_input_params: a window side of 1 ({kh} x {kw}) divides by zero in delta_border')
        if tie and (Ly == 1 or Lx == 1):
            raise ValueError(f'split_input_params: tie_braker with a {Ly} x {Lx} window grid: delta_border(Ly, Lx) divides by zero and '
                             'the reference\'s weights are NaN')
        wgt = torch.clip(_delta_border(kh, kw), key[4], key[5]).view(1, kh * kw, 1).repeat(1, 1, Ly * Lx)
        if tie:
            wgt = wgt * torch.clip(_delta_border(Ly, Lx), key[6][0], key[6][1]).view(1, 1, Ly * Lx)
        _weighting_cache[key] = wgt.view(kh, kw, Ly * Lx).permute(2, 0, 1).contiguous().float()
    return _weighting_cache[key]


def patch_unfold(x, c, ks, stride, l0, nl, out=None):
    """rows (l, b), l in [l0, l0 + nl), of windows of x [B, Cx, H, W] with those of c [B, Cc, H, W] (or None) behind them on the channel
    axis: [nl * B, Cx + Cc, kh, kw] fp32 (sdmi_k_patch_unfold)"""
    patch_grid(x.shape[2], x.shape[3], ks, stride)
    x = x.detach().float().contiguous()
    B, Cx, H, W = x.shape
    Cc = 0
    if c is not None:
        c = c.detach().float().contiguous()
        if c.shape[0] != B or tuple(c.shape[2:]) != (H, W):
            raise ValueError(f'the conditioning {tuple(c.shape)} does not match the latent {tuple(x.shape)}')
        Cc = c.shape[1]
    if out is None:
        out = torch.empty((nl * B, Cx + Cc, int(ks[0]), int(ks[1])), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().sdmi_k_patch_unfold(x.data_ptr(), _lib.ptr(c), out.data_ptr(), B, Cx, Cc, H, W, int(ks[0]), int(ks[1]),
                                               int(stride[0]), int(stride[1]), int(l0), int(nl), _lib.stream_ptr()))
    return out


def patch_fold(o, w, B, hw, ks, stride, uf=1, df=1, norm_only=False, out=None):
    """fold(o * weighting) / fold(weighting) of ddpm.py:979-984 (sdmi_k_patch_fold): o [L * B, C, kh', kw'] rows (l, b), w [L, kh', kw'] ->
    [B, C, H uf / df, W uf / df]; norm_only: fold(weighting) alone, [H uf / df, W uf / df].  hw / ks / stride are the unscaled geometry."""
    patch_grid(hw[0], hw[1], ks, stride)
    H, W = int(hw[0]), int(hw[1])
    uf, df = int(uf), int(df)
    if uf < 1 or df < 1 or (uf > 1 and df > 1):
        raise ValueError(f'patch_fold: uf {uf} and df {df}: positive, and at most one of them above 1')
    if (uf != 1 or df != 1) and int(ks[0]) != int(ks[1]):
        raise ValueError(f'patch_fold: a non-square window {tuple(ks)} with uf {uf} / df {df} (get_fold_unfold scales ks[0] on both axes)')
    if any(int(v) % df for v in (H, W, ks[0], ks[1], stride[0], stride[1])):
        raise ValueError(f'patch_fold: df {df} must divide the input {H} x {W}, the window {tuple(ks)} and the stride {tuple(stride)}')
    w = w.detach().float().contiguous()
    if not norm_only:
        o = o.detach().float().contiguous()
    if out is None:
        shape = (H * uf // df, W * uf // df)
        out = torch.empty(shape if norm_only else (B, o.shape[1]) + shape, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().sdmi_k_patch_fold(None if norm_only else o.data_ptr(), w.data_ptr(), out.data_ptr(), B, 1 if norm_only else o.shape[1],
                                             H, W, int(ks[0]), int(ks[1]), int(stride[0]), int(stride[1]), int(uf), int(df),
                                             1 if norm_only else 0, _lib.stream_ptr()))
    return out


class DiffusionWrapperHIP(nn.Module):
    def __init__(self, diffusion_model, conditioning_key='crossattn'):
        super().__init__()
        if conditioning_key not in (None, 'crossattn', 'concat'):
            raise NotImplementedError(f"conditioning_key {conditioning_key!r}: None, 'crossattn' and 'concat' only")
        self.diffusion_model = diffusion_model
        self.conditioning_key = conditioning_key

    def forward(self, x, t, c_concat=None, c_crossattn=None):
        if self.conditioning_key is None:              # ddpm.py:1408-1409
            return self.diffusion_model(x, t)
        if self.conditioning_key == 'concat':          # ddpm.py:1411-1413
            xc = torch.cat([x] + list(c_concat), dim=1)
            return self.diffusion_model(xc, t)
        cc = c_crossattn[0] if len(c_crossattn) == 1 else torch.cat(c_crossattn, 1)
        return self.diffusion_model(x, t, context=cc)


class LatentDiffusionHIP(nn.Module):
    """What the samplers touch on `model`: num_timesteps, betas, alphas_cumprod(_prev), device, apply_model."""

    def __init__(self, unet, timesteps=1000, linear_start=0.00085, linear_end=0.0120, conditioning_key='crossattn',
                 first_stage_model=None, scale_factor=1.0, cond_stage_key=None, clip_denoised=True, log_every_t=100, channels=None,
                 image_size=None):
        """The latent-inpainting model: linear_start=0.0015, linear_end=0.0205, conditioning_key='concat'
        (models/ldm/inpainting_big/config.yaml:5-14).  The unconditional LSUN-Churches model: linear_start=0.0015,
        linear_end=0.0155, conditioning_key=None (models/ldm/lsun_churches256/config.yaml:5-6, cond_stage_config
        '__is_unconditional__': ddpm.py:455-456 leaves the key at None); apply_model(x, t, None).
        `first_stage_model` (an AutoencoderKLHIP / VQModelInterfaceHIP), `scale_factor` and `cond_stage_key` serve decode_first_stage /
        encode_first_stage and the tiled apply_model; set the attribute `split_input_params` (ddpm.py's keys: ks, stride, vqf,
        patch_distributed_vq, tie_braker, clip_min_weight, clip_max_weight, clip_min_tie_weight, clip_max_tie_weight) to switch tiling on.
        `clip_denoised` / `log_every_t` are the DDPM constructor's (ddpm.py:53-54; its defaults, which the yaml files inherit -- the
        LSUN-Churches one sets log_every_t: 200) and serve the ancestral sampler; `channels` / `image_size` only give sample() /
        sample_log() their default shape (ddpm.py:1221, :1239)."""
        super().__init__()
        self.model = DiffusionWrapperHIP(unet, conditioning_key)
        self.first_stage_model = first_stage_model
        self.scale_factor = float(scale_factor)
        self.cond_stage_key = cond_stage_key
        self.clip_denoised = bool(clip_denoised)
        self.log_every_t = int(log_every_t)
        self.channels, self.image_size = channels, image_size
        self.shorten_cond_schedule = False
        from .samplers import ddpm_tables
        betas = make_beta_schedule_linear(timesteps, linear_start, linear_end)
        self.num_timesteps = int(timesteps)
        self.parameterization = 'eps'
        persistent = ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod')
        for name, tab in ddpm_tables(betas).items():      # every buffer of DDPM.register_schedule but lvlb_weights (a training loss weight)
            # (the posterior tables stay out of state_dict(): its keys are what they were before the ancestral sampler came)
            self.register_buffer(name, torch.from_numpy(tab), persistent=name in persistent)

    @property
    def device(self):
        return self.betas.device

    def apply_model(self, x_noisy, t, cond, return_ids=False):
        if not isinstance(cond, dict):          # ddpm.py:986-992
            key = 'c_concat' if self.model.conditioning_key == 'concat' else 'c_crossattn'
            cond = {key: [cond] if not isinstance(cond, list) else cond}
        if hasattr(self, 'split_input_params'):
            return self._apply_model_tiled(x_noisy, t, cond, return_ids)
        return self.model(x_noisy, t, **cond)

    # ---- sliding windows: ddpm.py:902-984 with all windows of all samples as rows of chunked calls --------------------------------
    def _window_chunks(self, L, B):
        """[(l0, nl)]: whole windows per call, rows nl * B <= MAX_ROWS (a batch above MAX_ROWS goes one window at a time and the UNet
        splits it).  Nine rows run as 8 + 1: 9.8 ms per tiled apply_model against 11.5 ms as 5 + 4 (profiles/bench_superres.txt)."""
        nl = max(1, MAX_ROWS // B)
        return [(l0, min(nl, L - l0)) for l0 in range(0, L, nl)]

    def _weights_on(self, kh, kw, Ly, Lx, device):
        if not hasattr(self, '_patch_w'):
            self._patch_w = {}
        device = torch.empty(0, device=device).device        # ('cuda' and 'cuda:0' are one device: the index resolved)
        key = (_weighting_key(kh, kw, Ly, Lx, self.split_input_params), device)
        if key not in self._patch_w:
            self._patch_w[key] = patch_weighting(kh, kw, Ly, Lx, self.split_input_params).to(device)
        return self._patch_w[key]

    def _apply_model_tiled(self, x_noisy, t, cond, return_ids):
        p = self.split_input_params
        assert len(cond) == 1            # ddpm.py:903
        assert not return_ids            # ddpm.py:904
        ks, stride = tuple(p['ks']), tuple(p['stride'])
        B, _, H, W = x_noisy.shape
        Ly, Lx = patch_grid(H, W, ks, stride)
        c_key, c_val = next(iter(cond.items()))
        c_img = None
        if self.cond_stage_key in PATCH_COND_KEYS and self.model.conditioning_key:
            assert len(c_val) == 1       # ddpm.py:921
            c_img = c_val[0]
        elif self.cond_stage_key == 'coordinates_bbox':
            raise NotImplementedError("split_input_params with cond_stage_key 'coordinates_bbox' (per-window bounding-box tokens)")
        w = self._weights_on(ks[0], ks[1], Ly, Lx, x_noisy.device)
        unet = self.model.diffusion_model
        hint = getattr(unet, '_t_hint', None)
        fused = c_img is not None and self.model.conditioning_key == 'concat'
        o = None
        for l0, nl in self._window_chunks(Ly * Lx, B):
            t_rows = t.repeat(nl)
            if hint is not None:
                unet.hint_timestep(hint)                 # (one-shot: every chunk is a forward of its own at the same timestep)
            if fused:                                    # the cat([x] + c_concat, 1) of DiffusionWrapper.forward inside the gather
                eps = unet(patch_unfold(x_noisy, c_img, ks, stride, l0, nl), t_rows)
            elif c_img is not None:
                eps = self.model(patch_unfold(x_noisy, None, ks, stride, l0, nl), t_rows,
                                 **{c_key: [patch_unfold(c_img, None, ks, stride, l0, nl)]})
            else:                                        # ddpm.py:972: every window gets the same cond
                eps = self.model(patch_unfold(x_noisy, None, ks, stride, l0, nl), t_rows,
                                 **{c_key: [c if c is None else c.repeat((nl,) + (1,) * (c.dim() - 1)) for c in c_val]})
            assert not isinstance(eps, tuple)            # ddpm.py:976
            if o is None:
                o = torch.empty((Ly * Lx * B,) + tuple(eps.shape[1:]), dtype=torch.float32, device=eps.device)
            o[l0 * B:(l0 + nl) * B].copy_(eps)
        return patch_fold(o, w, B, (H, W), ks, stride)

    def _reduced(self, h, w):
        """ddpm.py:721-727"""
        p = self.split_input_params
        ks, stride = tuple(p['ks']), tuple(p['stride'])
        if ks[0] > h or ks[1] > w:
            ks = (min(ks[0], h), min(ks[1], w))
        if stride[0] > h or stride[1] > w:
            stride = (min(stride[0], h), min(stride[1], w))
        return ks, stride

    def _first_stage_tiled(self, x, run, uf, df):
        B, _, H, W = x.shape
        ks, stride = self._reduced(H, W)
        Ly, Lx = patch_grid(H, W, ks, stride)
        if (uf != 1 or df != 1) and ks[0] != ks[1]:
            raise ValueError(f'split_input_params: a non-square window {ks} around the first stage (get_fold_unfold scales ks[0] on both axes)')
        if ks[0] % df or ks[1] % df or stride[0] % df or stride[1] % df or H % df or W % df:
            raise ValueError(f'split_input_params: vqf {df} must divide the image {H} x {W}, the window {ks} and the stride {stride}')
        w = self._weights_on(ks[0] * uf // df, ks[1] * uf // df, Ly, Lx, x.device)
        o = None
        for l0, nl in self._window_chunks(Ly * Lx, B):
            y = run(patch_unfold(x, None, ks, stride, l0, nl))
            if o is None:
                o = torch.empty((Ly * Lx * B,) + tuple(y.shape[1:]), dtype=torch.float32, device=y.device)
            o[l0 * B:(l0 + nl) * B].copy_(y)
        return patch_fold(o, w, B, (H, W), ks, stride, uf=uf, df=df)

    @torch.no_grad()
    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False):
        """ddpm.py:705-763"""
        from .vae import VQModelInterfaceHIP
        if predict_cids:
            raise NotImplementedError('predict_cids')
        fs = self.first_stage_model
        vq = isinstance(fs, VQModelInterfaceHIP)
        run = (lambda v: fs.decode(v, force_not_quantize=force_not_quantize)) if vq else fs.decode
        z = 1. / self.scale_factor * z
        if hasattr(self, 'split_input_params') and self.split_input_params['patch_distributed_vq']:
            return self._first_stage_tiled(z, run, int(self.split_input_params['vqf']), 1)
        return run(z)

    @torch.no_grad()
    def encode_first_stage(self, x):
        """ddpm.py:825-863"""
        fs = self.first_stage_model
        if hasattr(self, 'split_input_params') and self.split_input_params['patch_distributed_vq']:
            self.split_input_params['original_image_size'] = x.shape[-2:]
            return self._first_stage_tiled(x, fs.encode, 1, int(self.split_input_params['vqf']))
        return fs.encode(x)

    def q_sample(self, x_start, t, noise=None):
        """ddpm.py:274-277"""
        noise = torch.randn_like(x_start) if noise is None else noise
        sh = (t.shape[0],) + (1,) * (x_start.dim() - 1)
        return self.sqrt_alphas_cumprod.gather(-1, t).reshape(sh) * x_start + \
            self.sqrt_one_minus_alphas_cumprod.gather(-1, t).reshape(sh) * noise

    # ---- ancestral sampling (ddpm.py:1109-1247): DDPMSamplerHIP does the work ------------------------------------------------------
    @torch.no_grad()
    def p_sample_loop(self, cond, shape, **kwargs):
        """ddpm.py:1165-1214"""
        from .samplers import DDPMSamplerHIP
        return DDPMSamplerHIP(self).p_sample_loop(cond, shape, **kwargs)

    @torch.no_grad()
    def progressive_denoising(self, cond, shape, **kwargs):
        """ddpm.py:1109-1163"""
        from .samplers import DDPMSamplerHIP
        return DDPMSamplerHIP(self).progressive_denoising(cond, shape, **kwargs)

    def _default_shape(self):
        if self.channels is None or self.image_size is None:
            raise ValueError('no shape given and the model was built without channels / image_size')
        return (int(self.channels), int(self.image_size), int(self.image_size))

    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None, quantize_denoised=False,
               mask=None, x0=None, shape=None, **kwargs):
        """ddpm.py:1216-1232 (as there, further keywords are accepted and dropped)"""
        if shape is None:
            shape = (batch_size,) + self._default_shape()
        if cond is not None and not isinstance(cond, dict):
            cond = [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]
        return self.p_sample_loop(cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose, timesteps=timesteps,
                                  quantize_denoised=quantize_denoised, mask=mask, x0=x0)

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, **kwargs):
        """ddpm.py:1234-1247.  One keyword beyond the reference's: `shape=(C, H, W)`, for a model built without channels / image_size."""
        if ddim:
            from .samplers import DDIMSamplerHIP
            shape = kwargs.pop('shape', None) or self._default_shape()
            return DDIMSamplerHIP(self).sample(ddim_steps, batch_size, tuple(shape)[-3:], cond, verbose=False, **kwargs)
        shape = kwargs.pop('shape', None)
        if shape is not None and len(shape) == 3:
            shape = (batch_size,) + tuple(shape)
        return self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, shape=shape, **kwargs)
