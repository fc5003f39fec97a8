"""The two thin wrappers between the samplers and the UNet, restated so the hot path can be driven without
pytorch_lightning: `LatentDiffusion.apply_model` (ldm/models/diffusion/ddpm.py:891-900,986-992) and
`DiffusionWrapper.forward` (ddpm.py:1402-1421, conditioning_key 'crossattn', 'concat' for the latent-inpainting
model: the UNet reads cat([x, c_concat], 1) and no context, or None for the unconditional models: the UNet reads x and t
alone), plus the schedule buffers
`DDPM.register_schedule` registers (ddpm.py:117-169) that the samplers read.

With the real `ldm` package installed the reference's own LatentDiffusion does this job;
this module exists for bench.py / tests / multi-GPU sampling where only the UNet path is needed.
"""
import numpy as np
import torch
import torch.nn as nn


def make_beta_schedule_linear(n_timestep=1000, linear_start=0.00085, linear_end=0.0120):
    """util.py:21-25 with the SD-v1 yaml values (v1-inference.yaml:5-6,9)."""
    return np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=np.float64) ** 2


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

    def __init__(self, unet, timesteps=1000, linear_start=0.00085, linear_end=0.0120, conditioning_key='crossattn'):
        """The latent-inpainting model: linear_start=0.0015, linear_end=0.0205, conditioning_key='concat'
        (models/ldm/inpainting_big/config.yaml:5-14).  The unconditional LSUN-Churches model: linear_start=0.0015,
        linear_end=0.0155, conditioning_key=None (models/ldm/lsun_churches256/config.yaml:5-6, cond_stage_config
        '__is_unconditional__': ddpm.py:455-456 leaves the key at None); apply_model(x, t, None)."""
        super().__init__()
        self.model = DiffusionWrapperHIP(unet, conditioning_key)
        betas = make_beta_schedule_linear(timesteps, linear_start, linear_end)
        alphas_cumprod = np.cumprod(1. - betas, axis=0)
        self.num_timesteps = int(timesteps)
        self.parameterization = 'eps'
        f32 = lambda a: torch.tensor(a, dtype=torch.float32)
        self.register_buffer('betas', f32(betas))
        self.register_buffer('alphas_cumprod', f32(alphas_cumprod))
        self.register_buffer('alphas_cumprod_prev', f32(np.append(1., alphas_cumprod[:-1])))
        self.register_buffer('sqrt_alphas_cumprod', f32(np.sqrt(alphas_cumprod)))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', f32(np.sqrt(1. - alphas_cumprod)))

    @property
    def device(self):
        return self.betas.device

    def apply_model(self, x_noisy, t, cond, return_ids=False):
        if not isinstance(cond, dict):          # ddpm.py:986-992
            key = 'c_concat' if self.model.conditioning_key == 'concat' else 'c_crossattn'
            cond = {key: [cond] if not isinstance(cond, list) else cond}
        return self.model(x_noisy, t, **cond)

    def q_sample(self, x_start, t, noise=None):
        """ddpm.py:274-277"""
        noise = torch.randn_like(x_start) if noise is None else noise
        sh = (t.shape[0],) + (1,) * (x_start.dim() - 1)
        return self.sqrt_alphas_cumprod.gather(-1, t).reshape(sh) * x_start + \
            self.sqrt_one_minus_alphas_cumprod.gather(-1, t).reshape(sh) * noise
