"""`PLMSSamplerHIP` / `DDIMSamplerHIP` / `DPMSolverSamplerHIP` -- drop-ins for the reference samplers
(ldm/models/diffusion/plms.py PLMSSampler, ddim.py DDIMSampler, dpm_solver/sampler.py DPMSolverSampler): same
constructor, `make_schedule`, `sample(...) -> (samples, intermediates)`, and for DDIM `stochastic_encode` / `decode`
(scripts/img2img.py:237-262).

Per step the reference issues ~15 elementwise launches plus four `torch.full` from host scalars
(plms.py:178-236); here the classifier-free-guidance combine and the PLMS/DDIM latent update are one fused
gfx950 kernel (`sdmi_sampler_step`, csrc/sampler.hip) evaluated in the reference's fp32 operation order,
the duplicated `x_in`/`t_in`/`c_in` are built once, and the context tensor is kept identical across steps so
the UNet reuses its cross-attention K/V.  With `quantize_x0` the step is split at pred_x0 around `first_stage_model.quantize`.

`DDPMSamplerHIP` is the ancestral sampler of `LatentDiffusion` itself (ddpm.py `p_sample_loop` / `progressive_denoising`, what
`scripts/sample_diffusion.py --vanilla_sample` runs): one fused launch per step as well (`sdmi_ddpm_step`).
"""
import numpy as np
import torch

from . import _lib

try:                                    # progress bar only; the reference prints the same bars
    from tqdm import tqdm
except Exception:                       # pragma: no cover
    def tqdm(it, **kw):
        return it


# ---- schedule tables (host side; ldm/modules/diffusionmodules/util.py:46-74) --------------------------------------
def make_ddim_timesteps(num_ddim, num_ddpm, discretize='uniform'):
    if discretize == 'uniform':
        c = num_ddpm // num_ddim
        ts = np.asarray(list(range(0, num_ddpm, c)))
    elif discretize == 'quad':
        ts = ((np.linspace(0, np.sqrt(num_ddpm * .8), num_ddim)) ** 2).astype(int)
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{discretize}"')
    return ts + 1


def make_tables(alphas_cumprod, ddim_timesteps, eta):
    """alphas_cumprod: 1-D fp32 numpy.  Returns fp32 numpy tables (alphas_prev[0] = alphas_cumprod[0], util.py:66)."""
    ac = np.asarray(alphas_cumprod, dtype=np.float32)
    alphas = ac[ddim_timesteps]
    alphas_prev = np.asarray([ac[0]] + ac[ddim_timesteps[:-1]].tolist(), dtype=np.float32)
    # util.py:65-69 as the reference's types make it come out: alphas is an fp32 tensor there and alphas_prev a float64 array of the same
    # values, so (1 - alphas_prev) / (1 - alphas) is the tensor's __rtruediv__ -- the fp32 reciprocal of the fp32 difference, times the
    # float64 numerator -- and every other operation runs in float64; the step then rounds sigma to fp32
    ap64, a64 = alphas_prev.astype(np.float64), alphas.astype(np.float64)
    recip = (np.float32(1.0) / (1 - alphas)).astype(np.float64)
    sigmas = (eta * np.sqrt(recip * (1 - ap64) * (1 - a64 / ap64))).astype(np.float32)
    return dict(alphas=alphas, alphas_prev=alphas_prev, sigmas=sigmas,
                sqrt_one_minus_alphas=np.sqrt(1.0 - alphas).astype(np.float32))


def plms_plan(timesteps):
    """[(i, index, t, t_next, mode)] for the PLMS loop (plms.py:142-162,218-232); mode = multistep order code of
    sdmi_sampler_step (4 = first step: Euler predictor + second model evaluation)."""
    time_range = np.flip(timesteps)
    total = timesteps.shape[0]
    plan = []
    for i, step in enumerate(time_range):
        t_next = time_range[min(i + 1, len(time_range) - 1)]
        plan.append((i, total - i - 1, int(step), int(t_next), 4 if i == 0 else min(i, 3)))
    return plan


class _SamplerBase(object):
    def __init__(self, model, schedule='linear', **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self._lib = None

    def register_buffer(self, name, attr):   # kept for API compatibility (plms.py:18-22)
        setattr(self, name, attr)

    @staticmethod
    def _noise_like(shape, device):
        """util.py noise_like (ddim.py:200): one draw from the device RNG per step.  A separate method so that a parity test
        can hand out the recorded sequence of a reference run (tests/test_sampler_gpu.py)."""
        return torch.randn(shape, device=device)

    def _tables(self, ddim_num_steps, ddim_discretize, ddim_eta):
        self.ddim_timesteps = make_ddim_timesteps(ddim_num_steps, self.ddpm_num_timesteps, ddim_discretize)
        ac = self.model.alphas_cumprod
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        ac_np = ac.detach().to(torch.float32).cpu().numpy()
        t = make_tables(ac_np, self.ddim_timesteps, ddim_eta)
        self._tab = t
        to_t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        self.alphas_cumprod = ac.detach().to(torch.float32)
        self.ddim_sigmas, self.ddim_alphas = to_t(t['sigmas']), to_t(t['alphas'])
        self.ddim_alphas_prev = to_t(t['alphas_prev'])
        self.ddim_sqrt_one_minus_alphas = to_t(t['sqrt_one_minus_alphas'])

    # ---- one fused CFG + update launch ------------------------------------------------------------------
    def _step(self, eps_model, cfg, scale, x, mode, old, index, e_t_out, x_prev, pred_x0=None, noise=None, quantize=False):
        """Returns pred_x0 (with `quantize` the codebook rows first_stage_model.quantize put in its place: ddim.py:196-197, plms.py:208-209)."""
        if not x.is_cuda:
            raise RuntimeError('the HIP sampler step runs on MI355X device tensors only (no CPU fallback)')
        if self._lib is None:
            self._lib = _lib.load()
        t = self._tab
        o = list(old) + [None, None, None]
        if quantize:        # the step split at pred_x0: first half, the quantizer (sdmi_k_vq_quantize), second half
            pred_x0 = torch.empty_like(x) if pred_x0 is None else pred_x0
            ep = torch.empty_like(x)
            _lib.check(self._lib.sdmi_sampler_step_x0(
                eps_model.data_ptr(), int(cfg), float(scale), x.data_ptr(), int(mode), _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]),
                float(t['alphas'][index]), float(t['sqrt_one_minus_alphas'][index]), _lib.ptr(e_t_out), ep.data_ptr(),
                pred_x0.data_ptr(), x.numel(), _lib.stream_ptr()))
            pred_x0 = self.model.first_stage_model.quantize(pred_x0)[0].float().contiguous()
            _lib.check(self._lib.sdmi_sampler_step_from_x0(
                pred_x0.data_ptr(), ep.data_ptr(), float(t['alphas_prev'][index]), float(t['sigmas'][index]), _lib.ptr(noise),
                x_prev.data_ptr(), x.numel(), _lib.stream_ptr()))
            return pred_x0
        _lib.check(self._lib.sdmi_sampler_step(
            eps_model.data_ptr(), int(cfg), float(scale), x.data_ptr(), int(mode),
            _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]),
            float(t['alphas'][index]), float(t['alphas_prev'][index]), float(t['sigmas'][index]),
            float(t['sqrt_one_minus_alphas'][index]),
            _lib.ptr(noise), _lib.ptr(e_t_out), x_prev.data_ptr(), _lib.ptr(pred_x0), x.numel(), _lib.stream_ptr()))
        return pred_x0

    def _check_options(self, score_corrector, quantize_x0):
        if score_corrector is not None:
            raise NotImplementedError('score_corrector is not implemented here (the reference ships no corrector)')
        if quantize_x0 and not hasattr(getattr(self.model, 'first_stage_model', None), 'quantize'):
            raise NotImplementedError('quantize_x0 needs a first stage with a codebook: model.first_stage_model.quantize (VQModelInterfaceHIP)')

    def _hip_unet(self):
        """The UNetModelHIP behind model.apply_model, if any (LatentDiffusion.model.diffusion_model, ddpm.py:1398)."""
        from .unet import UNetModelHIP
        u = getattr(getattr(self.model, 'model', None), 'diffusion_model', None)
        return u if isinstance(u, UNetModelHIP) else None

    def _prepare(self, cond, shape, x_T, uc, scale):
        device = self.model.betas.device
        b = shape[0]
        img = torch.randn(shape, device=device) if x_T is None else x_T
        img = img.detach().float().contiguous()
        cfg = not (uc is None or scale == 1.)
        if cfg:
            c_in = torch.cat([uc, cond])                         # [uncond, cond] order, plms.py:184
            x_in = torch.empty((2 * b,) + tuple(shape[1:]), device=device, dtype=torch.float32)
        else:
            c_in, x_in = cond, torch.empty(tuple(shape), device=device, dtype=torch.float32)
        return device, b, img, cfg, c_in, x_in

    def _model_eps(self, x_in, img, t_val, c_in, cfg, b, t_dtype=torch.long):
        """apply_model on the (duplicated) latent; returns the raw model output [2b or b, C, H, W] fp32."""
        x_in[:b].copy_(img)
        if cfg:
            x_in[b:].copy_(img)
        t_in = torch.full((x_in.shape[0],), t_val, device=x_in.device, dtype=t_dtype)
        unet = self._hip_unet() if t_dtype == torch.long else None
        if unet is not None:
            unet.hint_timestep(int(t_val))          # every row of t_in is this int: rows of the timestep table, if cached
        try:
            out = self.model.apply_model(x_in, t_in, c_in)
        finally:
            if unet is not None:
                unet.clear_timestep_hint()          # (consumed by forward(); still set only if apply_model raised before it)
        return out.float().contiguous()


class PLMSSamplerHIP(_SamplerBase):
    def make_schedule(self, ddim_num_steps, ddim_discretize='uniform', ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        self._tables(ddim_num_steps, ddim_discretize, ddim_eta)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        if conditioning is not None and not isinstance(conditioning, dict) and conditioning.shape[0] != batch_size:
            print(f'Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}')
        if isinstance(conditioning, dict):
            raise NotImplementedError('dict conditioning (hybrid models) is outside the SD-v1 txt2img path')
        self._check_options(score_corrector, quantize_x0)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        print(f'Data shape for PLMS sampling is {size}')
        return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback, mask=mask, x0=x0,
                                  x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, quantize_denoised=quantize_x0)

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, callback=None, img_callback=None, mask=None, x0=None,
                      log_every_t=100, unconditional_guidance_scale=1., unconditional_conditioning=None, quantize_denoised=False):
        scale, uc = unconditional_guidance_scale, unconditional_conditioning
        device, b, img, cfg, c_in, x_in = self._prepare(cond, shape, x_T, uc, scale)
        plan = plms_plan(self.ddim_timesteps)
        total_steps = len(plan)
        print(f'Running PLMS Sampling with {total_steps} timesteps')
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        old_eps = []            # newest first
        unet = self._hip_unet()
        if unet is not None:
            unet.pin_context(c_in)
            unet.cache_timesteps([t for p in plan for t in (p[2], p[3]) if t is not None])
        try:
            img = self._plms_loop(plan, total_steps, device, b, img, cfg, c_in, x_in, scale, mask, x0, callback,
                                  img_callback, log_every_t, intermediates, old_eps, quantize_denoised)
        finally:
            if unet is not None:
                unet.unpin_context()
        return img, intermediates

    def _plms_loop(self, plan, total_steps, device, b, img, cfg, c_in, x_in, scale, mask, x0, callback, img_callback,
                   log_every_t, intermediates, old_eps, quantize=False):
        for (i, index, t, t_next, mode) in tqdm(plan, desc='PLMS Sampler', total=total_steps):
            if mask is not None:
                assert x0 is not None
                ts = torch.full((b,), t, device=device, dtype=torch.long)
                img = (self.model.q_sample(x0, ts) * mask + (1. - mask) * img).float().contiguous()
            eps = self._model_eps(x_in, img, t, c_in, cfg, b)
            e_t = torch.empty_like(img)
            x_prev = torch.empty_like(img)
            pred_x0 = torch.empty_like(img)
            if mode == 4:
                # Pseudo Improved Euler: predictor with e_t, second evaluation at t_next, then (e_t + e_t_next)/2
                self._step(eps, cfg, scale, img, 0, [], index, e_t, x_prev, quantize=quantize)
                eps_next = self._model_eps(x_in, x_prev, t_next, c_in, cfg, b)
                x_prev2 = torch.empty_like(img)
                pred_x0 = self._step(eps_next, cfg, scale, img, 4, [e_t], index, None, x_prev2, pred_x0, quantize=quantize)
                x_prev = x_prev2
            else:
                pred_x0 = self._step(eps, cfg, scale, img, mode, old_eps, index, e_t, x_prev, pred_x0, quantize=quantize)
            img = x_prev
            old_eps.insert(0, e_t)
            if len(old_eps) >= 4:
                old_eps.pop()
            if callback: callback(i)
            if img_callback: img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img


class DDIMSamplerHIP(_SamplerBase):
    def make_schedule(self, ddim_num_steps, ddim_discretize='uniform', ddim_eta=0., verbose=True):
        self._tables(ddim_num_steps, ddim_discretize, ddim_eta)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        if conditioning is not None and not isinstance(conditioning, dict) and conditioning.shape[0] != batch_size:
            print(f'Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}')
        if isinstance(conditioning, dict):
            raise NotImplementedError('dict conditioning (hybrid models) is outside the SD-v1 txt2img path')
        self._check_options(score_corrector, quantize_x0)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        print(f'Data shape for DDIM sampling is {size}, eta {eta}')
        return self._loop(conditioning, size, self.ddim_timesteps, x_T=x_T, callback=callback,
                          img_callback=img_callback, mask=mask, x0=x0, log_every_t=log_every_t,
                          temperature=temperature, noise_dropout=noise_dropout,
                          scale=unconditional_guidance_scale, uc=unconditional_conditioning, desc='DDIM Sampler',
                          quantize_denoised=quantize_x0)

    @torch.no_grad()
    def _loop(self, cond, shape, timesteps, x_T=None, callback=None, img_callback=None, mask=None, x0=None,
              log_every_t=100, temperature=1., noise_dropout=0., scale=1., uc=None, desc='DDIM Sampler', quantize_denoised=False):
        device, b, img, cfg, c_in, x_in = self._prepare(cond, shape, x_T, uc, scale)
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        print(f'Running DDIM Sampling with {total_steps} timesteps')
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        unet = self._hip_unet()
        if unet is not None:
            unet.pin_context(c_in)
            unet.cache_timesteps([int(t) for t in time_range])
        try:
            img = self._ddim_loop(time_range, total_steps, device, b, img, cfg, c_in, x_in, scale, mask, x0, callback,
                                  img_callback, log_every_t, temperature, noise_dropout, intermediates, desc, quantize_denoised)
        finally:
            if unet is not None:
                unet.unpin_context()
        return img, intermediates

    def _ddim_loop(self, time_range, total_steps, device, b, img, cfg, c_in, x_in, scale, mask, x0, callback,
                   img_callback, log_every_t, temperature, noise_dropout, intermediates, desc, quantize=False):
        for i, step in enumerate(tqdm(time_range, desc=desc, total=total_steps)):
            index = total_steps - i - 1
            if mask is not None:
                assert x0 is not None
                ts = torch.full((b,), int(step), device=device, dtype=torch.long)
                img = (self.model.q_sample(x0, ts) * mask + (1. - mask) * img).float().contiguous()
            eps = self._model_eps(x_in, img, int(step), c_in, cfg, b)
            # ddim.py:200 draws noise_like() on EVERY step, also at eta = 0 where sigma_t = 0 and the term vanishes: draw it
            # too, so the device RNG stream stays where the reference's is (the x_T of a later n_iter comes from it);
            # the kernel only reads it when sigma_t != 0.  The reference multiplies sigma_t * noise first, then the
            # temperature: the step kernel takes the product noise * temperature (identical at the default temperature 1).
            noise = self._noise_like(img.shape, device) * temperature
            if noise_dropout > 0.:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
            noise = noise.float().contiguous() if float(self._tab['sigmas'][index]) != 0.0 else None
            x_prev = torch.empty_like(img)
            pred_x0 = torch.empty_like(img)
            pred_x0 = self._step(eps, cfg, scale, img, 0, [], index, None, x_prev, pred_x0, noise, quantize=quantize)
            img = x_prev
            if callback: callback(i)
            if img_callback: img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """ddim.py:206-220 (runs once per image; plain torch, not on the hot loop)."""
        if use_original_steps:
            raise NotImplementedError('use_original_steps is not used by scripts/img2img.py')
        a = torch.sqrt(self.ddim_alphas).to(x0.device)
        s = self.ddim_sqrt_one_minus_alphas.to(x0.device)
        if noise is None:
            noise = torch.randn_like(x0)
        sh = (t.shape[0],) + (1,) * (x0.dim() - 1)
        return a.gather(-1, t).reshape(sh) * x0 + s.gather(-1, t).reshape(sh) * noise

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False):
        """ddim.py:222-241: timesteps[:t_start], flipped."""
        if use_original_steps:
            raise NotImplementedError('use_original_steps is not used by scripts/img2img.py')
        img, _ = self._loop(cond, tuple(x_latent.shape), self.ddim_timesteps[:t_start], x_T=x_latent,
                            scale=unconditional_guidance_scale, uc=unconditional_conditioning, desc='Decoding image')
        return img


# ---- ancestral DDPM sampling: scripts/sample_diffusion.py --vanilla_sample (LatentDiffusion.p_sample_loop, ddpm.py:1165-1214) --------
DDPM_TABLES = ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod',
               'log_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_variance',
               'posterior_log_variance_clipped', 'posterior_mean_coef1', 'posterior_mean_coef2')


def ddpm_tables(betas):
    """The buffers of DDPM.register_schedule (ddpm.py:117-157, v_posterior = 0) from float64 betas, computed as the reference computes
    them -- float64 numpy, expression for expression, then float32: {name: fp32 numpy [n]}."""
    betas = np.asarray(betas, dtype=np.float64)
    alphas = 1. - betas
    alphas_cumprod = np.cumprod(alphas, axis=0)
    alphas_cumprod_prev = np.append(1., alphas_cumprod[:-1])
    posterior_variance = (1 - 0.) * betas * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod) + 0. * betas
    t = dict(betas=betas, alphas_cumprod=alphas_cumprod, alphas_cumprod_prev=alphas_cumprod_prev,
             sqrt_alphas_cumprod=np.sqrt(alphas_cumprod), sqrt_one_minus_alphas_cumprod=np.sqrt(1. - alphas_cumprod),
             log_one_minus_alphas_cumprod=np.log(1. - alphas_cumprod), sqrt_recip_alphas_cumprod=np.sqrt(1. / alphas_cumprod),
             sqrt_recipm1_alphas_cumprod=np.sqrt(1. / alphas_cumprod - 1), posterior_variance=posterior_variance,
             posterior_log_variance_clipped=np.log(np.maximum(posterior_variance, 1e-20)),
             posterior_mean_coef1=betas * np.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod),
             posterior_mean_coef2=(1. - alphas_cumprod_prev) * np.sqrt(alphas) / (1. - alphas_cumprod))
    return {k: np.asarray(v, dtype=np.float32) for k, v in t.items()}


def ddpm_step_std(posterior_log_variance_clipped):
    """(0.5 * model_log_variance).exp() of p_sample (ddpm.py:1107) for every t: the same two fp32 torch ops on the CPU -> fp32 numpy [n].
    (The reference runs them on a [b, 1, 1, 1] gather of the table; torch's CPU exp gives an element the same bits in either shape --
    tests/test_ddpm_host.py holds this against the values a reference run recorded.)"""
    lv = torch.as_tensor(np.asarray(posterior_log_variance_clipped, dtype=np.float32))
    return (0.5 * lv).exp().numpy()


class DDPMSamplerHIP(_SamplerBase):
    """The ancestral sampler of LatentDiffusion -- `p_sample_loop` (ddpm.py:1165-1214) and `progressive_denoising` (:1109-1163) over
    `p_sample` / `p_mean_variance` (:1047-1107) -- for any `model` with betas, alphas_cumprod, num_timesteps and apply_model (the
    reference's LatentDiffusion over UNetModelHIP included).  Per step: one apply_model, one noise draw and ONE launch (sdmi_ddpm_step:
    predict_start_from_noise, clamp, q_posterior's mean, the noise term and the mask blend), where the reference issues about a dozen
    elementwise launches and gathers.  With quantize_denoised the step is two launches around first_stage_model.quantize.

    The schedule tables are the model's own registered buffers where it has them (LatentDiffusion, LatentDiffusionHIP); a model with
    betas alone gets ddpm_tables(betas) -- from its fp32 betas, so the last bit of a table entry may differ from a reference that
    started from float64 betas.  No classifier-free guidance: the reference's loop has none."""

    def __init__(self, model, **kwargs):
        super().__init__(model, **kwargs)
        if getattr(model, 'parameterization', 'eps') != 'eps':
            raise NotImplementedError(f"parameterization {model.parameterization!r}: the ancestral step is built for parameterization 'eps' only")
        if getattr(model, 'shorten_cond_schedule', False):
            raise NotImplementedError('shorten_cond_schedule (a noised conditioning per step) is not implemented here')
        have = all(hasattr(model, k) for k in DDPM_TABLES)
        if have:
            tab = {k: getattr(model, k).detach().to(torch.float32).cpu().numpy() for k in DDPM_TABLES}
        else:
            tab = ddpm_tables(model.betas.detach().cpu().numpy())
        assert tab['betas'].shape[0] == self.ddpm_num_timesteps, 'betas have to be defined for each timestep'
        self._tab = tab
        self._std = ddpm_step_std(tab['posterior_log_variance_clipped'])
        self.clip_denoised = bool(getattr(model, 'clip_denoised', True))          # DDPM.__init__'s default
        self.log_every_t = int(getattr(model, 'log_every_t', 100))

    @staticmethod
    def _q_noise_like(x0):
        """the draw inside q_sample(x0, ts) of the mask blend (ddpm.py:275); a method of its own for the same reason as _noise_like"""
        return torch.randn_like(x0)

    def step_scalars(self, t):
        """(c_recip, c_recipm1, coef1, coef2, s, sa, s1ma) of sdmi_ddpm_step at timestep t; s = nonzero_mask * std (ddpm.py:1100-1107)"""
        T = self._tab
        return (float(T['sqrt_recip_alphas_cumprod'][t]), float(T['sqrt_recipm1_alphas_cumprod'][t]), float(T['posterior_mean_coef1'][t]),
                float(T['posterior_mean_coef2'][t]), float(self._std[t]) if t != 0 else 0.0, float(T['sqrt_alphas_cumprod'][t]),
                float(T['sqrt_one_minus_alphas_cumprod'][t]))

    def _check(self, cond, quantize_denoised, score_corrector=None):
        if score_corrector is not None:
            raise NotImplementedError('score_corrector is not implemented here (the reference ships no corrector)')
        if isinstance(cond, dict):
            raise NotImplementedError('dict conditioning (hybrid models) is not implemented in the ancestral loop')
        if quantize_denoised and not hasattr(getattr(self.model, 'first_stage_model', None), 'quantize'):
            raise NotImplementedError('quantize_denoised needs a first stage with a codebook: model.first_stage_model.quantize '
                                      '(VQModelInterfaceHIP)')

    def _apply(self, img, t, cond, unet):
        ts = torch.full((img.shape[0],), t, device=img.device, dtype=torch.long)
        if unet is not None:
            unet.hint_timestep(t)
        try:
            out = self.model.apply_model(img, ts, cond)
        finally:
            if unet is not None:
                unet.clear_timestep_hint()
        return out.float().contiguous()

    def _p_sample(self, img, eps, t, noise, quantize, blend, want_x0):
        """one ancestral step: (x_prev, x0 or None); blend = (mask, x0_orig, q_noise) or None"""
        if not img.is_cuda:
            raise RuntimeError('the HIP sampler step runs on MI355X device tensors only (no CPU fallback)')
        c_recip, c_recipm1, coef1, coef2, s, sa, s1ma = self.step_scalars(t)
        if self._lib is None:
            self._lib = _lib.load()
        step, n, st = self._lib.sdmi_ddpm_step, img.numel(), _lib.stream_ptr()
        m, xo, qn = blend if blend is not None else (None, None, None)
        x_prev = torch.empty_like(img)
        x0 = torch.empty_like(img) if (want_x0 or quantize) else None
        clip = int(self.clip_denoised)
        if quantize:
            _lib.check(step(eps.data_ptr(), None, img.data_ptr(), c_recip, c_recipm1, clip, coef1, coef2, s, None, None, None, None,
                            sa, s1ma, x0.data_ptr(), None, n, st))
            x0 = self.model.first_stage_model.quantize(x0)[0].float().contiguous()
            _lib.check(step(None, x0.data_ptr(), img.data_ptr(), c_recip, c_recipm1, clip, coef1, coef2, s, noise.data_ptr(), _lib.ptr(m),
                            _lib.ptr(xo), _lib.ptr(qn), sa, s1ma, None, x_prev.data_ptr(), n, st))
        else:
            _lib.check(step(eps.data_ptr(), None, img.data_ptr(), c_recip, c_recipm1, clip, coef1, coef2, s, noise.data_ptr(), _lib.ptr(m),
                            _lib.ptr(xo), _lib.ptr(qn), sa, s1ma, _lib.ptr(x0), x_prev.data_ptr(), n, st))
        return x_prev, x0

    def _run(self, cond, shape, x_T, timesteps, mask, x0, quantize_denoised, temperature, noise_dropout, callback, img_callback,
             log_every_t, verbose, progressive, desc):
        device = self.model.betas.device
        img = torch.randn(tuple(shape), device=device) if x_T is None else x_T
        first = img
        img = img.detach().float().contiguous()
        blend0 = None
        if mask is not None:
            assert x0 is not None
            assert x0.shape[2:3] == mask.shape[2:3]  # spatial size has to match
            blend0 = (mask.detach().float().expand(img.shape).contiguous(), x0.detach().float().expand(img.shape).contiguous())
        steps = list(reversed(range(0, timesteps)))
        unet = self._hip_unet()
        if unet is not None:
            if torch.is_tensor(cond):
                unet.pin_context(cond)
            unet.cache_timesteps(steps)
        intermediates = [] if progressive else [first]
        try:
            for i in (tqdm(steps, desc=desc, total=timesteps) if verbose else steps):
                eps = self._apply(img, i, cond, unet)
                temp = temperature[i] if isinstance(temperature, (list, tuple)) else temperature
                noise = self._noise_like(img.shape, device)        # drawn at t = 0 too, as ddpm.py:1096 does
                if temp != 1.:
                    noise = noise * temp
                if noise_dropout > 0.:
                    noise = torch.nn.functional.dropout(noise, p=noise_dropout)
                noise = noise.float().contiguous()
                blend = None if blend0 is None else blend0 + (self._q_noise_like(blend0[1]).float().contiguous(),)
                img, x0_partial = self._p_sample(img, eps, i, noise, quantize_denoised, blend, progressive)
                if i % log_every_t == 0 or i == timesteps - 1:
                    intermediates.append(x0_partial if progressive else img)
                if callback: callback(i)
                if img_callback: img_callback(img, i)
        finally:
            if unet is not None:
                unet.unpin_context()
        return img, intermediates

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None, log_every_t=None):
        """ddpm.py:1165-1214: -> img, or (img, [x_T, ...img at every log_every_t-th t and the first step])."""
        self._check(cond, quantize_denoised)
        if not log_every_t:
            log_every_t = self.log_every_t
        if timesteps is None:
            timesteps = self.ddpm_num_timesteps
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        img, intermediates = self._run(cond, shape, x_T, timesteps, mask, x0, quantize_denoised, 1., 0., callback, img_callback,
                                       log_every_t, verbose, False, 'Sampling t')
        if return_intermediates:
            return img, intermediates
        return img

    @torch.no_grad()
    def progressive_denoising(self, cond, shape, verbose=True, callback=None, quantize_denoised=False, img_callback=None, mask=None,
                              x0=None, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, batch_size=None,
                              x_T=None, start_T=None, log_every_t=None):
        """ddpm.py:1109-1163: -> (img, [the x0 of every log_every_t-th t and the first step]); `temperature` a number or a per-t list."""
        self._check(cond, quantize_denoised, score_corrector)
        if not log_every_t:
            log_every_t = self.log_every_t
        timesteps = self.ddpm_num_timesteps
        if batch_size is not None:
            shape = [batch_size] + list(shape)
        else:
            batch_size = shape[0]
        if cond is not None:
            cond = [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        return self._run(cond, shape, x_T, timesteps, mask, x0, quantize_denoised, temperature, noise_dropout, callback, img_callback,
                         log_every_t, verbose, True, 'Progressive Generation')


# ---- DPM-Solver++ (2M): scripts/txt2img.py --dpm_solver ----------------------------------------------
class _DiscreteVP:
    """Host-side subset of NoiseScheduleVP('discrete', alphas_cumprod=...) (dpm_solver.py:96-156): log alpha_t is the
    piecewise-linear interpolant of 0.5 log(alphas_cumprod) over t_n = n / N, n = 1..N; fp32 torch ops on the CPU, in the
    reference's order, so the step coefficients equal the reference's."""

    def __init__(self, alphas_cumprod):
        ac = alphas_cumprod.detach().to(torch.float32).cpu()
        self.N = ac.shape[0]
        self.t_array = torch.linspace(0., 1., self.N + 1)[1:]
        self.log_alpha_array = 0.5 * torch.log(ac)

    @staticmethod
    def _interp(x, xp, yp):
        """interpolate_fn (dpm_solver.py:1132-1171) for a 1-D x: the segment its sort picks, then the same fp32 expression"""
        i = torch.clamp(torch.searchsorted(xp, x.contiguous()) - 1, 0, xp.shape[0] - 2)
        return yp[i] + (x - xp[i]) * (yp[i + 1] - yp[i]) / (xp[i + 1] - xp[i])

    def log_alpha(self, t):
        xp, yp = self.t_array, self.log_alpha_array
        if t.dim() == 1:                    # vector form (the plans of DPMSolverHIP); elementwise the 0-dim form below
            return self._interp(t, xp, yp)
        i = int(torch.clamp(torch.searchsorted(xp, t.reshape(1)) - 1, 0, self.N - 2))
        return yp[i] + (t - xp[i]) * (yp[i + 1] - yp[i]) / (xp[i + 1] - xp[i])

    def inverse_lambda(self, lamb):
        """dpm_solver.py:166-169 ('discrete'), lamb 1-D: t of a half-logSNR, through the flipped tables"""
        log_alpha = -0.5 * torch.logaddexp(torch.zeros((1,)), -2. * lamb)
        return self._interp(log_alpha, torch.flip(self.log_alpha_array, [0]), torch.flip(self.t_array, [0]))

    def alpha(self, t):
        return torch.exp(self.log_alpha(t))

    def sigma(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.log_alpha(t)))

    def lam(self, t):
        la = self.log_alpha(t)
        return la - 0.5 * torch.log(1. - torch.exp(2. * la))


def dpm_plan(ns, S):
    """Per model evaluation k = 0..S-1 (at time t_k, stepping to t_{k+1}; time-uniform from 1 to 1/N):
    (t_input, alpha_s, sigma_s, order, cx, a, inv_r0) for sdmi_dpm_solver_step -- DPM_Solver.sample(method='multistep',
    order=2, lower_order_final=True), dpm_solver.py:1068-1096."""
    if S < 2:
        raise ValueError('multistep DPM-Solver of order 2 needs at least 2 steps')      # `assert steps >= order`
    ts = torch.linspace(1., 1. / ns.N, S + 1)
    plan = []
    for k in range(S):
        s_, t_ = ts[k], ts[k + 1]
        step = k + 1
        order = 1 if step == 1 else (min(2, S + 1 - step) if S < 15 else 2)
        cx = ns.sigma(t_) / ns.sigma(s_)
        if order == 1:
            h = ns.lam(t_) - ns.lam(s_)
            a = ns.alpha(t_) * torch.expm1(-h)
            inv_r0 = torch.zeros(())
        else:
            l1, l0, lt = ns.lam(ts[k - 1]), ns.lam(s_), ns.lam(t_)
            h0, h = l0 - l1, lt - l0
            inv_r0 = 1. / (h0 / h)
            a = ns.alpha(t_) * (torch.exp(-h) - 1.)
        t_input = (s_ - 1. / ns.N) * 1000.
        plan.append((float(t_input), float(ns.alpha(s_)), float(ns.sigma(s_)), order, float(cx), float(a), float(inv_r0)))
    return plan


# ---- the rest of DPM_Solver (dpm_solver.py:351-1124): singlestep, order 3, adaptive, thresholding, either prediction type ---------
DPM_KEYWORDS = ('steps', 't_start', 't_end', 'order', 'skip_type', 'method', 'lower_order_final', 'denoise_to_zero', 'solver_type', 'atol',
                'rtol')
_EVAL, _UPDATE = 0, 1
_LIN, _DIFF, _SS3T, _MS3 = 0, 1, 2, 3           # the kernel forms of sdmi_dpm_update (csrc/dpm.hip)


def _c(v):
    """a host scalar as the fp32 the reference's tensor op sees: a one-element fp32 tensor's value, or a Python float rounded to fp32
    (what torch does with a Python scalar operand of an fp32 tensor op)"""
    return float(v.reshape(-1)[0]) if torch.is_tensor(v) else float(np.float32(v))


class DPMPlan:
    """What a non-adaptive DPM_Solver.sample does, op by op, with every scalar already evaluated:
    ops  int32 [n, 7]: (kind, form, dst, x, m0, m1, m2) -- slots name tensors, slot 0 is the initial x, -1 is none;
                       kind 0 = model evaluation at x (form 1: the data prediction whatever predict_x0 is -- denoise_to_zero_fn),
                       kind 1 = update of form `form` (sdmi_dpm_update)
    coef fp32 [n, 9]:  evaluation: (t, t_input, alpha_t, sigma_t); update: c0..c8
    timesteps, orders: the outer time grid and the order of each outer step;  result: the slot of the end point"""

    def __init__(self, ops, coef, timesteps, orders, result):
        self.ops = np.asarray(ops, dtype=np.int32).reshape(-1, 7)
        self.coef = np.asarray(coef, dtype=np.float32).reshape(-1, 9)
        self.timesteps = np.asarray(timesteps, dtype=np.float32)
        self.orders = np.asarray(orders, dtype=np.int32)
        self.result = int(result)

    def model_times(self):
        """t_input of every model evaluation, in order"""
        return [float(c[1]) for o, c in zip(self.ops, self.coef) if o[0] == _EVAL]


class _PlanBuilder:
    def __init__(self, ns):
        self.ns, self.ops, self.coef, self.n_slots = ns, [], [], 1

    def _emit(self, kind, form, x, ms, coef):
        dst = self.n_slots
        self.n_slots += 1
        ms = list(ms) + [-1] * (3 - len(ms))
        self.ops.append((kind, form, dst, x) + tuple(ms))
        self.coef.append([_c(v) for v in coef] + [0.0] * (9 - len(coef)))
        return dst

    def eval(self, x, t, data_prediction=False):
        ns = self.ns
        return self._emit(_EVAL, int(data_prediction), x, (), (t, (t - 1. / ns.N) * 1000., ns.alpha(t), ns.sigma(t)))

    def update(self, form, x, ms, coef):
        return self._emit(_UPDATE, form, x, ms, coef)


class DPMSolverHIP:
    """DPM_Solver (dpm_solver.py:351-1124) over a 'discrete' NoiseScheduleVP: `sample` with every keyword and default of the reference
    (:965-967).  The host evaluates each scalar sub-expression of an update with the reference's own torch ops on one-element fp32
    CPU tensors, in its order; the device runs one launch per model value and one per update (csrc/dpm.hip), whose bits equal the
    reference's elementwise expression.  For the non-adaptive methods the whole plan -- times, model-input times, orders, coefficients
    -- is computed before the loop (`plan`), the adaptive solver reads back its four-byte error once per iteration and nothing else.

    eps_fn(x, t_input) -> the raw model output, fp32 contiguous: [B, ...], or with cfg [2B, ...] = (unconditional, conditional) rows
    -- the noise_pred_fn of model_wrapper (:289-310, model_type 'noise') without the combine, which the model-value launch does.

    Refused, because the reference itself raises there: method='singlestep' with a skip_type other than 'logSNR'
    (dpm_solver.py:495), with order=1 and steps > 1 (:1114), and method='multistep', order=3, lower_order_final=True with
    4 <= steps < 15 (:773)."""

    def __init__(self, eps_fn, noise_schedule, predict_x0=False, thresholding=False, max_val=1., cfg=False, scale=1.):
        self.eps_fn, self.ns = eps_fn, noise_schedule
        self.predict_x0, self.thresholding, self.max_val = bool(predict_x0), bool(thresholding), float(max_val)
        self.cfg, self.scale = bool(cfg), float(scale)
        self.model_times = []           # t_input of every evaluation of the last run
        self.adaptive_log = []          # (E, accepted) of every iteration of the last adaptive run

    # ---- time grids (:410-437, :439-496) ----------------------------------------------------------------------------------------
    def get_time_steps(self, skip_type, t_T, t_0, N):
        ns = self.ns
        if skip_type == 'logSNR':
            lambda_T = ns.lam(torch.tensor([t_T]))
            lambda_0 = ns.lam(torch.tensor([t_0]))
            return ns.inverse_lambda(torch.linspace(lambda_T.item(), lambda_0.item(), N + 1))
        if skip_type == 'time_uniform':
            return torch.linspace(t_T, t_0, N + 1)
        if skip_type == 'time_quadratic':
            t_order = 2
            return torch.linspace(t_T ** (1. / t_order), t_0 ** (1. / t_order), N + 1).pow(t_order)
        raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'".format(skip_type))

    def get_orders_and_timesteps_for_singlestep_solver(self, steps, order, skip_type, t_T, t_0):
        if order == 3:
            K = steps // 3 + 1
            if steps % 3 == 0:
                orders = [3, ] * (K - 2) + [2, 1]
            elif steps % 3 == 1:
                orders = [3, ] * (K - 1) + [1]
            else:
                orders = [3, ] * (K - 1) + [2]
        elif order == 2:
            if steps % 2 == 0:
                K = steps // 2
                orders = [2, ] * K
            else:
                K = steps // 2 + 1
                orders = [2, ] * (K - 1) + [1]
        elif order == 1:
            K = 1
            orders = [1, ] * steps
            if steps > 1:
                raise ValueError("method='singlestep' with order=1 and steps > 1 raises in the reference (dpm_solver.py:1114: K = 1 gives "
                                 "two outer timesteps for `steps` steps); use method='singlestep_fixed' or 'multistep'")
        else:
            raise ValueError("'order' must be '1' or '2' or '3'.")
        if skip_type != 'logSNR':
            raise ValueError(f"method='singlestep' with skip_type={skip_type!r} raises in the reference (dpm_solver.py:495: torch.cumsum "
                             "without dim); only skip_type='logSNR' runs there")
        return self.get_time_steps(skip_type, t_T, t_0, K), orders

    # ---- the scalars of each update, transcribed expression for expression; s, t, ...: one-element fp32 tensors --------------------
    def _first(self, s, t):
        """dpm_solver_first_update (:518-545) -> (c0, c1) of form LIN"""
        ns = self.ns
        h = ns.lam(t) - ns.lam(s)
        if self.predict_x0:
            return ns.sigma(t) / ns.sigma(s), -(ns.alpha(t) * torch.expm1(-h))
        return torch.exp(ns.log_alpha(t) - ns.log_alpha(s)), -(ns.sigma(t) * torch.expm1(h))

    def _ss2(self, s, t, r1, solver_type):
        """singlestep_dpm_solver_second_update (:568-631) -> s1, (c0, c1) of x_s1 [LIN], (c0, c1, c2, 1) of x_t [DIFF]"""
        if solver_type not in ['dpm_solver', 'taylor']:
            raise ValueError("'solver_type' must be either 'dpm_solver' or 'taylor', got {}".format(solver_type))
        if r1 is None:
            r1 = 0.5
        ns = self.ns
        lambda_s, lambda_t = ns.lam(s), ns.lam(t)
        h = lambda_t - lambda_s
        s1 = ns.inverse_lambda(lambda_s + r1 * h)
        if self.predict_x0:
            phi_11 = torch.expm1(-r1 * h)
            phi_1 = torch.expm1(-h)
            a = (ns.sigma(s1) / ns.sigma(s), -(ns.alpha(s1) * phi_11))
            c0, c1 = ns.sigma(t) / ns.sigma(s), ns.alpha(t) * phi_1
            if solver_type == 'dpm_solver':
                c2 = -((0.5 / r1) * c1)
            else:
                c2 = (1. / r1) * (ns.alpha(t) * ((torch.exp(-h) - 1.) / h + 1.))
        else:
            phi_11 = torch.expm1(r1 * h)
            phi_1 = torch.expm1(h)
            a = (torch.exp(ns.log_alpha(s1) - ns.log_alpha(s)), -(ns.sigma(s1) * phi_11))
            c0, c1 = torch.exp(ns.log_alpha(t) - ns.log_alpha(s)), ns.sigma(t) * phi_1
            if solver_type == 'dpm_solver':
                c2 = -((0.5 / r1) * c1)
            else:
                c2 = -((1. / r1) * (ns.sigma(t) * ((torch.exp(h) - 1.) / h - 1.)))
        return s1, a, (c0, -c1, c2, 1.0)

    def _ss3(self, s, t, r1, r2, solver_type):
        """singlestep_dpm_solver_third_update (:653-753) -> s1, s2, x_s1 [LIN], x_s2 [DIFF], form and coefficients of x_t"""
        if solver_type not in ['dpm_solver', 'taylor']:
            raise ValueError("'solver_type' must be either 'dpm_solver' or 'taylor', got {}".format(solver_type))
        if r1 is None:
            r1 = 1. / 3.
        if r2 is None:
            r2 = 2. / 3.
        ns = self.ns
        lambda_s, lambda_t = ns.lam(s), ns.lam(t)
        h = lambda_t - lambda_s
        s1 = ns.inverse_lambda(lambda_s + r1 * h)
        s2 = ns.inverse_lambda(lambda_s + r2 * h)
        if self.predict_x0:
            phi_11 = torch.expm1(-r1 * h)
            phi_12 = torch.expm1(-r2 * h)
            phi_1 = torch.expm1(-h)
            phi_22 = torch.expm1(-r2 * h) / (r2 * h) + 1.
            phi_2 = phi_1 / h + 1.
            phi_3 = phi_2 / h - 0.5
            a = (ns.sigma(s1) / ns.sigma(s), -(ns.alpha(s1) * phi_11))
            b = (ns.sigma(s2) / ns.sigma(s), -(ns.alpha(s2) * phi_12), r2 / r1 * (ns.alpha(s2) * phi_22), 1.0)
            c0, c1 = ns.sigma(t) / ns.sigma(s), ns.alpha(t) * phi_1
            if solver_type == 'dpm_solver':
                return s1, s2, a, b, _DIFF, (c0, -c1, (1. / r2) * (ns.alpha(t) * phi_2), 1.0)
            return s1, s2, a, b, _SS3T, (c0, -c1, ns.alpha(t) * phi_2, -(ns.alpha(t) * phi_3), 1. / r1, 1. / r2, r2, r1, r2 - r1)
        phi_11 = torch.expm1(r1 * h)
        phi_12 = torch.expm1(r2 * h)
        phi_1 = torch.expm1(h)
        phi_22 = torch.expm1(r2 * h) / (r2 * h) - 1.
        phi_2 = phi_1 / h - 1.
        phi_3 = phi_2 / h - 0.5
        a = (torch.exp(ns.log_alpha(s1) - ns.log_alpha(s)), -(ns.sigma(s1) * phi_11))
        b = (torch.exp(ns.log_alpha(s2) - ns.log_alpha(s)), -(ns.sigma(s2) * phi_12), -(r2 / r1 * (ns.sigma(s2) * phi_22)), 1.0)
        c0, c1 = torch.exp(ns.log_alpha(t) - ns.log_alpha(s)), ns.sigma(t) * phi_1
        if solver_type == 'dpm_solver':
            return s1, s2, a, b, _DIFF, (c0, -c1, -((1. / r2) * (ns.sigma(t) * phi_2)), 1.0)
        return s1, s2, a, b, _SS3T, (c0, -c1, -(ns.sigma(t) * phi_2), -(ns.sigma(t) * phi_3), 1. / r1, 1. / r2, r2, r1, r2 - r1)

    def _ms2(self, t_prev_1, t_prev_0, t, solver_type):
        """multistep_dpm_solver_second_update (:769-810) -> (c0, c1, c2, 1 / r0) of form DIFF"""
        if solver_type not in ['dpm_solver', 'taylor']:
            raise ValueError("'solver_type' must be either 'dpm_solver' or 'taylor', got {}".format(solver_type))
        ns = self.ns
        lambda_prev_1, lambda_prev_0, lambda_t = ns.lam(t_prev_1), ns.lam(t_prev_0), ns.lam(t)
        h_0 = lambda_prev_0 - lambda_prev_1
        h = lambda_t - lambda_prev_0
        r0 = h_0 / h
        if self.predict_x0:
            c0, c1 = ns.sigma(t) / ns.sigma(t_prev_0), ns.alpha(t) * (torch.exp(-h) - 1.)
            c2 = -(0.5 * c1) if solver_type == 'dpm_solver' else ns.alpha(t) * ((torch.exp(-h) - 1.) / h + 1.)
        else:
            c0, c1 = torch.exp(ns.log_alpha(t) - ns.log_alpha(t_prev_0)), ns.sigma(t) * (torch.exp(h) - 1.)
            c2 = -(0.5 * c1) if solver_type == 'dpm_solver' else -(ns.sigma(t) * ((torch.exp(h) - 1.) / h - 1.))
        return (c0, -c1, c2, 1. / r0)

    def _ms3(self, t_prev_2, t_prev_1, t_prev_0, t):
        """multistep_dpm_solver_third_update (:826-857) -> c0..c7 of form MS3"""
        ns = self.ns
        lambda_prev_2, lambda_prev_1, lambda_prev_0, lambda_t = ns.lam(t_prev_2), ns.lam(t_prev_1), ns.lam(t_prev_0), ns.lam(t)
        h_1 = lambda_prev_1 - lambda_prev_2
        h_0 = lambda_prev_0 - lambda_prev_1
        h = lambda_t - lambda_prev_0
        r0, r1 = h_0 / h, h_1 / h
        tail = (1. / r0, 1. / r1, r0 / (r0 + r1), 1. / (r0 + r1))
        if self.predict_x0:
            alpha_t = ns.alpha(t)
            return (ns.sigma(t) / ns.sigma(t_prev_0), -(alpha_t * (torch.exp(-h) - 1.)), alpha_t * ((torch.exp(-h) - 1.) / h + 1.),
                    -(alpha_t * ((torch.exp(-h) - 1. + h) / h ** 2 - 0.5))) + tail
        sigma_t = ns.sigma(t)
        return (torch.exp(ns.log_alpha(t) - ns.log_alpha(t_prev_0)), -(sigma_t * (torch.exp(h) - 1.)),
                -(sigma_t * ((torch.exp(h) - 1.) / h - 1.)), -(sigma_t * ((torch.exp(h) - 1. - h) / h ** 2 - 0.5))) + tail

    # ---- the plan of a non-adaptive run (:1077-1123) --------------------------------------------------------------------------------
    def _singlestep(self, pb, x, s, t, order, solver_type, r1, r2):
        """singlestep_dpm_solver_update (:876-883) as plan ops -> the slot of x_t"""
        m = pb.eval(x, s)
        if order == 1:
            return pb.update(_LIN, x, (m,), self._first(s, t))
        if order == 2:
            s1, a, c = self._ss2(s, t, r1, solver_type)
            m1 = pb.eval(pb.update(_LIN, x, (m,), a), s1)
            return pb.update(_DIFF, x, (m, m1, m), c)
        if order == 3:
            s1, s2, a, b, form, c = self._ss3(s, t, r1, r2, solver_type)
            m1 = pb.eval(pb.update(_LIN, x, (m,), a), s1)
            m2 = pb.eval(pb.update(_DIFF, x, (m, m1, m), b), s2)
            return pb.update(form, x, (m, m2, m) if form == _DIFF else (m, m1, m2), c)
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))

    def _multistep(self, pb, x, model_prev_list, t_prev_list, t, order, solver_type):
        """multistep_dpm_solver_update (:900-907) as a plan op"""
        if order == 1:
            return pb.update(_LIN, x, (model_prev_list[-1],), self._first(t_prev_list[-1], t))
        if order == 2:
            model_prev_1, model_prev_0 = model_prev_list
            t_prev_1, t_prev_0 = t_prev_list
            return pb.update(_DIFF, x, (model_prev_0, model_prev_0, model_prev_1), self._ms2(t_prev_1, t_prev_0, t, solver_type))
        if order == 3:
            model_prev_2, model_prev_1, model_prev_0 = model_prev_list
            return pb.update(_MS3, x, (model_prev_0, model_prev_1, model_prev_2), self._ms3(*t_prev_list, t))
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))

    def plan(self, steps=20, t_start=None, t_end=None, order=3, skip_type='time_uniform', method='singlestep', lower_order_final=True,
             denoise_to_zero=False, solver_type='dpm_solver'):
        ns = self.ns
        t_0 = 1. / ns.N if t_end is None else t_end
        t_T = 1. if t_start is None else t_start
        pb, x, orders = _PlanBuilder(ns), 0, []
        if method == 'multistep':
            assert steps >= order
            if order == 3 and lower_order_final and 4 <= steps < 15:
                raise ValueError("method='multistep', order=3, lower_order_final=True with 4 <= steps < 15 raises in the reference "
                                 "(dpm_solver.py:773: the second-order update unpacks the three-entry history into two); "
                                 "pass lower_order_final=False or steps >= 15")
            timesteps = self.get_time_steps(skip_type, t_T, t_0, steps)
            assert timesteps.shape[0] - 1 == steps
            tt = [timesteps[k:k + 1] for k in range(steps + 1)]
            model_prev_list, t_prev_list = [pb.eval(x, tt[0])], [tt[0]]
            for init_order in range(1, order):
                x = self._multistep(pb, x, model_prev_list, t_prev_list, tt[init_order], init_order, solver_type)
                orders.append(init_order)
                model_prev_list.append(pb.eval(x, tt[init_order]))
                t_prev_list.append(tt[init_order])
            for step in range(order, steps + 1):
                step_order = min(order, steps + 1 - step) if lower_order_final and steps < 15 else order
                x = self._multistep(pb, x, model_prev_list, t_prev_list, tt[step], step_order, solver_type)
                orders.append(step_order)
                for i in range(order - 1):
                    t_prev_list[i] = t_prev_list[i + 1]
                    model_prev_list[i] = model_prev_list[i + 1]
                t_prev_list[-1] = tt[step]
                if step < steps:
                    model_prev_list[-1] = pb.eval(x, tt[step])
        elif method in ['singlestep', 'singlestep_fixed']:
            if method == 'singlestep':
                timesteps, orders = self.get_orders_and_timesteps_for_singlestep_solver(steps, order, skip_type, t_T, t_0)
            else:
                K = steps // order
                orders = [order, ] * K
                timesteps = self.get_time_steps(skip_type, t_T, t_0, K)
            for i, o in enumerate(orders):
                t_T_inner, t_0_inner = timesteps[i:i + 1], timesteps[i + 1:i + 2]
                timesteps_inner = self.get_time_steps(skip_type, t_T_inner.item(), t_0_inner.item(), o)
                lambda_inner = ns.lam(timesteps_inner)
                h = lambda_inner[-1] - lambda_inner[0]
                r1 = None if o <= 1 else (lambda_inner[1] - lambda_inner[0]) / h
                r2 = None if o <= 2 else (lambda_inner[2] - lambda_inner[0]) / h
                x = self._singlestep(pb, x, t_T_inner, t_0_inner, o, solver_type, r1, r2)
        else:
            raise ValueError(f"method {method!r}: 'singlestep', 'multistep', 'singlestep_fixed' or 'adaptive'")
        if denoise_to_zero:
            x = pb.eval(x, torch.ones((1,)) * t_0, data_prediction=True)
        return DPMPlan(pb.ops, pb.coef, timesteps.numpy(), orders, x)

    # ---- the device side ------------------------------------------------------------------------------------------------------------
    def _model_value(self, x, t_input, alpha_t, sigma_t, data_prediction):
        """model_fn (:401-408) / data_prediction_fn: one model call, then the model-value launch (twice around the scale with thresholding)"""
        if not x.is_cuda:
            raise RuntimeError('the HIP sampler step runs on MI355X device tensors only (no CPU fallback)')
        lib = _lib.load()
        eps = self.eps_fn(x, t_input)
        self.model_times.append(float(t_input))
        n, B = x.numel(), x.shape[0]
        assert eps.is_contiguous() and eps.dtype == torch.float32 and eps.numel() == (2 * n if self.cfg else n)
        out = torch.empty_like(x)
        value = lambda s: _lib.check(lib.sdmi_dpm_model_value(eps.data_ptr(), int(self.cfg), self.scale, x.data_ptr(), int(data_prediction),
                                                              alpha_t, sigma_t, _lib.ptr(s), n // B, out.data_ptr(), n, _lib.stream_ptr()))
        value(None)
        if data_prediction and self.thresholding:
            s = torch.empty((B,), device=x.device, dtype=torch.float32)
            _lib.check(lib.sdmi_dpm_threshold_scale(out.data_ptr(), B, n // B, self.max_val, s.data_ptr(), None, _lib.stream_ptr()))
            self.last_scale = s
            value(s)
        return out

    def _update(self, form, x, ms, coef):
        lib = _lib.load()
        out = torch.empty_like(x)
        ms = list(ms) + [None] * (3 - len(ms))
        c9 = (_lib.C.c_float * 9)(*([_c(v) for v in coef] + [0.0] * (9 - len(coef))))
        _lib.check(lib.sdmi_dpm_update(int(form), x.data_ptr(), ms[0].data_ptr(), _lib.ptr(ms[1]), _lib.ptr(ms[2]), c9, out.data_ptr(),
                                       x.numel(), _lib.stream_ptr()))
        return out

    def _error(self, x_higher, x_lower, x_prev, atol, rtol):
        """E of :952-954 -> 0-dim fp32 CPU tensor: two launches, then the loop's one read-back of four bytes"""
        lib = _lib.load()
        B, n = x_higher.shape[0], x_higher.numel()
        if getattr(self, '_err_ws', None) is None or self._err_ws[0].device != x_higher.device:
            ws_floats = int(lib.sdmi_dpm_adaptive_error_ws_floats(B, n // B))
            self._err_ws = (torch.empty((ws_floats,), device=x_higher.device, dtype=torch.float32),
                            torch.empty((1,), device=x_higher.device, dtype=torch.float32))
        ws, E = self._err_ws
        _lib.check(lib.sdmi_dpm_adaptive_error(x_higher.data_ptr(), x_lower.data_ptr(), x_prev.data_ptr(), float(atol), float(rtol), B, n // B,
                                               ws.data_ptr(), ws.numel(), E.data_ptr(), _lib.stream_ptr()))
        return E.cpu().reshape(())

    def run_plan(self, x, plan, callback=None):
        """the loop of a DPMPlan on the device: nothing but model calls and launches"""
        x = x.detach().float().contiguous()
        self.model_times = []
        last_use = {}
        for k, op in enumerate(plan.ops):
            for slot in op[3:]:
                last_use[int(slot)] = k
        last_use[plan.result] = len(plan.ops)
        buf = {0: x}
        for k, (op, c) in enumerate(zip(plan.ops, plan.coef)):
            kind, form, dst, xs = (int(v) for v in op[:4])
            if kind == _EVAL:
                buf[dst] = self._model_value(buf[xs], float(c[1]), float(c[2]), float(c[3]), self.predict_x0 or form == 1)
                if callback: callback(len(self.model_times) - 1)
            else:
                buf[dst] = self._update(form, buf[xs], [buf[int(m)] for m in op[4:] if m >= 0], c)
            for slot in [s for s, last in last_use.items() if last == k and s in buf]:
                del buf[slot]
        return buf[plan.result]

    def dpm_solver_adaptive(self, x, order, t_T, t_0, h_init=0.05, atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, solver_type='dpm_solver'):
        """dpm_solver_adaptive (:931-963).  The step size passes through the host (exp / log of the schedule) at run time; per iteration
        the device hands back the four bytes of E and nothing else."""
        if order not in (2, 3):
            raise ValueError("For adaptive step size solver, order must be 2 or 3, got {}".format(order))
        ns = self.ns
        x = x.detach().float().contiguous()
        B = x.shape[0]
        self.model_times, self.adaptive_log, self._err_ws = [], [], None
        value = lambda xx, t: self._model_value(xx, _c((t - 1. / ns.N) * 1000.), _c(ns.alpha(t)), _c(ns.sigma(t)), self.predict_x0)
        s = t_T * torch.ones((1,))
        lambda_s = ns.lam(s)
        lambda_0 = ns.lam(t_0 * torch.ones_like(s))
        h = h_init * torch.ones_like(s)
        x_prev = x
        nfe = 0
        while torch.abs((s - t_0)).repeat(B).mean() > t_err:
            t = ns.inverse_lambda(lambda_s + h)
            model_s = value(x, s)
            if order == 2:
                r1 = 0.5
                x_lower = self._update(_LIN, x, (model_s,), self._first(s, t))
                s1, a, c = self._ss2(s, t, r1, solver_type)
                model_s1 = value(self._update(_LIN, x, (model_s,), a), s1)
                x_higher = self._update(_DIFF, x, (model_s, model_s1, model_s), c)
            else:
                r1, r2 = 1. / 3., 2. / 3.
                s1, a, c = self._ss2(s, t, r1, solver_type)
                model_s1 = value(self._update(_LIN, x, (model_s,), a), s1)
                x_lower = self._update(_DIFF, x, (model_s, model_s1, model_s), c)
                _, s2, _, b, form, c = self._ss3(s, t, r1, r2, solver_type)
                model_s2 = value(self._update(_DIFF, x, (model_s, model_s1, model_s), b), s2)
                x_higher = self._update(form, x, (model_s, model_s2, model_s) if form == _DIFF else (model_s, model_s1, model_s2), c)
            E = self._error(x_higher, x_lower, x_prev, atol, rtol)
            if torch.isnan(E):
                raise FloatingPointError('the adaptive error estimate is NaN (the reference would reject every step from here on)')
            accepted = bool(torch.all(E <= 1.))
            self.adaptive_log.append((float(E), accepted))
            if accepted:
                x = x_higher
                s = t
                x_prev = x_lower
                lambda_s = ns.lam(s)
            h = torch.min(theta * h * torch.float_power(E, -1. / order).float(), lambda_0 - lambda_s)
            nfe += order
        print('adaptive solver nfe', nfe)
        return x

    @torch.no_grad()
    def sample(self, x, steps=20, t_start=None, t_end=None, order=3, skip_type='time_uniform', method='singlestep', lower_order_final=True,
               denoise_to_zero=False, solver_type='dpm_solver', atol=0.0078, rtol=0.05, callback=None):
        """DPM_Solver.sample (:965-1124)"""
        if method != 'adaptive':
            return self.run_plan(x, self.plan(steps, t_start, t_end, order, skip_type, method, lower_order_final, denoise_to_zero,
                                              solver_type), callback)
        t_0 = 1. / self.ns.N if t_end is None else t_end
        t_T = 1. if t_start is None else t_start
        x = self.dpm_solver_adaptive(x, order=order, t_T=t_T, t_0=t_0, atol=atol, rtol=rtol, solver_type=solver_type)
        if denoise_to_zero:
            t = torch.ones((1,)) * t_0
            x = self._model_value(x, _c((t - 1. / self.ns.N) * 1000.), _c(self.ns.alpha(t)), _c(self.ns.sigma(t)), True)
        return x


class DPMSolverSamplerHIP(_SamplerBase):
    """dpm_solver/sampler.py:9-82: `sample(...)` returns (x, None).  Without further keywords it runs what the reference's sampler
    hard-codes -- DPM-Solver++(2M): multistep, order 2, time_uniform, data prediction -- through the fused sdmi_dpm_solver_step;
    with any keyword of DPM_Solver / DPM_Solver.sample (method, order, skip_type, predict_x0, thresholding, max_val, t_start, t_end,
    lower_order_final, denoise_to_zero, solver_type, atol, rtol) it runs DPMSolverHIP with these and the reference sampler's values
    for the rest (steps = S, predict_x0 = True, method 'multistep', order 2, 'time_uniform', lower_order_final = True)."""

    def __init__(self, model, **kwargs):
        super().__init__(model, **kwargs)
        self.alphas_cumprod = model.alphas_cumprod.detach().to(torch.float32)

    def plan(self, S):
        """the scalars of the default run, one row per model evaluation (dpm_plan)"""
        return dpm_plan(_DiscreteVP(self.alphas_cumprod), S)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        if isinstance(conditioning, dict):
            raise NotImplementedError('dict conditioning (hybrid models) is outside the SD-v1 txt2img path')
        if conditioning is not None and conditioning.shape[0] != batch_size:
            print(f'Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}')
        C, H, W = shape
        scale, uc = unconditional_guidance_scale, unconditional_conditioning
        device, b, img, cfg, c_in, x_in = self._prepare(conditioning, (batch_size, C, H, W), x_T, uc, scale)
        if not img.is_cuda:
            raise RuntimeError('the HIP sampler step runs on MI355X device tensors only (no CPU fallback)')
        unet = self._hip_unet()
        opts = {k: kwargs[k] for k in DPM_KEYWORDS + ('predict_x0', 'thresholding', 'max_val') if k in kwargs}
        if opts:
            solver = DPMSolverHIP(lambda x, t_input: self._model_eps(x_in, x, t_input, c_in, cfg, b, t_dtype=torch.float32),
                                  _DiscreteVP(self.alphas_cumprod), predict_x0=opts.pop('predict_x0', True),
                                  thresholding=opts.pop('thresholding', False), max_val=opts.pop('max_val', 1.), cfg=cfg, scale=scale)
            self.solver = solver                # (model_times / adaptive_log of the run)
            opts = dict(dict(steps=S, order=2, skip_type='time_uniform', method='multistep', lower_order_final=True), **opts)
            if unet is not None:
                unet.pin_context(c_in)
            try:
                return solver.sample(img, callback=callback, **opts), None
            finally:
                if unet is not None:
                    unet.unpin_context()
        plan = self.plan(S)
        lib = _lib.load()
        if unet is not None:
            unet.pin_context(c_in)
        try:
            m_prev = None
            for k, (t_input, alpha_s, sigma_s, order, cx, a, inv_r0) in enumerate(plan):
                eps = self._model_eps(x_in, img, t_input, c_in, cfg, b, t_dtype=torch.float32)
                m_new, x_next = torch.empty_like(img), torch.empty_like(img)
                _lib.check(lib.sdmi_dpm_solver_step(eps.data_ptr(), int(cfg), float(scale), img.data_ptr(), _lib.ptr(m_prev),
                                                    alpha_s, sigma_s, cx, a, inv_r0, order, m_new.data_ptr(),
                                                    x_next.data_ptr(), img.numel(), _lib.stream_ptr()))
                m_prev, img = m_new, x_next
                if callback: callback(k)
                if img_callback: img_callback(m_new, k)
        finally:
            if unet is not None:
                unet.unpin_context()
        return img, None
