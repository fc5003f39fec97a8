"""What tools/make_golden_ddpm.py (the reference run), tests/test_ddpm_host.py and tests/test_ddpm_gpu.py share: the schedules, the
stub model, the seeded draws and the cases of tests/golden/ddpm.npz -- one definition, so that the three cannot drift apart.

The stub UNet is built only of individually rounded fp32 ops that CPU and GPU torch evaluate identically (scalar multiplies, adds,
clamp, t.float(); no transcendental), so a GPU run with the recorded draws equals the reference's CPU run bit for bit."""
import numpy as np
import torch

SCHEDULES = {'churches': dict(timesteps=1000, linear_start=0.0015, linear_end=0.0155),      # models/ldm/lsun_churches256/config.yaml:5-6
             's50': dict(timesteps=50, linear_start=0.0015, linear_end=0.25)}
SHAPE = (3, 3, 9, 11)            # 891 elements: three full blocks of the step kernel and a tail
QSHAPE = (2, 3, 5, 7)            # the quantized runs: 70 codebook look-ups per step
CODEBOOK = dict(n_embed=64, D=3, scale=0.6)
GAP = 1e-4                       # nearest vs second-nearest squared distance, relative to |z|^2 + |e|^2 (~1000x the fp32 rounding)

# name -> (schedule, method, keywords); the draws come from the seeds in the fixture
CASES = {
    'full': ('churches', 'p_sample_loop', dict(log_every_t=200)),                               # Churches' own log_every_t; reaches t = 0
    'start_T': ('churches', 'p_sample_loop', dict(start_T=40, log_every_t=10, clip_denoised=False)),
    'mask': ('s50', 'p_sample_loop', dict(mask=True, log_every_t=10)),
    'progressive': ('s50', 'progressive_denoising', dict(temperature=[0.5 + 0.015 * i for i in range(50)], log_every_t=10)),
    'quantized': ('s50', 'p_sample_loop', dict(quantize_denoised=True, log_every_t=10)),
    'quantized_progressive': ('s50', 'progressive_denoising', dict(quantize_denoised=True, start_T=20, log_every_t=5)),
}
QCASES = {'ddim_q_eta0': ('ddim', 0.0), 'ddim_q_eta05': ('ddim', 0.5), 'plms_q': ('plms', 0.0)}      # quantize_x0, S = QS on 'churches'
QS = 8           # (the eight timesteps at which torch's CPU sqrt is the correctly rounded one: tools/make_golden_ddpm.py asserts it)


def betas_of(schedule):
    """make_beta_schedule('linear', ...) (ldm/modules/diffusionmodules/util.py:21-25): float64"""
    s = SCHEDULES[schedule]
    return np.linspace(s['linear_start'] ** 0.5, s['linear_end'] ** 0.5, s['timesteps'], dtype=np.float64) ** 2


def stub_unet(x, t, c=None):
    h = 0.7 * x + 0.001 * t.float()[:, None, None, None]
    h = torch.clamp(h - 0.4, -1.5, 1.5) * 0.9
    return h + 0.1 * x


def _normals(rs, shape):
    """approximately normal draws (twelve uniforms summed, minus 6) out of exactly rounded operations alone: the same bits on every
    machine, which torch.randn's vectorised log / cos and numpy's normal() do not promise across CPU models"""
    u = rs.random_sample((12,) + tuple(shape))
    acc = u[0]
    for k in range(1, 12):
        acc = acc + u[k]
    return torch.from_numpy((acc - 6.0).astype(np.float32))


def draws(seed, n, shape):
    """n seeded draws of `shape`"""
    rs = np.random.RandomState(int(seed))
    return [_normals(rs, shape) for _ in range(n)]


def codebook(seed):
    rs = np.random.RandomState(int(seed) + 104729)
    return _normals(rs, (CODEBOOK['n_embed'], CODEBOOK['D'])) * CODEBOOK['scale']


def case_inputs(name, seed, shape):
    """x_T and, for the mask case, x0 / mask [B, 1, H, W] -- from the case's seed"""
    rs = np.random.RandomState(int(seed) + 7919)
    x_T = _normals(rs, shape)
    x0 = _normals(rs, shape) * 0.5
    mask = torch.from_numpy((rs.random_sample((shape[0], 1, shape[2], shape[3])) > 0.5).astype(np.float32))
    return x_T, x0, mask


def n_steps(name):
    sched, _, kw = CASES[name]
    return min(SCHEDULES[sched]['timesteps'], kw.get('start_T') or 10 ** 9)


class StubModel:
    """the reference LatentDiffusion's surface: registered buffers, num_timesteps, apply_model (the stub UNet), first_stage_model"""
    parameterization = 'eps'

    def __init__(self, G, sched, device='cpu', clip_denoised=True, log_every_t=100, e=None, quantize=None):
        """e: the codebook of a quantized case; quantize: z -> (z_q, idx), by default tests/vq_ref.py on e"""
        from stable_diffusion_amd.samplers import DDPM_TABLES
        import vq_ref
        for k in DDPM_TABLES:
            setattr(self, k, torch.from_numpy(G[f'{sched}_{k}']).to(device))
        self.num_timesteps = int(self.betas.shape[0])
        self.clip_denoised, self.log_every_t = clip_denoised, log_every_t
        self.calls, self.indices = [], []
        if e is not None:
            self.first_stage_model = self
            self._quantize = quantize or (lambda z: vq_ref.quantize(z, e))

    def apply_model(self, x, t, c):
        self.calls.append(int(t[0]))
        return stub_unet(x, t, c)

    def quantize(self, z):
        zq, idx = self._quantize(z)
        self.indices.append(idx.reshape(-1).cpu())
        return zq, None, (None, None, idx.reshape(-1))


def run_case(G, name, model_of, sampler_of, device='cpu'):
    """the case `name` of tests/ddpm_cases.py on a sampler; -> (model, end point, stacked intermediates)"""
    sched, method, kw = CASES[name]
    kw = dict(kw)
    seed = int(G[f'{name}_seed'])
    quant = bool(kw.get('quantize_denoised'))
    shape = QSHAPE if quant else SHAPE
    model = model_of(sched, clip_denoised=kw.pop('clip_denoised', True), e=codebook(seed) if quant else None)
    smp = sampler_of(model)
    # the reference run's exp(0.5 logvar) scalars are part of the fixture like its draws: torch's CPU exp gives other last bits on
    # another CPU model (same build: 23 of the 1000 Churches values between two hosts), so the sampler's own table -- held against the
    # recorded one in tests/test_ddpm_host.py -- is not what a trajectory recorded elsewhere can be compared through
    smp._std = np.asarray(G[f'{sched}_std'])
    n = n_steps(name)
    x_T, x0, mask = (v.to(device) for v in case_inputs(name, seed, shape))
    seq, qseq = [v.to(device) for v in draws(seed, n, shape)], [v.to(device) for v in draws(seed + 1, n, shape)]
    smp._noise_like = lambda shape, device: seq.pop(0)
    smp._q_noise_like = lambda x0: qseq.pop(0)
    blend = kw.pop('mask', False)
    if blend:
        kw.update(mask=mask, x0=x0)
    if method == 'p_sample_loop':
        img, inter = smp.p_sample_loop(None, shape, return_intermediates=True, x_T=x_T, verbose=False, **kw)
        assert inter[0] is x_T
        inter = inter[1:]
    else:
        img, inter = smp.progressive_denoising(None, shape[1:], verbose=False, batch_size=shape[0], x_T=x_T, **kw)
    assert not seq and len(qseq) == (0 if blend else n) and len(model.calls) == n and model.calls[0] == n - 1 and model.calls[-1] == 0
    return model, img, torch.stack(inter)



# ---- the ancestral loop in the reference's own torch expressions (ddpm.py:216-229, :1047-1107, :1165-1214), on any device: the e2e
# test's and tools/bench_ddpm.py's baseline -- what a user gets from the reference's LatentDiffusion over UNetModelHIP -----------------
def _extract(a, t, x_shape):
    b, *_ = t.shape
    return a.gather(-1, t).reshape(b, *((1,) * (len(x_shape) - 1)))


def reference_p_sample_loop(model, cond, shape, x_T, noises, timesteps=None, start_T=None, clip_denoised=True, quantize_denoised=False,
                            mask=None, x0=None, q_noises=None, std_on_cpu=False):
    """model: the registered buffers, apply_model, first_stage_model; noises / q_noises: lists handed out in order, or None to draw
    from the device RNG as noise_like / q_sample's randn_like do"""
    device = model.betas.device
    b = shape[0]
    img = x_T
    timesteps = model.num_timesteps if timesteps is None else timesteps
    if start_T is not None:
        timesteps = min(timesteps, start_T)
    noises, q_noises = (None if noises is None else list(noises)), (None if q_noises is None else list(q_noises))
    for i in reversed(range(0, timesteps)):
        t = torch.full((b,), i, device=device, dtype=torch.long)
        x = img
        model_out = model.apply_model(x, t, cond)
        x_recon = (_extract(model.sqrt_recip_alphas_cumprod, t, x.shape) * x -
                   _extract(model.sqrt_recipm1_alphas_cumprod, t, x.shape) * model_out)
        if clip_denoised:
            x_recon.clamp_(-1., 1.)
        if quantize_denoised:
            x_recon, _, [_, _, indices] = model.first_stage_model.quantize(x_recon)
        model_mean = (_extract(model.posterior_mean_coef1, t, x.shape) * x_recon +
                      _extract(model.posterior_mean_coef2, t, x.shape) * x)
        model_log_variance = _extract(model.posterior_log_variance_clipped, t, x.shape)
        noise = (torch.randn(x.shape, device=device) if noises is None else noises.pop(0)) * 1.          # (* temperature)
        nonzero_mask = (1 - (t == 0).float()).reshape(b, *((1,) * (len(x.shape) - 1)))
        if std_on_cpu:      # exp is the one transcendental of the step: evaluated where the reference run of the goldens evaluated it
            std = (0.5 * model_log_variance.cpu()).exp().to(device)
        else:
            std = (0.5 * model_log_variance).exp()
        img = model_mean + nonzero_mask * std * noise
        if mask is not None:
            img_orig = (_extract(model.sqrt_alphas_cumprod, t, x0.shape) * x0 +
                        _extract(model.sqrt_one_minus_alphas_cumprod, t, x0.shape) *
                        (torch.randn_like(x0) if q_noises is None else q_noises.pop(0)))
            img = img_orig * mask + (1. - mask) * img
    return img
