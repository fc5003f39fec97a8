"""What tools/make_golden_dpm_variants.py (the reference run), tests/test_dpm_variants_host.py, tests/test_dpm_variants_gpu.py and
tools/bench_dpm.py share: the schedule, the stub models, the seeded inputs, the cases of tests/golden/dpm_variants.npz, and the
DPM-Solver loops restated in the reference's torch expressions -- one definition, so that they cannot drift apart.

The stub models are built only of individually rounded fp32 ops that CPU and GPU torch evaluate identically (multiply, add, clamp,
where; no transcendental), so a GPU run over the recorded host scalars equals the reference's CPU run bit for bit."""
import numpy as np
import torch

from ddpm_cases import _normals

SHAPE = (3, 3, 9, 11)            # 891 elements: three full blocks of the elementwise kernels and a tail
COND = (0.5, -0.25, 1.0)         # the "conditioning": one number per sample; the unconditional one is 0
GAP = 1e-2                       # every recorded adaptive error keeps |E - 1| >= GAP: an accept / reject decision is not a rounding matter
ATOL, RTOL = 0.0078, 0.05        # DPM_Solver.sample's defaults


def alphas_cumprod():
    """SD-v1's schedule (configs/stable-diffusion/v1-inference.yaml: linear, 0.00085 .. 0.012, 1000 steps), float64 then fp32"""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return torch.from_numpy(np.cumprod(1. - betas, axis=0).astype(np.float32))


def stub_model(x, t, c):
    """model(x, t_input, cond) of model_wrapper: t the float model-input time [B], c one number per row"""
    h = 0.7 * x + 0.001 * t[:, None, None, None]
    h = torch.clamp(h - 0.4, -1.5, 1.5) * 0.9
    return h + 0.1 * x + c[:, None, None, None] * (0.25 * x)


def kink_model(x, t, c):
    """the stub plus a kink in time: the adaptive solver has to reject steps across it"""
    k = torch.where(t < 400, torch.full_like(t, 0.75), torch.full_like(t, -0.75))
    return stub_model(x, t, c) + k[:, None, None, None] * torch.clamp(x, -1., 1.)


MODELS = {'stub': stub_model, 'kink': kink_model}


def _both(name, scale_x0, scale_eps, **sample):
    return {f'{name}_x0': dict(predict_x0=True, scale=scale_x0, sample=sample), f'{name}_eps': dict(predict_x0=False, scale=scale_eps, sample=sample)}


# name -> predict_x0, guidance scale (None: no guidance), DPM_Solver.sample keywords [, thresholding, max_val]
CASES = {}
for _steps in (3, 4, 5, 6):                                                     # order lists [2,1], [3,1], [3,2], [3,2,1]
    CASES.update(_both(f'ss3_s{_steps}', 3.0, None, steps=_steps, order=3, skip_type='logSNR', method='singlestep'))
CASES.update(_both('ss2_s5', 3.0, None, steps=5, order=2, skip_type='logSNR', method='singlestep'))
CASES.update(_both('ssf3_uniform', None, 3.0, steps=6, order=3, skip_type='time_uniform', method='singlestep_fixed', denoise_to_zero=True))
CASES.update(_both('ssf2_quadratic', 3.0, None, steps=6, order=2, skip_type='time_quadratic', method='singlestep_fixed', denoise_to_zero=True))
CASES.update(_both('ms3_s16', 3.0, 3.0, steps=16, order=3, method='multistep'))
CASES.update(_both('ms3_s7', None, None, steps=7, order=3, method='multistep', lower_order_final=False, skip_type='time_quadratic'))
CASES.update(_both('ms2_t06', 3.0, None, steps=8, order=2, method='multistep', t_start=0.6))
CASES.update(_both('ms1', None, 3.0, steps=5, order=1, method='multistep'))
CASES.update(_both('ss3_s6_taylor', 3.0, None, steps=6, order=3, skip_type='logSNR', method='singlestep', solver_type='taylor'))
CASES.update(_both('ssf3_taylor', None, None, steps=3, order=3, skip_type='time_uniform', method='singlestep_fixed', solver_type='taylor'))
CASES.update(_both('ms2_taylor', None, 3.0, steps=6, order=2, method='multistep', solver_type='taylor'))
CASES['thresholding'] = dict(predict_x0=True, scale=3.0, thresholding=True, max_val=6.0,
                             sample=dict(steps=6, order=2, method='multistep', denoise_to_zero=True))
ADAPTIVE = {f'ad{o}_{"x0" if p else "eps"}': dict(predict_x0=p, scale=None, model='kink', sample=dict(order=o, method='adaptive'))
            for o in (2, 3) for p in (True, False)}
SINGLESTEP_STEPS = tuple(range(3, 10))       # recorded: the order list and the outer timesteps of method='singlestep', order 3, logSNR


def case_seed(name):
    return 500 + sorted(list(CASES) + list(ADAPTIVE)).index(name)


def case_x(seed, shape=SHAPE):
    return _normals(np.random.RandomState(int(seed) + 7919), shape)


def eps_fn_of(model, scale, calls=None, device='cpu'):
    """the raw-output function DPMSolverHIP takes, over a stub: [uncond rows, cond rows] with guidance, the conditional rows without
    (model_wrapper :336-344).  calls: a list receiving the model-input time of every call"""
    c = torch.tensor(COND, device=device)
    def fn(x, t_input):
        t = torch.full((x.shape[0],), t_input, device=x.device, dtype=torch.float32)
        if calls is not None:
            calls.append(float(t_input))
        if scale is None:
            return model(x, t, c).contiguous()
        return model(torch.cat([x] * 2), torch.cat([t] * 2), torch.cat([torch.zeros_like(c), c])).contiguous()
    return fn


# ---- DPM_Solver restated in the reference's torch expressions, on any device, over host scalars: what a user gets from the reference's
# DPM_Solver over UNetModelHIP -- the generator's cross-check on the CPU, the end-to-end tests' and tools/bench_dpm.py's baseline ------
def torch_model_value(eps, x, cfg, scale, data_prediction, alpha_t, sigma_t, thresholding=False, max_val=1.):
    """model_fn of model_wrapper (:340-344) and DPM_Solver.model_fn / data_prediction_fn (:386-408); alpha_t, sigma_t: 0-dim tensors"""
    if cfg:
        noise_uncond, noise = eps.chunk(2)
        noise = noise_uncond + scale * (noise - noise_uncond)
    else:
        noise = eps
    if not data_prediction:
        return noise
    x0 = (x - sigma_t * noise) / alpha_t
    if thresholding:
        s = torch.quantile(torch.abs(x0).reshape((x0.shape[0], -1)), 0.995, dim=1)
        s = torch.maximum(s, max_val * torch.ones_like(s))[:, None, None, None]
        x0 = torch.clamp(x0, -s, s) / s
    return x0


def torch_update(form, x, ms, c):
    """the four expression trees of sdmi_dpm_update; c: 0-dim tensors on x's device (a tensor divisor divides, a Python one may not)"""
    m0 = ms[0]
    if form == 0:
        return c[0] * x + c[1] * m0
    if form == 1:
        return c[0] * x + c[1] * m0 + c[2] * (c[3] * (ms[1] - ms[2]))
    if form == 2:
        D1_0 = c[4] * (ms[1] - m0)
        D1_1 = c[5] * (ms[2] - m0)
        D1 = (c[6] * D1_0 - c[7] * D1_1) / c[8]
        D2 = 2. * (D1_1 - D1_0) / c[8]
        return c[0] * x + c[1] * m0 + c[2] * D1 + c[3] * D2
    D1_0 = c[4] * (m0 - ms[1])
    D1_1 = c[5] * (ms[1] - ms[2])
    D1 = D1_0 + c[6] * (D1_0 - D1_1)
    D2 = c[7] * (D1_0 - D1_1)
    return c[0] * x + c[1] * m0 + c[2] * D1 + c[3] * D2


def _scalars(coef, device):
    return [torch.tensor(float(v), device=device, dtype=torch.float32) for v in coef]


def torch_plan_loop(plan, x, eps_fn, predict_x0, cfg, scale, thresholding=False, max_val=1.):
    """a DPMPlan (stable_diffusion_amd.samplers) executed with torch elementwise ops on x's device"""
    buf = {0: x}
    for op, coef in zip(plan.ops, plan.coef):
        kind, form, dst, xs = (int(v) for v in op[:4])
        c = _scalars(coef, x.device)
        if kind == 0:
            data = predict_x0 or form == 1
            buf[dst] = torch_model_value(eps_fn(buf[xs], float(coef[1])), buf[xs], cfg, scale, data, c[2], c[3], thresholding and data, max_val)
        else:
            buf[dst] = torch_update(form, buf[xs], [buf[int(m)] for m in op[4:] if m >= 0], c)
    return buf[plan.result]


def torch_adaptive_loop(solver, x, order, t_T=1., t_0=None, h_init=0.05, atol=ATOL, rtol=RTOL, theta=0.9, t_err=1e-5, solver_type='dpm_solver'):
    """dpm_solver_adaptive (:931-963) in torch expressions on x's device; the host scalars come from `solver` (a DPMSolverHIP, whose
    scalar methods run on the CPU).  -> (x, [(E, accepted)], model-input times)"""
    from stable_diffusion_amd.samplers import _c
    ns, dev = solver.ns, x.device
    t_0 = 1. / ns.N if t_0 is None else t_0
    sc = lambda coef: _scalars([_c(v) for v in coef], dev)
    times, log = [], []

    def value(xx, t):
        t_in = _c((t - 1. / ns.N) * 1000.)
        times.append(t_in)
        a, s = _scalars([_c(ns.alpha(t)), _c(ns.sigma(t))], dev)
        return torch_model_value(solver.eps_fn(xx, t_in), xx, solver.cfg, solver.scale, solver.predict_x0, a, s)
    s = t_T * torch.ones((1,))
    lambda_s, lambda_0 = ns.lam(s), ns.lam(t_0 * torch.ones_like(s))
    h = h_init * torch.ones_like(s)
    x_prev = x
    B = x.shape[0]
    while torch.abs((s - t_0)).repeat(B).mean() > t_err:
        t = ns.inverse_lambda(lambda_s + h)
        m = value(x, s)
        if order == 2:
            x_lower = torch_update(0, x, [m], sc(solver._first(s, t)))
            s1, a, c = solver._ss2(s, t, 0.5, solver_type)
            m1 = value(torch_update(0, x, [m], sc(a)), s1)
            x_higher = torch_update(1, x, [m, m1, m], sc(c))
        else:
            r1, r2 = 1. / 3., 2. / 3.
            s1, a, c = solver._ss2(s, t, r1, solver_type)
            m1 = value(torch_update(0, x, [m], sc(a)), s1)
            x_lower = torch_update(1, x, [m, m1, m], sc(c))
            _, s2, _, b, form, c = solver._ss3(s, t, r1, r2, solver_type)
            m2 = value(torch_update(1, x, [m, m1, m], sc(b)), s2)
            x_higher = torch_update(form, x, [m, m2, m] if form == 1 else [m, m1, m2], sc(c))
        delta = torch.max(torch.ones_like(x) * atol, rtol * torch.max(torch.abs(x_lower), torch.abs(x_prev)))
        norm_fn = lambda v: torch.sqrt(torch.square(v.reshape((v.shape[0], -1))).mean(dim=-1, keepdim=True))
        E = norm_fn((x_higher - x_lower) / delta).max().cpu()
        ok = bool(torch.all(E <= 1.))
        log.append((float(E), ok))
        if ok:
            x, s, x_prev = x_higher, t, x_lower
            lambda_s = ns.lam(s)
        h = torch.min(theta * h * torch.float_power(E, -1. / order).float(), lambda_0 - lambda_s)
    return x, log, times


def load_plan(G, name):
    from stable_diffusion_amd.samplers import DPMPlan
    return DPMPlan(G[f'{name}_ops'], G[f'{name}_coef'], G[f'{name}_timesteps'], G[f'{name}_orders'], int(G[f'{name}_result']))
