"""Ancestral DDPM sampling, host side (no GPU): the schedule tables and per-step scalars of DDPMSamplerHIP against the reference's
registered buffers and recorded values, and DDPMSamplerHIP's own loop -- its kernel call replaced by a torch emulation of
sdmi_ddpm_step's arithmetic, op for op -- against the reference trajectories of tests/golden/ddpm.npz (tools/make_golden_ddpm.py)."""
import os

import numpy as np
import pytest
import torch

import ddpm_cases as DC


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'ddpm.npz'))


@pytest.mark.parametrize('sched', list(DC.SCHEDULES))
def test_tables_equal_the_registered_buffers(G, sched):
    from stable_diffusion_amd.samplers import DDPM_TABLES, ddpm_tables
    tab = ddpm_tables(DC.betas_of(sched))
    assert set(tab) == set(DDPM_TABLES)
    for k in DDPM_TABLES:
        assert tab[k].dtype == np.float32 and np.array_equal(tab[k].view(np.uint32), G[f'{sched}_{k}'].view(np.uint32)), k
    assert tab['posterior_log_variance_clipped'][0] == np.float32(np.log(1e-20)) and tab['posterior_variance'][0] == 0.0


def test_latent_diffusion_hip_registers_them(G):
    from stable_diffusion_amd import LatentDiffusionHIP
    from stable_diffusion_amd.samplers import DDPM_TABLES
    s = DC.SCHEDULES['churches']
    ld = LatentDiffusionHIP(None, conditioning_key=None, **s)
    assert ld.clip_denoised is True and ld.log_every_t == 100 and ld.parameterization == 'eps'
    assert LatentDiffusionHIP(None, conditioning_key=None, clip_denoised=False, log_every_t=200, **s).log_every_t == 200
    for k in DDPM_TABLES:
        assert torch.equal(getattr(ld, k), torch.from_numpy(G[f'churches_{k}'])), k


@pytest.mark.parametrize('sched', list(DC.SCHEDULES))
def test_step_std_equals_the_recorded_scalars(G, sched):
    """exp(0.5 logvar) per step, by the op the reference applies (torch's CPU exp, fp32), against what the reference run recorded: bit for
    bit.  The last bit of that op depends on the CPU model (MKL's vector exp: 23 of the 1000 Churches values differ between two hosts
    with one torch build), so this holds on the CPU model the fixture was recorded on; the trajectory tests take the recorded scalars."""
    from stable_diffusion_amd import DDPMSamplerHIP
    smp = DDPMSamplerHIP(DC.StubModel(G, sched))
    assert smp._std.dtype == np.float32 and np.array_equal(smp._std.view(np.uint32), G[f'{sched}_std'].view(np.uint32))
    n = smp.ddpm_num_timesteps
    assert smp.step_scalars(0)[4] == 0.0 and smp.step_scalars(n - 1)[4] == float(G[f'{sched}_std'][n - 1])      # nonzero_mask
    # a model with betas alone: the tables come from its fp32 betas (the last bit may then differ from the float64 start)
    bare = type('M', (), dict(betas=torch.from_numpy(G[f'{sched}_betas']), num_timesteps=n, apply_model=None))()
    bare.alphas_cumprod = torch.from_numpy(G[f'{sched}_alphas_cumprod'])
    got = DDPMSamplerHIP(bare)._tab['posterior_mean_coef1']
    assert np.allclose(got, G[f'{sched}_posterior_mean_coef1'], rtol=1e-5, atol=0)


def emulate_ddpm_step(eps, x0_in, x, c_recip, c_recipm1, clip, coef1, coef2, s, noise, blend, sa, s1ma):
    """sdmi_ddpm_step (csrc/sampler.hip: ddpm_step_kernel) in torch, one individually rounded fp32 op per kernel statement"""
    T = lambda v: torch.tensor(v, dtype=torch.float32, device=x.device)
    if eps is not None:
        a = T(c_recip) * x
        b = T(c_recipm1) * eps
        x0 = a - b
        if clip:
            x0 = torch.where(x0 < -1., T(-1.), torch.where(x0 > 1., T(1.), x0))
    else:
        x0 = x0_in
    if noise is None:
        return x0, None
    m1 = T(coef1) * x0
    m2 = T(coef2) * x
    mean = m1 + m2
    nz = T(s) * noise
    xp = mean + nz
    if blend is not None:
        mask, x0_orig, q_noise = blend
        q1 = T(sa) * x0_orig
        q2 = T(s1ma) * q_noise
        q = q1 + q2
        qm = q * mask
        om = 1. - mask
        keep = om * xp
        xp = qm + keep
    return x0, xp


def emulated(smp):
    """DDPMSamplerHIP with the two kernel launches of _p_sample replaced by the emulation; the loop is the sampler's own"""
    def _p_sample(img, eps, t, noise, quantize, blend, want_x0):
        c_recip, c_recipm1, coef1, coef2, s, sa, s1ma = smp.step_scalars(t)
        clip = smp.clip_denoised
        if quantize:
            x0, _ = emulate_ddpm_step(eps, None, img, c_recip, c_recipm1, clip, coef1, coef2, s, None, None, sa, s1ma)
            x0 = smp.model.first_stage_model.quantize(x0)[0].float().contiguous()
            _, xp = emulate_ddpm_step(None, x0, img, c_recip, c_recipm1, clip, coef1, coef2, s, noise, blend, sa, s1ma)
        else:
            x0, xp = emulate_ddpm_step(eps, None, img, c_recip, c_recipm1, clip, coef1, coef2, s, noise, blend, sa, s1ma)
        return xp, x0
    smp._p_sample = _p_sample
    return smp


@pytest.mark.parametrize('name', list(DC.CASES))
def test_emulated_loop_reproduces_the_reference(G, name):
    from stable_diffusion_amd import DDPMSamplerHIP
    model, img, inter = DC.run_case(G, name, lambda sched, **kw: DC.StubModel(G, sched, **kw), lambda m: emulated(DDPMSamplerHIP(m)))
    assert torch.equal(img, torch.from_numpy(G[f'{name}_out']))
    assert inter.shape == G[f'{name}_inter'].shape and torch.equal(inter, torch.from_numpy(G[f'{name}_inter']))
    if model.indices:
        assert torch.equal(torch.stack(model.indices), torch.from_numpy(G[f'{name}_idx'].astype(np.int64)))


def test_refusals_name_their_argument(G):
    from stable_diffusion_amd import DDIMSamplerHIP, DDPMSamplerHIP, PLMSSamplerHIP
    m = DC.StubModel(G, 's50')
    smp = DDPMSamplerHIP(m)
    x = torch.zeros(DC.SHAPE)
    with pytest.raises(NotImplementedError, match='score_corrector'):
        smp.progressive_denoising(None, DC.SHAPE, score_corrector=object(), x_T=x, verbose=False)
    with pytest.raises(NotImplementedError, match='dict conditioning'):
        smp.p_sample_loop({'c_concat': [x]}, DC.SHAPE, x_T=x, verbose=False)
    with pytest.raises(NotImplementedError, match='dict conditioning'):
        smp.progressive_denoising({'c_concat': [x]}, DC.SHAPE, x_T=x, verbose=False)
    with pytest.raises(NotImplementedError, match='quantize_denoised'):
        smp.p_sample_loop(None, DC.SHAPE, x_T=x, quantize_denoised=True, verbose=False)
    m.parameterization = 'x0'
    with pytest.raises(NotImplementedError, match='parameterization'):
        DDPMSamplerHIP(m)
    m.parameterization, m.shorten_cond_schedule = 'eps', True
    with pytest.raises(NotImplementedError, match='shorten_cond_schedule'):
        DDPMSamplerHIP(m)
    m.shorten_cond_schedule = False
    with pytest.raises(RuntimeError, match='no CPU fallback'):         # the real step is a kernel: a CPU tensor is an error
        smp.p_sample_loop(None, DC.SHAPE, x_T=x, verbose=False)
    for cls in (DDIMSamplerHIP, PLMSSamplerHIP):
        with pytest.raises(NotImplementedError, match='score_corrector'):
            cls(m).sample(S=5, batch_size=3, shape=DC.SHAPE[1:], score_corrector=object(), verbose=False)
        with pytest.raises(NotImplementedError, match='quantize_x0'):
            cls(m).sample(S=5, batch_size=3, shape=DC.SHAPE[1:], quantize_x0=True, verbose=False)


def test_abi_is_additive():
    from stable_diffusion_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sdmi.h')).read()
    lib = _lib.load()
    for name in ('sdmi_ddpm_step', 'sdmi_sampler_step_x0', 'sdmi_sampler_step_from_x0'):
        assert name in _lib.exported_symbols() and name + '(' in hdr and hasattr(lib, name)
    assert '#define SDMI_ABI_VERSION 17' in hdr and lib.sdmi_abi_version() == 17
    # launcher checks, in launch_sampler_step's style: they fail before anything is launched
    assert lib.sdmi_ddpm_step(None, None, None, 1., 0., 0, 0., 1., 0., None, None, None, None, 1., 0., None, None, 891, None) != 0
    assert b'ddpm_step' in lib.sdmi_last_error()
    assert lib.sdmi_ddpm_step(8, 8, 8, 1., 0., 0, 0., 1., 0., 8, None, None, None, 1., 0., None, 8, 891, None) != 0
    assert b'exactly one of eps / x0_in' in lib.sdmi_last_error()
    assert lib.sdmi_ddpm_step(8, None, 8, 1., 0., 0, 0., 1., 0., None, None, None, None, 1., 0., None, 8, 891, None) != 0
    assert b'noise missing' in lib.sdmi_last_error()
    assert lib.sdmi_ddpm_step(8, None, 8, 1., 0., 0, 0., 1., 0., 8, 8, None, None, 1., 0., None, 8, 891, None) != 0
    assert b'the blend needs' in lib.sdmi_last_error()
    assert lib.sdmi_sampler_step_from_x0(None, 8, 1., 0., None, 8, 891, None) != 0
    assert lib.sdmi_sampler_step_x0(8, 0, 1., 8, 0, None, None, None, 1., 0., None, None, 8, 891, None) != 0     # ep_out is required
