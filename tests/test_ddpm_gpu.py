"""Ancestral DDPM sampling on the GPU: sdmi_ddpm_step and the split PLMS / DDIM step bit for bit against the reference's expressions,
DDPMSamplerHIP / quantize_x0 trajectories against the reference runs of tests/golden/ddpm.npz (tools/make_golden_ddpm.py), and the
loop end to end through UNetModelHIP against the same loop in the reference's torch expressions."""
import os

import numpy as np
import pytest
import torch

import ddpm_cases as DC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N = 3 * 3 * 9 * 11          # three full blocks and a tail


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'ddpm.npz'))


def same(a, b):
    """torch.equal, with a NaN equal to a NaN"""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def ddpm_step(eps, x0_in, x, sc, clip, s, noise, blend, x0_out, x_prev):
    from stable_diffusion_amd import _lib
    p = lambda t: None if t is None else t.data_ptr()
    m, xo, qn = blend or (None, None, None)
    _lib.check(_lib.load().sdmi_ddpm_step(p(eps), p(x0_in), p(x), sc['c_recip'], sc['c_recipm1'], int(clip), sc['coef1'], sc['coef2'], s,
                                          p(noise), p(m), p(xo), p(qn), sc['sa'], sc['s1ma'], p(x0_out), p(x_prev), x.numel(),
                                          _lib.stream_ptr()))
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def step_inputs():
    g = torch.Generator().manual_seed(31)
    r = lambda scale=1.0: (torch.randn(N, generator=g) * scale).to(DEV)
    x, eps, noise, x0o, qn = r(2.0), r(), r(), r(0.5), r()
    x[5], eps[700] = float('nan'), float('nan')                          # a NaN stays NaN through the clamp
    x[6], x[7], x[890] = 40.0, -40.0, 9.0                                # far outside +-1, the last element of the tail included
    mask = (torch.rand(N, generator=g) > 0.5).float().to(DEV)
    sc = dict(c_recip=1.3512345, c_recipm1=0.9087654, coef1=0.0123456, coef2=0.9871234, sa=0.7400821, s1ma=0.6725318)
    return dict(x=x, eps=eps, noise=noise, blend=(mask, x0o, qn), sc=sc)


def reference_step(I, clip, s, blend):
    """ddpm.py:216-229, :1066-1067, :1107, :1204-1205 op by op, on the device"""
    T = lambda v: torch.tensor(v, device=DEV)
    sc, x = I['sc'], I['x']
    x0 = T(sc['c_recip']) * x - T(sc['c_recipm1']) * I['eps']
    if clip:
        x0.clamp_(-1., 1.)
    mean = T(sc['coef1']) * x0 + T(sc['coef2']) * x
    xp = mean + T(s) * I['noise']
    if blend:
        mask, x0o, qn = I['blend']
        img_orig = T(sc['sa']) * x0o + T(sc['s1ma']) * qn
        xp = img_orig * mask + (1. - mask) * xp
    return x0, xp


@pytest.mark.parametrize('want_x0', [False, True])
@pytest.mark.parametrize('blend', [False, True])
@pytest.mark.parametrize('s', [0.0, 0.1245])
@pytest.mark.parametrize('clip', [False, True])
def test_ddpm_step_bit_exact(step_inputs, clip, s, blend, want_x0):
    I = step_inputs
    x0_ref, xp_ref = reference_step(I, clip, s, blend)
    assert x0_ref.isnan().sum() == 2 and (x0_ref.abs() > 1).any() != clip
    x0 = torch.full_like(I['x'], 7.0) if want_x0 else None
    xp = torch.full_like(I['x'], 7.0)
    ddpm_step(I['eps'], None, I['x'], I['sc'], clip, s, I['noise'], I['blend'] if blend else None, x0, xp)
    assert same(xp, xp_ref)
    if want_x0:
        assert same(x0, x0_ref)


@pytest.mark.parametrize('blend', [False, True])
def test_ddpm_step_in_place_and_partial_forms(step_inputs, blend):
    I = step_inputs
    x0_ref, xp_ref = reference_step(I, True, 0.1245, blend)
    b = I['blend'] if blend else None
    x = I['x'].clone()
    ddpm_step(I['eps'], None, x, I['sc'], True, 0.1245, I['noise'], b, None, x)              # x_prev is x
    assert same(x, xp_ref)
    # up to x0 only, then from that x0 (the identity in the quantizer's place): the fused step's bits
    x0, xp = torch.full_like(I['x'], 7.0), torch.full_like(I['x'], 7.0)
    ddpm_step(I['eps'], None, I['x'], I['sc'], True, 0.1245, None, None, x0, None)
    assert same(x0, x0_ref) and bool((xp == 7.0).all())
    ddpm_step(None, x0, I['x'], I['sc'], True, 0.1245, I['noise'], b, None, xp)
    assert same(xp, xp_ref)


@pytest.mark.parametrize('cfg', [0, 1])
@pytest.mark.parametrize('mode', [0, 1, 2, 3, 4])
def test_split_sampler_step_equals_the_fused_one(mode, cfg):
    """sdmi_sampler_step_x0 + sdmi_sampler_step_from_x0 with nothing in between == sdmi_sampler_step on the same inputs"""
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(17 + mode)
    r = lambda n=N: torch.randn(n, generator=g).to(DEV)
    eps, x, noise = r(2 * N if cfg else N), r() * 3, r()
    old = [r() for _ in range({0: 0, 1: 1, 2: 2, 3: 3, 4: 1}[mode])]
    o = [t.data_ptr() for t in old] + [None] * 3
    a_t, a_prev, sigma, s1m, scale = 0.5212, 0.5877, 0.2311, float(np.sqrt(np.float32(1.0 - 0.5212))), 7.5
    e1, xp1, p1 = (torch.empty_like(x) for _ in range(3))
    _lib.check(lib.sdmi_sampler_step(eps.data_ptr(), cfg, scale, x.data_ptr(), mode, o[0], o[1], o[2], a_t, a_prev, sigma, s1m,
                                     noise.data_ptr(), e1.data_ptr(), xp1.data_ptr(), p1.data_ptr(), N, _lib.stream_ptr()))
    e2, ep, p2 = (torch.empty_like(x) for _ in range(3))
    xp2 = torch.full_like(x, 7.0)
    _lib.check(lib.sdmi_sampler_step_x0(eps.data_ptr(), cfg, scale, x.data_ptr(), mode, o[0], o[1], o[2], a_t, s1m, e2.data_ptr(),
                                        ep.data_ptr(), p2.data_ptr(), N, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(e1, e2) and torch.equal(p1, p2) and bool((xp2 == 7.0).all())
    if mode == 0:
        assert torch.equal(ep, e1)
    _lib.check(lib.sdmi_sampler_step_from_x0(p2.data_ptr(), ep.data_ptr(), a_prev, sigma, noise.data_ptr(), xp2.data_ptr(), N,
                                             _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(xp1, xp2)
    # ... and against the reference's expressions (ddim.py:198-204), on the host as tests/test_kernels_gpu.py evaluates them
    T = lambda v: torch.full((1, 1, 1, 1), v)
    dir_xt = (1. - T(a_prev) - T(sigma) ** 2).sqrt() * ep.cpu()
    ref = T(a_prev).sqrt() * p2.cpu() + dir_xt + T(sigma) * noise.cpu()
    assert torch.equal(xp2.cpu(), ref.reshape(-1))


# ---- trajectories against the reference runs ------------------------------------------------------------------------------------
def _vq(e):
    """VQModelInterfaceHIP (its quantizer is sdmi_k_vq_quantize) holding the codebook e"""
    from stable_diffusion_amd import VQModelInterfaceHIP, synthetic
    dd = dict(synthetic.INPAINT_VQ_DDCONFIG, ch=64, ch_mult=[1, 2], num_res_blocks=1, z_channels=e.shape[1])
    vq = VQModelInterfaceHIP(embed_dim=e.shape[1], n_embed=e.shape[0], ddconfig=dd)
    with torch.no_grad():
        dict(vq.named_parameters())['quantize.embedding.weight'].copy_(e)
    return vq.cuda()


def _model(G, sched, e=None, **kw):
    if e is None:
        return DC.StubModel(G, sched, device=DEV, **kw)
    vq = _vq(e)

    def quantize(z):
        zq, _, (_, _, idx) = vq.quantize(z)
        return zq, idx
    return DC.StubModel(G, sched, device=DEV, e=e, quantize=quantize, **kw)


@pytest.mark.parametrize('name', list(DC.CASES))
def test_trajectory_equals_the_reference_run(G, name):
    """the stub UNet has no op that differs between CPU and GPU torch, the draws are the recorded ones: bit for bit.  `full` runs the
    1000-step Churches schedule down to t = 0, where posterior_log_variance_clipped is log 1e-20."""
    from stable_diffusion_amd import DDPMSamplerHIP
    model, img, inter = DC.run_case(G, name, lambda sched, **kw: _model(G, sched, **kw), DDPMSamplerHIP, device=DEV)
    if model.indices:       # one flipped index changes the trajectory: every look-up of every step
        idx = torch.stack(model.indices)
        ref = torch.from_numpy(G[f'{name}_idx'].astype(np.int64))
        assert idx.shape == ref.shape and torch.equal(idx, ref), f'{int((idx != ref).sum())} codebook indices differ'
    err = (img.cpu() - torch.from_numpy(G[f'{name}_out'])).abs().max().item()
    print(f'[{name}] {len(model.calls)} steps, max-abs vs the reference run {err:.3e}')
    assert torch.equal(img.cpu(), torch.from_numpy(G[f'{name}_out']))
    assert inter.shape == G[f'{name}_inter'].shape and torch.equal(inter.cpu(), torch.from_numpy(G[f'{name}_inter']))


@pytest.mark.parametrize('name', ['start_T', 'mask'])
def test_latent_diffusion_hip_sample_reaches_the_same_result(G, name):
    """LatentDiffusionHIP.sample / sample_log(ddim=False) -> DDPMSamplerHIP: the golden end point of the same case"""
    from stable_diffusion_amd import LatentDiffusionHIP
    from stable_diffusion_amd import samplers
    sched, _, kw = DC.CASES[name]
    seed, n = int(G[f'{name}_seed']), DC.n_steps(name)
    ld = LatentDiffusionHIP(None, conditioning_key=None, clip_denoised=kw.get('clip_denoised', True), log_every_t=kw['log_every_t'],
                            **DC.SCHEDULES[sched]).to(DEV)
    ld.apply_model = lambda x, t, c, return_ids=False: DC.stub_unet(x, t, c)
    x_T, x0, mask = (v.to(DEV) for v in DC.case_inputs(name, seed, DC.SHAPE))
    extra = dict(mask=mask, x0=x0) if kw.get('mask') else {}
    ref = torch.from_numpy(G[f'{name}_out'])
    for call in ('sample', 'sample_log'):
        seq, qseq = [v.to(DEV) for v in DC.draws(seed, n, DC.SHAPE)], [v.to(DEV) for v in DC.draws(seed + 1, n, DC.SHAPE)]
        old = samplers.DDPMSamplerHIP._noise_like, samplers.DDPMSamplerHIP._q_noise_like, samplers.ddpm_step_std
        samplers.ddpm_step_std = lambda lv: np.asarray(G[f'{sched}_std'])          # (recorded with the run: see ddpm_cases.run_case)
        samplers.DDPMSamplerHIP._noise_like = staticmethod(lambda shape, device: seq.pop(0))
        samplers.DDPMSamplerHIP._q_noise_like = staticmethod(lambda x0: qseq.pop(0))
        try:
            if call == 'sample':
                if 'start_T' in kw:          # sample() has no start_T (ddpm.py:1216-1232): its `timesteps` keyword does the same
                    extra = dict(extra, timesteps=kw['start_T'])
                img, inter = ld.sample(None, batch_size=3, return_intermediates=True, x_T=x_T, verbose=False, shape=DC.SHAPE, **extra)
            else:
                img, inter = ld.sample_log(None, 3, False, None, x_T=x_T, verbose=False, shape=DC.SHAPE[1:], **extra)
        finally:
            samplers.DDPMSamplerHIP._noise_like, samplers.DDPMSamplerHIP._q_noise_like, samplers.ddpm_step_std = old
        assert not seq and torch.equal(img.cpu(), ref), call
        assert torch.equal(torch.stack(inter[1:]).cpu(), torch.from_numpy(G[f'{name}_inter'])), call


@pytest.mark.parametrize('name', list(DC.QCASES))
def test_quantize_x0_trajectory_equals_the_reference_run(G, name):
    """DDIMSamplerHIP / PLMSSamplerHIP with quantize_x0 on VQModelInterfaceHIP.quantize: every index, every stored pred_x0, the end point"""
    from stable_diffusion_amd import DDIMSamplerHIP, PLMSSamplerHIP
    kind, eta = DC.QCASES[name]
    seed = int(G[f'{name}_seed'])
    model = _model(G, 'churches', e=DC.codebook(seed))
    smp = (DDIMSamplerHIP if kind == 'ddim' else PLMSSamplerHIP)(model)
    x_T, _, _ = DC.case_inputs(name, seed, DC.QSHAPE)
    seq = [v.to(DEV) for v in DC.draws(seed, DC.QS + 1, DC.QSHAPE)]
    smp._noise_like = lambda shape, device: seq.pop(0)
    img, inter = smp.sample(S=DC.QS, batch_size=DC.QSHAPE[0], shape=list(DC.QSHAPE[1:]), conditioning=None, verbose=False,
                            x_T=x_T.to(DEV), eta=eta, quantize_x0=True, log_every_t=3)
    idx, ref = torch.stack(model.indices), torch.from_numpy(G[f'{name}_idx'].astype(np.int64))
    assert idx.shape == ref.shape and torch.equal(idx, ref), f'{int((idx != ref).sum())} codebook indices differ'
    assert len(model.calls) == DC.QS + (1 if kind == 'plms' else 0)
    assert torch.equal(torch.stack(inter['pred_x0'][1:]).cpu(), torch.from_numpy(G[f'{name}_pred_x0']))
    assert torch.equal(img.cpu(), torch.from_numpy(G[f'{name}_out']))


def test_cpu_and_gpu_exp_of_the_step_std(G):
    """exp is the one transcendental of the step and its last bit is not portable: reports at how many timesteps this host's and the
    device's torch exp differ from the scalars recorded with the reference run (between two hosts with the same build: 23 of 1000 on
    the Churches schedule, the device: 82).  What must hold everywhere: each is within one ulp of the recorded value."""
    from stable_diffusion_amd.samplers import ddpm_step_std
    for sched in DC.SCHEDULES:
        lv, rec = G[f'{sched}_posterior_log_variance_clipped'], G[f'{sched}_std']
        host = ddpm_step_std(lv)
        dev = (0.5 * torch.from_numpy(lv).to(DEV)).exp().cpu().numpy()
        print(f'[{sched}] exp(0.5 logvar) != recorded: host at {int((host != rec).sum())}, device at {int((dev != rec).sum())} of {rec.size} timesteps')
        for v in (host, dev):
            assert np.abs(v.view(np.int32).astype(np.int64) - rec.view(np.int32).astype(np.int64)).max() <= 1


# ---- end to end through UNetModelHIP -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('quantized', [False, True])
def test_end_to_end_with_hip_unet(quantized):
    """the tiny stand-in UNet, an 8 x 8 latent, start_T = 20: DDPMSamplerHIP against the same loop in the reference's torch expressions
    driving the same UNet handle -- the same eps bits go in on both sides, so torch.equal.  (exp, the one transcendental, is taken
    from the host on both sides: see test_cpu_and_gpu_exp_of_the_step_std.)"""
    from oracle.plan import TINY
    from oracle.weights import make_inputs, make_state_dict
    from stable_diffusion_amd import DDPMSamplerHIP, LatentDiffusionHIP, UNetModelHIP
    unet = UNetModelHIP(**TINY.ref_kwargs())
    unet.load_state_dict(make_state_dict(TINY, 0), strict=True)
    vq = None
    if quantized:
        g = torch.Generator().manual_seed(3)
        vq = _vq(torch.randn(64, 4, generator=g) * 0.6)
    ld = LatentDiffusionHIP(unet, first_stage_model=vq).to(DEV)
    x_T, _, ctx = make_inputs(TINY, 2, 8, 8, seed=21)
    x_T, ctx = x_T.to(DEV), ctx.to(DEV)
    noises = [v.to(DEV) for v in DC.draws(5, 20, x_T.shape)]
    smp = DDPMSamplerHIP(ld)
    seq = list(noises)
    smp._noise_like = lambda shape, device: seq.pop(0)
    out = smp.p_sample_loop(ctx, tuple(x_T.shape), x_T=x_T, verbose=False, start_T=20, quantize_denoised=quantized)
    ref = DC.reference_p_sample_loop(ld, ctx, tuple(x_T.shape), x_T, noises, start_T=20, clip_denoised=True, quantize_denoised=quantized,
                                     std_on_cpu=True)
    torch.cuda.synchronize()
    print(f'[e2e tiny quantized={quantized}] |x| max {float(ref.abs().max()):.3f} max-abs {float((out - ref).abs().max()):.3e}')
    assert not seq and torch.isfinite(ref).all() and torch.equal(out, ref)
