"""Reference-run goldens for ancestral DDPM sampling and for quantize_x0 in DDIM / PLMS (needs the reference checkout; CPU only):

    python tools/make_golden_ddpm.py [--reference DIR]

Runs the reference's own, unmodified `LatentDiffusion.p_sample_loop` / `progressive_denoising` (ldm/models/diffusion/ddpm.py) and
`DDIMSampler.sample` / `PLMSSampler.sample` with quantize_x0 on the cases of tests/ddpm_cases.py.  Stand-ins, and nothing else:
  * `apply_model`: the stub UNet of tests/ddpm_cases.py (the LatentDiffusion object is made without its constructor -- no UNet, no
    first stage, no config is instantiated -- and `register_schedule` is the reference's);
  * `noise_like` (ddpm.py / ddim.py / plms.py) and `torch.randn_like` (q_sample's draw): seeded sequences, re-drawn by the tests from
    the seeds in the fixture;
  * `first_stage_model.quantize`: tests/vq_ref.py on a seeded codebook, recording every call's indices.
Writes tests/golden/ddpm.npz: the registered buffers of both schedules, the per-step std scalars as p_sample computes them, the seeds,
end points, intermediates and codebook indices.  No weights, no noise tensors.

A flipped codebook index changes a quantized trajectory, so each quantized case searches for a seed at which the reference run itself
is safe: at every look-up the nearest and second-nearest squared distances differ by at least GAP * (|z|^2 + |e|^2).  This is asserted
before the fixture is written and the smallest gap is printed."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import ddpm_cases as DC  # noqa: E402
import vq_ref  # noqa: E402

BUFFERS = ('betas', 'alphas_cumprod', 'alphas_cumprod_prev', 'sqrt_alphas_cumprod', 'sqrt_one_minus_alphas_cumprod',
           'log_one_minus_alphas_cumprod', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_variance',
           'posterior_log_variance_clipped', 'posterior_mean_coef1', 'posterior_mean_coef2')


class _Quantizer:
    """first_stage_model.quantize: VectorQuantizer2's (z_q, loss, (perplexity, min_encodings, indices)); records indices and gaps"""

    def __init__(self, e):
        self.e, self.indices, self.min_gap = e, [], float('inf')

    def quantize(self, z):
        zq, idx = vq_ref.quantize(z, self.e)
        d = vq_ref.distances(z, self.e).double()
        two = torch.topk(d, 2, dim=1, largest=False).values
        zf = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1]).double()
        scale = (zf ** 2).sum(1) + (self.e[idx.reshape(-1)].double() ** 2).sum(1)
        self.min_gap = min(self.min_gap, float(((two[:, 1] - two[:, 0]) / scale).min()))
        self.indices.append(idx.reshape(-1).clone())
        return zq, None, (None, None, idx.reshape(-1))


def make_model(ref_ddpm, schedule, clip_denoised=True, log_every_t=100):
    """a reference LatentDiffusion with its own register_schedule and sampling methods; nothing instantiated from a config"""
    m = ref_ddpm.LatentDiffusion.__new__(ref_ddpm.LatentDiffusion)
    torch.nn.Module.__init__(m)
    m.parameterization, m.v_posterior = 'eps', 0.
    m.clip_denoised, m.log_every_t = clip_denoised, log_every_t
    m.num_timesteps_cond = 1
    s = DC.SCHEDULES[schedule]
    m.register_schedule(beta_schedule='linear', timesteps=s['timesteps'], linear_start=s['linear_start'], linear_end=s['linear_end'])
    assert not m.shorten_cond_schedule
    m.calls = []
    m.apply_model = lambda x, t, c, return_ids=False: (m.calls.append(int(t[0])), DC.stub_unet(x, t, c))[1]
    return m


class _Draws:
    """noise_like / randn_like stand-in handing out a seeded sequence"""

    def __init__(self, seed, n, shape):
        self.seq = DC.draws(seed, n, shape)

    def noise_like(self, shape, device, repeat=False):
        return self.seq.pop(0)

    def randn_like(self, x):
        return self.seq.pop(0)


def run_case(ref_ddpm, name, seed, shape, e=None):
    sched, method, kw = DC.CASES[name]
    kw = dict(kw)
    m = make_model(ref_ddpm, sched, clip_denoised=kw.pop('clip_denoised', True))
    n = DC.n_steps(name)
    x_T, x0, mask = DC.case_inputs(name, seed, shape)
    noise, qn = _Draws(seed, n, shape), _Draws(seed + 1, n, shape)
    if e is not None:
        m.first_stage_model = _Quantizer(e)
    if kw.pop('mask', False):
        kw.update(mask=mask, x0=x0)
    orig = ref_ddpm.noise_like, torch.randn_like
    ref_ddpm.noise_like, torch.randn_like = noise.noise_like, qn.randn_like
    try:
        if method == 'p_sample_loop':
            img, inter = m.p_sample_loop(None, shape, return_intermediates=True, x_T=x_T, verbose=False, **kw)
            assert inter[0] is x_T
            inter = inter[1:]
        else:
            img, inter = m.progressive_denoising(None, shape[1:], verbose=False, batch_size=shape[0], x_T=x_T, **kw)
    finally:
        ref_ddpm.noise_like, torch.randn_like = orig
    assert not noise.seq and len(m.calls) == n and m.calls[-1] == 0 and len(qn.seq) == (0 if 'mask' in kw else n)
    out = {f'{name}_out': img.numpy(), f'{name}_inter': torch.stack(inter).numpy(), f'{name}_seed': np.int64(seed)}
    if e is not None:
        out[f'{name}_idx'] = torch.stack(m.first_stage_model.indices).numpy().astype(np.int16)
    return out, (m.first_stage_model.min_gap if e is not None else None)


def run_qcase(ref, name, seed, e, ref_ddpm):
    kind, eta = DC.QCASES[name]
    mod = ref['ddim'] if kind == 'ddim' else ref['plms']
    m = make_model(ref_ddpm, 'churches')
    m.first_stage_model = _Quantizer(e)
    shape = DC.QSHAPE
    x_T, _, _ = DC.case_inputs(name, seed, shape)
    noise = _Draws(seed, DC.QS + 1, shape)
    smp = (mod.DDIMSampler if kind == 'ddim' else mod.PLMSSampler)(m)
    smp.register_buffer = lambda k, v: setattr(smp, k, v)          # (the reference's moves every table to "cuda")
    orig = mod.noise_like
    mod.noise_like = noise.noise_like
    try:
        img, inter = smp.sample(S=DC.QS, batch_size=shape[0], shape=list(shape[1:]), conditioning=None, verbose=False, x_T=x_T, eta=eta,
                                quantize_x0=True, log_every_t=3)
    finally:
        mod.noise_like = orig
    # torch's CPU sqrt is not the correctly rounded one at every value (9 of the 1000 Churches alphas_cumprod on the recording host, other
    # values on another CPU model), the step kernel's host sqrtf is: the fixture keeps to timesteps where the reference run did not depend on it
    for i in range(DC.QS):
        a_t, a_prev, sig = (torch.full((shape[0], 1, 1, 1), float(getattr(smp, k)[i])) for k in ('ddim_alphas', 'ddim_alphas_prev', 'ddim_sigmas'))
        for v in (a_t, a_prev, 1. - a_prev - sig ** 2):
            assert float(v.sqrt().reshape(-1)[0]) == float(np.sqrt(np.float32(v.reshape(-1)[0].item()))), (name, i)
    n_q = DC.QS + (1 if kind == 'plms' else 0)
    assert len(m.first_stage_model.indices) == n_q and len(m.calls) == n_q
    n_noise = DC.QS + 1 - len(noise.seq)
    out = {f'{name}_out': img.numpy(), f'{name}_pred_x0': torch.stack(inter['pred_x0'][1:]).numpy(), f'{name}_seed': np.int64(seed),
           f'{name}_idx': torch.stack(m.first_stage_model.indices).numpy().astype(np.int16), f'{name}_draws': np.int64(n_noise)}
    return out, m.first_stage_model.min_gap


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', default=os.environ.get('SD_REFERENCE', '/root/reference'))
    args = ap.parse_args()
    import run_reference_script as rrs
    sys.path.insert(0, os.path.abspath(args.reference))
    rrs.install_stubs(False, offline_stubs=True, real_ckpt=False)
    import ldm.models.diffusion.ddim as ref_ddim
    import ldm.models.diffusion.ddpm as ref_ddpm
    import ldm.models.diffusion.plms as ref_plms
    from ldm.modules.diffusionmodules.util import extract_into_tensor
    torch.set_grad_enabled(False)
    out = {}

    # ---- registered buffers and the per-step std exactly as p_sample evaluates it (ddpm.py:1100-1107) on a [b, 1, 1, 1] gather --------
    for sched in DC.SCHEDULES:
        m = make_model(ref_ddpm, sched)
        for k in BUFFERS:
            out[f'{sched}_{k}'] = getattr(m, k).numpy()
        x = torch.zeros(DC.SHAPE)
        stds = {}
        for b in (1, 2, 3, 8):
            stds[b] = np.asarray([float((0.5 * extract_into_tensor(m.posterior_log_variance_clipped, torch.full((b,), i, dtype=torch.long),
                                                                   (b,) + DC.SHAPE[1:])).exp().reshape(-1)[0])
                                  for i in range(m.num_timesteps)], dtype=np.float32)
        same = all(np.array_equal(stds[3], v) for v in stds.values())
        print(f'[{sched}] std[0] {stds[3][0]:.3e} std[-1] {stds[3][-1]:.5f}; independent of the batch size (1, 2, 3, 8): {same}')
        assert same, 'the std scalar depends on how torch\'s CPU exp is called: record the variant per batch size'
        out[f'{sched}_std'] = stds[3]
        del x

    # ---- the plain cases ------------------------------------------------------------------------------------------------------------
    for i, name in enumerate(DC.CASES):
        if DC.CASES[name][2].get('quantize_denoised'):
            continue
        o, _ = run_case(ref_ddpm, name, 100 + i, DC.SHAPE)
        out.update(o)
        print(f'[{name}] end |x| max {np.abs(o[name + "_out"]).max():.3f}, {o[name + "_inter"].shape[0]} intermediates')

    # ---- the quantized cases: a seed at which the reference run keeps GAP at every look-up ------------------------------------------
    def search(run, name):
        best = (-1.0, None)
        for seed in range(1000, 1400):
            o, gap = run(seed)
            best = max(best, (gap, seed))
            if gap >= DC.GAP:
                print(f'[{name}] seed {seed}: smallest relative gap {gap:.3e} >= {DC.GAP:g} over {o[name + "_idx"].size} look-ups, '
                      f'{len(np.unique(o[name + "_idx"]))} distinct codes')
                return o
        raise SystemExit(f'[{name}] no safe seed in 1000..1399 (best gap {best[0]:.3e} at {best[1]})')
    for name in DC.CASES:
        if DC.CASES[name][2].get('quantize_denoised'):
            out.update(search(lambda seed: run_case(ref_ddpm, name, seed, DC.QSHAPE, DC.codebook(seed)), name))
    refs = dict(ddim=ref_ddim, plms=ref_plms)
    for name in DC.QCASES:
        out.update(search(lambda seed: run_qcase(refs, name, seed, DC.codebook(seed), ref_ddpm), name))

    path = os.path.join(ROOT, 'tests', 'golden', 'ddpm.npz')
    np.savez_compressed(path, **out)
    print('written', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
