"""Reference-run goldens for the sampler pool (needs the reference checkout; CPU only):

    python tools/make_golden_sampler_pool.py --reference DIR

Runs the reference's own, unmodified `DDIMSampler.sample` / `DDIMSampler.decode` / `PLMSSampler.sample` on the six requests of
tests/sampler_pool_cases.py, ONE REQUEST AT A TIME -- the pool's claim is that sharing UNet calls changes nothing.  Stand-ins, and
nothing else:
  * `apply_model`: the stub UNet of tests/sampler_pool_cases.py (the LatentDiffusion object is made without its constructor; its
    `register_schedule` is the reference's);
  * `noise_like` (ddim.py / plms.py): a recorded sequence per request.
Writes tests/golden/sampler_pool.npz: the schedule, every request's inputs and draws, its end point and its logged pred_x0 / x_inter.

The step's table scalars pass through torch's CPU sqrt in the reference run and through the host's sqrtf in the library; torch's is not
the correctly rounded one at every value (tools/make_golden_ddpm.py).  So the schedule's linear_end is searched for a value at which the
reference run did not depend on it at any step of any request, and that is asserted before the fixture is written."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import sampler_pool_cases as PC  # noqa: E402


def make_model(ref_ddpm, linear_end):
    """a reference LatentDiffusion with its own register_schedule; nothing instantiated from a config"""
    m = ref_ddpm.LatentDiffusion.__new__(ref_ddpm.LatentDiffusion)
    torch.nn.Module.__init__(m)
    m.parameterization, m.v_posterior = 'eps', 0.
    m.num_timesteps_cond = 1
    m.register_schedule(beta_schedule='linear', timesteps=PC.TIMESTEPS, linear_start=PC.LINEAR_START, linear_end=linear_end)
    m.calls = []
    m.apply_model = lambda x, t, c, return_ids=False: (m.calls.append(int(x.shape[0])), PC.stub_unet(x, t, c))[1]
    return m


def sqrt_safe(smp, name):
    """torch's CPU sqrt gave the correctly rounded value at every table scalar the request's steps used"""
    b = PC.REQUESTS[name]['samples']
    steps = PC.REQUESTS[name].get('t_start') or len(smp.ddim_alphas)
    for i in range(steps):
        a_t, a_prev, sig = (torch.full((b, 1, 1, 1), float(getattr(smp, k)[i])) for k in ('ddim_alphas', 'ddim_alphas_prev', 'ddim_sigmas'))
        for v in (a_t, a_prev, 1. - a_prev - sig ** 2):
            if float(v.sqrt().reshape(-1)[0]) != float(np.sqrt(np.float32(v.reshape(-1)[0].item()))):
                return False
    return True


def run_request(mods, ref_ddpm, name, linear_end):
    r = PC.REQUESTS[name]
    x_T, c, uc, draws = PC.inputs(name)
    seq = list(draws)
    mod = mods[r['sampler']]
    m = make_model(ref_ddpm, linear_end)
    smp = (mod.DDIMSampler if r['sampler'] == 'ddim' else mod.PLMSSampler)(m)
    smp.register_buffer = lambda k, v: setattr(smp, k, v)          # (the reference's moves every table to "cuda")
    orig = mod.noise_like
    mod.noise_like = lambda shape, device, repeat=False: seq.pop(0)
    kw = dict(unconditional_guidance_scale=r['scale'], unconditional_conditioning=uc if PC.guided(name) else None)
    try:
        if r.get('t_start') is not None:
            smp.make_schedule(ddim_num_steps=r['S'], ddim_eta=0., verbose=False)
            img, inter = smp.decode(x_T, c, r['t_start'], **kw), None
        else:
            img, inter = smp.sample(S=r['S'], batch_size=r['samples'], shape=list(PC.SHAPE), conditioning=c, verbose=False, x_T=x_T,
                                    eta=r.get('eta', 0.), log_every_t=r['log_every_t'], **kw)
    finally:
        mod.noise_like = orig
    assert not seq, (name, len(seq))
    rows = r['samples'] * (2 if PC.guided(name) else 1)
    assert m.calls == [rows] * PC.n_draws(name), (name, m.calls)
    out = {f'{name}_x_T': x_T.numpy(), f'{name}_c': c.numpy(), f'{name}_uc': uc.numpy(), f'{name}_draws': torch.stack(draws).numpy(),
           f'{name}_out': img.numpy()}
    if inter is not None:
        assert inter['x_inter'][0] is x_T
        out[f'{name}_pred_x0'] = torch.stack(inter['pred_x0'][1:]).numpy()
        out[f'{name}_x_inter'] = torch.stack(inter['x_inter'][1:]).numpy()
    return out, sqrt_safe(smp, name), m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', default=os.environ.get('SD_REFERENCE'), help='the reference checkout (or $SD_REFERENCE)')
    args = ap.parse_args()
    if not args.reference:
        ap.error('pass --reference DIR or set SD_REFERENCE')
    import run_reference_script as rrs
    sys.path.insert(0, os.path.abspath(args.reference))
    rrs.install_stubs(False, offline_stubs=True, real_ckpt=False)
    import ldm.models.diffusion.ddim as ref_ddim
    import ldm.models.diffusion.ddpm as ref_ddpm
    import ldm.models.diffusion.plms as ref_plms
    torch.set_grad_enabled(False)
    mods = dict(ddim=ref_ddim, plms=ref_plms)

    for linear_end in [0.0155 + 0.0005 * k for k in range(40)]:
        out, safe = {}, True
        for name in PC.REQUESTS:
            o, ok, m = run_request(mods, ref_ddpm, name, linear_end)
            out.update(o)
            safe = safe and ok
            if not safe:
                break
        if safe:
            break
        print(f'linear_end {linear_end:.4f}: a step of {name} depended on torch\'s sqrt rounding; next')
    else:
        raise SystemExit('no linear_end in the searched range at which every step is independent of the CPU\'s sqrt')
    out['betas'] = m.betas.numpy()
    out['alphas_cumprod'] = m.alphas_cumprod.numpy()
    out['linear_end'] = np.float64(linear_end)
    for name in PC.REQUESTS:
        n_log = out[f'{name}_pred_x0'].shape[0] if f'{name}_pred_x0' in out else 0
        print(f'[{name}] {PC.n_draws(name)} model calls, end |x| max {np.abs(out[name + "_out"]).max():.3f}, {n_log} logged steps')
    path = os.path.join(ROOT, 'tests', 'golden', 'sampler_pool.npz')
    np.savez_compressed(path, **out)
    print(f'linear_end {linear_end:.4f}; written', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
