"""Time the DPM-Solver variants on one MI355X: the SD-v1 UNet (seeded synthetic weights), a 4 x 64 x 64 latent, B = 1 with guidance.

    python tools/bench_dpm.py [--out profiles/bench_dpm_variants.txt]

Per variant (singlestep order 3 at 15 evaluations, multistep order 3 at 20, adaptive order 3) two loops, a host clock around each,
ending in a synchronise:
  (a) DPMSolverSamplerHIP.sample with the variant's keywords -- one model-value launch and one update launch per evaluation;
  (b) the same variant in the reference's torch expressions over the same UNetModelHIP (tests/dpm_cases.py: torch_plan_loop /
      torch_adaptive_loop): what a user gets from the reference's DPM_Solver over this library.  Both take their scalars from the host.
(a) and (b) alternate, three times, after a warm-up of each; reported: ms per model evaluation, every run.
Then the thresholding scale (sdmi_dpm_threshold_scale) against torch.quantile on the device at 4 x 64 x 64 and 3 x 256 x 256, B = 1 and 8:
us per call over 200 calls between two synchronises.  ONE RUN ON ONE BOX: no confidence interval; nothing here is a promise of speed."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    import dpm_cases as DC
    from stable_diffusion_amd import DPMSolverSamplerHIP, LatentDiffusionHIP, UNetModelHIP, _lib
    from stable_diffusion_amd.samplers import DPMSolverHIP, _DiscreteVP
    from stable_diffusion_amd.synthetic import SD_V1_UNET_KWARGS, randomize_
    dev = 'cuda'
    unet = UNetModelHIP(**SD_V1_UNET_KWARGS)
    ld = LatentDiffusionHIP(unet).to(dev).eval()
    randomize_(unet, 0)
    g = torch.Generator().manual_seed(0)
    x_T = torch.randn(1, 4, 64, 64, generator=g).to(dev)
    ctx, uc = torch.randn(1, 77, 768, generator=g).to(dev), torch.randn(1, 77, 768, generator=g).to(dev)
    scale = 7.5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    smp = DPMSolverSamplerHIP(ld)
    c_in = torch.cat([uc, ctx])

    def eps_fn(x, t_input):
        t_in = torch.full((2 * x.shape[0],), t_input, device=x.device, dtype=torch.float32)
        return ld.apply_model(torch.cat([x] * 2), t_in, c_in).float().contiguous()
    ref = DPMSolverHIP(eps_fn, _DiscreteVP(ld.alphas_cumprod.detach().float().cpu()), predict_x0=True, cfg=True, scale=scale)
    hip = lambda **kw: smp.sample(S=kw.pop('steps', 0), batch_size=1, shape=[4, 64, 64], conditioning=ctx, verbose=False, x_T=x_T,
                                  unconditional_guidance_scale=scale, unconditional_conditioning=uc, **kw)[0]
    say(f'bench_dpm: ONE RUN ON ONE BOX ({torch.cuda.get_device_name(0)}); SD-v1 UNet, synthetic weights, B = 1 with guidance {scale}, 4 x 64 x 64, '
        f'data prediction')
    variants = {
        'singlestep-3, 15 evaluations': dict(steps=15, order=3, method='singlestep', skip_type='logSNR'),
        'multistep-3, 20 evaluations': dict(steps=20, order=3, method='multistep', skip_type='time_uniform'),
        'adaptive-3': dict(order=3, method='adaptive'),
    }
    for name, kw in variants.items():
        if kw['method'] == 'adaptive':
            a = lambda: (hip(**kw), len(smp.solver.model_times))[1]
            b = lambda: len(DC.torch_adaptive_loop(ref, x_T, kw['order'])[2])
        else:
            a = lambda: (hip(**kw), len(smp.solver.model_times))[1]
            b = lambda: (DC.torch_plan_loop(ref.plan(**kw), x_T, eps_fn, True, True, scale), kw['steps'])[1]
        a(), b()          # warm: tapes, workspaces, the allocator
        ta, tb = [], []
        for _ in range(args.repeats):
            t, n = timed(a)
            ta.append(t / n)
            na = n
            t, n = timed(b)
            tb.append(t / n)
            nb = n
        per = lambda ts: ' / '.join(f'{t:.3f}' for t in ts)
        say(f'[{name}] ms per model evaluation: (a) HIP loop ({na} evaluations) {per(ta)}   (b) reference expressions ({nb} evaluations) {per(tb)}   '
            f'best (a) / best (b) = {min(ta) / min(tb):.4f}')

    lib = _lib.load()
    for (C, H) in ((4, 64), (3, 256)):
        for B in (1, 8):
            x = torch.randn(B, C * H * H, generator=g).to(dev)
            s = torch.empty(B, device=dev)
            one_hip = lambda: _lib.check(lib.sdmi_dpm_threshold_scale(x.data_ptr(), B, x.shape[1], 1.0, s.data_ptr(), None, _lib.stream_ptr()))

            def one_torch():
                q = torch.quantile(torch.abs(x), 0.995, dim=1)
                return torch.maximum(q, 1.0 * torch.ones_like(q))
            res = []
            for fn in (one_hip, one_torch):
                for _ in range(10):
                    fn()
                t, _ = timed(lambda: [fn() for _ in range(200)])
                res.append(t / 200 * 1e3)
            same = torch.equal(s, one_torch())
            say(f'[thresholding scale {C} x {H} x {H}, B = {B}] us per call: sdmi_dpm_threshold_scale {res[0]:.1f}   torch.abs + quantile + maximum '
                f'{res[1]:.1f}   ratio {res[0] / res[1]:.3f}   equal bits: {same}')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
