"""Time the class-conditional ImageNet model on one MI355X as the cell of scripts/latent_imagenet_diffusion.ipynb runs it:
6 samples of one class, classifier-free guidance (scale 3.0, class 1000 as the unconditional label), 20 DDIM steps, eta 0,
decode -- 12 rows per UNet call = library calls of 8 + 4 rows -- with seeded synthetic weights.

    python tools/bench_cin.py [--samples 6] [--steps 20] [--calls 10] [--rounds 5] [--profile-only]

Prints one JSON line: ms per 12-row UNet call with the one-token collapse of attn2 and with SDMI_CTX1=0 (the same call, alternating,
median of the rounds), ms per cell and images/s.  --profile-only runs 2 x `calls` UNet calls at the default setting and nothing else (for a kernel trace)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=6)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--cls', type=int, default=25)
    ap.add_argument('--profile-only', action='store_true')
    args = ap.parse_args()
    from stable_diffusion_amd import ClassEmbedderHIP, DDIMSamplerHIP, LatentDiffusionHIP, UNetModelHIP, VQModelInterfaceHIP, synthetic
    dev = 'cuda'

    def seeded(m):
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0))
        return m.to(dev)
    unet = seeded(UNetModelHIP(**synthetic.CIN_UNET_KWARGS))
    vq = seeded(VQModelInterfaceHIP(**synthetic.CIN_VQ_KWARGS))
    emb = seeded(ClassEmbedderHIP(**synthetic.CIN_CLASS_KWARGS))
    ld = LatentDiffusionHIP(unet, **synthetic.CIN_SCHEDULE).to(dev)
    n = args.samples
    with torch.no_grad():
        uc = emb({'class_label': torch.tensor(n * [1000], device=dev)})
        c = emb({'class_label': torch.tensor(n * [args.cls], device=dev)})
    ev = lambda: torch.cuda.Event(enable_timing=True)

    # ---- one 2n-row UNet call (what the sampler issues per step), with and without the collapse ----
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2 * n, 3, 64, 64, generator=g).to(dev)
    t = torch.full((2 * n,), 501, dtype=torch.long, device=dev)
    ctx = torch.cat([uc, c])

    def calls(env):
        if env is None:
            os.environ.pop('SDMI_CTX1', None)
        else:
            os.environ['SDMI_CTX1'] = env
        a, b = ev(), ev()
        a.record()
        for _ in range(args.calls):
            unet(x, t, context=ctx)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.calls
    if args.profile_only:                      # (the default setting only: a kernel trace of the path the sampler takes)
        calls(None)
        calls(None)
        return
    for env in (None, '0', None, '0'):
        calls(env)
    on, off = [], []
    for _ in range(args.rounds):
        on.append(calls(None))
        off.append(calls('0'))
    os.environ.pop('SDMI_CTX1', None)

    # ---- the notebook's cell ----
    sampler = DDIMSamplerHIP(ld)

    def cell():
        a, b, d = ev(), ev(), ev()
        a.record()
        samples, _ = sampler.sample(S=args.steps, conditioning=c, batch_size=n, shape=[3, 64, 64], verbose=False,
                                    unconditional_guidance_scale=3.0, unconditional_conditioning=uc, eta=0.0)
        b.record()
        img = torch.clamp((vq.decode(samples) + 1.0) / 2.0, min=0.0, max=1.0)
        d.record()
        torch.cuda.synchronize()
        return img, a.elapsed_time(b), b.elapsed_time(d)
    with contextlib.redirect_stdout(io.StringIO()):
        cell()
        runs = [cell() for _ in range(3)]
    ms_s, ms_d = statistics.median(r[1] for r in runs), statistics.median(r[2] for r in runs)
    res = {'metric': 'cin256_v2', 'samples': n, 'rows_per_unet_call': 2 * n, 'ddim_steps': args.steps,
           'ms_per_unet_call_collapse': round(statistics.median(on), 3), 'ms_per_unet_call_ctx1_0': round(statistics.median(off), 3),
           'collapse_series_ms': [round(v, 3) for v in on], 'ctx1_0_series_ms': [round(v, 3) for v in off],
           'ms_sample': round(ms_s, 2), 'ms_decode': round(ms_d, 2), 'images_per_s': round(n / ((ms_s + ms_d) * 1e-3), 2),
           'finite': bool(torch.isfinite(runs[-1][0]).all())}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
