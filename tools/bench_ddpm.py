"""Time the 1000-step ancestral sampler on one MI355X: the LSUN-Churches UNet (seeded synthetic weights), B = 8, a 4 x 32 x 32 latent.

    python tools/bench_ddpm.py [--steps 1000] [--batch 8] [--out profiles/bench_ddpm.txt]

Per variant (plain, with an inpainting mask, with quantize_denoised) three loops, a host clock around each, ending in a synchronise:
  (a) DDPMSamplerHIP.p_sample_loop -- one fused sdmi_ddpm_step launch per step;
  (b) the same loop in the reference's own torch expressions (tests/ddpm_cases.py: reference_p_sample_loop) over the same UNetModelHIP:
      what a user gets from the reference's LatentDiffusion over this library;
  (c) `steps` bare apply_model calls.
(a) and (b) alternate, twice, so the spread shows; every shape is warmed first.  Reports ms per step and the step overhead (a) - (c),
(b) - (c).  The quantizer is a VQModelInterfaceHIP codebook of the face model's size (8192 codes) at the Churches latent's 4 channels.
Also measures the device memory unet.cache_timesteps() takes for all 1000 timesteps.  ONE RUN ON ONE BOX: no confidence interval."""
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
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import ddpm_cases as DC
    from stable_diffusion_amd import DDPMSamplerHIP, LatentDiffusionHIP, UNetModelHIP, VQModelInterfaceHIP, synthetic
    dev = 'cuda'
    kw = synthetic.CHURCHES_UNET_KWARGS
    unet = UNetModelHIP(**kw)
    unet.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], 0))
    unet = unet.to(dev)
    dd = dict(synthetic.INPAINT_VQ_DDCONFIG, ch=64, ch_mult=[1, 2], num_res_blocks=1, z_channels=4)
    vq = VQModelInterfaceHIP(embed_dim=4, n_embed=8192, ddconfig=dd)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        dict(vq.named_parameters())['quantize.embedding.weight'].copy_(torch.randn(8192, 4, generator=g) * 0.6)
    vq = vq.to(dev)
    ld = LatentDiffusionHIP(unet, first_stage_model=vq, log_every_t=200, **synthetic.CHURCHES_SCHEDULE).to(dev)
    lat = kw['image_size']
    shape = (args.batch, 4, lat, lat)
    x_T = torch.randn(shape, generator=g).to(dev)
    x0 = (torch.randn(shape, generator=g) * 0.5).to(dev)
    mask = torch.ones(args.batch, 1, lat, lat)
    mask[:, :, lat // 4:3 * lat // 4, lat // 4:3 * lat // 4] = 0.            # log_images' centre square (ddpm.py:1326-1330)
    mask = mask.to(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    free0 = torch.cuda.mem_get_info()[0]
    unet(x_T, torch.full((args.batch,), 1, dtype=torch.long, device=dev))            # (packs the weights, sizes the workspace)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    unet.cache_timesteps(range(1000))
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    say(f'bench_ddpm: ONE RUN ON ONE BOX ({torch.cuda.get_device_name(0)}); Churches UNet, B = {args.batch}, 4 x {lat} x {lat}, {args.steps} steps')
    say(f'cache_timesteps(all 1000 timesteps): {(free1 - free2) / 2 ** 20:.1f} MiB of device memory (n x emb_total fp32 rows; '
        f'{(free1 - free2) / 4 / 1000:.0f} floats per timestep); the first forward before it took {(free0 - free1) / 2 ** 20:.1f} MiB')

    smp = DDPMSamplerHIP(ld)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def bare(n):
        x = x_T
        for i in reversed(range(n)):
            ld.apply_model(x, torch.full((args.batch,), i, device=dev, dtype=torch.long), None)

    variants = {'plain': {}, 'mask': dict(mask=mask, x0=x0), 'quantize_denoised': dict(quantize_denoised=True)}
    for name, v in variants.items():
        a = lambda n: smp.p_sample_loop(None, shape, x_T=x_T, verbose=False, timesteps=n, **v)
        b = lambda n: DC.reference_p_sample_loop(ld, None, shape, x_T, None, timesteps=n, clip_denoised=ld.clip_denoised, **v)
        for fn in (a, b, bare):          # warm every shape: tapes, workspaces, the allocator
            fn(5)
        ta, tb, tc = [], [], []
        for _ in range(2):
            ta.append(timed(lambda: a(args.steps)))
            tb.append(timed(lambda: b(args.steps)))
        for _ in range(2):
            tc.append(timed(lambda: bare(args.steps)))
        per = lambda ts: ' / '.join(f'{t / args.steps:.4f}' for t in ts)
        ma, mb, mc = (min(t) / args.steps for t in (ta, tb, tc))
        say(f'[{name}] ms per step, two runs each: (a) DDPMSamplerHIP {per(ta)}   (b) reference expressions {per(tb)}   (c) bare UNet calls {per(tc)}')
        say(f'[{name}] step overhead over the bare call (best of two): (a) - (c) = {1e3 * (ma - mc):.1f} us   (b) - (c) = {1e3 * (mb - mc):.1f} us   '
            f'(a) / (b) = {ma / mb:.4f}')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
