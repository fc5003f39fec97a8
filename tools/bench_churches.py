"""Time the unconditional LSUN-Churches model on one MI355X: one batch as scripts/sample_diffusion.py runs it (10 samples, 50
DDIM steps at eta 1.0 on a 4 x 32 x 32 latent -- the UNet sees them as 8 + 2 rows -- and the KL-f8 decode to 256 x 256), and one
UNet call at 8 rows and at 2 rows, with seeded synthetic weights.

    python tools/bench_churches.py [--batch 10] [--steps 50] [--calls 20] [--precision mixed] [--kernels]

Prints one JSON line: ms per UNet call at 8 / 2 rows, ms per batch (sampling, decode), images per second.
--kernels adds, on the same box in the same process: the scale-shift GroupNorm-apply launch against the plain one at the model's
shapes, and the d = 24 / 48 attention launches at 1024 and 256 tokens (us per launch)."""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def kernel_timings(calls=200):
    """us per launch; every pair runs back to back in this process (same box, same clocks)"""
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    s = _lib.stream_ptr()
    res = {}
    g = torch.Generator().manual_seed(0)
    for Cc, HW in ((192, 1024), (384, 256), (384, 64), (768, 16), (768, 4)):
        B = 8
        x = torch.randn(B, HW, Cc, generator=g).cuda()
        gamma, beta = torch.ones(Cc).cuda(), torch.zeros(Cc).cuda()
        rows = (0.25 * torch.randn(B, 2 * Cc, generator=g)).cuda()
        out = torch.empty(B, HW, Cc, dtype=torch.float16, device='cuda')
        n = lib.sdmi_k_groupnorm_ws_floats(B, HW)
        ws = torch.empty(n, device='cuda')

        def run(film):
            _lib.check(lib.sdmi_k_groupnorm_film(x.data_ptr(), None, Cc, 0, B, HW, gamma.data_ptr(), beta.data_ptr(), 1e-5, 1, film,
                                                 2 * Cc, out.data_ptr(), None, None, None, None, ws.data_ptr(), n, s))
        # (statistics + apply + the accumulator memset, both times: the difference is the apply launch's)
        plain = _timed(lambda: run(None), calls)
        film = _timed(lambda: run(rows.data_ptr()), calls)
        plain2 = _timed(lambda: run(None), calls)
        res[f'groupnorm_C{Cc}_HW{HW}_us'] = {'plain': round(1e3 * min(plain, plain2), 2), 'scale_shift': round(1e3 * film, 2)}
    for d, n in ((24, 1024), (48, 256), (48, 64), (96, 16)):
        B, heads = 8, 8
        q = torch.randn(B * heads, n, d, generator=g).half().cuda()
        k = torch.randn(B * heads, n, d, generator=g).half().cuda()
        vt = torch.randn(B * heads, d, (n + 7) // 8 * 8, generator=g).half().cuda()
        out = torch.empty(B, n, heads * d, dtype=torch.float16, device='cuda')
        ms = _timed(lambda: _lib.check(lib.sdmi_k_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), B * heads, heads,
                                                            n, n, vt.shape[2], d, d ** -0.5, s)), calls)
        res[f'attention_d{d}_n{n}_B8_us'] = round(1e3 * ms, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--precision', default='mixed', choices=['mixed', 'full'])
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--unet-only', type=int, default=-1, metavar='N',
                    help='one warm-up call and N more UNet calls at 8 rows, nothing else: under a kernel trace, the difference of two '
                         'such runs divided by the difference of their N is the launch count of one call')
    args = ap.parse_args()
    from bench_inpaint import MFMA_PEAK_TFLOPS, unet_flops
    from stable_diffusion_amd import AutoencoderKLHIP, DDIMSamplerHIP, LatentDiffusionHIP, UNetModelHIP, synthetic
    dev = 'cuda'
    kw = synthetic.CHURCHES_UNET_KWARGS
    unet = UNetModelHIP(**kw, hip_precision=args.precision)
    unet.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], 0))
    unet = unet.to(dev)
    lat = kw['image_size']
    g = torch.Generator().manual_seed(0)
    if args.unet_only >= 0:
        x = torch.randn(8, 4, lat, lat, generator=g).to(dev)
        t = torch.full((8,), 501, dtype=torch.long, device=dev)
        for _ in range(1 + args.unet_only):
            unet(x, t)
        torch.cuda.synchronize()
        print(json.dumps({'metric': 'lsun_churches256_unet_only', 'calls': 1 + args.unet_only}), flush=True)
        return
    ld = LatentDiffusionHIP(unet, **synthetic.CHURCHES_SCHEDULE).to(dev)
    vae = AutoencoderKLHIP(synthetic.CHURCHES_VAE_DDCONFIG, None, 4)
    vae.load_state_dict(synthetic.synthetic_vae_state_dict(synthetic.CHURCHES_VAE_DDCONFIG, 4, 0))
    vae = vae.to(dev)

    # ---- one UNet call at 8 and at 2 rows (replayed launch tapes, as inside the sampling loop) ----
    ms_rows = {}
    for rows in (8, 2):
        x = torch.randn(rows, 4, lat, lat, generator=g).to(dev)
        t = torch.full((rows,), 501, dtype=torch.long, device=dev)
        ms_rows[rows] = _timed(lambda: unet(x, t), args.calls)
    flops = unet_flops(kw, 8, lat, lat)

    # ---- one sample_diffusion.py batch: convsample_ddim + decode_first_stage ----
    sampler = DDIMSamplerHIP(ld)
    scale_factor = 0.2                               # (a scale_by_std model stores 1 / std(z) in its checkpoint; the value costs nothing)

    def batch_once():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        samples, _ = sampler.sample(args.steps, batch_size=args.batch, shape=(4, lat, lat), eta=1.0, verbose=False)
        ev[1].record()
        x_sample = vae.decode(samples, z_scale=1.0 / scale_factor)
        ev[2].record()
        torch.cuda.synchronize()
        return x_sample, [ev[i].elapsed_time(ev[i + 1]) for i in range(2)]

    with contextlib.redirect_stdout(io.StringIO()):
        batch_once()
        out, parts = batch_once()
    res = {'metric': 'lsun_churches256', 'precision': args.precision, 'batch': args.batch, 'latent': lat, 'ddim_steps': args.steps,
           'eta': 1.0, 'ms_per_unet_call_8rows': round(ms_rows[8], 3), 'ms_per_unet_call_2rows': round(ms_rows[2], 3),
           'unet_gflop_per_call_8rows': round(flops / 1e9, 1),
           'unet_mfma_peak_fraction_8rows': round(flops / (ms_rows[8] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
           'ms_per_batch': round(sum(parts), 2), 'ms_sample': round(parts[0], 2), 'ms_decode': round(parts[1], 2),
           'images_per_s': round(args.batch / (sum(parts) * 1e-3), 2), 'image': list(out.shape[-2:]),
           'finite': bool(torch.isfinite(out).all())}
    if args.kernels:
        res['kernels'] = kernel_timings()
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
