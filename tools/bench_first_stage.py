"""Time the SD first stage in both precisions, and the wide-head split-fp16 attention kernel alone, on one MI355X.

    python tools/bench_first_stage.py [--iters 5] [--rounds 5] [--out profiles/bench_first_stage_full.txt]

First stage: AutoencoderKLHIP with SD v1's ddconfig and seeded random weights, B = 1: decode of a 64 x 64 latent (a 512 x 512 image)
and encode of a 512 x 512 image.  hip_precision='mixed' and 'full' live in one process and are timed alternately, `rounds` times
`iters` back-to-back calls between two events; the median round is reported.
Kernel: sdmi_k_attention_split16 at d = 512 (csrc/attn_wide_split16.hip), one head, 4096 and 1024 tokens (the mid block at a
64 x 64 and a 32 x 32 latent).  There is no speed bar on this mode: the numbers are reported, not promised."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fns, iters, rounds):
    """alternate the callables; median ms per call of each"""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    acc = [[] for _ in fns]
    for _ in range(rounds):
        for fn, a in zip(fns, acc):
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            a.append(e0.elapsed_time(e1) / iters)
    return [statistics.median(a) for a in acc]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    from stable_diffusion_amd import AutoencoderKLHIP, _lib
    from stable_diffusion_amd.synthetic import SD_V1_VAE_DDCONFIG, synthetic_vae_state_dict
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f'# {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds x {args.iters} calls, mixed and full alternating in one process')
    sd = synthetic_vae_state_dict(SD_V1_VAE_DDCONFIG, 4, 0)
    models = {}
    for prec in ('mixed', 'full'):
        m = AutoencoderKLHIP(SD_V1_VAE_DDCONFIG, None, 4, hip_precision=prec)
        m.load_state_dict(sd, strict=True)
        models[prec] = m.cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(0)
    lat = torch.randn(1, 4, 64, 64, device='cuda', generator=g) * 5.0
    img = torch.rand(1, 3, 512, 512, device='cuda', generator=g) * 2 - 1
    say('# SD first stage, B = 1              mixed_ms   full_ms  full/mixed  max-abs(full - mixed)')
    for name, call, x in (('decode 64x64 latent -> 512x512', 'decode', lat), ('encode 512x512 image -> 64x64', 'encode_moments', img)):
        fns = [lambda p=prec: getattr(models[p], call)(x) for prec in ('mixed', 'full')]
        outs = [fn() for fn in fns]
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        diff = float((outs[0] - outs[1]).abs().max())
        tm, tf = _time(fns, args.iters, args.rounds)
        say(f'{name:34s} {tm:9.2f} {tf:9.2f} {tf / tm:11.2f}  {diff:.2e}')

    lib = _lib.load()
    s = _lib.stream_ptr()
    say('# sdmi_k_attention_split16 alone (csrc/attn_wide_split16.hip), BH = 1, one head')
    say('# tokens d_head      ms   TFLOP/s (algorithmic: 4 n^2 d; the kernel executes three MFMA passes of it)')
    for n, d in ((4096, 512), (1024, 512)):
        q, k, vt = (torch.randn(shape, device='cuda', generator=g) for shape in ((1, n, d), (1, n, d), (1, d, n)))
        ops = []
        for t in (q, k, vt):
            hi = t.half()
            ops += [hi, (t - hi.float()).half()]
        out, out_lo = (torch.empty(1, n, d, dtype=torch.float16, device='cuda') for _ in range(2))

        def attend():
            _lib.check(lib.sdmi_k_attention_split16(*[o.data_ptr() for o in ops], out.data_ptr(), out_lo.data_ptr(), 1, 1, n, n, n, d,
                                                    d ** -0.5, s))
        for _ in range(3):
            attend()
        torch.cuda.synchronize()
        (ms,) = _time([attend], max(args.iters, 10), args.rounds)
        say(f'{n:6d} {d:6d} {ms:8.3f} {4.0 * n * n * d / (ms * 1e-3) * 1e-12:9.2f}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
