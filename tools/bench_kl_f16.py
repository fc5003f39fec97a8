"""Time the KL-f16 first stage of the retrieval-augmented model, and one of its attention blocks in two forms, on one MI355X.

    python tools/bench_kl_f16.py [--iters 3] [--rounds 5] [--out profiles/bench_kl_f16.txt]

First stage: AutoencoderKLHIP with the yaml's ddconfig (ch 128, ch_mult [1,1,2,2,4], z 16, attn_resolutions [16]) and seeded random
weights: decode of the native 48 x 48 latent (a 768 x 768 image) and encode of a 768 x 768 image, B = 1 and 2, hip_precision 'mixed' and
'full' alive in one process and timed alternately, `rounds` times `iters` back-to-back calls between two events; the median round.
Attention: one head of d = 512 over N = 2304 tokens (a level-4 AttnBlock at the native size), fp16 operands, as
  flash   one sdmi_k_attention launch (csrc/attn_wide.hip) -- what a handle with level attention runs;
  gemm    q k^T (sdmi_k_igemm into fp32 S [N][N]), sdmi_k_softmax_rows (S -> fp16 P), P v (sdmi_k_igemm) -- the form of the handles
          without level attention, through the kernel entry points the tests use.
Both are timed on the same q, k, v^T; their outputs are compared.  Nothing is promised about these times: they are reported."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _time(fns, iters, rounds):
    """alternate the callables; median ms per call of each"""
    acc = [[] for _ in fns]
    for _ in range(rounds):
        for fn, a in zip(fns, acc):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            a.append(e0.elapsed_time(e1) / iters)
    return [statistics.median(a) for a in acc]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import kernels as K
    from stable_diffusion_amd import AutoencoderKLHIP, _lib
    from stable_diffusion_amd.synthetic import KL_F16_KWARGS, KL_F16_SCALE_FACTOR, synthetic_kl_f16_state_dict
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f'# {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds x {args.iters} calls, mixed and full alternating in one process')
    sd = synthetic_kl_f16_state_dict(0)
    models = {}
    for prec in ('mixed', 'full'):
        m = AutoencoderKLHIP(KL_F16_KWARGS['ddconfig'], None, KL_F16_KWARGS['embed_dim'], hip_precision=prec)
        m.load_state_dict(sd, strict=True)
        models[prec] = m.cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(0)
    say('# KL-f16 first stage                       mixed_ms   full_ms  full/mixed  max-abs(full - mixed)')
    for B in (1, 2):
        lat = torch.randn(B, 16, 48, 48, device='cuda', generator=g) / KL_F16_SCALE_FACTOR
        img = torch.rand(B, 3, 768, 768, device='cuda', generator=g) * 2 - 1
        for name, call, x in ((f'decode B={B} 48x48 latent -> 768x768', 'decode', lat), (f'encode B={B} 768x768 image -> 48x48', 'encode_moments', img)):
            fns = [lambda p=prec: getattr(models[p], call)(x) for prec in ('mixed', 'full')]
            outs = [fn() for fn in fns]
            torch.cuda.synchronize()
            diff = float((outs[0] - outs[1]).abs().max())
            del outs
            tm, tf = _time(fns, args.iters, args.rounds)
            say(f'{name:40s} {tm:9.2f} {tf:9.2f} {tf / tm:11.2f}  {diff:.2e}')

    lib = _lib.load()
    s = _lib.stream_ptr()
    n, d = 2304, 512
    q, k = (torch.randn((n, d), device='cuda', generator=g).half() for _ in range(2))
    vt = torch.randn((d, n), device='cuda', generator=g).half()
    out_flash, out_gemm = (torch.empty((n, d), dtype=torch.float16, device='cuda') for _ in range(2))
    S = torch.empty((n, n), dtype=torch.float32, device='cuda')
    P = torch.empty((n, n), dtype=torch.float16, device='cuda')

    def flash():
        _lib.check(lib.sdmi_k_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out_flash.data_ptr(), 1, 1, n, n, n, d, d ** -0.5, s))

    def gemm():
        K.igemm(q, k, n, 1, n, 1, n, 1, out_f32=S, splitk=1)
        _lib.check(lib.sdmi_k_softmax_rows(S.data_ptr(), P.data_ptr(), n, n, d ** -0.5, s))
        K.igemm(P, vt, d, 1, n, 1, n, 1, out_f16=out_gemm, splitk=1)

    for _ in range(3):
        flash()
        gemm()
    torch.cuda.synchronize()
    diff = float((out_flash.float() - out_gemm.float()).abs().max())
    tf, tg = _time([flash, gemm], max(args.iters, 10), args.rounds)
    say(f'# one AttnBlock attention, N = {n} tokens, d = {d}, one head, one image (max-abs flash - gemm {diff:.2e})')
    say('# form     ms   TFLOP/s (algorithmic: 4 N^2 d)   buffers beside q / k / v^T / out')
    say(f'flash  {tf:7.3f} {4.0 * n * n * d / (tf * 1e-3) * 1e-12:9.2f}   none')
    say(f'gemm   {tg:7.3f} {4.0 * n * n * d / (tg * 1e-3) * 1e-12:9.2f}   S fp32 + P fp16 = {6 * n * n / 2 ** 20:.1f} MB; three launches')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
