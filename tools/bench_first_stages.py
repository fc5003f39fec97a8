"""Time the first stages that came with KL-f32 and the VQ level-attention family, and the three wide fp32 kernels, on one MI355X.

    python tools/bench_first_stages.py [--iters 3] [--rounds 5] [--out profiles/bench_first_stages.txt]

First stages, with seeded random weights, decode and encode of the native latent at B = 1 and 2, hip_precision 'mixed' and 'full' alive
in one process and timed alternately, `rounds` times `iters` back-to-back calls between two events; the median round:
  KL-f32  8 x 8 <-> 256 x 256 and 16 x 16 <-> 512 x 512      VQ-f8  32 x 32 <-> 256 x 256      VQ-f16  16 x 16 <-> 256 x 256
(VQ decodes go through the quantizer, as VQModelInterface.decode does.)
Kernels, at KL-f32's shapes on the 16 x 16 latent (B = 2), each beside F.conv2d of PyTorch-ROCm on the same fp32 tensors in the same
process -- the layouts differ (conv_in64 writes NHWC, conv_out128 reads NHWC and packed OHWI weights; F.conv2d runs NCHW / OIHW):
  sdmi_k_conv_in64 64 -> 512      sdmi_k_conv_out128 512 -> 128      sdmi_k_pointwise_nchw128 128 -> 128 and 64 -> 64
Warm caches (the same buffers every call), launch-to-launch time including the launch gap: these kernels run once per decode / encode.
Nothing is promised about these times: they are reported, slower cases included.  Reads nothing of the reference."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    from stable_diffusion_amd import _lib
    from stable_diffusion_amd.synthetic import FIRST_STAGES, make_first_stage, synthetic_named_state_dict
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f'# {torch.cuda.get_device_name(0)}; median of {args.rounds} rounds x {args.iters} calls, mixed and full alternating in one process')
    g = torch.Generator(device='cuda').manual_seed(0)
    say('# first stage                                     mixed_ms   full_ms  full/mixed  max-abs(full - mixed)')
    for tag, sizes in (('kl_f32', ((8, 256), (16, 512))), ('vq_f8', ((32, 256),)), ('vq_f16', ((16, 256),))):
        kw = FIRST_STAGES[tag]
        models = {}
        for prec in ('mixed', 'full'):
            m = make_first_stage(kw, prec)
            m.load_state_dict(synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
            models[prec] = m.cuda().eval()
        for lat_side, img_side in sizes:
            for B in (1, 2):
                lat = torch.randn(B, kw['embed_dim'], lat_side, lat_side, device='cuda', generator=g)
                img = torch.rand(B, 3, img_side, img_side, device='cuda', generator=g) * 2 - 1
                for name, call, x in ((f'{tag} decode B={B} {lat_side}x{lat_side} -> {img_side}x{img_side}', 'decode', lat),
                                      (f'{tag} encode B={B} {img_side}x{img_side} -> {lat_side}x{lat_side}', 'encode_moments', img)):
                    fns = [lambda p=prec: getattr(models[p], call)(x) for prec in ('mixed', 'full')]
                    outs = [fn() for fn in fns]
                    torch.cuda.synchronize()
                    diff = float((outs[0] - outs[1]).abs().max())
                    del outs
                    tm, tf = _time(fns, args.iters, args.rounds)
                    say(f'{name:48s} {tm:9.2f} {tf:9.2f} {tf / tm:11.2f}  {diff:.2e}')
        del models
        torch.cuda.empty_cache()

    lib = _lib.load()
    s = _lib.stream_ptr()
    B, H, W = 2, 16, 16
    it = max(args.iters, 20)
    say(f'# the wide fp32 ends at KL-f32\'s shapes, B = {B}, {H} x {W} latent; us per call, median of {args.rounds} rounds x {it} calls, warm')
    say('# kernel                               hip_us  F.conv2d_us  hip/torch  max-abs(hip - torch)')

    def report(name, hip, ref, got, want):
        for _ in range(3):
            hip()
            ref()
        torch.cuda.synchronize()
        diff = float((got() - want()).abs().max())
        th, tr = _time([hip, ref], it, args.rounds)
        say(f'{name:36s} {1e3 * th:7.1f} {1e3 * tr:12.1f} {th / tr:10.2f}  {diff:.2e}')

    # conv_in64: NCHW -> NHWC
    x = torch.randn(B, 64, H, W, device='cuda', generator=g)
    w = torch.randn(512, 64, 3, 3, device='cuda', generator=g) / 24.0
    b = torch.randn(512, device='cuda', generator=g)
    o = torch.empty(B, H, W, 512, device='cuda')
    keep = {}
    report('sdmi_k_conv_in64 64 -> 512',
           lambda: _lib.check(lib.sdmi_k_conv_in64(x.data_ptr(), w.data_ptr(), b.data_ptr(), o.data_ptr(), B, 64, H, W, 512, s)),
           lambda: keep.__setitem__('r', F.conv2d(x, w, b, padding=1)), lambda: o.permute(0, 3, 1, 2), lambda: keep['r'])
    # conv_out128: NHWC -> NCHW, weights packed OHWI
    h = torch.randn(B, H, W, 512, device='cuda', generator=g)
    hn = h.permute(0, 3, 1, 2).contiguous()
    w2 = torch.randn(128, 512, 3, 3, device='cuda', generator=g) / 68.0
    b2 = torch.randn(128, device='cuda', generator=g)
    wp = torch.empty(128, 3, 3, 512, device='cuda')
    _lib.check(lib.sdmi_k_pack_conv_out(w2.data_ptr(), wp.data_ptr(), 128, 512, s))
    o2 = torch.empty(B, 128, H, W, device='cuda')
    report('sdmi_k_conv_out128 512 -> 128',
           lambda: _lib.check(lib.sdmi_k_conv_out128(h.data_ptr(), wp.data_ptr(), b2.data_ptr(), o2.data_ptr(), B, H, W, 512, 128, s)),
           lambda: keep.__setitem__('r', F.conv2d(hn, w2, b2, padding=1)), lambda: o2, lambda: keep['r'])
    # pointwise: quant_conv 128 -> 128, post_quant_conv 64 -> 64
    for c in (128, 64):
        xp = torch.randn(B, c, H * W, device='cuda', generator=g)
        w3 = torch.randn(c, c, device='cuda', generator=g) / c ** 0.5
        b3 = torch.randn(c, device='cuda', generator=g)
        o3 = torch.empty(B, c, H * W, device='cuda')
        x4, w4 = xp.view(B, c, H, W), w3.view(c, c, 1, 1)
        report(f'sdmi_k_pointwise_nchw128 {c} -> {c}',
               lambda: _lib.check(lib.sdmi_k_pointwise_nchw128(xp.data_ptr(), w3.data_ptr(), b3.data_ptr(), o3.data_ptr(), B, c, c, H * W, 1.0, s)),
               lambda: keep.__setitem__('r', F.conv2d(x4, w4, b3)), lambda: o3.view(B, c, H, W), lambda: keep['r'])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
