"""Time the wide-head attention kernel (csrc/attn_wide.hip) against the unfused route on one MI355X.

    python tools/bench_attn_wide.py [--iters 50] [--rounds 7]

Shapes: the class-conditional ImageNet UNet's self-attentions, (tokens, d_head) = (1024, 384), (256, 576), (64, 960), at BH = 2 and 8
rows per call.  Fused: one sdmi_k_attention launch.  Unfused: the method of the first stage's mid block (csrc/vae.cpp attn_block)
built from the existing kernel entry points, per row S = Q K^T (sdmi_k_igemm, fp32), softmax (sdmi_k_softmax_rows), P V
(sdmi_k_igemm): 3 launches per row.  (The first stage's third GEMM, the V^T projection, is left out: both routes here start from the
same q / k / v^T, which favours the unfused one.)  Both routes are warmed up and then timed alternately, `rounds` times `iters`
back-to-back calls between two events; the median round is reported.  The descriptors are built once, outside the timed loops."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 384), (256, 576), (64, 960)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    s = _lib.stream_ptr()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    print(f'# {torch.cuda.get_device_name(0)}; us per attention, median of {args.rounds} rounds x {args.iters} calls, routes alternating')
    print('# tokens d_head BH  fused_us  unfused_us  unfused/fused  max-abs(fused - unfused)')
    worst = 0.0
    for n, d in SHAPES:
        for BH in (2, 8):
            g = torch.Generator(device='cuda').manual_seed(n + d + BH)
            q = torch.randn(BH, n, d, device='cuda', generator=g).half()
            k = torch.randn(BH, n, d, device='cuda', generator=g).half()
            vt = torch.randn(BH, d, n, device='cuda', generator=g).half()
            scale = d ** -0.5
            out_f = torch.empty(BH, n, d, dtype=torch.float16, device='cuda')
            out_u = torch.empty_like(out_f)
            Sm = torch.empty(n, n, dtype=torch.float32, device='cuda')
            Pm = torch.empty(n, n, dtype=torch.float16, device='cuda')

            def desc(a, w, N, K, rows, out32=None, out16=None):
                x = _lib.IGemmDesc()
                x.a0 = a.data_ptr(); x.c0 = K; x.lda0 = K
                x.B, x.Hin, x.Win, x.Hout, x.Wout, x.ksize, x.stride, x.up = 1, rows, 1, rows, 1, 1, 1, 0
                x.w = w.data_ptr(); x.N = N
                x.out_f32 = _lib.ptr(out32); x.out_f16 = _lib.ptr(out16); x.ldo = N
                x.splitk, x.tile, x.dma = 1, -1, -1
                return x
            ds = [desc(q[b], k[b], n, d, n, out32=Sm) for b in range(BH)]
            dp = [desc(Pm, vt[b], d, n, n, out16=out_u[b]) for b in range(BH)]

            def fused():
                _lib.check(lib.sdmi_k_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out_f.data_ptr(), BH, 1, n, n, n, d, scale, s))

            def unfused():
                for b in range(BH):
                    _lib.check(lib.sdmi_k_igemm(C.byref(ds[b]), s))
                    _lib.check(lib.sdmi_k_softmax_rows(Sm.data_ptr(), Pm.data_ptr(), n, n, scale, s))
                    _lib.check(lib.sdmi_k_igemm(C.byref(dp[b]), s))
            for _ in range(10):
                fused(); unfused()
            torch.cuda.synchronize()
            diff = float((out_f.float() - out_u.float()).abs().max())
            tf, tu = [], []
            for _ in range(args.rounds):
                for fn, acc in ((fused, tf), (unfused, tu)):
                    a, b = ev(), ev()
                    a.record()
                    for _ in range(args.iters):
                        fn()
                    b.record()
                    torch.cuda.synchronize()
                    acc.append(a.elapsed_time(b) * 1e3 / args.iters)
            f_us, u_us = statistics.median(tf), statistics.median(tu)
            worst = max(worst, f_us / u_us)
            print(f'{n:6d} {d:5d} {BH:3d} {f_us:9.1f} {u_us:11.1f} {u_us / f_us:13.2f}  {diff:.2e}', flush=True)
    print(f'# worst fused / unfused ratio {worst:.3f} ({"fused never slower" if worst <= 1.0 else "FUSED SLOWER SOMEWHERE"})')
    return 0 if worst <= 1.0 else 1


if __name__ == '__main__':
    sys.exit(main())
