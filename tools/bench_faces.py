"""Time the face / bedroom LDMs (models/ldm/celeba256, ffhq256, lsun_beds256: one UNet, model_channels 224) and bsr_sr's UNet (160) on
one MI355X: one batch as scripts/sample_diffusion.py runs it (10 samples, 50 DDIM steps at eta 1.0 on a 3 x 64 x 64 latent -- the UNet
sees them as 8 + 2 rows -- and the VQ-f4 decode to 256 x 256), one UNet call at 8 rows and at 2 rows, and the profiled launches of one
8-row call, with seeded synthetic weights.

    python tools/bench_faces.py [--model faces|bsr] [--batch 10] [--steps 50] [--calls 20] [--precision mixed]
    python tools/bench_faces.py --ktail [--lib-b other/libsdmi.so]

Prints one JSON line: ms per UNet call at 8 / 2 rows, profiled launches per call, ms per batch (sampling, decode), images per second
(bsr: the UNet calls only -- its image pipeline is not part of this project).
--ktail: what a half k-tile costs.  The 3x3 convs (224 | 224) -> 224 at 64 x 64 and 672 -> 672 at 16 x 16, batch 8, against the same
problem with every source zero-padded to the next multiple of 64 -- (256 | 256) and 704 -- at the same tile and split-K, alternating in
one process; and once more with the logical channels stored at the padded row pitch (what the 64-byte row starts of a 448- / 1344-byte
pitch cost, apart from the half tile itself).  With --lib-b the padded problem runs on that library (an older build that knows whole 64-channel chunks only), loaded
beside the product one.  Prints one JSON line per problem: median us of each, and the spread (min .. max of the per-round medians)."""
import argparse
import contextlib
import ctypes as C
import io
import json
import math
import os
import statistics
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


def profiled_launches(unet, x, t):
    """launch scopes of one UNet call through the executor (the library's own profiler: a profiled call is not replayed from a tape)"""
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    unet(x, t)
    torch.cuda.synchronize()
    _lib.check(lib.sdmi_profile_begin())
    unet(x, t)
    buf = C.create_string_buffer(1 << 20)
    _lib.check(lib.sdmi_profile_end(buf, len(buf)))
    recs = json.loads(buf.value.decode())
    return sum(r['launches'] for r in recs), sum(r['launches'] for r in recs if r['name'].startswith(('igemm_', 'gemm_split16_')))


def ktail(lib_b_path, rounds=7, calls=200):
    from stable_diffusion_amd import _lib
    lib_a = _lib.load()
    lib_b = lib_a
    if lib_b_path:
        lib_b = C.CDLL(lib_b_path)
        for name in ('sdmi_k_igemm', 'sdmi_k_pack_conv_weight'):
            getattr(lib_b, name).restype, getattr(lib_b, name).argtypes = _lib._SIGS[name]
    s = _lib.stream_ptr()
    g = torch.Generator().manual_seed(0)
    B = 8
    # name, sources, N, H, (tile, split-K) -- the 8-wave 256 x 128 tile unsplit, and the many-workgroup 64 x 64 tile unsplit / split in 2
    alive = []
    problems = [('conv3 (224|224)->224 64x64', (224, 224), 224, 64), ('conv3 672->672 16x16', (672,), 672, 16)]
    for name, split, N, H in problems:
        M = B * H * H
        pad = tuple((c + 63) // 64 * 64 for c in split)
        Np = N                       # (the output width is the padded run's too: the comparison is about K)
        res = {'problem': name, 'batch': B, 'padded_sources': list(pad), 'lib_b': os.path.basename(lib_b_path) if lib_b_path else 'same library'}
        for tile, sk in ((3, 1), (5, 1), (5, 2)):
            def make(lib, srcs, pitch=None):
                Cin = sum(srcs)
                w = torch.randn(Np, Cin, 3, 3, generator=g).cuda() / math.sqrt(9 * Cin)
                wp = torch.empty((Np, 9 * Cin), dtype=torch.float16, device='cuda')
                if len(srcs) > 1 and any(c % 64 for c in srcs):
                    _lib.check(lib.sdmi_k_pack_conv_weight_src(w.data_ptr(), wp.data_ptr(), Np, Cin, 3, 3, srcs[0], srcs[1], 0, s))
                else:
                    assert lib.sdmi_k_pack_conv_weight(w.data_ptr(), wp.data_ptr(), Np, Cin, 3, 3, s) == 0
                # (pitch: the logical channels inside rows of `pitch` halves -- a 128-byte aligned row start for every pixel)
                a = [torch.randn(M, pitch or c, generator=g).half().cuda()[:, :c] for c in srcs]
                out = torch.empty((M, Np), dtype=torch.float32, device='cuda')
                ws = torch.empty((4 * (M + 255) * (Np + 255),), dtype=torch.float32, device='cuda')
                d = _lib.IGemmDesc()
                d.a0 = a[0].data_ptr(); d.c0 = srcs[0]; d.lda0 = a[0].stride(0)
                if len(srcs) > 1:
                    d.a1 = a[1].data_ptr(); d.c1 = srcs[1]; d.lda1 = a[1].stride(0)
                d.B, d.Hin, d.Win, d.Hout, d.Wout, d.ksize, d.stride, d.up = B, H, H, H, H, 3, 1, 0
                d.w = wp.data_ptr(); d.N = Np; d.mode = 0; d.out_f32 = out.data_ptr(); d.ldo = Np
                d.splitk, d.tile, d.dma = sk, tile, -1
                d.splitk_ws = ws.data_ptr(); d.splitk_ws_floats = ws.numel()
                alive.append((a, wp, out, ws))            # (the descriptor holds raw pointers)

                def run():
                    assert lib.sdmi_k_igemm(C.byref(d), s) == 0
                return run
            new, padded, new128 = make(lib_a, split), make(lib_b, pad), make(lib_a, split, pitch=pad[0])
            t_new, t_pad, t_128 = [], [], []
            for _ in range(rounds):              # alternating, in one process
                t_pad.append(1e3 * _timed(padded, calls))
                t_new.append(1e3 * _timed(new, calls))
                t_128.append(1e3 * _timed(new128, calls))
            res[f'tile{tile}_splitk{sk}'] = {'half_tile_us': round(statistics.median(t_new), 2), 'padded_us': round(statistics.median(t_pad), 2),
                                             'half_tile_at_padded_pitch_us': round(statistics.median(t_128), 2),
                                             'half_tile_min_max_us': [round(min(t_new), 2), round(max(t_new), 2)],
                                             'padded_min_max_us': [round(min(t_pad), 2), round(max(t_pad), 2)]}
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='faces', choices=['faces', 'bsr'])
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--precision', default='mixed', choices=['mixed', 'full'])
    ap.add_argument('--ktail', action='store_true')
    ap.add_argument('--lib-b', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_faces.py needs the MI355X'
    if args.ktail:
        ktail(args.lib_b)
        return
    from bench_inpaint import MFMA_PEAK_TFLOPS, unet_flops
    from stable_diffusion_amd import DDIMSamplerHIP, LatentDiffusionHIP, UNetModelHIP, VQModelInterfaceHIP, synthetic
    dev = 'cuda'
    kw = synthetic.FACES_UNET_KWARGS if args.model == 'faces' else synthetic.BSR_UNET_KWARGS
    unet = UNetModelHIP(**kw, hip_precision=args.precision)
    unet.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], 0))
    unet = unet.to(dev)
    lat, cin = kw['image_size'], kw['in_channels']
    g = torch.Generator().manual_seed(0)

    # ---- one UNet call at 8 and at 2 rows (replayed launch tapes, as inside the sampling loop) ----
    ms_rows = {}
    for rows in (8, 2):
        x = torch.randn(rows, cin, lat, lat, generator=g).to(dev)
        t = torch.full((rows,), 501, dtype=torch.long, device=dev)
        ms_rows[rows] = _timed(lambda: unet(x, t), args.calls)
    x8 = torch.randn(8, cin, lat, lat, generator=g).to(dev)
    n_launch, n_gemm = profiled_launches(unet, x8, torch.full((8,), 501, dtype=torch.long, device=dev))
    flops = unet_flops(kw, 8, lat, lat)
    res = {'metric': 'ldm_faces256' if args.model == 'faces' else 'bsr_sr_unet', 'precision': args.precision, 'latent': lat,
           'ms_per_unet_call_8rows': round(ms_rows[8], 3), 'ms_per_unet_call_2rows': round(ms_rows[2], 3),
           'profiled_launches_per_call_8rows': n_launch, 'gemm_launches_per_call_8rows': n_gemm,
           'unet_gflop_per_call_8rows': round(flops / 1e9, 1),
           'unet_mfma_peak_fraction_8rows': round(flops / (ms_rows[8] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4)}
    if args.model == 'faces':
        # ---- one sample_diffusion.py batch: convsample_ddim + decode_first_stage ----
        ld = LatentDiffusionHIP(unet, **synthetic.FACES_SCHEDULE).to(dev)
        vq = VQModelInterfaceHIP(**synthetic.FACES_VQ_KWARGS)
        vq.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in vq.state_dict().items()], 0))
        vq = vq.to(dev)
        sampler = DDIMSamplerHIP(ld)

        def batch_once():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            samples, _ = sampler.sample(args.steps, batch_size=args.batch, shape=(3, lat, lat), eta=1.0, verbose=False)
            ev[1].record()
            x_sample = vq.decode(samples)
            ev[2].record()
            torch.cuda.synchronize()
            return x_sample, [ev[i].elapsed_time(ev[i + 1]) for i in range(2)]

        with contextlib.redirect_stdout(io.StringIO()):
            batch_once()
            out, parts = batch_once()
        res.update({'batch': args.batch, 'ddim_steps': args.steps, 'eta': 1.0, 'ms_per_batch': round(sum(parts), 2),
                    'ms_sample': round(parts[0], 2), 'ms_decode': round(parts[1], 2),
                    'images_per_s': round(args.batch / (sum(parts) * 1e-3), 2), 'image': list(out.shape[-2:]),
                    'finite': bool(torch.isfinite(out).all())})
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
