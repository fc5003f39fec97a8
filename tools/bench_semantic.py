"""Time the semantic-synthesis model on one MI355X: the cond stage (csrc/rescale.hip against the torch route), one UNet call, and
`synthesize` from labels at 512 x 512.

    python tools/bench_semantic.py [--rounds 5] [--calls 30] [--steps 50] [--skip-synthesize] [--out profiles/bench_semantic.txt]

Rescale, at 182 x 512 x 512 and 182 x 512 x 1024, B = 1 and 4, four routes alternating in one process (device events, every shape warmed):
    fused          sdmi_k_spatial_rescale on the one-hot tensor (it is already on the device)
    labels         sdmi_k_spatial_rescale_labels on the int32 label map (without encode_labels' range check, a device sync)
    torch          F.interpolate twice + F.conv2d on PyTorch-ROCm, on the one-hot tensor
    torch+one_hot  the same with the F.one_hot(...).permute(...).float() a caller with labels needs first
A 512 x 512 one-hot sample is 190.8 MB, less than the 256 MB Infinity Cache, so every route rotates over enough distinct inputs that at
least 768 MB lie between two reads of one buffer.  The fused kernel's achieved bytes/s are its input bytes over its time; the floor is the
5.6 - 6.0 TB/s read sweep of profiles/knn_search.txt.
UNet: one call at latent 128 x 128 (B = 1, 8) and 128 x 256 (B = 1), mixed and full, with the profiled launches of a call.
synthesize: labels 512 x 512, eta 1.0, B = 1 and 4, images per second.
Prints one JSON line per measurement (and appends them to --out)."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLASSES = 182
ROTATE_BYTES = 768 << 20


def _timed(fn, calls, warm=2):
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
    return sum(r['launches'] for r in json.loads(buf.value.decode()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--skip-rescale', action='store_true')
    ap.add_argument('--skip-unet', action='store_true')
    ap.add_argument('--skip-synthesize', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_semantic.py needs the MI355X'
    from stable_diffusion_amd import SemanticSynthesisHIP
    dev = 'cuda'

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    def rounds(fns, calls, warm=2):
        res = {k: [] for k in fns}
        for _ in range(args.rounds):                # alternating, in one process
            for k, fn in fns.items():
                res[k].append(_timed(fn, calls, warm))
        return {k: {'median_us': round(1e3 * statistics.median(v), 1), 'min_max_us': [round(1e3 * min(v), 1), round(1e3 * max(v), 1)]}
                for k, v in res.items()}

    m = SemanticSynthesisHIP().load_synthetic(0).to(dev)
    r = m.cond_stage_model
    w4 = r.channel_mapper.weight.detach()

    # ---- the cond stage ----
    for H, W in (() if args.skip_rescale else ((512, 512), (512, 1024))):
        for B in (1, 4):
            in_bytes = B * CLASSES * H * W * 4
            n_buf = max(2, -(-ROTATE_BYTES // in_bytes) + 1)
            g = torch.Generator(device=dev).manual_seed(H + W + B)
            labs = [torch.randint(0, CLASSES, (B, H, W), generator=g, device=dev) for _ in range(n_buf)]
            labs32 = [l.to(torch.int32) for l in labs]
            hots = [F.one_hot(l, CLASSES).permute(0, 3, 1, 2).float().contiguous() for l in labs]
            turn = {'i': 0}

            def nxt(seq):
                turn['i'] += 1
                return seq[turn['i'] % n_buf]

            def torch_route(x):
                for _ in range(r.n_stages):
                    x = F.interpolate(x, scale_factor=0.5, mode='bilinear')
                return F.conv2d(x, w4)

            def torch_from_labels(l):
                return torch_route(F.one_hot(l, CLASSES).permute(0, 3, 1, 2).float())
            a, b, c = r.encode(hots[0]), r.encode_labels(labs32[0]), torch_route(hots[0])
            torch.cuda.synchronize()
            res = rounds({'fused': lambda: r.encode(nxt(hots)), 'labels': lambda: r.encode_labels(nxt(labs32), check_range=False),
                          'torch': lambda: torch_route(nxt(hots)), 'torch+one_hot': lambda: torch_from_labels(nxt(labs))}, args.calls)
            t_f = res['fused']['median_us'] * 1e-6
            emit({'metric': 'spatial_rescale', 'map': [CLASSES, H, W], 'B': B, 'input_MB': round(in_bytes / 1e6, 1), 'buffers_rotated': n_buf,
                  'labels_equals_fused_bits': bool(torch.equal(a, b)), 'max_abs_fused_vs_torch': float((a - c).abs().max()),
                  'fused_TB_per_s': round(in_bytes / t_f / 1e12, 3), 'fused_us_per_sample': round(res['fused']['median_us'] / B, 1),
                  'torch_over_fused': round(res['torch']['median_us'] / res['fused']['median_us'], 2),
                  'torch+one_hot_over_labels': round(res['torch+one_hot']['median_us'] / res['labels']['median_us'], 2), **res})
            del labs, labs32, hots
            torch.cuda.empty_cache()

    # ---- one UNet call ----
    for prec in (() if args.skip_unet else ('mixed', 'full')):
        mm = m if prec == 'mixed' else SemanticSynthesisHIP(hip_precision='full').load_synthetic(0).to(dev)
        unet = mm.model.diffusion_model
        for B, h, w in ((1, 128, 128), (8, 128, 128), (1, 128, 256)):
            x = torch.randn(B, 6, h, w, generator=torch.Generator().manual_seed(B + h + w)).to(dev)
            t = torch.full((B,), 501, dtype=torch.long, device=dev)
            t0 = time.perf_counter()
            out = unet(x, t)
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            ms = [_timed(lambda: unet(x, t), 5) for _ in range(args.rounds)]
            emit({'metric': 'semantic_unet_call', 'precision': prec, 'B': B, 'latent': [h, w], 'finite': bool(torch.isfinite(out).all()),
                  'first_call_s': round(first, 3), 'median_ms': round(statistics.median(ms), 3), 'min_max_ms': [round(min(ms), 3), round(max(ms), 3)],
                  'profiled_launches_per_call': profiled_launches(unet, x, t)})
        if mm is not m:
            del mm, unet
            torch.cuda.empty_cache()

    # ---- synthesize from labels ----
    for B in (() if args.skip_synthesize else (1, 4)):
        labels = torch.randint(0, CLASSES, (B, 512, 512), generator=torch.Generator().manual_seed(B)).to(dev)
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            img = m.synthesize(labels=labels, steps=2, eta=1.0)                  # (warms every shape of the loop and the decode)
            torch.cuda.synchronize()
            secs = []
            for _ in range(3):
                t0 = time.perf_counter()
                img = m.synthesize(labels=labels, steps=args.steps, eta=1.0)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
        emit({'metric': 'semantic_synthesize_from_labels', 'image': [512, 512], 'B': B, 'ddim_steps': args.steps, 'eta': 1.0,
              'finite': bool(torch.isfinite(img).all()), 'median_s': round(statistics.median(secs), 3),
              'min_max_s': [round(min(secs), 3), round(max(secs), 3)], 'images_per_s': round(B / statistics.median(secs), 3)})


if __name__ == '__main__':
    main()
