"""Time bsr_sr's tiled x4 super-resolution on one MI355X: a 256 x 256 input to 1024 x 1024, B = 1, nine 128 x 128 windows at stride 64.

    python tools/bench_superres.py [--size 256] [--steps 100] [--rounds 5] [--vq-ks 128] [--out profiles/bench_superres.txt]

New path: SuperResolutionHIP -- all windows as rows of chunked UNet / first-stage calls, sdmi_k_patch_unfold (with the concat) and
sdmi_k_patch_fold.  Yardstick: the reference's algorithm (ddpm.py:902-984, 715-752) on the same library -- torch Unfold on the GPU, one
UNetModelHIP / VQModelInterfaceHIP call of B rows per window, stack, multiply by the weighting, torch Fold, divide -- as the parent commit
would run it.  Both alternate in one process; medians over rounds, with the spread.  Also: nine rows as 8 + 1 against 5 + 4, and the
first-stage decode of one window on its own (its mid-block attention runs over (vq-ks)^2 tokens at 512 channels).
Prints one JSON line per measurement (and appends them to --out)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, calls, warm=1):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--vq-ks', type=int, default=128, help='window of the first stage (latent pixels)')
    ap.add_argument('--skip-upscale', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_superres.py needs the MI355X'
    from stable_diffusion_amd import DDIMSamplerHIP, SuperResolutionHIP
    from stable_diffusion_amd.ldm_shim import patch_grid, patch_weighting
    from stable_diffusion_amd.superres import DEFAULT_SPLIT_INPUT_PARAMS
    dev = 'cuda'
    S = args.size

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    sr = SuperResolutionHIP().load_synthetic(0).to(dev)
    unet, vq = sr.model.diffusion_model, sr.first_stage_model
    g = torch.Generator().manual_seed(0)
    lr = (0.5 * torch.randn(1, 3, S, S, generator=g)).clamp(-1, 1).to(dev)
    x = torch.randn(1, 3, S, S, generator=g).to(dev)
    t = torch.full((1,), 501, dtype=torch.long, device=dev)
    assert sr.configure_tiling(S, S)
    p = sr.split_input_params
    ks, stride = p['ks'], p['stride']
    Ly, Lx = patch_grid(S, S, ks, stride)
    L = Ly * Lx

    # ---- the yardstick: the reference's loop on this library ----
    def ref_parts(h, w, ks_, stride_, uf):
        ly, lx = patch_grid(h, w, ks_, stride_)
        wgt = patch_weighting(ks_[0] * uf, ks_[1] * uf, ly, lx, p).to(dev).permute(1, 2, 0)[None, None].contiguous()   # (1, 1, kh, kw, L)
        unfold = torch.nn.Unfold(kernel_size=ks_, stride=stride_)
        fold = torch.nn.Fold(output_size=(h * uf, w * uf), kernel_size=(ks_[0] * uf, ks_[1] * uf), stride=(stride_[0] * uf, stride_[1] * uf))
        norm = fold(wgt.view(1, -1, ly * lx)).view(1, 1, h * uf, w * uf)
        return unfold, fold, norm, wgt

    am_parts = ref_parts(S, S, ks, stride, 1)

    def ref_apply_model(xx, tt, cc):
        unfold, fold, norm, wgt = am_parts
        z = unfold(xx)
        z = z.view(z.shape[0], -1, ks[0], ks[1], z.shape[-1])
        c = unfold(cc)
        c = c.view(c.shape[0], -1, ks[0], ks[1], c.shape[-1])
        outs = [unet(torch.cat([z[:, :, :, :, i], c[:, :, :, :, i]], 1), tt) for i in range(z.shape[-1])]
        o = torch.stack(outs, -1) * wgt
        return fold(o.view(o.shape[0], -1, o.shape[-1])) / norm

    vks = (min(args.vq_ks, S),) * 2
    vstride = (max(1, vks[0] // 2),) * 2
    dec_parts = ref_parts(S, S, vks, vstride, p['vqf'])

    def ref_decode(zz):
        unfold, fold, norm, wgt = dec_parts
        z = unfold(zz)
        z = z.view(z.shape[0], -1, vks[0], vks[1], z.shape[-1])
        outs = [vq.decode(z[:, :, :, :, i]) for i in range(z.shape[-1])]
        o = torch.stack(outs, -1) * wgt
        return fold(o.view(o.shape[0], -1, o.shape[-1])) / norm

    def new_decode(zz):
        keep = sr.split_input_params
        sr.split_input_params = dict(keep, ks=vks, stride=vstride)
        try:
            return sr.decode_first_stage(zz)
        finally:
            sr.split_input_params = keep

    def rounds(fns, calls, warm=1):
        res = {k: [] for k in fns}
        for _ in range(args.rounds):                # alternating, in one process
            for k, fn in fns.items():
                res[k].append(_timed(fn, calls, warm))
        return {k: {'median_ms': round(statistics.median(v), 3), 'min_max_ms': [round(min(v), 3), round(max(v), 3)]} for k, v in res.items()}

    # ---- one tiled apply_model: 8 + 1 rows, 5 + 4 rows, the per-window loop ----
    def chunked(n):                                 # n windows per call, set on the instance for the call alone
        def run():
            sr._window_chunks = lambda L_, B_: [(l0, min(n, L_ - l0)) for l0 in range(0, L_, n)]
            try:
                return sr.apply_model(x, t, lr)
            finally:
                del sr._window_chunks
        return run
    a, b = chunked(8)(), ref_apply_model(x, t, lr)
    torch.cuda.synchronize()
    emit({'metric': 'bsr_sr_tiled_apply_model', 'input': [S, S], 'windows': L, 'window': list(ks), 'stride': list(stride),
          'max_abs_new_vs_per_window_loop': float((a - b).abs().max()),
          **rounds({'rows_8+1': chunked(8), 'rows_5+4': chunked(5), 'per_window_loop_torch_fold': lambda: ref_apply_model(x, t, lr)}, args.calls)})

    # ---- the first stage: one window alone (its mid-block attention), then the tiled decode ----
    zlat = torch.randn(1, 3, S, S, generator=g).to(dev)
    t0 = time.perf_counter()
    one = vq.decode(zlat[:, :, :vks[0], :vks[1]])
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    emit({'metric': 'vq_f4_decode_one_window', 'latent_window': list(vks), 'mid_attention_tokens': vks[0] * vks[1],
          'first_call_s': round(first, 3), 'ms_per_call': round(_timed(lambda: vq.decode(zlat[:, :, :vks[0], :vks[1]]), 3), 3),
          'finite': bool(torch.isfinite(one).all())})
    a, b = new_decode(zlat), ref_decode(zlat)
    torch.cuda.synchronize()
    emit({'metric': 'bsr_sr_tiled_decode', 'latent': [S, S], 'image': list(a.shape[-2:]), 'window': list(vks), 'stride': list(vstride),
          'max_abs_new_vs_per_window_loop': float((a - b).abs().max()),
          **rounds({'tiled': lambda: new_decode(zlat), 'per_window_loop_torch_fold': lambda: ref_decode(zlat)}, 2)})
    if args.skip_upscale:
        return

    # ---- the whole upscale ----
    class RefLoop:
        """the sampler's view of the model with the reference's per-window apply_model"""
        def __init__(self):
            self.num_timesteps, self.betas, self.alphas_cumprod, self.model = sr.num_timesteps, sr.betas, sr.alphas_cumprod, sr.model

        def apply_model(self, xx, tt, cc):
            return ref_apply_model(xx, tt, cc)

    def up_new():
        samples, _ = DDIMSamplerHIP(sr).sample(args.steps, batch_size=1, shape=(3, S, S), conditioning=lr, eta=1.0, verbose=False)
        return new_decode(samples)

    def up_ref():
        samples, _ = DDIMSamplerHIP(RefLoop()).sample(args.steps, batch_size=1, shape=(3, S, S), conditioning=lr, eta=1.0, verbose=False)
        return ref_decode(samples)
    with contextlib.redirect_stdout(io.StringIO()):
        out = up_new()                      # (the warm-up of both loops' shapes: every call above ran them)
        res = rounds({'tiled': up_new, 'per_window_loop_torch_fold': up_ref}, 1, warm=0)
    emit({'metric': 'bsr_sr_upscale', 'input': [S, S], 'image': list(out.shape[-2:]), 'ddim_steps': args.steps, 'eta': 1.0,
          'finite': bool(torch.isfinite(out).all()), **res})


if __name__ == '__main__':
    main()
