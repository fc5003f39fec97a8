"""Time the image tail of the sampling scripts on one MI355X: from the clamped device image to the safety checker's pixel_values, and the whole
safety check, the reference's host route against the HIP feature extractor.

    python tools/bench_image_tail.py [--iters 20] [--rounds 7] [--out profiles/bench_image_tail.txt]

Per image size (512 x 512, 768 x 768) and batch (1, 4), from the clamped fp32 [B, 3, H, W] image on the device to pixel_values on the device:
  (a) the reference's route (scripts/txt2img.py:314-317, 88-90): .cpu(), uint8 PIL images, transformers' CLIP image processor on its PIL
      backend, .cuda() -- when Pillow and transformers are installed on the host; the report says so when they are not
  (b) CLIPFeatureExtractorHIP on the device tensor (two launches)
and beside (b) a plain 16-byte read sweep of the same input bytes (its floor) and the ViT-L/14 tower the values feed (seeded random weights).
Then the whole safety check from the raw decoder output both ways: the reference's route with StableDiffusionSafetyCheckerHIP.forward behind it,
and postprocess.check_safety.  Every callable is warmed up, then timed in `rounds` windows of `iters` calls, the routes alternating; a window
is closed by a device synchronise and read on the host clock (what a caller waits for: for the two-launch paths that is mostly launch cost),
and on a pair of device events (the device's own span) where the path has no host work.  Median window, with the spread.  Nothing here is a
bar: the numbers are reported, not promised."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fns, iters, rounds):
    """alternate the callables -> per callable ((median, min, max) host-clock ms per call, the same from device events)"""
    host, dev = [[] for _ in fns], [[] for _ in fns]
    for _ in range(rounds):
        for i, (fn, n) in enumerate(zip(fns, iters)):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            host[i].append((time.perf_counter() - t0) * 1e3 / n)
            dev[i].append(e0.elapsed_time(e1) / n)
    stat = lambda a: (statistics.median(a), min(a), max(a))      # noqa: E731
    return [(stat(h), stat(d)) for h, d in zip(host, dev)]


def _fmt(t):
    return f'{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})'


def _processor():
    """transformers' CLIP image processor on its PIL backend and PIL.Image, or (None, why)"""
    try:
        from PIL import Image
    except ImportError as e:
        return None, f'Pillow is not installed here ({e})'
    try:
        try:
            from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil as Proc
        except ImportError:
            from transformers import CLIPImageProcessor as Proc
        return (Proc(size={'shortest_edge': 224}, crop_size={'height': 224, 'width': 224}, resample=Image.BICUBIC), Image), None
    except Exception as e:      # noqa: BLE001
        return None, f'transformers\' CLIP image processor is not usable here ({type(e).__name__}: {e})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_image_tail.py needs the MI355X'
    from stable_diffusion_amd import _lib, postprocess, synthetic, vision
    lib = _lib.load()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    proc, why = _processor()
    checker = vision.StableDiffusionSafetyCheckerHIP()
    sd = synthetic.synthetic_vision_state_dict(None, 1234)
    sd = {('vision_model.' + k if k.startswith('vision_model.') else k): v for k, v in sd.items()}
    g = torch.Generator().manual_seed(1234)
    sd.update(concept_embeds=torch.randn(checker.concept_embeds.shape, generator=g), concept_embeds_weights=torch.full(checker.concept_embeds_weights.shape, 2.0),
              special_care_embeds=torch.randn(checker.special_care_embeds.shape, generator=g),
              special_care_embeds_weights=torch.full(checker.special_care_embeds_weights.shape, 2.0))
    checker.load_state_dict(sd, strict=True)
    checker.cuda()
    tower = checker._tower[0]
    fe = vision.CLIPFeatureExtractorHIP()
    sink = torch.zeros(4, device='cuda')
    say(f'# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median (min .. max) ms per call of {args.rounds} windows, the routes alternating '
        f'in one process; calls per window: {args.iters * 5} for (b) and the read sweep, {args.iters} for the tower and the HIP check, '
        f'{max(2, args.iters // 4)} for the host routes')
    say('# host = host clock around the window, closed by a device synchronise; device = a pair of device events around the same window')
    if proc is None:
        say(f'# (a) the reference\'s route was NOT measured on this host: {why}.  The only comparison is the build machine\'s CPU figure: 6.9 ms '
            'per 512 x 512 image at B = 4 for the processor alone, of which Image.resize 2.8 ms')
    else:
        import PIL
        import transformers
        say(f'# (a) = .cpu() -> uint8 PIL images -> {type(proc[0]).__name__} (Pillow {PIL.__version__}, transformers {transformers.__version__}) -> .cuda(); '
            f'torch host threads {torch.get_num_threads()}')

    def ref_route(x01):
        x = x01.cpu().permute(0, 2, 3, 1).numpy()
        pils = [proc[1].fromarray(im) for im in (x * 255).round().astype(np.uint8)]
        return proc[0](pils, return_tensors='pt')['pixel_values'], x

    n_host = max(2, args.iters // 4)
    with torch.no_grad():
        for S in (512, 768):
            for B in (1, 4):
                xs = (torch.randn((B, 3, S, S), generator=torch.Generator().manual_seed(S + B)) * 0.6).cuda()     # a raw decoder output
                x01 = torch.clamp((xs + 1.0) / 2.0, min=0.0, max=1.0)
                n4 = x01.numel() // 4 * 4
                pv = fe(x01, layout='NCHW').pixel_values
                fns = [lambda: fe(x01, layout='NCHW').pixel_values,
                       lambda: _lib.check(lib.sdmi_k_knn_stream_read(x01.data_ptr(), n4, sink.data_ptr(), _lib.stream_ptr())),
                       lambda: tower(pv),
                       lambda: postprocess.check_safety(xs, checker, fe)]
                names = ['(b) CLIPFeatureExtractorHIP', f'    read sweep of the input ({x01.numel() * 4 / 1e6:.1f} MB)', '    the ViT-L/14 tower it feeds',
                         'check_safety, HIP extractor']
                iters = [args.iters * 5, args.iters * 5, args.iters, args.iters]
                if proc is not None:
                    pv_ref = ref_route(x01)[0].cuda()
                    diff = float((pv_ref - pv).abs().max())

                    def ref_check():
                        p, x = ref_route(torch.clamp((xs + 1.0) / 2.0, min=0.0, max=1.0))
                        return checker(clip_input=p, images=x)
                    fns += [lambda: ref_route(x01)[0].cuda(), ref_check]
                    names += ["(a) the reference's host route", 'check_safety, host extractor']
                    iters += [n_host, n_host]
                for fn in fns:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                res = dict(zip(names, _time(fns, iters, args.rounds)))
                say(f'## {S} x {S}, B = {B}' + (f'   max |pixel_values (a) - (b)| = {diff:.3e}' if proc is not None else ''))
                say(f'{"":44s} {"host ms":>30s}   {"device ms":>30s}')
                order = names[4:5] + names[:3] + names[5:] + names[3:4]          # (a), (b) and what stands beside it, then the whole check
                for name in order:
                    h, d = res[name]
                    host_work = 'host' in name
                    say(f'{name:44s} {_fmt(h):>30s}   {("-" if host_work else _fmt(d)):>30s}')
                if proc is not None:
                    a, b = res["(a) the reference's host route"][0][0], res['(b) CLIPFeatureExtractorHIP'][0][0]
                    ca, cb = res['check_safety, host extractor'][0][0], res['check_safety, HIP extractor'][0][0]
                    say(f'(a) / (b) = {a / b:.1f}; check_safety host / HIP = {ca / cb:.2f}; (b) device span / read sweep = '
                        f'{res["(b) CLIPFeatureExtractorHIP"][1][0] / res[names[1]][1][0]:.1f}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
