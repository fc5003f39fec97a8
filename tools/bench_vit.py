"""Time the CLIP image encoder on one MI355X: the HIP tower against transformers' CLIPVisionModelWithProjection on stock PyTorch-ROCm.

    python tools/bench_vit.py [--iters 20] [--rounds 7] [--layers 24] [--out profiles/vit_latency.txt]

The full ViT-L/14 (24 layers, 257 tokens, 304 M seeded random parameters) at B = 1 and B = 3: CLIPVisionHIP (fp16 MFMA operands, fp32
accumulation and residual stream) and the transformers model in fp32 and in fp16 (its default attention implementation) live in one process
and are timed alternately between two device events, `rounds` windows of `iters` forwards each after a warm-up of every shape; the median
window is reported with the spread.  Then the safety checker's concept head alone (17 + 3 concepts, E = 768) and the image embedder's
preprocess (512 x 512 -> 224), same method, and one B = 1 forward under the library's own profiler (an event pair per launch) by kernel class.
No bar is set on any of these numbers: they are reported, not promised."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fns, iters, rounds):
    """alternate the callables; (median, min, max) ms per call of each"""
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
    return [(statistics.median(a), min(a), max(a)) for a in acc]


def _fmt(t):
    return f'{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--layers', type=int, default=24)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_vit.py needs the MI355X'
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from stable_diffusion_amd import _lib, synthetic, vision
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    cfg = dict(vision.CLIP_VIT_L14_VISION, num_hidden_layers=args.layers)
    sd = synthetic.synthetic_vision_state_dict(cfg, 0)
    hip = vision.CLIPVisionHIP(cfg)
    hip.load_state_dict(sd, strict=True)
    hip.cuda()
    hc = CLIPVisionConfig(hidden_size=cfg['hidden_size'], intermediate_size=cfg['intermediate_size'], projection_dim=cfg['projection_dim'],
                          num_hidden_layers=cfg['num_hidden_layers'], num_attention_heads=cfg['num_attention_heads'],
                          image_size=cfg['image_size'], patch_size=cfg['patch_size'], hidden_act='quick_gelu', layer_norm_eps=1e-5)
    ref32 = CLIPVisionModelWithProjection(hc).float().eval()
    ref32.load_state_dict(sd, strict=False)
    ref32.cuda()
    ref16 = CLIPVisionModelWithProjection(hc).eval()
    ref16.load_state_dict(sd, strict=False)
    ref16.half().cuda()
    say(f'# {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median (min .. max) ms of {args.rounds} windows x {args.iters} forwards, '
        'the three implementations alternating in one process')
    say(f'# CLIP ViT-L/14 vision tower with projection, {args.layers} layers, 257 tokens, seeded random weights')
    say('# batch   libsdmi (mixed)              transformers fp32            transformers fp16            fp32/hip fp16/hip  max|hip - fp32|  max|fp16 - fp32|')
    with torch.no_grad():
        for B in (1, 3):
            px = torch.randn((B, 3, 224, 224), generator=torch.Generator().manual_seed(B)).cuda()
            px16 = px.half()
            fns = [lambda: hip(px), lambda: ref32(pixel_values=px).image_embeds, lambda: ref16(pixel_values=px16).image_embeds]
            outs = [fn() for fn in fns]
            for _ in range(3):
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
            e_hip = float((outs[0][0] - outs[1]).abs().max())
            e_16 = float((outs[2].float() - outs[1]).abs().max())
            th, t32, t16 = _time(fns, args.iters, args.rounds)
            say(f'B = {B}    {_fmt(th)}  {_fmt(t32)}  {_fmt(t16)}  {t32[0] / th[0]:7.2f} {t16[0] / th[0]:7.2f}  {e_hip:14.3e}  {e_16:15.3e}')
        del ref32, ref16
        torch.cuda.empty_cache()
        # where the HIP forward's time goes: the library's own per-launch events (they serialise the launches: the sum exceeds the forward)
        lib = _lib.load()
        px = torch.randn((1, 3, 224, 224), generator=torch.Generator().manual_seed(1)).cuda()
        hip(px)
        torch.cuda.synchronize()
        _lib.check(lib.sdmi_profile_begin())
        hip(px)
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 20)
        _lib.check(lib.sdmi_profile_end(buf, len(buf)))
        rows = sorted(json.loads(buf.value.decode()), key=lambda r: -r['ms'])
        say(f'# libsdmi, B = 1, per kernel class (one event pair per launch): {sum(r["ms"] for r in rows):.3f} ms in '
            f'{sum(r["launches"] for r in rows)} timed launches')
        for r in rows:
            tf = r['flops'] / (r['ms'] * 1e-3) / 1e12 if r['flops'] else 0.0
            say(f'  {r["name"]:<28} n = {r["launches"]:>3} {r["ms"]:8.3f} ms  {tf:7.1f} TFLOP/s  {r["bytes"] / (r["ms"] * 1e-3) / 1e9:8.1f} GB/s')
        g = torch.Generator().manual_seed(5)
        emb = torch.randn((3, 768), generator=g).cuda()
        ce, se = torch.randn((17, 768), generator=g).cuda(), torch.randn((3, 768), generator=g).cuda()
        ct, st = torch.rand((17,), generator=g).cuda(), torch.rand((3,), generator=g).cuda()
        out = vision.safety_head(emb, ce, se, ct, st)
        x = (torch.rand((3, 3, 512, 512), generator=g) * 2 - 1).cuda()
        embedder = vision.FrozenClipImageEmbedderHIP(dict(cfg, num_hidden_layers=1))
        fns = [lambda: vision.safety_head(emb[:1], ce, se, ct, st, out=tuple(o[:1] for o in out)), lambda: vision.safety_head(emb, ce, se, ct, st, out=out),
               lambda: embedder.preprocess(x[:1]), lambda: embedder.preprocess(x)]
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        res = _time(fns, args.iters * 5, args.rounds)
        say('# the small kernels alone (one launch each, through the Python wrapper): ms per call')
        for name, t in zip(('safety_head, B = 1 (17 + 3 concepts, E = 768)', 'safety_head, B = 3', 'vit_preprocess 512 x 512 -> 224, B = 1',
                            'vit_preprocess 512 x 512 -> 224, B = 3'), res):
            say(f'{name:48s} {_fmt(t)}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
