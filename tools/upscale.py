"""x4 super-resolution of one PNG with bsr_sr on the MI355X (stable_diffusion_amd.SuperResolutionHIP).

    python tools/upscale.py --ckpt models/ldm/bsr_sr/model.ckpt in.png out.png [--steps 100] [--eta 1.0] [--seed 0] [--precision mixed]
    python tools/upscale.py --ckpt synthetic in.png out.png        (seeded random weights: exercises the path, not the picture)

Inputs with a side above 128 pixels run tiled (128 x 128 windows at stride 64) and must measure 128 + n * 64 on both sides; the tool
names the nearest valid sizes otherwise.  Nothing is padded or resized silently."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ckpt', required=True, help="a reference bsr_sr checkpoint, or 'synthetic'")
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--eta', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--precision', default='mixed', choices=['mixed', 'full'])
    ap.add_argument('input')
    ap.add_argument('output')
    args = ap.parse_args()
    from PIL import Image
    from stable_diffusion_amd import SuperResolutionHIP, postprocess
    if not torch.cuda.is_available():
        raise SystemExit('tools/upscale.py needs the MI355X (there is no CPU path)')
    img = np.asarray(Image.open(args.input).convert('RGB'), dtype=np.float32) / 127.5 - 1.0
    lr = torch.from_numpy(img).permute(2, 0, 1)[None].contiguous()
    sr = SuperResolutionHIP(hip_precision=args.precision)
    sr = (sr.load_synthetic(0) if args.ckpt == 'synthetic' else sr.load_checkpoint(args.ckpt)).cuda()
    try:
        sr.configure_tiling(lr.shape[2], lr.shape[3])
    except ValueError as e:
        raise SystemExit(str(e))
    torch.manual_seed(args.seed)
    up = sr.upscale(lr.cuda(), steps=args.steps, eta=args.eta)
    postprocess.save_png(postprocess.to_uint8_images(up)[0], args.output)
    print(f'{args.input} {tuple(lr.shape[2:])} -> {args.output} {tuple(up.shape[2:])}')


if __name__ == '__main__':
    main()
