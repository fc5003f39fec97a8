"""An image from a segmentation map with the semantic-synthesis model (models/ldm/semantic_synthesis256 / 512): label map -> the
SpatialRescaler cond stage (csrc/rescale.hip, straight from the labels) -> DDIM over the concat-conditioned UNet -> the VQ-f4 decode -> PNGs.

    python tools/semantic_synthesis.py --labels map.png --ckpt model.ckpt [--steps 50] [--eta 1.0] [--seed 0] [--out outdir]
    python tools/semantic_synthesis.py --labels map.npy --ckpt synthetic

--labels   a label map: a single-channel (mode L / P / I) PNG whose pixel values are class indices, or a `.npy` of [H, W] or [B, H, W]
           integers; classes 0 .. 181.  H and W must be multiples of 16 (resize or crop the map: nothing is padded).
--ckpt     a reference checkpoint (`state_dict` with model.diffusion_model.*, first_stage_model.*, cond_stage_model.*), or `synthetic`
           for seeded random weights
--steps / --eta   DDIM steps and eta;  --seed  the seed of x_T and of the per-step noise;  --hip-precision  the UNet's mode
--out      a directory (default .): one PNG per sample, semantic_00000.png ...
Any map that fits the device runs as one canvas: sliding-window tiling (split_input_params) is not built for this model.
Runs on the GPU only: there is no CPU path."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stable_diffusion_amd import SemanticSynthesisHIP  # noqa: E402


def load_labels(path):
    """[B, H, W] int64 on the host"""
    if path.endswith('.npy'):
        a = np.load(path)
    else:
        from PIL import Image
        img = Image.open(path)
        if img.mode not in ('L', 'P', 'I', 'I;16'):
            raise SystemExit(f'{path}: mode {img.mode}; a label map is single-channel (pixel value = class index)')
        a = np.asarray(img)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or not np.issubdtype(a.dtype, np.integer):
        raise SystemExit(f'{path}: a label map is [H, W] or [B, H, W] of integers, got {a.shape} {a.dtype}')
    return torch.from_numpy(a.astype(np.int64))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--labels', required=True)
    ap.add_argument('--ckpt', required=True)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--eta', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--hip-precision', default='mixed', choices=['mixed', 'full'])
    ap.add_argument('--out', default='.')
    a = ap.parse_args()
    labels = load_labels(a.labels)
    SemanticSynthesisHIP.check_size(int(labels.shape[1]), int(labels.shape[2]))
    if not torch.cuda.is_available():
        raise SystemExit('semantic_synthesis.py needs the GPU: the model has no CPU path')
    from PIL import Image
    m = SemanticSynthesisHIP(hip_precision=a.hip_precision)
    m = (m.load_synthetic(0) if a.ckpt == 'synthetic' else m.load_checkpoint(a.ckpt)).cuda()
    torch.manual_seed(a.seed)
    B, H, W = labels.shape
    x_T = torch.randn(B, 3, H // 4, W // 4, generator=torch.Generator().manual_seed(a.seed)).cuda()
    x = m.synthesize(labels=labels.cuda(), steps=a.steps, eta=a.eta, x_T=x_T)
    x = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)
    os.makedirs(a.out, exist_ok=True)
    paths = []
    for i, img in enumerate((255.0 * x).permute(0, 2, 3, 1).cpu().numpy()):
        paths.append(os.path.join(a.out, f'semantic_{i:05d}.png'))
        Image.fromarray(img.astype(np.uint8)).save(paths[-1])
    print(f'images: {tuple(x.shape)} finite {bool(torch.isfinite(x).all())} mean {float(x.mean()):.3f}; wrote {", ".join(paths)}')


if __name__ == '__main__':
    main()
