"""The reference's `scripts/sample_diffusion.py` `run()` for the unconditional models, on the HIP classes:

    python tools/sample_diffusion.py --model churches --vanilla_sample -n 8 --batch_size 8 [--ckpt model.ckpt] [--logdir out]
    python tools/sample_diffusion.py --model faces --custom_steps 50 --eta 1.0 -n 16 --batch_size 8

--model          churches (LSUN-Churches: KL-f8 first stage, 4 x 32 x 32 latent) or faces (the face / bedroom family: VQ-f4, 3 x 64 x 64)
--vanilla_sample the 1000-step ancestral sampler: LatentDiffusionHIP.progressive_denoising, as the script's convsample calls it
                 (sample_diffusion.py:54-65, :91-93); without it --custom_steps / --eta run DDIMSamplerHIP (:69-75)
--quantize       quantize_denoised (vanilla) / quantize_x0 (DDIM) on the VQ first stage's codebook (faces only)
--ckpt           a reference checkpoint (`state_dict` with model.diffusion_model.* and first_stage_model.*); default: seeded synthetic
                 weights -- the images are then noise-like, the run is the real one
Writes <logdir>/img/sample_000000.png ... and <logdir>/numpy/<N>x<H>x<W>x3-samples.npz (uint8, as custom_to_np: sample_diffusion.py:27-33).
Runs on the GPU only: there is no CPU path."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_model(a):
    from stable_diffusion_amd import AutoencoderKLHIP, LatentDiffusionHIP, UNetModelHIP, VQModelInterfaceHIP, synthetic
    if a.model == 'churches':
        ukw, sched = synthetic.CHURCHES_UNET_KWARGS, synthetic.CHURCHES_SCHEDULE
        fs = AutoencoderKLHIP(synthetic.CHURCHES_VAE_DDCONFIG, None, 4)
        log_every_t = 200                                     # models/ldm/lsun_churches256/config.yaml
    else:
        ukw, sched = synthetic.FACES_UNET_KWARGS, synthetic.FACES_SCHEDULE
        fs = VQModelInterfaceHIP(**synthetic.FACES_VQ_KWARGS)
        log_every_t = 100
    unet = UNetModelHIP(**ukw, hip_precision=a.hip_precision)
    if a.ckpt:
        sd = torch.load(a.ckpt, map_location='cpu')
        sd = sd.get('state_dict', sd)
        for prefix, m in (('model.diffusion_model.', unet), ('first_stage_model.', fs)):
            want = set(m.state_dict())
            m.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix) and k[len(prefix):] in want}, strict=True)
        scale_factor = float(sd['scale_factor']) if 'scale_factor' in sd else 1.0         # (a scale_by_std model stores it)
    else:
        for m in (unet, fs):
            m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], a.seed), strict=True)
        scale_factor = 1.0
    ld = LatentDiffusionHIP(unet, first_stage_model=fs, scale_factor=scale_factor, log_every_t=log_every_t, channels=ukw['in_channels'],
                            image_size=ukw['image_size'], **sched)
    return ld.cuda()


@torch.no_grad()
def make_convolutional_sample(model, a):
    """sample_diffusion.py:78-106"""
    from stable_diffusion_amd import DDIMSamplerHIP
    unet = model.model.diffusion_model
    shape = [a.batch_size, unet.in_channels, unet.image_size, unet.image_size]
    t0 = time.time()
    if a.vanilla_sample:
        sample, _ = model.progressive_denoising(None, shape, verbose=True, quantize_denoised=a.quantize)
    else:
        sample, _ = DDIMSamplerHIP(model).sample(a.custom_steps, batch_size=shape[0], shape=shape[1:], eta=a.eta, verbose=False,
                                                 quantize_x0=a.quantize)
    torch.cuda.synchronize()
    t1 = time.time()
    x_sample = model.decode_first_stage(sample)
    print(f'Throughput for this batch: {sample.shape[0] / (t1 - t0)}')
    return x_sample


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--model', choices=['churches', 'faces'], default='churches')
    ap.add_argument('--ckpt', default=None)
    ap.add_argument('-n', '--n_samples', type=int, default=8)
    ap.add_argument('--batch_size', type=int, default=8)
    ap.add_argument('-v', '--vanilla_sample', action='store_true')
    ap.add_argument('-c', '--custom_steps', type=int, default=50)
    ap.add_argument('-e', '--eta', type=float, default=1.0)
    ap.add_argument('--quantize', action='store_true')
    ap.add_argument('-l', '--logdir', default='sample_diffusion_out')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--hip-precision', dest='hip_precision', choices=['mixed', 'full'], default='mixed')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/sample_diffusion.py needs the MI355X (the HIP path has no CPU fallback)')
    from stable_diffusion_amd import postprocess
    torch.manual_seed(a.seed)
    model = build_model(a)
    if a.vanilla_sample:
        print(f'Using Vanilla DDPM sampling with {model.num_timesteps} sampling steps.')
    else:
        print(f'Using DDIM sampling with {a.custom_steps} sampling steps and eta={a.eta}')
    imgdir, npdir = os.path.join(a.logdir, 'img'), os.path.join(a.logdir, 'numpy')
    os.makedirs(imgdir, exist_ok=True)
    os.makedirs(npdir, exist_ok=True)
    tstart, all_images, n_saved = time.time(), [], 0
    while n_saved < a.n_samples:
        x = make_convolutional_sample(model, a)
        u8 = ((x.detach().float() + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu()     # custom_to_np
        for img in u8[:a.n_samples - n_saved]:
            postprocess.save_png(img, os.path.join(imgdir, f'sample_{n_saved:06}.png'))
            n_saved += 1
        all_images.append(u8.numpy())
    all_img = np.concatenate(all_images, axis=0)[:a.n_samples]
    path = os.path.join(npdir, 'x'.join(str(v) for v in all_img.shape) + '-samples.npz')
    np.savez(path, all_img)
    print(f'sampling of {n_saved} images finished in {(time.time() - tstart) / 60.:.2f} minutes; {path}')


if __name__ == '__main__':
    main()
