"""Time the latent-inpainting model on one MI355X: one UNet call, and one inpaint image as scripts/inpaint.py runs it
(encode the masked image, 50 DDIM steps with the concat conditioning, decode), with seeded synthetic weights.

    python tools/bench_inpaint.py [--image 512] [--steps 50] [--calls 20] [--precision mixed]

Prints one JSON line: ms per UNet call, ms per image (and its parts), the UNet's fraction of the dense fp16 MFMA peak, and the
quantizer's time at the image's latent size."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0      # dense fp16 MFMA peak of the MI355X (bench.py)


def unet_flops(kw, B, H, W):
    """Multiply-add FLOPs (x 2) of one UNetModel call of the AttentionBlock family: 3x3 / 1x1 convs and both attention products."""
    mc, mult, nrb, attn = kw['model_channels'], kw['channel_mult'], kw['num_res_blocks'], set(kw['attention_resolutions'])
    f = 0.0
    conv = lambda hw, ci, co, k: 2.0 * B * hw * ci * co * k * k

    def res(hw_in, hw_out, ci, co):
        return conv(hw_out, ci, co, 3) + conv(hw_out, co, co, 3) + (conv(hw_out, ci, co, 1) if ci != co else 0.0)

    def att(hw, c):
        return conv(hw, c, 3 * c, 1) + conv(hw, c, c, 1) + 4.0 * B * hw * hw * c
    hw, ds, ch = H * W, 1, mc
    f += conv(hw, kw['in_channels'], mc, 3)
    chans = [ch]
    for lvl, m in enumerate(mult):
        for _ in range(nrb):
            f += res(hw, hw, ch, m * mc); ch = m * mc
            if ds in attn: f += att(hw, ch)
            chans.append(ch)
        if lvl != len(mult) - 1:
            f += res(hw, hw // 4, ch, ch); hw //= 4; ds *= 2; chans.append(ch)
    f += 2 * res(hw, hw, ch, ch) + att(hw, ch)
    for lvl in reversed(range(len(mult))):
        for i in range(nrb + 1):
            ich = chans.pop()
            f += res(hw, hw, ch + ich, mult[lvl] * mc); ch = mult[lvl] * mc
            if ds in attn: f += att(hw, ch)
            if lvl and i == nrb:
                f += res(hw, hw * 4, ch, ch); hw *= 4; ds //= 2
    f += conv(hw, mc, kw['out_channels'], 3)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--image', type=int, default=512)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--precision', default='mixed', choices=['mixed', 'full'])
    args = ap.parse_args()
    from stable_diffusion_amd import DDIMSamplerHIP, LatentDiffusionHIP, UNetModelHIP, VQModelInterfaceHIP, synthetic
    dev = 'cuda'
    unet = UNetModelHIP(**synthetic.INPAINT_UNET_KWARGS, hip_precision=args.precision)
    unet.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], 0))
    unet = unet.to(dev)
    vq = VQModelInterfaceHIP(**synthetic.INPAINT_VQ_KWARGS)
    vq.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in vq.state_dict().items()], 0))
    vq = vq.to(dev)
    ld = LatentDiffusionHIP(unet, **synthetic.INPAINT_SCHEDULE).to(dev)
    S, lat = args.image, args.image // 4
    g = torch.Generator().manual_seed(0)
    image = (torch.rand(1, 3, S, S, generator=g) * 2 - 1).to(dev)
    mask = torch.zeros(1, 1, S, S)
    mask[:, :, S // 4: 3 * S // 4, S // 4: 3 * S // 4] = 1
    mask = mask.to(dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    # ---- one UNet call ----
    x = torch.randn(1, 7, lat, lat, generator=g).to(dev)
    t = torch.full((1,), 501, dtype=torch.long, device=dev)
    for _ in range(3):
        unet(x, t)
    torch.cuda.synchronize()
    a, b = ev(), ev()
    a.record()
    for _ in range(args.calls):
        unet(x, t)
    b.record()
    torch.cuda.synchronize()
    ms_unet = a.elapsed_time(b) / args.calls
    flops = unet_flops(synthetic.INPAINT_UNET_KWARGS, 1, lat, lat)

    # ---- quantizer alone ----
    z = torch.randn(1, 3, lat, lat, generator=g).to(dev)
    vq.quantize(z)
    torch.cuda.synchronize()
    a.record()
    for _ in range(20):
        vq.quantize(z)
    b.record()
    torch.cuda.synchronize()
    ms_quant = a.elapsed_time(b) / 20

    # ---- one inpaint image (scripts/inpaint.py loop body) ----
    sampler = DDIMSamplerHIP(ld)

    def image_once():
        parts = [ev() for _ in range(4)]
        parts[0].record()
        masked = (1 - mask) * image
        c = vq.encode(masked)
        cc = torch.nn.functional.interpolate(mask, size=c.shape[-2:])
        c = torch.cat((c, cc), dim=1)
        parts[1].record()
        samples, _ = sampler.sample(S=args.steps, conditioning=c, batch_size=c.shape[0], shape=(c.shape[1] - 1,) + tuple(c.shape[2:]),
                                    verbose=False)
        parts[2].record()
        x_samples = vq.decode(samples)
        img = torch.clamp((image + 1.0) / 2.0, min=0.0, max=1.0)
        m = torch.clamp((mask + 1.0) / 2.0, min=0.0, max=1.0)
        pred = torch.clamp((x_samples + 1.0) / 2.0, min=0.0, max=1.0)
        out = (1 - m) * img + m * pred
        parts[3].record()
        torch.cuda.synchronize()
        return out, [parts[i].elapsed_time(parts[i + 1]) for i in range(3)]

    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        image_once()
        out, ms_parts = image_once()
    res = {'metric': 'inpaint_big', 'precision': args.precision, 'image': S, 'latent': lat, 'ddim_steps': args.steps,
           'ms_per_unet_call': round(ms_unet, 3), 'unet_gflop_per_call': round(flops / 1e9, 1),
           'unet_mfma_peak_fraction': round(flops / (ms_unet * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
           'ms_per_image': round(sum(ms_parts), 2), 'ms_encode': round(ms_parts[0], 2), 'ms_sample': round(ms_parts[1], 2),
           'ms_decode_blend': round(ms_parts[2], 2), 'ms_quantize': round(ms_quant, 4), 'finite': bool(torch.isfinite(out).all())}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
