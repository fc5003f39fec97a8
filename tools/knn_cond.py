"""The reference's `scripts/knn2img.py --use_neighbors`: prompts (or token ids) -> CLIP text embeds -> exact k-NN in a retrieval database ->
the conditioning tensor c [B, 1 + k, D] -> (with --unet-weights) DDIM sampling with the retrieval-augmented UNet -> decode_first_stage with
the KL-f16 first stage -> PNGs.

    python tools/knn_cond.py --database DIR --knn 10 --prompt "a painting of a virus monster playing guitar" [--text-weights CKPT]
    python tools/knn_cond.py --database DIR --knn 10 --ids-file ids.txt --text-weights CKPT --out cond.pt

--database       a directory of `.npz` files in the reference's layout (embedding, img_id, patch_coords)
--prompt / --from-file   prompts; they need a tokenizer (`--tokenizer`, a local transformers CLIPTokenizer directory)
--ids-file       one line of whitespace-separated token ids per sample instead (no tokenizer needed)
--text-weights   a torch checkpoint of the text encoder: an OpenAI-CLIP state dict or transformers' CLIPTextModelWithProjection one
--queries        skip the text encoder: a `.npy` / `.pt` of query vectors [B, D] (e.g. image embeds)
--unet-weights   also sample (knn2img.py:362-375): a torch checkpoint of the UNet (`model.diffusion_model.*` keys of the model checkpoint, or bare
                 UNetModel keys), or `synthetic` for seeded random weights; --unet picks the configuration (rdm = the yaml; rdm64 = the
                 64-wide stand-in), --steps / --scale / --ddim-eta / --H / --W are the script's options (uc = zeros_like(c) unless --scale 1.0),
                 --out-latents saves samples_ddim [B, 16, H / 16, W / 16].
--vae-weights    the KL-f16 first stage that decodes samples_ddim (knn2img.py:377-378: decode_first_stage, clamp((x + 1) / 2, 0, 1)): a torch
                 checkpoint (`first_stage_model.*` keys of the model checkpoint, or bare AutoencoderKL keys), or `synthetic`; default: whatever
                 --unet-weights is (the model checkpoint holds both).  --outdir (default .) receives one PNG per sample, knn_00000.png ...
Prints the neighbour row ids, image ids and cosines per sample; --out saves {'c', 'nns', 'scores', 'img_ids', 'patch_coords'}.
Runs on the GPU only: there is no CPU path."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stable_diffusion_amd import FrozenCLIPTextEmbedderHIP, SearcherHIP, vision  # noqa: E402


def load_text_encoder(a):
    sd = torch.load(a.text_weights, map_location='cpu')
    sd = sd.get('state_dict', sd)
    if 'text_projection' in sd or 'token_embedding.weight' in sd:
        sd = vision.openai_clip_text_to_transformers(sd)
    sd = {k[len('transformer.'):] if k.startswith('transformer.') else k: v for k, v in sd.items()}
    W = sd['text_model.embeddings.token_embedding.weight'].shape[1]
    layers = 1 + max(int(k.split('.')[3]) for k in sd if k.startswith('text_model.encoder.layers.'))
    tc = dict(vocab_size=sd['text_model.embeddings.token_embedding.weight'].shape[0], hidden_size=W,
              intermediate_size=sd['text_model.encoder.layers.0.mlp.fc1.weight'].shape[0], num_hidden_layers=layers,
              num_attention_heads=max(1, W // 64), max_position_embeddings=sd['text_model.embeddings.position_embedding.weight'].shape[0],
              projection_dim=sd['text_projection.weight'].shape[0])
    tok = object()
    if a.tokenizer:
        from transformers import CLIPTokenizer
        tok = CLIPTokenizer.from_pretrained(a.tokenizer)
    m = FrozenCLIPTextEmbedderHIP(text_config=tc, tokenizer=tok, hip_precision=a.hip_precision)
    m.load_state_dict({'transformer.' + k: v.float() for k, v in sd.items() if not k.endswith('position_ids')}, strict=False)
    return m.cuda()


def sample_latents(cond, a):
    """knn2img.py:362-375 on HIP classes: uc = zeros_like(c), DDIM on a [16, H / 16, W / 16] latent"""
    from stable_diffusion_amd import DDIMSamplerHIP, LatentDiffusionHIP, UNetModelHIP, synthetic
    kw = synthetic.RDM_STANDINS[a.unet]
    unet = UNetModelHIP(**kw, hip_precision=a.hip_precision)
    if a.unet_weights == 'synthetic':
        sd = synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], 0)
    else:
        sd = torch.load(a.unet_weights, map_location='cpu')
        sd = sd.get('state_dict', sd)
        pre = 'model.diffusion_model.'
        if any(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    unet.load_state_dict(sd, strict=True)
    if cond.shape[2] != kw['context_dim']:
        raise SystemExit(f'the conditioning has {cond.shape[2]} channels, this UNet takes context_dim = {kw["context_dim"]}')
    ld = LatentDiffusionHIP(unet.cuda(), **synthetic.RDM_SCHEDULE).cuda()
    uc = torch.zeros_like(cond) if a.scale != 1.0 else None
    shape = [kw['in_channels'], a.H // 16, a.W // 16]                # (knn2img.py:366: hardcoded for the f16 model)
    samples, _ = DDIMSamplerHIP(ld).sample(S=a.steps, conditioning=cond, batch_size=cond.shape[0], shape=shape, verbose=False,
                                           unconditional_guidance_scale=a.scale, unconditional_conditioning=uc, eta=a.ddim_eta)
    return samples


def decode_latents(samples, a):
    """knn2img.py:377-386: x = decode_first_stage(samples_ddim) with the yaml's scale_factor, clamp((x + 1) / 2, 0, 1), one PNG per sample"""
    from PIL import Image
    from stable_diffusion_amd import AutoencoderKLHIP, synthetic
    kw = synthetic.KL_F16_KWARGS
    vae = AutoencoderKLHIP(kw['ddconfig'], None, kw['embed_dim'], parts=1, hip_precision=a.hip_precision)
    src = a.vae_weights or a.unet_weights
    if src == 'synthetic':
        sd = synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in vae.state_dict().items()], 0)
    else:
        sd = torch.load(src, map_location='cpu')
        sd = sd.get('state_dict', sd)
        pre = 'first_stage_model.'
        if any(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        sd = {k: v for k, v in sd.items() if k in vae.state_dict()}          # (a decoder-only handle: encoder.* / loss.* are not its keys)
    vae.load_state_dict(sd, strict=True)
    x = vae.cuda().decode_first_stage(samples, scale_factor=synthetic.KL_F16_SCALE_FACTOR)
    x = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)
    os.makedirs(a.outdir, exist_ok=True)
    paths = []
    for i, img in enumerate((255.0 * x).permute(0, 2, 3, 1).cpu().numpy()):
        paths.append(os.path.join(a.outdir, f'knn_{i:05d}.png'))
        Image.fromarray(img.astype(np.uint8)).save(paths[-1])
    return x, paths


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--database', required=True)
    ap.add_argument('--knn', type=int, default=10)
    ap.add_argument('--prompt', action='append')
    ap.add_argument('--from-file')
    ap.add_argument('--ids-file')
    ap.add_argument('--queries')
    ap.add_argument('--text-weights')
    ap.add_argument('--tokenizer')
    ap.add_argument('--hip-precision', default='mixed', choices=['mixed', 'full'])
    ap.add_argument('--out')
    ap.add_argument('--unet-weights')
    ap.add_argument('--unet', default='rdm', choices=['rdm', 'rdm64'])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--scale', type=float, default=5.0)
    ap.add_argument('--ddim-eta', type=float, default=0.0)
    ap.add_argument('--H', type=int, default=768)
    ap.add_argument('--W', type=int, default=768)
    ap.add_argument('--out-latents')
    ap.add_argument('--vae-weights')
    ap.add_argument('--outdir', default='.')
    a = ap.parse_args()
    if a.unet_weights and (a.H % 128 or a.W % 128):
        raise SystemExit('--H and --W must be multiples of 128 (a 16x smaller latent, halved three times by the UNet)')
    if not torch.cuda.is_available():
        raise SystemExit('knn_cond.py needs the GPU: the text encoder and the search have no CPU path')
    if a.queries:
        q = np.load(a.queries) if a.queries.endswith('.npy') else torch.load(a.queries, map_location='cpu')
        c = torch.as_tensor(q, dtype=torch.float32).reshape(len(q), 1, -1).cuda()
    else:
        if not a.text_weights:
            raise SystemExit('give --text-weights (the text encoder checkpoint) or --queries (ready query vectors)')
        enc = load_text_encoder(a)
        if a.ids_file:
            ids = torch.tensor([[int(t) for t in line.split()] for line in open(a.ids_file) if line.strip()], dtype=torch.int64)
            c = enc.encode_ids(ids.cuda())[:, None]
        else:
            prompts = list(a.prompt or [])
            if a.from_file:
                prompts += [line.rstrip('\n') for line in open(a.from_file) if line.strip()]
            if not prompts:
                raise SystemExit('give --prompt, --from-file or --ids-file')
            if not a.tokenizer:
                raise SystemExit('prompts need --tokenizer (a local CLIPTokenizer directory); --ids-file takes token ids instead')
            c = enc.encode(prompts)                        # knn2img.py: c = clip_text_encoder.encode(prompts)
    searcher = SearcherHIP(a.database)
    cond, idx, score = searcher.condition(c, a.knn, return_neighbours=True)      # knn2img.py: searcher(c, opt.knn) + torch.cat([c, nn], dim=1)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    for b in range(idx.shape[0]):
        print(f'sample {b}:')
        for j in range(idx.shape[1]):
            print(f'  {j:2d}  row {idx[b, j]:9d}  img_id {searcher.img_id[idx[b, j]]}  cosine {score[b, j]:.6f}')
    print(f'c: {tuple(cond.shape)} {cond.dtype} on {cond.device}')
    if a.out:
        torch.save({'c': cond.cpu(), 'nns': torch.from_numpy(idx.astype(np.int64)), 'scores': torch.from_numpy(score),
                    'img_ids': torch.from_numpy(np.asarray(searcher.img_id[idx]).astype(np.int64)),
                    'patch_coords': torch.from_numpy(np.asarray(searcher.patch_coords[idx]))}, a.out)
    if a.unet_weights:
        samples = sample_latents(cond, a)
        print(f'samples_ddim: {tuple(samples.shape)} finite {bool(torch.isfinite(samples).all())} |x| max {float(samples.abs().max()):.3f}')
        if a.out_latents:
            torch.save(samples.cpu(), a.out_latents)
        x, paths = decode_latents(samples, a)
        print(f'x_samples_ddim: {tuple(x.shape)} finite {bool(torch.isfinite(x).all())} mean {float(x.mean()):.3f}; wrote {", ".join(paths)}')


if __name__ == '__main__':
    main()
