"""The LAION-400M model's txt2img path on the GPU vs the composed CPU restatement (scripts/txt2img.py --laion400m):

    token ids -> BERTEmbedder (cond / uncond) -> PLMSSampler.sample (5 steps, CFG 7.5) -> decode_first_stage (z / 0.18215)
    -> clamp((x + 1) / 2, 0, 1)

as tests/test_pipeline_gpu.py does for the SD-v1 chain, with the BERT encoder in place of CLIP: tests/bert_ref.py +
oracle.unet_ref + oracle.samplers_ref + oracle.vae_ref against BERTEmbedderHIP + PLMSSamplerHIP + AutoencoderKLHIP, on
small configurations (the tiny encoder, dim 128, feeds the tiny UNet, context_dim 128).  The BERT padding ([PAD] = 0 tokens)
is attended, as in the reference.  Tolerances: 2 x the errors measured on an MI355X."""
import torch
import pytest

pytestmark = pytest.mark.gpu

import bert_ref  # noqa: E402
from oracle import samplers_ref, unet_ref, vae_ref  # noqa: E402
from oracle.plan import TINY  # noqa: E402
from oracle.weights import make_state_dict  # noqa: E402

# measured (MI355X): context 2.18e-3, latent 9.28e-3 (|z| max 19), image 5.43e-4 -> 2x
CTX_TOL, LAT_TOL, IMG_TOL = 4.4e-3, 1.9e-2, 1.1e-3


def test_laion_txt2img_pipeline_matches_restatement():
    from stable_diffusion_amd import AutoencoderKLHIP, BERTEmbedderHIP, LatentDiffusionHIP, PLMSSamplerHIP, UNetModelHIP
    bcfg, ucfg, vcfg = bert_ref.TINY_BERT, TINY, vae_ref.TINY_VAE
    assert bcfg.dim == ucfg.context_dim
    bsd = bert_ref.make_bert_state_dict(bcfg, 0)
    usd = make_state_dict(ucfg, 0)
    vsd = vae_ref.make_vae_state_dict(vcfg, 0, encoder=False)
    S, scale, h, w = 5, 7.5, 16, 16
    ids = bert_ref.make_bert_ids(bcfg, 2, 77, seed=3)
    ids[1] = 0
    ids[1, :2] = torch.tensor([101, 102])                         # row 1: the "" of the uncond branch ([CLS] [SEP] [PAD]...)
    g = torch.Generator().manual_seed(42)
    x_T = torch.randn(1, 4, h, w, generator=g)

    # ---- restatement (CPU fp32) ---------------------------------------------------------------------------------------
    ctx = bert_ref.bert_forward(bsd, bcfg, ids)
    c, uc = ctx[0:1], ctx[1:2]
    _, ac = samplers_ref.make_alphas_cumprod()
    z_ref = samplers_ref.plms_sample(lambda x, t, cc: unet_ref.unet_forward(usd, ucfg, x, t, cc), ac, S, x_T, c, scale, uc)
    img_ref = torch.clamp((vae_ref.decode_first_stage(vsd, vcfg, z_ref) + 1.0) / 2.0, min=0.0, max=1.0)

    # ---- HIP (every stage through libsdmi) ------------------------------------------------------------------------------
    bert = BERTEmbedderHIP(**bcfg.embedder_kwargs(), use_tokenizer=False)
    bert.load_state_dict({'transformer.' + k: v for k, v in bsd.items()}, strict=True)
    bert = bert.cuda()
    unet = UNetModelHIP(**ucfg.ref_kwargs())
    unet.load_state_dict(usd, strict=True)
    ld = LatentDiffusionHIP(unet).cuda()
    vae = AutoencoderKLHIP(vcfg.ddconfig(), None, vcfg.embed_dim, parts=1)
    vae.load_state_dict(vsd, strict=True)
    vae = vae.cuda()
    c_h = bert.encode(ids[0:1].cuda())                            # use_tokenizer=False: encode(tokens) (modules.py:94-103)
    uc_h = bert.encode(ids[1:2].cuda())
    z_h, _ = PLMSSamplerHIP(ld).sample(S=S, batch_size=1, shape=[4, h, w], conditioning=c_h, verbose=False, x_T=x_T.cuda(),
                                       unconditional_guidance_scale=scale, unconditional_conditioning=uc_h, eta=0.0)
    img_h = torch.clamp((vae.decode_first_stage(z_h) + 1.0) / 2.0, min=0.0, max=1.0)
    torch.cuda.synchronize()

    e_ctx = max((c_h.float().cpu() - c).abs().max().item(), (uc_h.float().cpu() - uc).abs().max().item())
    e_z = (z_h.float().cpu() - z_ref).abs().max().item()
    e_img = (img_h.float().cpu() - img_ref).abs().max().item()
    print(f'[laion pipeline plms S={S}] context err {e_ctx:.3e} | latent err {e_z:.3e} (|z| max {z_ref.abs().max():.2f}) | '
          f'image err {e_img:.3e} on [0,1] (mean {img_ref.mean():.3f})', flush=True)
    assert img_h.shape == (1, 3, h * vae.factor, w * vae.factor) and torch.isfinite(img_h).all()
    assert e_ctx <= CTX_TOL and e_z <= LAT_TOL and e_img <= IMG_TOL, (e_ctx, e_z, e_img)
