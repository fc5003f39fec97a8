"""Seeded random weights in the SD-v1 UNet architecture (there is no checkpoint in the build environment).

Used by bench.py, the launcher and smoke runs.  Default-initialised reference weights give eps == 0
(`zero_module`, openaimodel.py:229-231,685; attention.py:244-248), so every tensor is drawn here.
Throughput is value independent; the values only need to keep activations O(1).
"""
import math

import torch


@torch.no_grad()
def randomize_(unet, seed=0):
    """In-place init of a UNetModelHIP (or anything with the same parameter names)."""
    dev = next(unet.parameters()).device
    g = torch.Generator(device=dev).manual_seed(seed)
    for name, p in unet.named_parameters():
        if name.endswith('.weight') and p.dim() >= 2:
            fan_in = p[0].numel()
            zero_init = name.endswith('out_layers.3.weight') or name.endswith('proj_out.weight') or name == 'out.2.weight'
            std = (0.5 if zero_init else 0.577) / math.sqrt(fan_in)
            p.copy_(torch.randn(p.shape, generator=g, device=dev) * std)
        elif name.endswith('.weight'):      # norm gamma
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g, device=dev))
        else:                               # biases / norm beta
            p.copy_(0.02 * torch.randn(p.shape, generator=g, device=dev))
    if hasattr(unet, 'mark_dirty'):
        unet.mark_dirty()
    return unet


@torch.no_grad()
def randomize_vae_(vae, seed=0):
    """In-place unit-gain init of an AutoencoderKLHIP (or anything with the same parameter names)."""
    dev = next(vae.parameters()).device
    g = torch.Generator(device=dev).manual_seed(seed)
    for name, p in vae.named_parameters():
        if name.endswith('.weight') and p.dim() >= 2:
            p.copy_(torch.randn(p.shape, generator=g, device=dev) / math.sqrt(p[0].numel()))
        elif name.endswith('.weight'):
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g, device=dev))
        else:
            p.copy_(0.02 * torch.randn(p.shape, generator=g, device=dev))
    if hasattr(vae, 'mark_dirty'):
        vae.mark_dirty()
    return vae


def synthetic_state_dict(unet_kwargs, seed=0):
    """CPU state_dict (reference key names) of a seeded random SD-v1-architecture UNet."""
    from .unet import UNetModelHIP
    m = UNetModelHIP(**unet_kwargs)
    randomize_(m, seed)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def synthetic_vae_state_dict(ddconfig, embed_dim=4, seed=0):
    """CPU state_dict (reference key names: encoder.*, decoder.*, quant_conv.*, post_quant_conv.*) of a seeded random
    first stage in the given architecture."""
    from .vae import AutoencoderKLHIP
    m = AutoencoderKLHIP(ddconfig, None, embed_dim)
    randomize_vae_(m, seed)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@torch.no_grad()
def synthetic_clip_state_dict(text_config=None, seed=0):
    """CPU state_dict (keys `transformer.text_model.*`, as under `cond_stage_model.` in an SD checkpoint) of a seeded
    random CLIP text tower."""
    from .clip import FrozenCLIPEmbedderHIP
    m = FrozenCLIPEmbedderHIP(text_config=text_config, tokenizer=object())
    g = torch.Generator().manual_seed(seed)
    for name, p in m.named_parameters():
        if 'embedding' in name:
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
        elif name.endswith('.weight') and p.dim() == 2:
            p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p.shape[1]))
        elif name.endswith('.weight'):
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
        else:
            p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}



# ---- the CLIP vision tower (safety checker, image embedder) ------------------------------------------------------------------------------
# the smallest geometry with every tail: 5 tokens (padded to 8), d = 32, GEMM rows 15 (B = 3), K = 588 zero-padded to 640
VIT_TINY = dict(image_size=28, patch_size=14, hidden_size=64, num_attention_heads=2, num_hidden_layers=2, intermediate_size=128,
                projection_dim=32)
# ViT-L/14's widths and its 257 tokens (nkv_pad 264, eight 32-query slices plus one row, d = 64) with 2 of the 24 layers
VIT_L14_THIN = dict(image_size=224, patch_size=14, hidden_size=1024, num_attention_heads=16, num_hidden_layers=2, intermediate_size=4096,
                    projection_dim=768)


@torch.no_grad()
def synthetic_vision_state_dict(cfg=None, seed=0):
    """CPU state_dict (CLIPVisionModelWithProjection key names) of a seeded random CLIP vision tower, one generator per key.  Scaled so that
    every LayerNorm input has rms of order 1: class / position embeddings 0.5 N, the patch convolution 1 / sqrt(3 p^2) N (unit gain on
    N(0, 1) pixel values), linear weights 1 / sqrt(fan_in) N, norm gammas 1 + 0.1 N, biases / betas 0.02 N."""
    from .vision import CLIPVisionHIP
    specs = CLIPVisionHIP(cfg)._specs
    sd = {}
    for name, shape in specs:
        g = _key_generator(name, seed)
        if name.endswith(('class_embedding', 'position_embedding.weight')):
            t = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith('.weight') and len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        elif name.endswith('.weight'):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.02 * torch.randn(shape, generator=g)
        sd[name] = t
    return sd


@torch.no_grad()
def synthetic_bert_state_dict(n_embed=1280, n_layer=32, vocab_size=30522, max_seq_len=77, seed=0):
    """CPU state_dict (keys `transformer.*`, as under `cond_stage_model.` in the LAION-400M checkpoint) of a seeded random
    BERTEmbedder transformer, to_logits included."""
    from .bert import make_bert_cfg, _BertHandle
    specs = _BertHandle(make_bert_cfg(n_embed, n_layer, vocab_size, max_seq_len)).weight_specs()
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in specs:
        if name.startswith(('token_emb', 'pos_emb')):
            t = torch.randn(shape, generator=g) * 0.5
        elif name.endswith('.weight') and len(shape) == 2:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        elif name.endswith('.weight'):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.02 * torch.randn(shape, generator=g)
        sd['transformer.' + name] = t
    return sd

SD_V1_UNET_KWARGS = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320,
                         attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8,
                         use_spatial_transformer=True, transformer_depth=1, context_dim=768, use_checkpoint=True,
                         legacy=False)   # configs/stable-diffusion/v1-inference.yaml:29-44

SD_V1_VAE_DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                          ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)   # yaml:51-65

LAION_UNET_KWARGS = dict(SD_V1_UNET_KWARGS, context_dim=1280)     # configs/latent-diffusion/txt2img-1p4B-eval.yaml:21-42
LAION_BERT_KWARGS = dict(n_embed=1280, n_layer=32)                 # yaml:67-71

# ---- the latent-inpainting model (models/ldm/inpainting_big/config.yaml) ----------------------------------------------------
INPAINT_UNET_KWARGS = dict(image_size=64, in_channels=7, out_channels=3, model_channels=256, attention_resolutions=[8, 4, 2],
                           num_res_blocks=2, channel_mult=[1, 2, 3, 4], num_heads=8, resblock_updown=True)   # yaml:24-41
INPAINT_VQ_DDCONFIG = dict(attn_type='none', double_z=False, z_channels=3, resolution=256, in_channels=3, out_ch=3, ch=128,
                           ch_mult=[1, 2, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)          # yaml:45-61
INPAINT_VQ_KWARGS = dict(embed_dim=3, n_embed=8192, ddconfig=INPAINT_VQ_DDCONFIG)
INPAINT_SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.0205, conditioning_key='concat')   # yaml:5-14


# ---- the class-conditional ImageNet model (configs/latent-diffusion/cin256-v2.yaml) -----------------------------------------
CIN_UNET_KWARGS = dict(image_size=64, in_channels=3, out_channels=3, model_channels=192, attention_resolutions=[8, 4, 2],
                       num_res_blocks=2, channel_mult=[1, 2, 3, 5], num_heads=1, use_spatial_transformer=True, transformer_depth=1,
                       context_dim=512)                                                                    # yaml:19-39 (legacy stays True)
# (no attn_type in this yaml: the first stage's mid-block attention is on, unlike the inpainting model's)
CIN_VQ_DDCONFIG = dict(double_z=False, z_channels=3, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4],
                       num_res_blocks=2, attn_resolutions=[], dropout=0.0)                                 # yaml:46-59
CIN_VQ_KWARGS = dict(embed_dim=3, n_embed=8192, ddconfig=CIN_VQ_DDCONFIG)
CIN_SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.0195)                                # yaml:5-9, conditioning_key crossattn
CIN_CLASS_KWARGS = dict(n_classes=1001, embed_dim=512, key='class_label')                                  # yaml:63-68 (class 1000 = unconditional)


# ---- the unconditional LSUN-Churches model (models/ldm/lsun_churches256/config.yaml) ------------------------------------------
CHURCHES_UNET_KWARGS = dict(image_size=32, in_channels=4, out_channels=4, model_channels=192, attention_resolutions=[1, 2, 4, 8],
                            num_res_blocks=2, channel_mult=[1, 2, 2, 4, 4], num_heads=8, use_scale_shift_norm=True,
                            resblock_updown=True)                                                          # yaml:33-52
CHURCHES_VAE_DDCONFIG = SD_V1_VAE_DDCONFIG                     # yaml:57-71: the KL-f8 autoencoder with SD v1's ddconfig, embed_dim 4
CHURCHES_SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.0155, conditioning_key=None)   # yaml:5-6,9; unconditional


def _key_generator(name, seed):
    """One CPU generator per tensor, seeded by (seed, key name): the values do not depend on the order the keys are listed in
    (the reference modules and the HIP modules enumerate their parameters in different orders)."""
    import zlib
    return torch.Generator().manual_seed((int(seed) * 1000003 + zlib.crc32(name.encode())) & 0x7fffffffffffffff)


@torch.no_grad()
def synthetic_named_state_dict(specs, seed=0, codebook_std=1.0):
    """CPU fp32 state_dict for a list of (key, shape): deterministic per (seed, key).  Every `zero_module` tensor of the reference
    (out_layers.3, proj_out, out.2) is drawn too -- at 0.5 / sqrt(fan_in) -- so that the attention and ResBlock branches contribute;
    other weights 0.577 / sqrt(fan_in) (unit gain through the 1x1 / 3x3 convs), norm gammas 1 + 0.1 N, biases / betas 0.02 N,
    a codebook (quantize.embedding.weight) codebook_std * N, a class table (embedding.weight) N."""
    sd = {}
    for name, shape in specs:
        shape = tuple(int(s) for s in shape)
        g = _key_generator(name, seed)
        if name == 'quantize.embedding.weight':
            t = codebook_std * torch.randn(shape, generator=g)
        elif name == 'embedding.weight':               # ClassEmbedder: nn.Embedding's own N(0, 1), so that the context is O(1)
            t = torch.randn(shape, generator=g)
        elif name.endswith('.weight') and len(shape) >= 2:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            zero_init = name.endswith('out_layers.3.weight') or name.endswith('proj_out.weight') or name == 'out.2.weight'
            t = torch.randn(shape, generator=g) * ((0.5 if zero_init else 0.577) / math.sqrt(fan_in))
        elif name.endswith('.weight'):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.02 * torch.randn(shape, generator=g)
        sd[name] = t
    return sd


def synthetic_inpaint_unet_state_dict(seed=0, unet_kwargs=None):
    """CPU state_dict (reference UNetModel key names) of a seeded random latent-inpainting UNet."""
    from .unet import UNetModelHIP
    m = UNetModelHIP(**(unet_kwargs or INPAINT_UNET_KWARGS))
    return synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)


def synthetic_inpaint_vq_state_dict(seed=0, vq_kwargs=None):
    """CPU state_dict (reference VQModelInterface key names, without loss.*) of a seeded random VQ first stage."""
    from .vae import VQModelInterfaceHIP
    m = VQModelInterfaceHIP(**(vq_kwargs or INPAINT_VQ_KWARGS))
    return synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)


def synthetic_churches_unet_state_dict(seed=0, unet_kwargs=None):
    """CPU state_dict (reference UNetModel key names) of a seeded random unconditional LSUN-Churches UNet."""
    from .unet import UNetModelHIP
    m = UNetModelHIP(**(unet_kwargs or CHURCHES_UNET_KWARGS))
    return synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)


# ---- the face / bedroom models (models/ldm/celeba256, ffhq256, lsun_beds256: one unet_config) and bsr_sr's UNet -----------------
FACES_UNET_KWARGS = dict(image_size=64, in_channels=3, out_channels=3, model_channels=224, attention_resolutions=[8, 4, 2],
                         num_res_blocks=2, channel_mult=[1, 2, 3, 4], num_head_channels=32)                # celeba256 yaml:17-33
FACES_VQ_KWARGS = dict(embed_dim=3, n_embed=8192, ddconfig=CIN_VQ_DDCONFIG)                               # yaml:34-52: VQ-f4, mid-block attention on
FACES_SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.0195, conditioning_key=None)      # yaml:5-6,9; __is_unconditional__
BSR_UNET_KWARGS = dict(image_size=64, in_channels=6, out_channels=3, model_channels=160, attention_resolutions=[16, 8],
                       num_res_blocks=2, channel_mult=[1, 2, 2, 4], num_head_channels=32)                  # bsr_sr yaml:16-31
BSR_SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.0155, conditioning_key='concat')    # yaml:5-6,8,14 (concat_mode)


# ---- the semantic-synthesis models (models/ldm/semantic_synthesis256, semantic_synthesis512: one unet_config but image_size) ----------
SEMANTIC_UNET_KWARGS = dict(image_size=128, in_channels=6, out_channels=3, model_channels=128, attention_resolutions=[32, 16, 8],
                            num_res_blocks=2, channel_mult=[1, 4, 8], num_heads=8)                         # semantic_synthesis512 yaml:16-32
SEMANTIC_RESCALER_KWARGS = dict(n_stages=2, in_channels=182, out_channels=3)                               # yaml:55-60 (the VQ-f4 stage: FACES_VQ_KWARGS)
SEMANTIC_SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.0205, conditioning_key='concat')   # yaml:5-6,8,14 (concat_mode)


def synthetic_faces_unet_state_dict(seed=0, unet_kwargs=None):
    """CPU state_dict (reference UNetModel key names) of a seeded random face / bedroom UNet (or, with BSR_UNET_KWARGS, bsr_sr's)."""
    from .unet import UNetModelHIP
    m = UNetModelHIP(**(unet_kwargs or FACES_UNET_KWARGS))
    return synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)


def synthetic_faces_vq_state_dict(seed=0, vq_kwargs=None):
    """CPU state_dict (reference VQModelInterface key names, without loss.*) of a seeded random VQ-f4 first stage of the face models."""
    from .vae import VQModelInterfaceHIP
    m = VQModelInterfaceHIP(**(vq_kwargs or FACES_VQ_KWARGS))
    return synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)


# ---- the retrieval-augmented model (configs/retrieval-augmented-diffusion/768x768.yaml) and layout-to-image -------------------
# SD v1's SpatialTransformer blocks with num_head_channels = 32 (14 / 28 / 42 / 56 heads at 448 .. 1792 channels), 16 latent channels
RDM_UNET_KWARGS = dict(image_size=48, in_channels=16, out_channels=16, model_channels=448, attention_resolutions=[4, 2, 1],
                       num_res_blocks=2, channel_mult=[1, 2, 3, 4], use_scale_shift_norm=False, resblock_updown=False,
                       num_head_channels=32, use_spatial_transformer=True, transformer_depth=1, context_dim=768,
                       use_checkpoint=True)                                                                # yaml:19-42
RDM_SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.015, conditioning_key='crossattn')   # yaml:5-6,9,15
LAYOUT_UNET_KWARGS = dict(image_size=64, in_channels=3, out_channels=3, model_channels=128, attention_resolutions=[8, 4, 2],
                          num_res_blocks=2, channel_mult=[1, 2, 3, 4], num_head_channels=32, use_spatial_transformer=True,
                          transformer_depth=3, context_dim=512)              # models/ldm/layout2img-openimages256/config.yaml:16-36
# stand-ins of the retrieval-augmented UNet for the tests.  RDM64: the yaml at model_channels 64 (2 / 4 / 6 / 8 heads, 30.2 M parameters).
# RDM448X2: the real width over two levels -- the real head counts 14 / 28 and the real 14 / 28 / 42 channels per GroupNorm group.
RDM64_UNET_KWARGS = dict(RDM_UNET_KWARGS, model_channels=64)
RDM448X2_UNET_KWARGS = dict(RDM_UNET_KWARGS, channel_mult=[1, 2], attention_resolutions=[1, 2], num_res_blocks=1)
# RDM320X1: one level of 320 channels -- 10 heads of 32: the one width at which this family runs the row-strip chain launches (C == 320)
RDM320X1_UNET_KWARGS = dict(RDM_UNET_KWARGS, model_channels=320, channel_mult=[1], attention_resolutions=[1], num_res_blocks=1)
RDM_STANDINS = {'rdm64': RDM64_UNET_KWARGS, 'rdm448x2': RDM448X2_UNET_KWARGS, 'rdm320x1': RDM320X1_UNET_KWARGS, 'layout': LAYOUT_UNET_KWARGS,
                'rdm': RDM_UNET_KWARGS}


def synthetic_rdm_unet_state_dict(seed=0, unet_kwargs=None):
    """CPU state_dict (reference UNetModel key names) of a seeded random retrieval-augmented UNet (or a stand-in / layout-to-image)."""
    from .unet import UNetModelHIP
    m = UNetModelHIP(**(unet_kwargs or RDM_UNET_KWARGS))
    return synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)


# ---- KL-f16, the first stage of the retrieval-augmented model (models/first_stage_models/kl-f16) ------------------------------------------
# AttnBlocks after every ResBlock of the 16 x 16 level (level 4: d = 512), 16 latent channels: a 32-channel encoder.conv_out and quant_conv
KL_F16_DDCONFIG = dict(double_z=True, z_channels=16, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 1, 2, 2, 4],
                       num_res_blocks=2, attn_resolutions=[16], dropout=0.0)                                   # 768x768.yaml:48-64
KL_F16_KWARGS = dict(embed_dim=16, ddconfig=KL_F16_DDCONFIG)                                                   # yaml:47
KL_F16_SCALE_FACTOR = 0.22765929                                                                               # yaml:13
# stand-ins for the tests.  kl_f16_thin: the yaml at ch 64 -- level attention at d = 256 (the wide flash kernel), z = 16.  kl_narrow: two levels
# with attention on the lower one at d = 128 (attn.hip), z = 4.  kl_two_levels: the same with attention on both levels (two mask bits), d = 64
# at the full image resolution.
KL_F16_THIN_DDCONFIG = dict(KL_F16_DDCONFIG, ch=64)
KL_NARROW_DDCONFIG = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2], num_res_blocks=2,
                          attn_resolutions=[16], dropout=0.0)
KL_TWO_LEVELS_DDCONFIG = dict(KL_NARROW_DDCONFIG, attn_resolutions=[32, 16])
KL_F16_STANDINS = {'kl_f16': KL_F16_KWARGS, 'kl_f16_thin': dict(embed_dim=16, ddconfig=KL_F16_THIN_DDCONFIG),
                   'kl_narrow': dict(embed_dim=4, ddconfig=KL_NARROW_DDCONFIG), 'kl_two_levels': dict(embed_dim=4, ddconfig=KL_TWO_LEVELS_DDCONFIG)}


def synthetic_kl_f16_state_dict(seed=0, kwargs=None):
    """CPU state_dict (reference AutoencoderKL key names) of a seeded random KL-f16 first stage (or a stand-in)."""
    from .vae import AutoencoderKLHIP
    kw = kwargs or KL_F16_KWARGS
    m = AutoencoderKLHIP(kw['ddconfig'], None, kw['embed_dim'])
    return synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)


# ---- the rest of the first-stage zoo (models/first_stage_models/*, configs/autoencoder/*) ------------------------------------------------
# KL-f32: six levels, AttnBlocks after every ResBlock of the 16 x 16 and 8 x 8 levels (levels 4 and 5: mask 0b110000, d = 512), 64 latent
# channels -- decoder.conv_in 64 -> 512, encoder.conv_out 512 -> 128, quant_conv 128 -> 128, post_quant_conv 64 -> 64 (the wide fp32 ends)
KL_F32_DDCONFIG = dict(double_z=True, z_channels=64, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 1, 2, 2, 4, 4],
                       num_res_blocks=2, attn_resolutions=[16, 8], dropout=0.0)            # kl-f32/config.yaml:13-31 = autoencoder_kl_8x8x64.yaml
KL_F32_KWARGS = dict(embed_dim=64, ddconfig=KL_F32_DDCONFIG)                               # yaml:6
# KL-f4: three levels, no level attention, 3 latent channels (a 6-channel encoder.conv_out and quant_conv)
KL_F4_DDCONFIG = dict(double_z=True, z_channels=3, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4], num_res_blocks=2,
                      attn_resolutions=[], dropout=0.0)                                    # kl-f4/config.yaml:13-26 = autoencoder_kl_64x64x3.yaml
KL_F4_KWARGS = dict(embed_dim=3, ddconfig=KL_F4_DDCONFIG)                                  # yaml:6
# VQ-f8 (also the first stage of models/ldm/cin256 and configs/latent-diffusion/cin-ldm-vq-f8.yaml): level attention at 32 x 32 (level 3)
VQ_F8_DDCONFIG = dict(double_z=False, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 2, 4], num_res_blocks=2,
                      attn_resolutions=[32], dropout=0.0)                                  # vq-f8/config.yaml:8-23
VQ_F8_KWARGS = dict(embed_dim=4, n_embed=16384, ddconfig=VQ_F8_DDCONFIG)                   # yaml:5-6
VQ_F8_N256_KWARGS = dict(embed_dim=4, n_embed=256, ddconfig=VQ_F8_DDCONFIG)                # vq-f8-n256/config.yaml:5-23 (the same ddconfig)
# VQ-f16: level attention at 16 x 16 (level 4), an 8-dimensional codebook
VQ_F16_DDCONFIG = dict(double_z=False, z_channels=8, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 1, 2, 2, 4],
                       num_res_blocks=2, attn_resolutions=[16], dropout=0.0)               # vq-f16/config.yaml:7-23
VQ_F16_KWARGS = dict(embed_dim=8, n_embed=16384, ddconfig=VQ_F16_DDCONFIG)                 # yaml:5-6
# stand-ins for the tests: the yamls at ch 64 (level and mid attention at d = 256), and VQ-f8-n256 at ch 64
FIRST_STAGES = {'kl_f32': KL_F32_KWARGS, 'kl_f32_thin': dict(embed_dim=64, ddconfig=dict(KL_F32_DDCONFIG, ch=64)),
                'kl_f4': KL_F4_KWARGS,
                'vq_f8': VQ_F8_KWARGS, 'vq_f8_thin': dict(VQ_F8_KWARGS, ddconfig=dict(VQ_F8_DDCONFIG, ch=64)),
                'vq_f8_n256': VQ_F8_N256_KWARGS, 'vq_f8_n256_thin': dict(VQ_F8_N256_KWARGS, ddconfig=dict(VQ_F8_DDCONFIG, ch=64)),
                'vq_f16': VQ_F16_KWARGS, 'vq_f16_thin': dict(VQ_F16_KWARGS, ddconfig=dict(VQ_F16_DDCONFIG, ch=64))}


def make_first_stage(kwargs, hip_precision='mixed'):
    """AutoencoderKLHIP or VQModelInterfaceHIP from one of the kwargs dicts above."""
    from .vae import AutoencoderKLHIP, VQModelInterfaceHIP
    if 'n_embed' in kwargs:
        return VQModelInterfaceHIP(hip_precision=hip_precision, **kwargs)
    return AutoencoderKLHIP(kwargs['ddconfig'], None, kwargs['embed_dim'], hip_precision=hip_precision)


def synthetic_first_stage_state_dict(seed=0, kwargs=None):
    """CPU state_dict (reference AutoencoderKL / VQModelInterface key names, without loss.*) of a seeded random first stage."""
    m = make_first_stage(kwargs or KL_F32_KWARGS)
    return synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)


# ---- the older class-conditional ImageNet model (models/ldm/cin256/config.yaml) -------------------------------------------------------------
# many heads of 32 channels (8 / 16 / 32 at 256 / 512 / 1024 channels) over ClassEmbedder's one-token context; VQ-f8 first stage
CIN256_OLD_UNET_KWARGS = dict(image_size=32, in_channels=4, out_channels=4, model_channels=256, attention_resolutions=[4, 2, 1],
                              num_res_blocks=2, channel_mult=[1, 2, 4], num_head_channels=32, use_spatial_transformer=True,
                              transformer_depth=1, context_dim=512)                                        # yaml:17-36
CIN256_OLD_VQ_KWARGS = VQ_F8_KWARGS                                                                        # yaml:37-57
CIN256_OLD_CLASS_KWARGS = dict(embed_dim=512, key='class_label')                                           # yaml:60-64 (n_classes: the default 1000)
CIN256_OLD_SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.0195, conditioning_key='crossattn')   # yaml:5-6,9,15
