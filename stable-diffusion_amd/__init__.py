"""stable-diffusion_amd: MI355X-native txt2img sampling hot path (UNet eps prediction + PLMS/DDIM loop).

The arithmetic lives in libsdmi.so (hand-written gfx950 HIP kernels behind a C ABI, include/sdmi.h);
this package is the host-side mirror of the reference's interfaces for that path:

    UNetModelHIP      <- ldm.modules.diffusionmodules.openaimodel.UNetModel
    PLMSSamplerHIP    <- ldm.models.diffusion.plms.PLMSSampler
    DDIMSamplerHIP    <- ldm.models.diffusion.ddim.DDIMSampler
    DPMSolverSamplerHIP <- ldm.models.diffusion.dpm_solver.sampler.DPMSolverSampler
    DPMSolverHIP      <- ldm.models.diffusion.dpm_solver.dpm_solver.DPM_Solver (every method, order, skip type and solver type)
    SamplerPoolHIP    <- no counterpart: DDIM / PLMS / DPM-Solver requests that arrive one after another share UNet calls (sampler_pool.py)
    DDPMSamplerHIP    <- LatentDiffusion.p_sample_loop / progressive_denoising (scripts/sample_diffusion.py --vanilla_sample)
    AutoencoderKLHIP  <- ldm.models.autoencoder.AutoencoderKL (decode / encode)
    VQModelInterfaceHIP <- ldm.models.autoencoder.VQModelInterface (the latent-inpainting model's first stage)
    FrozenCLIPEmbedderHIP <- ldm.modules.encoders.modules.FrozenCLIPEmbedder
    BERTEmbedderHIP   <- ldm.modules.encoders.modules.BERTEmbedder (the LAION-400M model's text encoder)
    ClassEmbedderHIP  <- ldm.modules.encoders.modules.ClassEmbedder (the class-conditional ImageNet model's conditioner)
    SuperResolutionHIP <- LatentDiffusion at models/ldm/bsr_sr (tiled x4 super-resolution: split_input_params)
    SpatialRescalerHIP <- ldm.modules.encoders.modules.SpatialRescaler (the semantic-synthesis models' cond stage)
    SemanticSynthesisHIP <- LatentDiffusion at models/ldm/semantic_synthesis256 / 512 (an image from a segmentation map)
    CLIPVisionHIP     <- transformers.CLIPVisionModelWithProjection (the tower of the two modules below)
    StableDiffusionSafetyCheckerHIP <- diffusers' StableDiffusionSafetyChecker (scripts/txt2img.py:check_safety)
    FrozenClipImageEmbedderHIP <- ldm.modules.encoders.modules.FrozenClipImageEmbedder
    FrozenCLIPTextEmbedderHIP <- ldm.modules.encoders.modules.FrozenCLIPTextEmbedder (OpenAI CLIP encode_text: pooled, projected)
    SearcherHIP       <- scripts/knn2img.py: Searcher (exact k-NN over the retrieval database, on the device)

Importable as `stable_diffusion_amd` (see stable_diffusion_amd.py at the repo root).
"""
from . import _lib  # noqa: F401
from .unet import UNetModelHIP  # noqa: F401
from .samplers import PLMSSamplerHIP, DDIMSamplerHIP, DPMSolverSamplerHIP, DDPMSamplerHIP, DPMSolverHIP  # noqa: F401
from .sampler_pool import SamplerPoolHIP, plan_calls  # noqa: F401
from .vae import AutoencoderKLHIP, VQModelInterfaceHIP  # noqa: F401
from .clip import FrozenCLIPEmbedderHIP, FrozenCLIPTextEmbedderHIP  # noqa: F401
from .bert import BERTEmbedderHIP  # noqa: F401
from .class_embedder import ClassEmbedderHIP  # noqa: F401
from .ldm_shim import LatentDiffusionHIP, DiffusionWrapperHIP  # noqa: F401
from .superres import SuperResolutionHIP  # noqa: F401
from .rescaler import SpatialRescalerHIP  # noqa: F401
from .semantic import SemanticSynthesisHIP  # noqa: F401
from .vision import CLIPVisionHIP, StableDiffusionSafetyCheckerHIP, FrozenClipImageEmbedderHIP, CLIPFeatureExtractorHIP  # noqa: F401
from .retrieval import SearcherHIP  # noqa: F401
from . import debug, postprocess  # noqa: F401

__all__ = ['UNetModelHIP', 'AutoencoderKLHIP', 'VQModelInterfaceHIP', 'FrozenCLIPEmbedderHIP', 'BERTEmbedderHIP', 'ClassEmbedderHIP', 'PLMSSamplerHIP', 'DDIMSamplerHIP', 'DPMSolverSamplerHIP', 'DPMSolverHIP', 'DDPMSamplerHIP', 'SamplerPoolHIP', 'LatentDiffusionHIP', 'DiffusionWrapperHIP', 'SuperResolutionHIP', 'SpatialRescalerHIP', 'SemanticSynthesisHIP', 'CLIPVisionHIP', 'StableDiffusionSafetyCheckerHIP', 'FrozenClipImageEmbedderHIP', 'FrozenCLIPTextEmbedderHIP', 'SearcherHIP']
