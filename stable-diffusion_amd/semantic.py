"""The semantic-synthesis models (models/ldm/semantic_synthesis256 / semantic_synthesis512 config.yaml), an image from a segmentation map,
as one pipeline on HIP classes:

    SemanticSynthesisHIP <- ldm.models.diffusion.ddpm.LatentDiffusion at those configs: the 182-class one-hot map goes through the
                            SpatialRescaler cond stage (two halvings and a 1x1 convolution to 3 channels: the latent's resolution), DDIM
                            runs over a latent conditioned on it by concatenation (concat_mode, cond_stage_key 'segmentation'), and the
                            VQ-f4 first stage decodes.

The UNet is convolutional and its only attention is the middle block's, so any canvas that fits the device runs directly; the
reference's `split_input_params` tiling is NOT built for this model (larger canvases than fit are out of scope).  State-dict keys are
the reference checkpoint's (`model.diffusion_model.*`, `first_stage_model.*`, `cond_stage_model.*`).
"""
import torch

from . import synthetic
from .ldm_shim import LatentDiffusionHIP
from .rescaler import SpatialRescalerHIP
from .samplers import DDIMSamplerHIP
from .unet import UNetModelHIP
from .vae import VQModelInterfaceHIP

SEMANTIC_VQ_KWARGS = synthetic.FACES_VQ_KWARGS    # yaml first_stage_config.params: the VQ-f4 first stage of the face models
SIZE_MULTIPLE = 16                                # f = 4 of the first stage times the UNet's two Downsamples


def nearest_valid_sizes(side, m=SIZE_MULTIPLE):
    """the multiples of m next to `side` (below, above); below is None under m"""
    lo = side // m * m
    return (lo or None), lo if lo == side and lo else lo + m


class SemanticSynthesisHIP(LatentDiffusionHIP):
    def __init__(self, unet_kwargs=None, vq_kwargs=None, rescaler_kwargs=None, schedule=None, hip_precision='mixed'):
        sched = dict(synthetic.SEMANTIC_SCHEDULE if schedule is None else schedule)
        unet = UNetModelHIP(**(synthetic.SEMANTIC_UNET_KWARGS if unet_kwargs is None else unet_kwargs), hip_precision=hip_precision)
        vq = VQModelInterfaceHIP(**(SEMANTIC_VQ_KWARGS if vq_kwargs is None else vq_kwargs))
        super().__init__(unet, first_stage_model=vq, scale_factor=1.0, cond_stage_key='segmentation', **sched)
        self.cond_stage_model = SpatialRescalerHIP(**(synthetic.SEMANTIC_RESCALER_KWARGS if rescaler_kwargs is None else rescaler_kwargs))

    @classmethod
    def from_config(cls, config, hip_precision='mixed'):
        """`config`: a parsed models/ldm/semantic_synthesis*/config.yaml (tests/golden/semantic_synthesis512_config.json)"""
        p = config['model']['params']
        cs = p.get('cond_stage_config')
        if (not p.get('concat_mode') or p.get('cond_stage_key') != 'segmentation' or not isinstance(cs, dict)
                or cs.get('target', '').rsplit('.', 1)[-1] != 'SpatialRescaler'):
            raise NotImplementedError('SemanticSynthesisHIP: a concat_mode model conditioned on segmentation through a SpatialRescaler cond stage')
        fs = p['first_stage_config']['params']
        return cls(dict(p['unet_config']['params']),
                   dict(embed_dim=fs['embed_dim'], n_embed=fs['n_embed'], ddconfig=dict(fs['ddconfig']),
                        **({'hip_precision': fs['hip_precision']} if 'hip_precision' in fs else {})),     # (the first stage's own mode)
                   dict(cs.get('params') or {}),
                   dict(timesteps=p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'], conditioning_key='concat'),
                   hip_precision)

    def _parts(self):
        return (('model.diffusion_model.', self.model.diffusion_model), ('first_stage_model.', self.first_stage_model),
                ('cond_stage_model.', self.cond_stage_model))

    def load_synthetic(self, seed=0):
        """seeded random weights under the reference's key names (there is no checkpoint in the build environment)"""
        for _, m in self._parts():
            m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed), strict=True)
        return self

    def load_checkpoint(self, path):
        """a reference semantic_synthesis checkpoint: `state_dict` with model.diffusion_model.*, first_stage_model.* and cond_stage_model.*
        (loss.* and EMA copies ignored)"""
        sd = torch.load(path, map_location='cpu')
        sd = sd.get('state_dict', sd)
        for prefix, m in self._parts():
            want = set(m.state_dict())
            m.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix) and k[len(prefix):] in want}, strict=True)
        return self

    def get_learned_conditioning(self, c):
        """ddpm.py:551-562: the cond stage has `encode`"""
        return self.cond_stage_model.encode(c)

    @staticmethod
    def check_size(H, W):
        """H and W multiples of 16: the latent H/4 x W/4 goes through two Downsamples.  Nothing is padded."""
        if H < SIZE_MULTIPLE or W < SIZE_MULTIPLE or H % SIZE_MULTIPLE or W % SIZE_MULTIPLE:
            def near(side):
                lo, hi = nearest_valid_sizes(side)
                return f'{hi}' if lo is None or lo == hi else f'{lo} or {hi}'
            raise ValueError(f'SemanticSynthesisHIP: a {H} x {W} map; height and width must be multiples of {SIZE_MULTIPLE} (the latent is '
                             f'H/4 x W/4 and the UNet halves it twice); nearest valid sizes: height {near(H)}, width {near(W)} '
                             '(resize or crop the map: nothing is padded silently)')

    @torch.no_grad()
    def synthesize(self, segmentation=None, labels=None, steps=50, eta=1.0, x_T=None):
        """Exactly one of `segmentation` (fp32 one-hot [B, 182, H, W]) and `labels` ([B, H, W] of uint8 / int32 / int64) -> images
        [B, 3, H, W] in [-1, 1].  The conditioning is computed once; the canvas runs un-tiled (split_input_params is not built here)."""
        if (segmentation is None) == (labels is None):
            raise ValueError('synthesize: exactly one of segmentation and labels')
        src = segmentation if labels is None else labels
        if src.dim() != (4 if labels is None else 3):
            raise ValueError(f'synthesize: segmentation [B, C, H, W] or labels [B, H, W], got {tuple(src.shape)}')
        B, (H, W) = src.shape[0], src.shape[-2:]
        self.check_size(int(H), int(W))
        src = src.to(self.device)
        c = self.get_learned_conditioning(src.float()) if labels is None else self.cond_stage_model.encode_labels(src)
        samples, _ = DDIMSamplerHIP(self).sample(steps, batch_size=B, shape=(3, H // 4, W // 4), conditioning=c, eta=eta, verbose=False,
                                                 x_T=x_T)
        return self.decode_first_stage(samples)
