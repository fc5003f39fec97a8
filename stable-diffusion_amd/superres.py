"""bsr_sr, the x4 super-resolution model (models/ldm/bsr_sr/config.yaml), as one image-to-image pipeline on HIP classes:

    SuperResolutionHIP <- ldm.models.diffusion.ddpm.LatentDiffusion at bsr_sr's config, sampled as notebook / script users do:
                          DDIM over a latent of the low-resolution image's size, conditioned on that image by concatenation
                          (concat_mode, cond_stage_config torch.nn.Identity, cond_stage_key 'LR_image'), then the VQ-f4 decode.

Inputs larger than the window run tiled (`split_input_params`, ldm_shim.py): the UNet and the first stage see `ks` windows at `stride`,
all windows of all samples as rows of calls of up to 8 rows.  The reference names ks (128, 128) / stride (64, 64) in comments only
(ddpm.py:717-718); they are this project's defaults.  State-dict keys are the reference checkpoint's (`model.diffusion_model.*`,
`first_stage_model.*`).
"""
import torch

from . import synthetic
from .ldm_shim import LatentDiffusionHIP, patch_grid
from .samplers import DDIMSamplerHIP
from .unet import UNetModelHIP
from .vae import VQModelInterfaceHIP

BSR_VQ_KWARGS = synthetic.FACES_VQ_KWARGS        # bsr_sr yaml first_stage_config.params: the VQ-f4 first stage of the face models
DEFAULT_SPLIT_INPUT_PARAMS = dict(ks=(128, 128), stride=(64, 64), vqf=4, patch_distributed_vq=True, tie_braker=False,
                                  clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)


def nearest_valid_sizes(side, k, s):
    """the sizes k + n * s next to `side` (below, above); below is None under the window"""
    if side < k:
        return None, k
    lo = k + (side - k) // s * s
    return lo, lo if lo == side else lo + s


class SuperResolutionHIP(LatentDiffusionHIP):
    def __init__(self, split_input_params=None, unet_kwargs=None, vq_kwargs=None, schedule=None, hip_precision='mixed'):
        sched = dict(synthetic.BSR_SCHEDULE if schedule is None else schedule)
        unet = UNetModelHIP(**(synthetic.BSR_UNET_KWARGS if unet_kwargs is None else unet_kwargs), hip_precision=hip_precision)
        vq = VQModelInterfaceHIP(**(BSR_VQ_KWARGS if vq_kwargs is None else vq_kwargs))
        super().__init__(unet, first_stage_model=vq, scale_factor=1.0, cond_stage_key='LR_image', **sched)
        self.cond_stage_model = torch.nn.Identity()
        self.tile_params = dict(DEFAULT_SPLIT_INPUT_PARAMS if split_input_params is None else split_input_params)
        self.tile_params['ks'], self.tile_params['stride'] = tuple(self.tile_params['ks']), tuple(self.tile_params['stride'])

    @classmethod
    def from_config(cls, config, split_input_params=None, hip_precision='mixed'):
        """`config`: the parsed models/ldm/bsr_sr/config.yaml (tests/golden/bsr_sr_config.json)"""
        p = config['model']['params']
        fs = p['first_stage_config']['params']
        if not p.get('concat_mode') or p.get('cond_stage_key') != 'LR_image':
            raise NotImplementedError('SuperResolutionHIP: a concat_mode model conditioned on LR_image')
        return cls(split_input_params, dict(p['unet_config']['params']),
                   dict(embed_dim=fs['embed_dim'], n_embed=fs['n_embed'], ddconfig=dict(fs['ddconfig']),
                        **({'hip_precision': fs['hip_precision']} if 'hip_precision' in fs else {})),     # (the first stage's own mode)
                   dict(timesteps=p['timesteps'], linear_start=p['linear_start'], linear_end=p['linear_end'], conditioning_key='concat'),
                   hip_precision)

    def load_synthetic(self, seed=0):
        """seeded random weights under the reference's key names (there is no checkpoint in the build environment)"""
        for m in (self.model.diffusion_model, self.first_stage_model):
            m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed), strict=True)
        return self

    def load_checkpoint(self, path):
        """a reference bsr_sr checkpoint: `state_dict` with model.diffusion_model.* and first_stage_model.* (loss.* and EMA copies ignored)"""
        sd = torch.load(path, map_location='cpu')
        sd = sd.get('state_dict', sd)
        for prefix, m in (('model.diffusion_model.', self.model.diffusion_model), ('first_stage_model.', self.first_stage_model)):
            want = set(m.state_dict())
            m.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix) and k[len(prefix):] in want}, strict=True)
        return self

    def configure_tiling(self, h, w):
        """Tiling is on when a side exceeds the window; then both sides must lie on the ks + n * stride grid (no silent padding)."""
        ks, stride = self.tile_params['ks'], self.tile_params['stride']
        if h <= ks[0] and w <= ks[1]:
            if hasattr(self, 'split_input_params'):
                del self.split_input_params
            return False
        try:
            patch_grid(h, w, ks, stride)
        except ValueError:
            def near(side, k, s):
                lo, hi = nearest_valid_sizes(side, k, s)
                return f'{hi}' if lo is None or lo == hi else f'{lo} or {hi}'
            raise ValueError(f'SuperResolutionHIP: a {h} x {w} input does not tile into {ks[0]} x {ks[1]} windows at stride {stride[0]} x '
                             f'{stride[1]}; nearest valid sizes: height {near(h, ks[0], stride[0])}, width {near(w, ks[1], stride[1])} '
                             '(resize or crop the input: nothing is padded silently)') from None
        self.split_input_params = dict(self.tile_params)
        return True

    @torch.no_grad()
    def upscale(self, lr, steps=100, eta=1.0, x_T=None):
        """lr [B, 3, h, w] in [-1, 1] -> [B, 3, 4h, 4w]"""
        if lr.dim() != 4 or lr.shape[1] != 3:
            raise ValueError(f'upscale: a [B, 3, h, w] image batch, got {tuple(lr.shape)}')
        B, _, h, w = lr.shape
        self.configure_tiling(h, w)
        c = self.cond_stage_model(lr.to(self.device).float().contiguous())
        samples, _ = DDIMSamplerHIP(self).sample(steps, batch_size=B, shape=(3, h, w), conditioning=c, eta=eta, verbose=False, x_T=x_T)
        return self.decode_first_stage(samples)
