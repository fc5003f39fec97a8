"""Generate the fixtures of bsr_sr's tiled image pipeline under tests/golden/ from the reference code (build container only).

    PYTHONPATH=. python tools/make_golden_superres.py

Everything tiled comes from the reference's own text: the unbound `LatentDiffusion.meshgrid / delta_border / get_weighting /
get_fold_unfold / apply_model / decode_first_stage / encode_first_stage` (ldm/models/diffusion/ddpm.py:564-651, 705-763, 825-863, 891-992)
are called on a stand-in object that carries the attributes they read; `ldm.models.diffusion.ddpm` is imported through the stand-ins of
tools/run_reference_script.py (pytorch_lightning, omegaconf and taming are not installed in the build container).  The UNet is the
reference UNetModel at bsr_sr's unet_config behind the reference DiffusionWrapper ('concat'); the first stage is the reference
VQModelInterface's own encode / decode over the reference Encoder / Decoder, with taming's quantizer restated in tests/vq_ref.py.
Weights: stable_diffusion_amd.synthetic.synthetic_named_state_dict, seed 0.  The fixtures hold outputs and seeds, never weights.

superres_fold.npz            weighting / normalization of get_fold_unfold and fold(o * weighting) / normalization on seeded o, per geometry
superres_apply_model_24x32   tiled apply_model, B = 2, latent 24 x 32, ks 16, stride 8 (6 windows), t = (981, 1); tie_braker off and on
superres_vq_24x32            tiled decode_first_stage (vqf 4) of a latent of codebook rows plus noise; tiled encode_first_stage at 64 x 96
superres_pipeline_24x32      10 DDIM steps (eta 1.0) of the reference DDIMSampler over the tiled apply_model, then the tiled decode; run twice,
                             the second time with every eps moved by 1e-3 sign(randn): the divergence of `samples` is the test's bar
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle.make_golden import REF  # noqa: E402  (the reference checkout: $SD_REFERENCE)
OUT = os.path.join(ROOT, 'tests', 'golden')

CLIPS = dict(clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
# name, (H, W), ks, stride, uf, df, tie_braker -- the geometries of tests/test_superres_gpu.py's fold test
FOLD_GEOMS = [('s1', (32, 32), (16, 16), (16, 16), 1, 1, False), ('s2', (24, 32), (16, 16), (8, 8), 1, 1, False),
              ('s4', (32, 32), (16, 16), (4, 4), 1, 1, False), ('s2_tie', (24, 32), (16, 16), (8, 8), 1, 1, True),
              ('s4_tie', (32, 32), (16, 16), (4, 4), 1, 1, True), ('uf4', (24, 32), (16, 16), (8, 8), 4, 1, False),
              ('uf4_tie', (24, 32), (16, 16), (8, 8), 4, 1, True), ('df4', (64, 96), (32, 32), (16, 16), 1, 4, False),
              ('rect', (24, 24), (16, 8), (8, 8), 1, 1, False), ('unaligned', (21, 27), (9, 11), (3, 4), 1, 1, False),
              ('unaligned_tie', (21, 27), (9, 11), (3, 4), 1, 1, True)]
FOLD_B, FOLD_C = 2, 2
GEOM = dict(h=24, w=32, ks=(16, 16), stride=(8, 8), vqf=4)
ENC = dict(h=64, w=96, ks=(32, 32), stride=(16, 16))
PIPE = dict(steps=10, batch=1, eta=1.0, input_seed=3, noise_seed=4, perturb_seed=5, cond_seed=6, perturb=1e-3)
VQ_NOISE = 1e-3


def fold_input(name, shape):
    import zlib
    return torch.randn(shape, generator=torch.Generator().manual_seed(zlib.crc32(name.encode())))


def seeded(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def pipeline_noise(seed, steps, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), [torch.randn(shape, generator=g) for _ in range(steps)]


def split_params(ks, stride, tie=False, vqf=4):
    return dict(ks=tuple(ks), stride=tuple(stride), vqf=vqf, patch_distributed_vq=True, tie_braker=tie, **CLIPS)


def main():
    import json
    import vq_ref
    import run_reference_script as rrs
    from stable_diffusion_amd.synthetic import BSR_SCHEDULE, BSR_UNET_KWARGS, FACES_VQ_KWARGS, synthetic_named_state_dict
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.path.insert(0, REF)
    rrs.install_stubs(False, offline_stubs=True)
    import ldm.models.diffusion.ddim as ref_ddim
    import ldm.models.diffusion.ddpm as ref_ddpm
    from ldm.models.autoencoder import VQModelInterface
    from ldm.modules.diffusionmodules.model import Decoder, Encoder
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from ldm.modules.diffusionmodules.util import make_beta_schedule
    LD = ref_ddpm.LatentDiffusion

    with open(os.path.join(OUT, 'bsr_sr_config.json')) as f:
        pb = json.load(f)['model']['params']
    fsp = pb['first_stage_config']['params']
    assert dict(pb['unet_config']['params']) == BSR_UNET_KWARGS
    assert dict(embed_dim=fsp['embed_dim'], n_embed=fsp['n_embed'], ddconfig=dict(fsp['ddconfig'])) == FACES_VQ_KWARGS
    assert pb['cond_stage_key'] == 'LR_image' and pb['concat_mode'] is True

    class Stand:
        """what the reference's patch methods read on `self`"""
        device = torch.device('cpu')
        scale_factor = 1.0
        cond_stage_key = pb['cond_stage_key']

        def __init__(self, params, model=None, first_stage_model=None):
            self.split_input_params = params
            self.model, self.first_stage_model = model, first_stage_model
    for name in ('meshgrid', 'delta_border', 'get_weighting', 'get_fold_unfold', 'apply_model', 'decode_first_stage', 'encode_first_stage'):
        setattr(Stand, name, getattr(LD, name))

    # ---- fold: weighting, normalization and the folded result on seeded window outputs ----
    fold = {}
    for name, (H, W), ks, stride, uf, df, tie in FOLD_GEOMS:
        st = Stand(split_params(ks, stride, tie))
        fo, _, norm, wgt = st.get_fold_unfold(torch.zeros(1, 1, H, W), ks, stride, uf=uf, df=df)
        kh, kw, L = wgt.shape[2:]
        o = fold_input(name, (L * FOLD_B, FOLD_C, kh, kw))                    # rows (l, b), the library's layout
        o5 = o.view(L, FOLD_B, FOLD_C, kh, kw).permute(1, 2, 3, 4, 0)          # the reference's (b, c, kh, kw, L)
        folded = fo((o5 * wgt).reshape(FOLD_B, -1, L)) / norm
        assert float(norm.min()) > 0 and bool(torch.isfinite(folded).all()), name
        fold[f'{name}_weighting'] = wgt.numpy()
        fold[f'{name}_normalization'] = norm.numpy()
        fold[f'{name}_folded'] = folded.numpy().astype(np.float32)
        print(f'[fold {name}] L {L} window {kh} x {kw} out {tuple(folded.shape)} norm min {float(norm.min()):.4f}', flush=True)
    np.savez_compressed(os.path.join(OUT, 'superres_fold.npz'), **fold)

    # ---- tiled apply_model ----
    unet = UNetModel(**pb['unet_config']['params']).eval()
    unet.load_state_dict(synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], 0), strict=True)
    dw = ref_ddpm.DiffusionWrapper.__new__(ref_ddpm.DiffusionWrapper)
    nn.Module.__init__(dw)
    dw.diffusion_model, dw.conditioning_key = unet, 'concat'
    h, w = GEOM['h'], GEOM['w']
    x, c, t = seeded((2, 3, h, w), 1), seeded((2, 3, h, w), 2), torch.tensor((981, 1), dtype=torch.int64)
    am = {}
    for tag, tie in (('eps', False), ('eps_tie', True)):
        with torch.no_grad():
            am[tag] = Stand(split_params(GEOM['ks'], GEOM['stride'], tie), dw).apply_model(x, t, c).numpy().astype(np.float32)
        print(f'[apply_model {tag}] |eps| max {np.abs(am[tag]).max():.3f}', flush=True)
    np.savez_compressed(os.path.join(OUT, 'superres_apply_model_24x32.npz'), weight_seed=0, x_seed=1, c_seed=2, t=t.numpy(), batch=2, h=h, w=w,
                        ks=GEOM['ks'], stride=GEOM['stride'], **am)

    # ---- tiled first stage ----
    dd = fsp['ddconfig']
    dec, enc = Decoder(**dd).eval(), Encoder(**dd).eval()
    pqc, qc = nn.Conv2d(fsp['embed_dim'], dd['z_channels'], 1), nn.Conv2d(dd['z_channels'], fsp['embed_dim'], 1)
    specs = ([('decoder.' + k, tuple(v.shape)) for k, v in dec.state_dict().items()] + [('encoder.' + k, tuple(v.shape)) for k, v in enc.state_dict().items()] +
             [('quantize.embedding.weight', (fsp['n_embed'], fsp['embed_dim']))] + [('post_quant_conv.' + k, tuple(v.shape)) for k, v in pqc.state_dict().items()] +
             [('quant_conv.' + k, tuple(v.shape)) for k, v in qc.state_dict().items()])
    vsd = synthetic_named_state_dict(specs, 0)
    for mod, pre in ((dec, 'decoder.'), (enc, 'encoder.'), (pqc, 'post_quant_conv.'), (qc, 'quant_conv.')):
        mod.load_state_dict({k[len(pre):]: v for k, v in vsd.items() if k.startswith(pre)}, strict=True)
    e = vsd['quantize.embedding.weight']

    class Quant(nn.Module):
        def forward(self, hh):
            zq, idx = vq_ref.quantize(hh, e)
            return zq, None, (None, None, idx.reshape(-1))
    fs = VQModelInterface.__new__(VQModelInterface)            # the reference's own encode / decode text over reference modules
    nn.Module.__init__(fs)
    fs.encoder, fs.decoder, fs.quant_conv, fs.post_quant_conv, fs.quantize = enc, dec, qc, pqc, Quant()
    idx = torch.randint(0, fsp['n_embed'], (2, h, w), generator=torch.Generator().manual_seed(7))
    z = e[idx].permute(0, 3, 1, 2).contiguous() + seeded((2, 3, h, w), 8, VQ_NOISE)
    d = vq_ref.distances(z, e)
    d2, i2 = torch.topk(d, 2, dim=1, largest=False)
    assert torch.equal(i2[:, 0].view(2, h, w), idx) and bool(((d2[:, 1] - d2[:, 0]) >= 0.01 * d2[:, 1]).all()), 'a nearest code wins by less than 1 %'
    st = Stand(split_params(GEOM['ks'], GEOM['stride']), None, fs)
    with torch.no_grad():
        x_dec = st.decode_first_stage(z)
    xe = seeded((1, 3, ENC['h'], ENC['w']), 9, 0.5)
    ste = Stand(split_params(ENC['ks'], ENC['stride']), None, fs)
    with torch.no_grad():
        h_enc = ste.encode_first_stage(xe)
    assert tuple(ste.split_input_params['original_image_size']) == (ENC['h'], ENC['w'])
    print(f'[vq] decode {tuple(x_dec.shape)} |x| max {x_dec.abs().max():.3f}; encode {tuple(h_enc.shape)} |h| max {h_enc.abs().max():.3f}', flush=True)
    assert tuple(x_dec.shape) == (2, 3, 4 * h, 4 * w) and tuple(h_enc.shape) == (1, 3, ENC['h'] // 4, ENC['w'] // 4)
    np.savez_compressed(os.path.join(OUT, 'superres_vq_24x32.npz'), weight_seed=0, idx=idx.numpy().astype(np.int32), z=z.numpy(), noise_seed=8,
                        x_dec=x_dec.numpy().astype(np.float32), enc_seed=9, enc_h=ENC['h'], enc_w=ENC['w'], enc_ks=ENC['ks'],
                        enc_stride=ENC['stride'], h_enc=h_enc.numpy().astype(np.float32), ks=GEOM['ks'], stride=GEOM['stride'], vqf=GEOM['vqf'])

    # ---- pipeline: the reference DDIMSampler over the tiled apply_model, then the tiled decode ----
    class CpuDDIM(ref_ddim.DDIMSampler):
        def register_buffer(self, name, attr):            # (the reference moves its tables to cuda)
            setattr(self, name, attr)

    class Model(Stand):
        def __init__(self, perturb_seed=None):
            super().__init__(split_params(GEOM['ks'], GEOM['stride']), dw, fs)
            betas = make_beta_schedule('linear', pb['timesteps'], linear_start=pb['linear_start'], linear_end=pb['linear_end'])
            ac = np.cumprod(1. - betas, axis=0)
            self.num_timesteps = int(pb['timesteps'])
            self.betas = torch.tensor(betas, dtype=torch.float32)
            self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
            self.alphas_cumprod_prev = torch.tensor(np.append(1., ac[:-1]), dtype=torch.float32)
            self.g = None if perturb_seed is None else torch.Generator().manual_seed(perturb_seed)

        def apply_model(self, xx, tt, cc):
            eps = LD.apply_model(self, xx, tt, cc)
            if self.g is not None:
                eps = eps + PIPE['perturb'] * torch.sign(torch.randn(eps.shape, generator=self.g))
            return eps
    assert (pb['timesteps'], pb['linear_start'], pb['linear_end']) == tuple(BSR_SCHEDULE[k] for k in ('timesteps', 'linear_start', 'linear_end'))
    shape = (PIPE['batch'], 3, h, w)
    lr = seeded(shape, PIPE['cond_seed'], 0.5).clamp(-1, 1)

    def run(perturb_seed):
        x_T, noises = pipeline_noise(PIPE['noise_seed'], PIPE['steps'], shape)
        seq = list(noises)
        ref_ddim.noise_like = lambda shp, device, repeat=False: seq.pop(0)
        with torch.no_grad():
            samples, _ = CpuDDIM(Model(perturb_seed)).sample(PIPE['steps'], batch_size=shape[0], shape=shape[1:], conditioning=lr, eta=PIPE['eta'],
                                                             verbose=False, x_T=x_T)
        assert not seq
        return samples
    keep = ref_ddim.noise_like
    try:
        samples = run(None)
        samples_p = run(PIPE['perturb_seed'])
    finally:
        ref_ddim.noise_like = keep
    with torch.no_grad():
        zq, pidx = vq_ref.quantize(samples, e)              # decoded on the golden's own codes: a code flip near a cell boundary is not the UNet's
        x_up = Model().decode_first_stage(zq, force_not_quantize=True)
    bar_s = float((samples_p - samples).abs().max())
    print(f'[pipeline] |samples| max {samples.abs().max():.3f}; |x_up| max {x_up.abs().max():.3f} {tuple(x_up.shape)}; bar from eps + '
          f'{PIPE["perturb"]:g} sign: samples {bar_s:.3e}', flush=True)
    np.savez_compressed(os.path.join(OUT, 'superres_pipeline_24x32.npz'), samples=samples.numpy().astype(np.float32),
                        x_up=x_up.numpy().astype(np.float32), idx=pidx.numpy().astype(np.int32), bar_samples=bar_s, weight_seed=0, h=h, w=w,
                        ks=GEOM['ks'], stride=GEOM['stride'], vqf=GEOM['vqf'], **PIPE)
    print('bsr_sr tiled fixtures written to', OUT)


if __name__ == '__main__':
    main()
