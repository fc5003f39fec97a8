"""Generate the fixtures of the KL-f16 first stage under tests/golden/ from the reference code (build container only).

    PYTHONPATH=. python tools/make_golden_kl_f16.py

The reference `Encoder` / `Decoder` (ldm/modules/diffusionmodules/model.py) plus the two 1x1 quant convs, as `AutoencoderKL.encode` /
`.decode` run them (autoencoder.py:324-333; the Lightning wrapper itself needs pytorch_lightning and taming, see oracle/make_golden_vae.py,
whose module is reused), at configs/retrieval-augmented-diffusion/768x768.yaml's first_stage_config (ch 128, ch_mult [1,1,2,2,4],
z_channels 16, embed_dim 16, attn_resolutions [16]) and at the three stand-ins of `stable_diffusion_amd.synthetic` (kl_f16_thin: the yaml
at ch 64; kl_narrow: two levels, attention on the lower; kl_two_levels: attention on both).  Weights from `synthetic_named_state_dict`
over the module's own key list (seeded per key, so the GPU tests regenerate the same tensors from the HIP module's key list), fp32 on the
CPU.  Decode inputs are unit-variance latents divided by the yaml's scale_factor (what decode_first_stage hands to the decoder), encode
inputs uniform images in [-1, 1].
Every case stores its fp16-operand floor: the reference arithmetic with the operands of every 3x3 conv, of the q / k / v / proj_out
convs and of both attention products (q k^T, p v; p = exp(s - max) rounded, the denominator summed from the rounded p) rounded to fp16
once, fp32 accumulation, against the unrounded run, as `floor_maxabs`.  It comes from the reference, never from the library.  The tests
hold every mixed-precision case to the first-stage bars of tests/test_vae_gpu.py (decode 3.0e-3, moments 3.5e-3); a case measured above
its bar is listed by name in the test and held to 1.25 x its floor (README's rule of the outlier family).  This tool compares every floor
with the bar / 1.25 -- would the reference arithmetic at fp16 operands pass on its own? -- and lists the cases where it would not in
kl_f16_floors_above_bar.json: with these weights (0.577 / sqrt(fan_in) convs under a final GroupNorm, images of |x| up to 3) the decodes
of the five-level configurations do not, at any input seed tried (5.5e-3 .. 7.4e-3 at ch 128; the SD v1 decoder with the same weights has
3.0e-3 .. 3.4e-3), almost all of it from the 3x3 convs (the attention's share is 2e-4); every moments case does.
Also written: the key / shape list of the real configuration, the mask of attention levels read off the reference modules for the three
attn_resolutions the host test checks, and the parsed ddconfig.  The fixtures hold outputs and seeds, never weights.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden_vae import REF, _RefAutoencoderKL  # noqa: E402  (the reference checkout: $SD_REFERENCE)
OUT = os.path.join(ROOT, 'tests', 'golden')
RDM_YAML = os.path.join('configs', 'retrieval-augmented-diffusion', '768x768.yaml')
DEC_BAR, ENC_BAR = 3.0e-3, 3.5e-3             # tests/test_vae_gpu.py DEC_TOL / ENC_TOL

# (case, batch, latent h, latent w); the encode case of the same name takes the image of that latent (h * f, w * f)
KL_F16_CASES = [('6x10_b1', 1, 6, 10), ('8x8_b1', 1, 8, 8), ('8x8_b2', 2, 8, 8), ('10x12_b1', 1, 10, 12)]
KL_F16_THIN_CASES = [('6x10_b1', 1, 6, 10), ('8x8_b1', 1, 8, 8), ('10x12_b1', 1, 10, 12), ('8x8_b10', 10, 8, 8)]
KL_SMALL_CASES = [('8x8_b2', 2, 8, 8), ('8x12_b2', 2, 8, 12)]          # 16 x 16 and 16 x 24 images (f = 2)
CASES = {'kl_f16': KL_F16_CASES, 'kl_f16_thin': KL_F16_THIN_CASES, 'kl_narrow': KL_SMALL_CASES, 'kl_two_levels': KL_SMALL_CASES}


def case_seed(tag, case, kind):
    import zlib
    return zlib.crc32(f'{tag}/{case}/{kind}'.encode()) & 0x7fffffff


def decode_input(tag, case, batch, channels, h, w, scale_factor):
    g = torch.Generator().manual_seed(case_seed(tag, case, 'dec'))
    return torch.randn(batch, channels, h, w, generator=g) / scale_factor


def encode_input(tag, case, batch, channels, h, w):
    g = torch.Generator().manual_seed(case_seed(tag, case, 'enc'))
    return torch.rand(batch, channels, h, w, generator=g) * 2 - 1


def install_fp16_floor(m):
    """Round the operands named in the module docstring on the reference modules.  Returns the undo list."""
    from ldm.modules.diffusionmodules.model import AttnBlock
    from oracle.fp16_floor import r16
    undo = []

    def conv_forward(mod):
        return lambda x: F.conv2d(r16(x), r16(mod.weight), mod.bias, mod.stride, mod.padding)

    def attn_forward(mod):
        def forward(x):                                    # model.py:172-202 with the two products on rounded operands
            h_ = mod.norm(x)
            q, k, v = mod.q(h_), mod.k(h_), mod.v(h_)
            b, c, h, w = q.shape
            q, k, v = r16(q.reshape(b, c, h * w).permute(0, 2, 1)), r16(k.reshape(b, c, h * w)), r16(v.reshape(b, c, h * w))
            sim = torch.bmm(q, k) * (int(c) ** (-0.5))
            p16 = r16(torch.exp(sim - sim.amax(dim=2, keepdim=True)))
            out = torch.bmm(v, p16.permute(0, 2, 1)) / p16.sum(dim=2)[:, None, :]
            return x + mod.proj_out(out.reshape(b, c, h, w))
        return forward

    attn_convs = set()
    for name, mod in m.named_modules():
        if isinstance(mod, AttnBlock):
            undo.append(mod)
            mod.forward = attn_forward(mod)
            attn_convs.update(id(c) for c in (mod.q, mod.k, mod.v, mod.proj_out))
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Conv2d) and (mod.kernel_size == (3, 3) or id(mod) in attn_convs):
            undo.append(mod)
            mod.forward = conv_forward(mod)
    return undo


def remove_fp16_floor(undo):
    for mod in undo:
        del mod.forward


def reference_mask(Encoder, Decoder, ddconfig):
    """bit l = level l carries AttnBlocks, read off the constructed reference modules (both must agree)"""
    import contextlib
    import io
    with torch.device('meta'), contextlib.redirect_stdout(io.StringIO()):
        e, d = Encoder(**ddconfig), Decoder(**ddconfig)
    me = sum(1 << l for l, lv in enumerate(e.down) if len(lv.attn) > 0)
    md = sum(1 << l for l, lv in enumerate(d.up) if len(lv.attn) > 0)
    assert me == md, (me, md)
    for l, lv in enumerate(e.down):
        assert len(lv.attn) in (0, ddconfig['num_res_blocks'])
    for l, lv in enumerate(d.up):
        assert len(lv.attn) in (0, ddconfig['num_res_blocks'] + 1)
    return me


def main():
    import yaml
    sys.path.insert(0, REF)
    from ldm.modules.diffusionmodules.model import Decoder, Encoder
    from stable_diffusion_amd.synthetic import (KL_F16_DDCONFIG, KL_F16_KWARGS, KL_F16_SCALE_FACTOR, KL_F16_STANDINS, KL_NARROW_DDCONFIG,
                                                synthetic_named_state_dict)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    with open(os.path.join(REF, RDM_YAML)) as f:
        params = yaml.safe_load(f)['model']['params']
    fs = params['first_stage_config']['params']
    assert dict(fs['ddconfig']) == KL_F16_DDCONFIG and fs['embed_dim'] == KL_F16_KWARGS['embed_dim']
    assert params['scale_factor'] == KL_F16_SCALE_FACTOR
    masks = {json.dumps(r): reference_mask(Encoder, Decoder, dict(KL_NARROW_DDCONFIG, attn_resolutions=r)) for r in ([16], [32, 16], [])}
    masks['kl_f16'] = reference_mask(Encoder, Decoder, KL_F16_DDCONFIG)
    with torch.device('meta'):
        real = _RefAutoencoderKL(Encoder, Decoder, KL_F16_DDCONFIG, KL_F16_KWARGS['embed_dim'])
    specs = [(k, tuple(v.shape)) for k, v in real.state_dict().items()]
    n_params = sum(int(np.prod(s)) for _, s in specs)
    print(f'[kl_f16] {len(specs)} keys, {n_params} parameters; attention level masks {masks}', flush=True)
    with open(os.path.join(OUT, 'kl_f16_state_dict_keys.json'), 'w') as f:
        json.dump({'module': 'AutoencoderKL(**retrieval-augmented-diffusion/768x768.yaml first_stage_config.params) minus loss.*',
                   'n_params': n_params, 'first_stage_params': {'embed_dim': fs['embed_dim'], 'ddconfig': dict(fs['ddconfig'])},
                   'scale_factor': params['scale_factor'], 'narrow_ddconfig': KL_NARROW_DDCONFIG, 'attn_level_masks': masks,
                   'keys': [[k, list(s)] for k, s in specs]}, f)

    worst, above = {'dec': 0.0, 'enc': 0.0}, []
    for tag, cases in CASES.items():
        kw = KL_F16_STANDINS[tag]
        dd, ed = kw['ddconfig'], kw['embed_dim']
        m = _RefAutoencoderKL(Encoder, Decoder, dd, ed).eval()
        m.load_state_dict(synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        f_ = 2 ** (len(dd['ch_mult']) - 1)
        for case, b, h, w in cases:
            z = decode_input(tag, case, b, ed, h, w, KL_F16_SCALE_FACTOR)
            x = encode_input(tag, case, b, dd['in_channels'], h * f_, w * f_)
            with torch.no_grad():
                img, mom = m.decode(z), m.encode_moments(x)
                undo = install_fp16_floor(m)
                try:
                    fl_dec, fl_enc = float((m.decode(z) - img).abs().max()), float((m.encode_moments(x) - mom).abs().max())
                finally:
                    remove_fp16_floor(undo)
                assert torch.equal(m.decode(z), img)                  # (the rounding is gone again)
            print(f'[{tag} {case}] decode |img| max {img.abs().max():.3f} floor {fl_dec:.3e}; moments max {mom.abs().max():.3f} '
                  f'floor {fl_enc:.3e}', flush=True)
            assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(mom).all())
            if fl_dec > DEC_BAR / 1.25: above.append((tag, 'dec', case, fl_dec))
            if fl_enc > ENC_BAR / 1.25: above.append((tag, 'enc', case, fl_enc))
            worst['dec'], worst['enc'] = max(worst['dec'], fl_dec), max(worst['enc'], fl_enc)
            # (B = 10, the module's two library calls of 8 + 2: the images on both sides of the seam and the two ends are kept, all ten
            # are decoded by the test -- ten 128 x 128 images would be a 1.8 MB fixture; the floor is over all ten)
            keep = list(range(b)) if b <= 8 else [0, 7, 8, b - 1]
            np.savez_compressed(os.path.join(OUT, f'{tag}_dec_{case}.npz'), out=img[keep].numpy().astype(np.float32), samples=np.array(keep),
                                floor_maxabs=fl_dec,
                                weight_seed=0, input_seed=case_seed(tag, case, 'dec'), batch=b, h=h, w=w,
                                scale_factor=KL_F16_SCALE_FACTOR)
            np.savez_compressed(os.path.join(OUT, f'{tag}_enc_{case}.npz'), moments=mom.numpy().astype(np.float32), floor_maxabs=fl_enc,
                                weight_seed=0, input_seed=case_seed(tag, case, 'enc'), batch=b, h=h * f_, w=w * f_)
    print(f'KL-f16 fixtures written to {OUT}; largest floor: decode {worst["dec"]:.3e} (bar / 1.25 = {DEC_BAR / 1.25:.3e}), '
          f'moments {worst["enc"]:.3e} (bar / 1.25 = {ENC_BAR / 1.25:.3e})')
    for tag, kind, case, fl in above:
        print(f'  floor above bar / 1.25: {tag} {kind} {case} {fl:.3e}')
    with open(os.path.join(OUT, 'kl_f16_floors_above_bar.json'), 'w') as f:
        json.dump({'dec_bar': DEC_BAR, 'enc_bar': ENC_BAR, 'above_bar_over_1.25': [[t, k, c, fl] for t, k, c, fl in above]}, f)


if __name__ == '__main__':
    main()
