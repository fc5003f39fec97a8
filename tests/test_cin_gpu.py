"""The class-conditional ImageNet model (configs/latent-diffusion/cin256-v2.yaml) on the MI355X.

The wide-head attention kernel (csrc/attn_wide.hip: single-headed SpatialTransformers, d_head = C = 384 / 576 / 960) against fp64 on
the fp16-rounded operands; the whole UNet against goldens of the reference's own UNetModel (tools/make_golden_cin.py; weights
regenerated from the seeded per-key generator stable_diffusion_amd.synthetic.synthetic_named_state_dict) at the project's one
mixed-precision bar, with the one-token collapse of the cross-attention and with SDMI_CTX1=0; launch tapes, the timestep table and the pinned
context; 12 rows against 8 + 4."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import synthetic  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MIXED_TOL = 1e-3           # the project's mixed-precision bar, max-abs on eps
CTX1_TOL = 1e-4            # collapse against the general path: a tenth of the bar (measured on the reference modules: 4.2e-7 per block)
ATTN_TOL = 4e-3            # tests/test_inpaint_gpu.py test_attention_d96_vs_fp64: same operand / output types, unit-variance scores
_models = {}


def _lib():
    from stable_diffusion_amd import _lib as L
    return L


# ---- the wide-head kernel -------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(1024, 1024), (256, 256), (64, 64), (77, 77), (257, 129), (33, 1001), (64, 1), (16, 4), (1, 1)]


def _attention(q, k, vt, B, heads, nq, nkv, nkv_pad, d, scale):
    lib = _lib().load()
    out = torch.empty(B, nq, heads * d, dtype=torch.float16, device='cuda')
    _lib().check(lib.sdmi_k_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), B * heads, heads, nq, nkv, nkv_pad, d,
                                      scale, _lib().stream_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('heads', [1, 2])
@pytest.mark.parametrize('BH', [2, 8])
@pytest.mark.parametrize('nq,nkv', ATTN_SHAPES)
@pytest.mark.parametrize('d', [192, 384, 576, 960])
def test_attention_wide_vs_fp64(d, nq, nkv, BH, heads):
    """Measured on an MI355X (max over BH and heads, max-abs against fp64 on the same fp16 operands): see DESIGN.md section 2."""
    torch.manual_seed(d + nq + nkv)
    B, nkv_pad = BH // heads, (nkv + 7) // 8 * 8
    q = torch.randn(BH, nq, d, device='cuda').half()
    k = torch.randn(BH, nkv, d, device='cuda').half()
    v = torch.randn(BH, nkv, d, device='cuda').half()
    # the V^T pad columns hold garbage: masked keys must not reach the product at all
    garbage = (nq, nkv) in [(257, 129), (64, 1)]
    vt = torch.full((BH, d, nkv_pad), 1e4 if garbage else 0.0, device='cuda').half()
    vt[:, :, :nkv] = v.transpose(1, 2)
    scale = d ** -0.5
    out = _attention(q, k, vt, B, heads, nq, nkv, nkv_pad, d, scale)
    ref = torch.softmax(q.double() @ k.double().transpose(1, 2) * scale, dim=-1) @ v.double()           # [BH][nq][d]
    ref = ref.view(B, heads, nq, d).permute(0, 2, 1, 3).reshape(B, nq, heads * d)
    err = float((out.double() - ref).abs().max())
    print(f'[attn wide d={d} nq={nq} nkv={nkv} BH={BH} heads={heads}] max-abs {err:.3e}', flush=True)
    assert torch.isfinite(out).all()
    assert err <= ATTN_TOL
    if nkv == 1:          # softmax over one key is exactly 1: the output is V itself
        want = v.view(B, heads, 1, d).permute(0, 2, 1, 3).reshape(B, 1, heads * d).expand(B, nq, heads * d)
        assert torch.equal(out, want)


def test_attention_wide_pad_columns_nan():
    """The pad columns of V^T may hold anything, NaN included: the last key tile replaces them by zeros before the product."""
    torch.manual_seed(3)
    BH, nq, nkv, d = 2, 40, 13, 384
    q = torch.randn(BH, nq, d, device='cuda').half()
    k = torch.randn(BH, nkv, d, device='cuda').half()
    v = torch.randn(BH, nkv, d, device='cuda').half()
    vt = torch.full((BH, d, 16), float('nan'), device='cuda').half()
    vt[:, :, :nkv] = v.transpose(1, 2)
    out = _attention(q, k, vt, BH, 1, nq, nkv, 16, d, d ** -0.5)
    ref = torch.softmax(q.double() @ k.double().transpose(1, 2) * d ** -0.5, dim=-1) @ v.double()
    assert torch.isfinite(out).all()
    assert float((out.double() - ref).abs().max()) <= ATTN_TOL


def test_attention_head_dim_between_the_kernels_is_an_error():
    lib = _lib().load()
    z = torch.zeros(2 * 8 * 176, dtype=torch.float16, device='cuda')
    rc = lib.sdmi_k_attention(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 2, 1, 8, 8, 8, 176, 1.0, _lib().stream_ptr())
    assert rc != 0
    with pytest.raises(RuntimeError, match='head dim 176 not instantiated'):
        _lib().check(rc)


# ---- whole UNet vs the reference's goldens ------------------------------------------------------------------------------------
UNET_CASES = ['64x64_b1', '64x64_b2', '32x32_b2', '96x96_b1', '16x16_b2', '64x64_b6']


def _unet():
    if 'unet' not in _models:
        torch.cuda.empty_cache()
        from stable_diffusion_amd import UNetModelHIP
        m = UNetModelHIP(**synthetic.CIN_UNET_KWARGS)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models['unet'] = m.cuda().eval()
    return _models['unet']


def _embedder():
    if 'emb' not in _models:
        from stable_diffusion_amd import ClassEmbedderHIP
        m = ClassEmbedderHIP(**synthetic.CIN_CLASS_KWARGS)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models['emb'] = m.cuda().eval()
    return _models['emb']


def _unet_inputs(batch, h, w, ts, seed=1):       # (tools/make_golden_cin.py unet_inputs)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, 3, h, w, generator=g).cuda(), torch.tensor(ts, dtype=torch.int64).cuda()


def _context(classes):
    with torch.no_grad():
        return _embedder()({'class_label': torch.as_tensor(classes, dtype=torch.int64).cuda()})


def _case(name):
    z = np.load(os.path.join(GOLD, f'cin_unet_{name}.npz'))
    x, t = _unet_inputs(int(z['batch']), int(z['h']), int(z['w']), [int(v) for v in z['t']], int(z['input_seed']))
    return z, x, t


def _both_paths(case, monkeypatch):
    z, x, t = _case(case)
    ctx = _context(z['classes'])
    assert ctx.shape == (x.shape[0], 1, 512)
    m = _unet()
    monkeypatch.delenv('SDMI_CTX1', raising=False)
    eps1 = m(x, t, context=ctx).clone()
    monkeypatch.setenv('SDMI_CTX1', '0')
    eps0 = m(x, t, context=ctx.clone()).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(eps1).all() and torch.isfinite(eps0).all()
    return eps1, eps0, torch.tensor(z['eps']).cuda()


@pytest.mark.parametrize('case', UNET_CASES)
def test_cin_unet_vs_reference(case, monkeypatch):
    """One-token contexts: with the collapse of the cross-attention (its output copied from the cached V^T) and with SDMI_CTX1=0 (the
    general cross-attention at one key on the wide kernel); both meet the project's bar.  Measured on an MI355X, max-abs (either
    path: they are bit-identical): 64x64_b1 5.69e-4, 64x64_b2 5.71e-4, 32x32_b2 6.36e-4, 96x96_b1 5.79e-4, 16x16_b2 4.65e-4,
    64x64_b6 6.72e-4."""
    eps1, eps0, ref = _both_paths(case, monkeypatch)
    e1, e0 = float((eps1 - ref).abs().max()), float((eps0 - ref).abs().max())
    print(f'[cin unet {case}] max-abs vs reference: collapse {e1:.3e}, SDMI_CTX1=0 {e0:.3e} (|eps| max {float(ref.abs().max()):.3f})', flush=True)
    assert e1 <= MIXED_TOL and e0 <= MIXED_TOL


@pytest.mark.parametrize('case', UNET_CASES)
def test_cin_collapse_vs_general_path(case, monkeypatch):
    """The collapse against SDMI_CTX1=0 at a tenth of the bar (1e-4).  Measured on an MI355X: 0 on every case -- the collapse leaves
    out launches whose result is known (to_q, the attention at one key: fp16(V) bit for bit) and changes no other, so no fp32 sum is
    taken in another order.  That is what the bound takes on this UNet: a collapse that also folded the second out-projection into a
    row vector added by attn1's out-projection (same fp16 operands, another fp32 summation order) measured 4.07e-4 ... 4.96e-4 from
    SDMI_CTX1=0, and SDMI_CONV_IN_STATS=0 -- other fp32 partials of the first GroupNorm's sums, nothing else -- moves eps by 4.31e-4
    (profiles/ctx1_drift.txt): an fp32 ulp in the token stream flips fp16 roundings of the next MFMA operands, and the flips cascade to
    the mixed-precision rounding floor."""
    eps1, eps0, _ = _both_paths(case, monkeypatch)
    d = float((eps1 - eps0).abs().max())
    print(f'[cin unet {case}] collapse vs SDMI_CTX1=0: max-abs {d:.3e} rms {float((eps1 - eps0).pow(2).mean().sqrt()):.3e}', flush=True)
    assert d <= CTX1_TOL


def _launches(fn):
    """{profiler name: launches} of the library launches fn() makes"""
    import json
    lib = _lib().load()
    _lib().check(lib.sdmi_profile_begin())
    try:
        fn()
    finally:
        buf = C.create_string_buffer(1 << 20)
        _lib().check(lib.sdmi_profile_end(buf, len(buf)))
    return {r['name']: r['launches'] for r in json.loads(buf.value.decode())}


def test_cin_collapse_leaves_out_to_q_and_the_cross_attention(monkeypatch):
    """16 transformer blocks: with the collapse 16 self-attention launches and 16 copies of V, no attention over the context; with
    SDMI_CTX1=0 the 16 cross-attentions at one key, and 16 GEMM launches more (to_q)."""
    z, x, t = _case('32x32_b2')
    ctx = _context(z['classes'])
    m = _unet()
    m(x, t, context=ctx)                                   # (packs)
    monkeypatch.delenv('SDMI_CTX1', raising=False)
    on = _launches(lambda: m(x, t, context=ctx.clone()))
    monkeypatch.setenv('SDMI_CTX1', '0')
    off = _launches(lambda: m(x, t, context=ctx.clone()))
    attn = lambda d: sum(n for k, n in d.items() if k.startswith('attn_d'))
    print(f'[cin launches] collapse {sum(on.values())} (attention {attn(on)}), SDMI_CTX1=0 {sum(off.values())} (attention {attn(off)})', flush=True)
    assert on.get('ctx1_broadcast') == 16 and 'ctx1_broadcast' not in off
    assert attn(on) == 16 and attn(off) == 32
    assert sum(off.values()) - sum(on.values()) >= 16      # to_q (and its split-K reductions where it is split): attention and copy cancel


def test_cin_unet_four_token_context_vs_reference():
    """[B, 4, 512]: the general cross-attention (to_q, the wide kernel at four keys, the second out-projection)."""
    z, x, t = _case('32x32_b2_ctx4')
    ctx = torch.randn(int(z['batch']), 4, 512, generator=torch.Generator().manual_seed(int(z['ctx_seed']))).cuda()
    eps = _unet()(x, t, context=ctx)
    err = float((eps - torch.tensor(z['eps']).cuda()).abs().max())
    print(f'[cin unet 32x32_b2_ctx4] max-abs vs reference {err:.3e}', flush=True)
    assert err <= MIXED_TOL


# ---- tapes, timestep table, pinned context ----------------------------------------------------------------------------------
@pytest.mark.parametrize('ctx1', ['1', '0'])
def test_cin_taped_hinted_pinned_calls_are_bit_identical(ctx1, monkeypatch):
    monkeypatch.setenv('SDMI_CTX1', ctx1)
    m = _unet()
    x, t = _unet_inputs(2, 32, 32, (981, 981))
    x2, _ = _unet_inputs(2, 32, 32, (981, 981), seed=5)
    ctx_a, ctx_b = _context([25, 1000]), _context([992, 7])
    monkeypatch.setenv('SDMI_REPLAY', '0')
    m.unpin_context()
    m.cache_timesteps([])
    want_a, want_b, want_a2 = m(x, t, context=ctx_a).clone(), m(x, t, context=ctx_b).clone(), m(x2, t, context=ctx_a.clone()).clone()
    assert not torch.equal(want_a, want_b)
    monkeypatch.setenv('SDMI_REPLAY', '1')
    rec = m(x, t, context=ctx_a.clone()).clone()            # records
    rep = m(x, t, context=ctx_a.clone()).clone()            # replays
    rep2 = m(x2, t, context=ctx_a.clone()).clone()
    assert torch.equal(rec, want_a) and torch.equal(rep, want_a) and torch.equal(rep2, want_a2)
    m.cache_timesteps([981, 1])
    m.hint_timestep(981)
    assert torch.equal(m(x, t, context=ctx_a.clone()), want_a)
    m.pin_context(ctx_a)
    for _ in range(2):                                      # (record, replay: ctx = NULL, the cached K / V^T)
        m.hint_timestep(981)
        assert torch.equal(m(x, t, context=ctx_a), want_a)
    # another class while ctx_a is pinned: that class's result, not the pinned V
    m.hint_timestep(981)
    assert torch.equal(m(x, t, context=ctx_b), want_b)
    assert torch.equal(m(x, t, context=ctx_a.clone()), want_a)
    monkeypatch.setenv('SDMI_REPLAY_VERIFY', '1')
    assert torch.equal(m(x, t, context=ctx_a.clone()), want_a)
    m.unpin_context()
    m.cache_timesteps([])


def test_cin_twelve_rows_equal_eight_plus_four():
    """The notebook's cell: 6 samples with guidance = 12 rows per call = chunks of 8 + 4 (rows are independent)."""
    m = _unet()
    x, t = _unet_inputs(12, 32, 32, (981,) * 12, seed=4)
    ctx = _context([1000] * 6 + [25] * 6)
    all12 = m(x, t, context=ctx).clone()
    first, rest = m(x[:8], t[:8], context=ctx[:8]).clone(), m(x[8:], t[8:], context=ctx[8:]).clone()
    assert torch.equal(all12, torch.cat([first, rest]))


# ---- first stage (VQ-f4 with mid-block attention) --------------------------------------------------------------------------
# max-abs, 1.25 x measured on an MI355X: h 1.603e-3, decode 4.892e-3 (rms 5.3e-4).  The attention-free VQ stage of the inpainting model
# measured 1.63e-3 / 3.98e-3 (tests/test_inpaint_gpu.py): the mid-block attention moves the encoder not at all and the decoder by 1.2 x.
VQ_PINS = {'h': 2.0e-3, 'dec_q': 6.1e-3}


def _vq():
    if 'vq' not in _models:
        from stable_diffusion_amd import VQModelInterfaceHIP
        m = VQModelInterfaceHIP(**synthetic.CIN_VQ_KWARGS)
        m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 0), strict=True)
        _models['vq'] = m.cuda()
    return _models['vq']


def _vq_inputs(seed=1, img=128):                 # (tools/make_golden_cin.py vq_inputs)
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(2, 3, img // 8, img // 8, generator=g) * 2 - 1
    x = torch.nn.functional.interpolate(low, scale_factor=8, mode='bilinear', align_corners=False)
    x = (x + 0.1 * torch.randn(x.shape, generator=g)).clamp(-1, 1)
    return x, torch.randn(2, 3, img // 4, img // 4, generator=g)


def test_cin_first_stage_matches_reference():
    z = np.load(os.path.join(GOLD, 'cin_vq_128.npz'))
    img, lat = _vq_inputs(seed=int(z['input_seed']), img=int(z['img']))
    m = _vq()
    h = m.encode(img.cuda()).cpu()
    dec_q = m.decode(lat.cuda()).cpu()
    torch.cuda.synchronize()
    errs = {}
    for name, got in (('h', h), ('dec_q', dec_q)):
        ref = torch.from_numpy(z[name])
        assert got.shape == ref.shape
        err = (got - ref).abs()
        errs[name] = float(err.max())
        print(f'[cin vq {name}] max-abs {err.max():.3e} rms {err.pow(2).mean().sqrt():.3e} |ref|max {ref.abs().max():.3f} '
              f'(pin {VQ_PINS[name]:.1e})', flush=True)
    assert all(errs[k] <= VQ_PINS[k] for k in errs), errs


# ---- pipeline: the cell of scripts/latent_imagenet_diffusion.ipynb ----------------------------------------------------------
# max-abs (samples: relative to |samples| max = 144.8), 1.25 x measured 2.301e-4 / 2.833e-3
PIPE_PIN = {'samples_rel': 2.9e-4, 'x_dec': 3.5e-3}


def test_cin_pipeline_matches_reference_loop():
    """Classes 25 and 992, two samples each, classifier-free guidance (scale 3.0) against class 1000, 10 DDIM steps, eta 0, on the
    HIP classes -- against the same loop on the reference modules and the reference DDIMSampler.  Compared: the conditioning (a table
    lookup: exact), the sampled latent, and the decode of the golden's own sampled latent (a code flip near a boundary would make an
    image-to-image comparison after quantization unfair)."""
    from stable_diffusion_amd import DDIMSamplerHIP, LatentDiffusionHIP
    z = np.load(os.path.join(GOLD, 'cin_pipeline_96.npz'))
    n, classes = int(z['n_samples_per_class']), [int(c) for c in z['classes']]
    ld = LatentDiffusionHIP(_unet(), **synthetic.CIN_SCHEDULE).cuda()
    emb = _embedder()
    g = torch.Generator().manual_seed(int(z['input_seed']))
    ref_s = torch.from_numpy(z['samples'])
    hw = tuple(ref_s.shape[-2:])
    conds, lats = [], []
    with torch.no_grad():
        uc = emb({'class_label': torch.tensor(n * [1000]).cuda()})
        for cls in classes:
            x_T = torch.randn(n, 3, *hw, generator=g)
            c = emb({'class_label': torch.tensor(n * [cls]).cuda()})
            with contextlib.redirect_stdout(io.StringIO()):
                s, _ = DDIMSamplerHIP(ld).sample(S=int(z['steps']), conditioning=c, batch_size=n, shape=[3, *hw], verbose=False,
                                                 x_T=x_T.cuda(), unconditional_guidance_scale=float(z['scale']),
                                                 unconditional_conditioning=uc, eta=float(z['eta']))
            conds.append(c)
            lats.append(s)
    samples = torch.cat(lats)
    x_dec = _vq().decode(ref_s.cuda())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(conds).cpu(), torch.from_numpy(z['cond'])) and torch.equal(uc.cpu(), torch.from_numpy(z['uc']))
    e_s = float((samples.cpu() - ref_s).abs().max()) / float(ref_s.abs().max())
    e_x = float((x_dec.cpu() - torch.from_numpy(z['x_dec'])).abs().max())
    print(f'[cin pipeline] samples max-abs / |samples|max {e_s:.3e} (|samples| max {ref_s.abs().max():.2f}); '
          f'decode of the golden latent max-abs {e_x:.3e}', flush=True)
    assert bool(torch.isfinite(samples).all())
    assert e_s <= PIPE_PIN['samples_rel'] and e_x <= PIPE_PIN['x_dec']
