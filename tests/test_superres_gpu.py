"""bsr_sr's tiled image pipeline on the MI355X (LatentDiffusion.split_input_params, ddpm.py:564-651, 715-752, 826-858, 902-984).

Kernels in guarded buffers (tests/guard.py): sdmi_k_patch_unfold bit-equal to torch.nn.Unfold plus the channel concat on the 16-byte and
the element-wise path; sdmi_k_patch_fold against an fp64 evaluation of the same expression at a derived per-element bar and against the
reference's own fp32 fold at twice that bar; the launcher's refusals.  Then the tiled apply_model, decode_first_stage and
encode_first_stage and a 10-step DDIM pipeline against goldens of the reference's own methods (tools/make_golden_superres.py).  The
fold is a convex combination of window outputs (weights positive, normalised), so the folded error cannot exceed the worst window's:
the bars of the tiled tests are the un-tiled ones of the UNet and the VQ-f4 first stage."""
import contextlib
import io
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
from stable_diffusion_amd import _lib, ldm_shim, synthetic  # noqa: E402

DEV = 'cuda'
MIXED_TOL = 1e-3        # tests/test_faces_gpu.py: the UNet's mixed-precision bar
FULL_TOL = 2e-5         # ... and its full-mode bar
VQ_DEC_PIN = 6.1e-3     # tests/test_faces_gpu.py VQ_DEC_PIN = tests/test_cin_gpu.py VQ_PINS['dec_q']: the un-tiled VQ-f4 decode
VQ_ENC_PIN = 2.0e-3     # tests/test_cin_gpu.py VQ_PINS['h']: the un-tiled VQ-f4 encode
U = 2.0 ** -24          # fp32 unit roundoff
CLIPS = dict(clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
# name, (H, W), ks, stride, uf, df, tie_braker (tools/make_golden_superres.py FOLD_GEOMS): stride = ks (one covering window), ks / 2 (<= 4),
# ks / 4 (<= 16), the scaled folds around the first stage, a non-square window, and a geometry no quantity of which is a multiple of 4
FOLD_GEOMS = [('s1', (32, 32), (16, 16), (16, 16), 1, 1, False), ('s2', (24, 32), (16, 16), (8, 8), 1, 1, False),
              ('s4', (32, 32), (16, 16), (4, 4), 1, 1, False), ('s2_tie', (24, 32), (16, 16), (8, 8), 1, 1, True),
              ('s4_tie', (32, 32), (16, 16), (4, 4), 1, 1, True), ('uf4', (24, 32), (16, 16), (8, 8), 4, 1, False),
              ('uf4_tie', (24, 32), (16, 16), (8, 8), 4, 1, True), ('df4', (64, 96), (32, 32), (16, 16), 1, 4, False),
              ('rect', (24, 24), (16, 8), (8, 8), 1, 1, False), ('unaligned', (21, 27), (9, 11), (3, 4), 1, 1, False),
              ('unaligned_tie', (21, 27), (9, 11), (3, 4), 1, 1, True)]
FOLD_B, FOLD_C = 2, 2
_models = {}


def params(ks, stride, tie=False, vqf=4):
    return dict(ks=tuple(ks), stride=tuple(stride), vqf=vqf, patch_distributed_vq=True, tie_braker=tie, **CLIPS)


def seeded(shape, seed, scale=1.0):                         # (tools/make_golden_superres.py seeded)
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---- unfold -----------------------------------------------------------------------------------------------------------------------
# name, B, Cx, Cc, (H, W), ks, stride, l0, nl (None = all windows)
UNFOLD_CASES = [('concat', 2, 3, 3, (24, 32), (16, 16), (8, 8), 0, None), ('no-cond', 2, 3, 0, (24, 32), (16, 16), (8, 8), 0, None),
                ('rect', 2, 3, 3, (24, 24), (16, 8), (8, 8), 0, None), ('unaligned', 2, 3, 3, (21, 27), (9, 11), (3, 4), 0, None),
                ('sub-range', 2, 3, 3, (24, 32), (16, 16), (8, 8), 2, 3), ('unaligned-sub-range', 1, 2, 1, (21, 27), (9, 11), (3, 4), 7, 5),
                ('one-window', 1, 3, 3, (16, 16), (16, 16), (8, 8), 0, None)]


@pytest.mark.parametrize('name,B,Cx,Cc,hw,ks,stride,l0,nl', UNFOLD_CASES, ids=[c[0] for c in UNFOLD_CASES])
def test_unfold_is_bit_equal_to_torch_unfold_plus_cat(name, B, Cx, Cc, hw, ks, stride, l0, nl):
    H, W = hw
    x, c = seeded((B, Cx, H, W), 11), seeded((B, Cc, H, W), 12) if Cc else None
    xc = x if c is None else torch.cat([x, c], 1)
    cols = torch.nn.Unfold(ks, stride=stride)(xc)                                        # (B, C kh kw, L)
    L = cols.shape[-1]
    nl = L if nl is None else nl
    ref = cols.view(B, Cx + Cc, ks[0], ks[1], L).permute(4, 0, 1, 2, 3)[l0:l0 + nl].reshape(nl * B, Cx + Cc, ks[0], ks[1])
    P = guard.Pool(DEV)
    gx, gc = P.put('x', x), P.put('c', c) if Cc else None
    out = P.new('out', (nl * B, Cx + Cc, ks[0], ks[1]), torch.float32)
    got = ldm_shim.patch_unfold(gx, gc, ks, stride, l0, nl, out=out)
    torch.cuda.synchronize()
    assert got is out
    P.check(f'unfold {name}')
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(gx.cpu(), x) and (c is None or torch.equal(gc.cpu(), c))


# ---- fold ----------------------------------------------------------------------------------------------------------------------
def _fold64(o, w, B, hw, ks, stride, uf, df):
    """fp64 evaluation of sum_l w[l] o[(l, b)] / sum_l w[l] through torch's Fold, with sum |w o| and the number of covering windows"""
    L, kh, kw = w.shape
    shape = (hw[0] * uf // df, hw[1] * uf // df)
    f = torch.nn.Fold(shape, (kh, kw), stride=(stride[0] * uf // df, stride[1] * uf // df))
    o5 = o.double().view(L, B, -1, kh, kw).permute(1, 2, 3, 4, 0)                       # (B, C, kh, kw, L)
    w5 = w.double().permute(1, 2, 0)[None, None]
    num, absnum = f((o5 * w5).reshape(B, -1, L)), f((o5 * w5).abs().reshape(B, -1, L))
    den, n = f(w5.reshape(1, -1, L)), f(torch.ones(1, kh * kw, L, dtype=torch.float64))
    return num / den, absnum, den, n


@pytest.mark.parametrize('name,hw,ks,stride,uf,df,tie', FOLD_GEOMS, ids=[g[0] for g in FOLD_GEOMS])
def test_fold_vs_fp64_and_reference(name, hw, ks, stride, uf, df, tie, golden_dir):
    """Bar per element, derived: each of the n products w o is rounded once and the two running sums take n - 1 additions each, the
    quotient one more rounding -- (n + 3) 2^-24 sum |w o| / sum w covers the products, the additions of the numerator as they
    accumulate and the quotient; the reference's fp32 fold carries an error of the same size, hence twice the bar against it."""
    z = np.load(os.path.join(golden_dir, 'superres_fold.npz'))
    w = torch.from_numpy(z[f'{name}_weighting'])[0, 0].permute(2, 0, 1).contiguous()        # [L, kh', kw']
    L, kh, kw = w.shape
    o = torch.randn((L * FOLD_B, FOLD_C, kh, kw), generator=torch.Generator().manual_seed(zlib.crc32(name.encode())))
    ref64, absnum, den, n = _fold64(o, w, FOLD_B, hw, ks, stride, uf, df)
    bar = (n + 3) * U * absnum / den
    assert int(n.max()) == {'s1': 1, 's2': 4, 's4': 16, 'df4': 4, 'rect': 2}.get(name.split('_')[0], int(n.max())) and int(n.min()) >= 1
    P = guard.Pool(DEV)
    go, gw = P.put('o', o), P.put('w', w)
    outs = []
    for _ in range(2):
        out = P.new('out', tuple(ref64.shape), torch.float32)
        assert ldm_shim.patch_fold(go, gw, FOLD_B, hw, ks, stride, uf=uf, df=df, out=out) is out
        outs.append(out)
    norm = P.new('norm', tuple(ref64.shape[2:]), torch.float32)
    ldm_shim.patch_fold(None, gw, FOLD_B, hw, ks, stride, uf=uf, df=df, norm_only=True, out=norm)
    torch.cuda.synchronize()
    P.check(f'fold {name}')
    assert torch.equal(go.cpu(), o) and torch.equal(gw.cpu(), w)
    got = outs[0].cpu()
    assert torch.equal(outs[0], outs[1]), 'two runs differ'
    e64 = (got.double() - ref64).abs()
    eref = (got.double() - torch.from_numpy(z[f'{name}_folded']).double()).abs()
    print(f'[fold {name}] n <= {int(n.max())}: vs fp64 max-abs {e64.max():.3e}, worst err / bar {(e64 / bar).max():.3f}; vs the reference fold '
          f'max-abs {eref.max():.3e}, worst err / (2 bar) {(eref / (2 * bar)).max():.3f}', flush=True)
    assert bool(torch.isfinite(got).all())
    assert bool((e64 <= bar).all()) and bool((eref <= 2 * bar).all())
    # normalisation alone, pinned bit for bit: sequential fp32 additions of the golden weighting in ascending window index (numpy adds one
    # window at a time into an fp32 map, so every pixel sees its covering windows in ascending l) are what the kernel is specified to do
    Ly, Lx = ldm_shim.patch_grid(hw[0], hw[1], ks, stride)
    syo, sxo = stride[0] * uf // df, stride[1] * uf // df
    wnp = w.numpy()
    seq = np.zeros(tuple(ref64.shape[2:]), dtype=np.float32)
    for l in range(L):
        y0, x0 = (l // Lx) * syo, (l % Lx) * sxo
        seq[y0:y0 + kh, x0:x0 + kw] += wnp[l]
    gnorm32 = torch.from_numpy(z[f'{name}_normalization'])[0, 0]
    few = n[0, 0] <= 2
    enorm = (norm.cpu().double() - gnorm32.double()).abs()
    print(f'[fold {name}] normalisation: {int((norm.cpu() != torch.from_numpy(seq)).sum())} elements differ from the ascending-l fp32 sum; vs the '
          f'reference max-abs {enorm.max():.3e} ({int(few.sum())} of {few.numel()} elements under <= 2 windows)', flush=True)
    assert torch.equal(norm.cpu(), torch.from_numpy(seq))
    # against the reference's own map: fp32 addition is commutative, so at most two terms give the same bits in any order ...
    assert torch.equal(norm.cpu()[few], gnorm32[few])
    # ... and elsewhere torch's Fold may add the same n positive terms in another order: either sum is within (n - 1) 2^-24 sum w of the exact one
    assert bool((enorm <= 2 * (n[0, 0] - 1) * U * den[0, 0]).all())


BAD_GEOMS = [('kh > H', (12, 32), (16, 16), (8, 8), 1, 1), ('kw > W', (24, 12), (16, 16), (8, 8), 1, 1),
             ('off-grid y', (28, 32), (16, 16), (8, 8), 1, 1), ('off-grid x', (24, 30), (16, 16), (8, 8), 1, 1),
             ('uf and df', (32, 32), (16, 16), (8, 8), 4, 4), ('non-square uf', (24, 24), (16, 8), (8, 8), 4, 1),
             ('non-square df', (24, 24), (16, 8), (8, 8), 1, 4)]


@pytest.mark.parametrize('name,hw,ks,stride,uf,df', BAD_GEOMS, ids=[g[0].replace(' ', '-') for g in BAD_GEOMS])
def test_launcher_refuses_bad_geometry_and_launches_nothing(name, hw, ks, stride, uf, df):
    lib = _lib.load()
    P = guard.Pool(DEV)
    x = P.new('x', (1, 2, hw[0], hw[1]), torch.float32, fill=1.0)
    o = P.new('o', (64, 2, 64, 64), torch.float32, fill=1.0)          # larger than any window count / window of these cases
    w = P.new('w', (64, 64, 64), torch.float32, fill=1.0)
    out = P.new('out', (64, 2, 128, 128), torch.float32)              # stays 0xFF
    s = _lib.stream_ptr()
    if uf == 1 and df == 1:
        assert lib.sdmi_k_patch_unfold(x.data_ptr(), None, out.data_ptr(), 1, 2, 0, hw[0], hw[1], ks[0], ks[1], stride[0], stride[1], 0, 1, s) != 0
        assert b'patch unfold' in lib.sdmi_last_error()
    for norm_only in (0, 1):
        assert lib.sdmi_k_patch_fold(o.data_ptr(), w.data_ptr(), out.data_ptr(), 1, 2, hw[0], hw[1], ks[0], ks[1], stride[0], stride[1], uf, df,
                                     norm_only, s) != 0
        assert b'patch fold' in lib.sdmi_last_error()
    torch.cuda.synchronize()
    P.check(f'refused {name}')
    assert bool((out.view(torch.int32) == -1).all()), 'a refused call wrote its output'


def test_launcher_refuses_window_range_outside_the_grid():
    lib = _lib.load()
    P = guard.Pool(DEV)
    x = P.new('x', (1, 2, 24, 32), torch.float32, fill=1.0)
    out = P.new('out', (8, 2, 16, 16), torch.float32)
    for l0, nl in ((5, 2), (6, 1), (-1, 2), (0, 0)):
        assert lib.sdmi_k_patch_unfold(x.data_ptr(), None, out.data_ptr(), 1, 2, 0, 24, 32, 16, 16, 8, 8, l0, nl, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    P.check('window range')
    assert bool((out.view(torch.int32) == -1).all())


# ---- tiled apply_model ------------------------------------------------------------------------------------------------------------
def _named_synthetic(m, seed=0):
    m.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed), strict=True)
    return m


def _unet(prec, fresh=False):
    from stable_diffusion_amd import UNetModelHIP
    if fresh:
        return _named_synthetic(UNetModelHIP(**synthetic.BSR_UNET_KWARGS, hip_precision=prec)).cuda()
    if prec not in _models:
        _models.clear()
        torch.cuda.empty_cache()
        _models[prec] = _named_synthetic(UNetModelHIP(**synthetic.BSR_UNET_KWARGS, hip_precision=prec)).cuda()
    return _models[prec]


def _ld(unet, ks, stride, tie=False, first_stage_model=None):
    from stable_diffusion_amd import LatentDiffusionHIP
    ld = LatentDiffusionHIP(unet, first_stage_model=first_stage_model, cond_stage_key='LR_image', **synthetic.BSR_SCHEDULE).cuda()
    ld.split_input_params = params(ks, stride, tie)
    return ld


@pytest.mark.parametrize('prec', ['mixed', 'full'])
def test_tiled_apply_model_matches_reference(prec, golden_dir):
    """B = 2, latent 24 x 32, ks 16, stride 8: six windows, twelve rows, calls of 8 + 4 rows; rows of one call carry t = (981, 1) repeated
    per window; tie_braker off and on"""
    z = np.load(os.path.join(golden_dir, 'superres_apply_model_24x32.npz'))
    b, h, w = int(z['batch']), int(z['h']), int(z['w'])
    ks, stride = tuple(int(v) for v in z['ks']), tuple(int(v) for v in z['stride'])
    x, c = seeded((b, 3, h, w), int(z['x_seed'])).cuda(), seeded((b, 3, h, w), int(z['c_seed'])).cuda()
    t = torch.from_numpy(z['t']).cuda()
    tol = MIXED_TOL if prec == 'mixed' else FULL_TOL
    unet = _unet(prec)
    calls = []
    hook = unet.register_forward_pre_hook(lambda m, a: calls.append(tuple(a[0].shape)))
    errs = {}
    try:
        for tag, tie in (('eps', False), ('eps_tie', True)):
            ld = _ld(unet, ks, stride, tie)
            eps = ld.apply_model(x, t, c)
            torch.cuda.synchronize()
            ref = torch.from_numpy(z[tag])
            assert eps.shape == ref.shape and eps.dtype == torch.float32 and bool(torch.isfinite(eps).all())
            errs[tag] = float((eps.cpu() - ref).abs().max())
            print(f'[tiled apply_model {tag} {prec}] max-abs {errs[tag]:.3e} |eps|max {ref.abs().max():.3f} (tol {tol:.1e})', flush=True)
    finally:
        hook.remove()
    assert calls == [(8, 6, 16, 16), (4, 6, 16, 16)] * 2, calls
    assert all(e <= tol for e in errs.values()), errs


class _StubUNet(torch.nn.Module):
    """records its calls; eps = x, + the per-row sum of a token context, or + a windowed image context"""
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, x, t, context=None):
        self.calls.append((tuple(x.shape), t.clone(), None if context is None else tuple(context.shape)))
        if context is None:
            return 2.0 * x
        return x + (context if context.dim() == 4 else context.sum((1, 2)).view(-1, 1, 1, 1))


@pytest.mark.parametrize('kind', ['crossattn-tokens', 'crossattn-image', 'unconditional'])
def test_tiled_apply_model_branches_that_do_not_fuse_the_concat(kind):
    """Every window gets the same cross-attention tokens (ddpm.py:972) or None; an image conditioning that is not concatenated is cut into
    the same windows (ddpm.py:917-928).  With a stub UNet whose output is its input plus a term that is the same wherever windows overlap,
    the fold is a weighted mean of equal values v: the expected result is v within the fold's (n + 3) 2^-24 |v|, n <= 4.  The token
    context holds multiples of 1 / 8, so its sums are exact whatever their order."""
    from stable_diffusion_amd import LatentDiffusionHIP
    B, H, W, ks, stride = 2, 24, 32, (16, 16), (8, 8)
    x = seeded((B, 3, H, W), 31).cuda()
    t = torch.tensor([981, 1], device=DEV)
    stub = _StubUNet()
    if kind == 'crossattn-tokens':
        ld, cond = LatentDiffusionHIP(stub, conditioning_key='crossattn', cond_stage_key='caption'), (torch.round(seeded((B, 5, 7), 32)) / 8).cuda()
        want, ctx_shape = x + cond.sum((1, 2)).view(-1, 1, 1, 1), lambda rows: (rows, 5, 7)
    elif kind == 'crossattn-image':
        ld, cond = LatentDiffusionHIP(stub, conditioning_key='crossattn', cond_stage_key='image'), seeded((B, 3, H, W), 33).cuda()
        want, ctx_shape = x + cond, lambda rows: (rows, 3, 16, 16)
    else:
        ld, cond = LatentDiffusionHIP(stub, conditioning_key=None), None
        want, ctx_shape = 2.0 * x, lambda rows: None
    ld = ld.cuda()
    ld.split_input_params = params(ks, stride)
    got = ld.apply_model(x, t, cond)
    torch.cuda.synchronize()
    assert [(c[0], c[2]) for c in stub.calls] == [((8, 3, 16, 16), ctx_shape(8)), ((4, 3, 16, 16), ctx_shape(4))]
    assert torch.equal(stub.calls[0][1], t.repeat(4)) and torch.equal(stub.calls[1][1], t.repeat(2))
    assert tuple(got.shape) == (B, 3, H, W)
    err = (got - want).abs()
    print(f'[tiled apply_model {kind}] max-abs {float(err.max()):.3e}', flush=True)
    assert bool((err <= 7 * U * want.abs()).all())


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def test_tiled_apply_model_replayed_from_the_tape_equals_a_fresh_module():
    """two timesteps in succession (and the first again), every chunk announced by hint_timestep as the samplers do, against a fresh
    module that records nothing and takes no hint"""
    ks, stride = (16, 16), (8, 8)
    x, c = seeded((2, 3, 24, 32), 21).cuda(), seeded((2, 3, 24, 32), 22).cuda()
    ts = {v: torch.full((2,), v, dtype=torch.long, device=DEV) for v in (981, 1)}
    with _env('SDMI_REPLAY', '0'):
        fresh = _ld(_unet('mixed', fresh=True), ks, stride)
        want = {v: fresh.apply_model(x, ts[v], c).clone() for v in (981, 1)}
    del fresh
    unet = _unet('mixed')
    ld = _ld(unet, ks, stride)
    unet.cache_timesteps([981, 1])
    try:
        got = []
        for v in (981, 1, 981):
            unet.hint_timestep(v)
            got.append((v, ld.apply_model(x, ts[v], c).clone()))
            assert getattr(unet, '_t_hint', None) is None
    finally:
        unet.cache_timesteps([])
    torch.cuda.synchronize()
    assert not torch.equal(want[981], want[1])
    for v, eps in got:
        assert torch.equal(eps, want[v]), f't = {v}'


# ---- tiled first stage ---------------------------------------------------------------------------------------------------------------
def _vq():
    if 'vq' not in _models:
        from stable_diffusion_amd import VQModelInterfaceHIP
        _models['vq'] = _named_synthetic(VQModelInterfaceHIP(**synthetic.FACES_VQ_KWARGS)).cuda()
    return _models['vq']


def test_tiled_decode_and_encode_match_reference(golden_dir):
    """decode: latent 24 x 32 of codebook rows plus noise (every nearest code wins by at least 1 %, asserted by the golden tool), six 16 x 16
    windows decoded to 64 x 64 and folded with uf = 4 into 96 x 128; encode: 64 x 96, fifteen 32 x 32 windows, folded with df = 4"""
    z = np.load(os.path.join(golden_dir, 'superres_vq_24x32.npz'))
    ld = _ld(torch.nn.Identity(), tuple(int(v) for v in z['ks']), tuple(int(v) for v in z['stride']), first_stage_model=_vq())
    x_dec = ld.decode_first_stage(torch.from_numpy(z['z']).cuda())
    lde = _ld(torch.nn.Identity(), tuple(int(v) for v in z['enc_ks']), tuple(int(v) for v in z['enc_stride']), first_stage_model=_vq())
    img = seeded((1, 3, int(z['enc_h']), int(z['enc_w'])), int(z['enc_seed']), 0.5)
    h_enc = lde.encode_first_stage(img.cuda())
    torch.cuda.synchronize()
    assert tuple(lde.split_input_params['original_image_size']) == (int(z['enc_h']), int(z['enc_w']))
    e_d = float((x_dec.cpu() - torch.from_numpy(z['x_dec'])).abs().max())
    e_e = float((h_enc.cpu() - torch.from_numpy(z['h_enc'])).abs().max())
    print(f'[tiled vq] decode max-abs {e_d:.3e} (pin {VQ_DEC_PIN:.1e}); encode max-abs {e_e:.3e} (pin {VQ_ENC_PIN:.1e})', flush=True)
    assert tuple(x_dec.shape) == (2, 3, 96, 128) and tuple(h_enc.shape) == (1, 3, 16, 24)
    assert bool(torch.isfinite(x_dec).all()) and bool(torch.isfinite(h_enc).all())
    assert e_d <= VQ_DEC_PIN and e_e <= VQ_ENC_PIN, (e_d, e_e)


# ---- pipeline ------------------------------------------------------------------------------------------------------------------------
def _pipeline_noise(seed, steps, shape):          # (tools/make_golden_superres.py pipeline_noise)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), [torch.randn(shape, generator=g) for _ in range(steps)]


def test_superres_pipeline_matches_reference_loop(golden_dir):
    """SuperResolutionHIP at ks 16 / stride 8 on a 24 x 32 input: the tiled apply_model inside DDIM at eta 1.0 (the per-step noise handed
    out from the seeded sequence the golden tool used) against the reference DDIMSampler over the reference's tiled apply_model, at the
    fixture's bar (how far `samples` of that loop moves when every eps is off by 1e-3 on every element); the tiled decode on the golden's
    own latent at its own code indices; and upscale() end to end for shape and finiteness."""
    from stable_diffusion_amd import DDIMSamplerHIP, SuperResolutionHIP
    z = np.load(os.path.join(golden_dir, 'superres_pipeline_24x32.npz'))
    steps, b, h, w = int(z['steps']), int(z['batch']), int(z['h']), int(z['w'])
    assert float(z['perturb']) == MIXED_TOL
    _models.clear()
    torch.cuda.empty_cache()
    sr = SuperResolutionHIP(params(tuple(int(v) for v in z['ks']), tuple(int(v) for v in z['stride']), vqf=int(z['vqf'])))
    sr = sr.load_synthetic(int(z['weight_seed'])).cuda()
    lr = seeded((b, 3, h, w), int(z['cond_seed']), 0.5).clamp(-1, 1).cuda()
    assert sr.configure_tiling(h, w) is True
    x_T, noises = _pipeline_noise(int(z['noise_seed']), steps, (b, 3, h, w))
    seq = [n.cuda() for n in noises]
    smp = DDIMSamplerHIP(sr)
    smp._noise_like = lambda shape, device: seq.pop(0)
    with contextlib.redirect_stdout(io.StringIO()):
        samples, _ = smp.sample(steps, batch_size=b, shape=(3, h, w), conditioning=lr, eta=float(z['eta']), verbose=False, x_T=x_T.cuda())
    e = sr.first_stage_model.state_dict()['quantize.embedding.weight']
    zq = e[torch.from_numpy(z['idx']).long().to(e.device)].permute(0, 3, 1, 2).contiguous()
    x_up = sr.decode_first_stage(zq, force_not_quantize=True)
    with contextlib.redirect_stdout(io.StringIO()):
        up = sr.upscale(lr, steps=2)
    torch.cuda.synchronize()
    assert not seq and bool(torch.isfinite(samples).all()) and bool(torch.isfinite(x_up).all())
    e_s = float((samples.cpu() - torch.from_numpy(z['samples'])).abs().max())
    e_x = float((x_up.cpu() - torch.from_numpy(z['x_up'])).abs().max())
    bar_s = float(z['bar_samples'])
    print(f'[superres pipeline] samples max-abs {e_s:.3e} (bar {bar_s:.3e}); tiled decode of the golden latent max-abs {e_x:.3e} '
          f'(pin {VQ_DEC_PIN:.1e})', flush=True)
    assert tuple(up.shape) == (b, 3, 4 * h, 4 * w) and bool(torch.isfinite(up).all())
    assert e_s <= bar_s and e_x <= VQ_DEC_PIN, (e_s, bar_s, e_x)
