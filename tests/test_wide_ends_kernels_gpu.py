"""The wide latent ends of the first stages with 32 / 64 latent channels, against fp64 in guarded buffers (tests/guard.py), inputs and
weights verified unmodified; every output judged per element against the worst-case bound of one fp32 accumulator chain (the bounds
tests/test_kl_f16_kernels_gpu.py derives):

* sdmi_k_conv_in64, 17 .. 64 input channels (the 36 KB-patch form of conv_in_kernel): 9 Cin 2^-24 sum |w x| (+ |bias|); one pixel row, a block of 16 pixels that
  is not full, more than one block; and the accumulation order depends on Cin alone -- two equal images of 15 pixels, whose pixels sit at
  different places of different blocks, give the same bits;
* sdmi_k_conv_out128, 33 .. 128 outputs (the sliced kernels with 5 .. 16 slices): 9 Cin 2^-24 sum |w x| (+ |bias|), on the one-pixel form
  ((3, 5)) and the 4-pixel form ((4, 8)), Cin 64 (one channel pass) and 512 (both);
* sdmi_k_pointwise_nchw128, 33 .. 128 input channels (pointwise_nchw_wide_kernel): Cin 2^-24 (sum |w x| + |bias|), with and without in_scale;
* at the old limits the new entries give the bits of the old ones (conv_in 4 / 16, conv_out 8 / 32, pointwise 16 / 32);
* one past the new limits each entry refuses and launches nothing (the poisoned output stays NaN);
* the flash attention at d = 512 and 256 over 6, 15, 16 and 24 keys -- the token counts of KL-f32's two lowest levels at 2 x 3 .. 4 x 4
  latents (the smallest tested before was 60) -- with the probe V of tests/attn_probes.py, the pad columns of V^T filled with NaN;
* sdmi_k_vq_quantize at the codebooks of VQ-f16 (16384 x 8), VQ-f8 (16384 x 4) and VQ-f8-n256 (256 x 4), with the inputs, the clear-gap
  rule and the tie band of tests/test_inpaint_gpu.py on 2 x 32 x 32 pixels."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import test_attention_probes_gpu as TAP  # noqa: E402  (its _run: the probe cases of one shape, guarded, judged per element)
import vq_ref  # noqa: E402
from stable_diffusion_amd import _lib  # noqa: E402

DEV = 'cuda'
U = 2.0 ** -24


def _g(*xs):
    return torch.Generator(device=DEV).manual_seed(sum((i + 1) * 7919 * int(x) for i, x in enumerate(xs)) % (2 ** 31))


# ---- conv_in ----------------------------------------------------------------------------------------------------------------------------
def _conv_in(entry, x, w, b):
    """x NCHW, w OIHW -> (rc, out NHWC) through guarded buffers"""
    Bn, Cin, H, W = x.shape
    Cout = w.shape[0]
    lib = _lib.load()
    P = guard.Pool(DEV)
    x_d, w_d, b_d = P.put('x', x), P.put('w', w), P.put('bias', b)
    out = P.new('out', (Bn, H, W, Cout), torch.float32)
    rc = getattr(lib, entry)(x_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), Bn, Cin, H, W, Cout, _lib.stream_ptr())
    torch.cuda.synchronize()
    P.check(f'{entry} {Cin}->{Cout} {H}x{W} B{Bn}')
    assert torch.equal(x_d, x) and torch.equal(w_d, w) and torch.equal(b_d, b), 'an input was modified'
    return rc, out


def _conv_in_case(Cin, Cout, H, W, Bn):
    g = _g(Cin, Cout, H, W, Bn)
    x = torch.randn((Bn, Cin, H, W), generator=g, device=DEV)
    w = torch.randn((Cout, Cin, 3, 3), generator=g, device=DEV) / (9 * Cin) ** 0.5
    b = 0.1 * torch.randn((Cout,), generator=g, device=DEV)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    bound = 9 * Cin * U * F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1).permute(0, 2, 3, 1)
    return x, w, b, ref, bound


@pytest.mark.parametrize('Cout', [256, 512])
@pytest.mark.parametrize('Cin', [17, 32, 33, 63, 64])
def test_conv_in_17_to_64_channels_vs_fp64(Cin, Cout):
    worst = 0.0
    for H, W in ((1, 2), (3, 5), (4, 8), (5, 16)):
        for Bn in (1, 2):
            x, w, b, ref, bound = _conv_in_case(Cin, Cout, H, W, Bn)
            rc, out = _conv_in('sdmi_k_conv_in64', x, w, b)
            _lib.check(rc)
            assert bool(torch.isfinite(out).all())
            ratio = float(((out.double() - ref).abs() / bound).max())
            print(f'[conv_in64 {Cin}->{Cout} {H}x{W} B{Bn}] max-abs {float((out.double() - ref).abs().max()):.3e}, worst err / bound {ratio:.4f}',
                  flush=True)
            worst = max(worst, ratio)
    assert worst <= 1.0, worst


@pytest.mark.parametrize('Cin', [17, 64])
def test_conv_in_order_depends_on_cin_alone(Cin):
    """two equal images of 3 x 5 pixels in one batch: pixel p of image 1 is pixel 15 + p of the launch, in another block and at another place
    of it; a 3 x 5 image alone (B = 1) is a third placement.  All give the same bits."""
    x, w, b, _, _ = _conv_in_case(Cin, 256, 3, 5, 1)
    rc1, one = _conv_in('sdmi_k_conv_in64', x, w, b)
    rc2, two = _conv_in('sdmi_k_conv_in64', torch.cat([x, x]).contiguous(), w, b)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(two[0], two[1]) and torch.equal(two[0], one[0])


@pytest.mark.parametrize('Cin', [4, 16])
def test_conv_in_up_to_16_channels_same_bits_through_both_entries(Cin):
    for Cout in (128, 512):
        for H, W in ((3, 5), (4, 8)):
            x, w, b, ref, bound = _conv_in_case(Cin, Cout, H, W, 2)
            rc_old, old = _conv_in('sdmi_k_conv_in', x, w, b)
            rc_new, new = _conv_in('sdmi_k_conv_in64', x, w, b)
            assert rc_old == 0 and rc_new == 0 and torch.equal(old, new), (Cin, Cout, H, W)
            assert float(((new.double() - ref).abs() / bound).max()) <= 1.0


def test_conv_in_limits_are_refused():
    x, w, b, _, _ = _conv_in_case(65, 256, 4, 8, 1)
    rc, out = _conv_in('sdmi_k_conv_in64', x, w, b)
    assert rc != 0 and b'in_channels <= 64' in _lib.load().sdmi_last_error()
    assert bool(torch.isnan(out).all())          # (nothing was launched: the output keeps its poison)
    x, w, b, _, _ = _conv_in_case(17, 256, 4, 8, 1)
    rc, out = _conv_in('sdmi_k_conv_in', x, w, b)                       # the old entry keeps its limit
    assert rc != 0 and b'in_channels <= 16' in _lib.load().sdmi_last_error()
    assert bool(torch.isnan(out).all())


# ---- conv_out ---------------------------------------------------------------------------------------------------------------------------
def _conv_out(entry, h, w, b, Bn, H, W):
    """h NHWC [Bn, H, W, Cin], w OIHW -> (rc, out NCHW) through guarded buffers; the packed weights and the inputs must come back unchanged"""
    Cout, Cin = w.shape[0], w.shape[1]
    lib = _lib.load()
    P = guard.Pool(DEV)
    h_d, w_d, b_d = P.put('h', h), P.put('w', w), P.put('bias', b)
    wp = P.new('w_ohwi', (Cout, 3, 3, Cin), torch.float32)
    _lib.check(lib.sdmi_k_pack_conv_out(w_d.data_ptr(), wp.data_ptr(), Cout, Cin, _lib.stream_ptr()))
    wp_keep = wp.clone()
    out = P.new('out', (Bn, Cout, H, W), torch.float32)
    rc = getattr(lib, entry)(h_d.data_ptr(), wp.data_ptr(), b_d.data_ptr(), out.data_ptr(), Bn, H, W, Cin, Cout, _lib.stream_ptr())
    torch.cuda.synchronize()
    P.check(f'{entry} {Cin}->{Cout} {H}x{W} B{Bn}')
    assert torch.equal(h_d, h) and torch.equal(b_d, b) and torch.equal(wp, wp_keep), 'an input was modified'
    return rc, out


def _conv_out_case(Cin, Cout, H, W, Bn):
    g = _g(Cin, Cout, H, W, Bn)
    h = torch.randn((Bn, H, W, Cin), generator=g, device=DEV)
    w = torch.randn((Cout, Cin, 3, 3), generator=g, device=DEV) / (9 * Cin) ** 0.5
    b = 0.1 * torch.randn((Cout,), generator=g, device=DEV)
    x64 = h.double().permute(0, 3, 1, 2)
    ref = F.conv2d(x64, w.double(), b.double(), padding=1)
    bound = 9 * Cin * U * (F.conv2d(x64.abs(), w.double().abs(), b.double().abs(), padding=1))
    return h, w, b, ref, bound


@pytest.mark.parametrize('Cin', [64, 512])
@pytest.mark.parametrize('Cout', [33, 64, 127, 128])
def test_conv_out_33_to_128_channels_vs_fp64(Cout, Cin):
    worst = 0.0
    for H, W in ((3, 5), (4, 8)):
        for Bn in (1, 2):
            h, w, b, ref, bound = _conv_out_case(Cin, Cout, H, W, Bn)
            rc, out = _conv_out('sdmi_k_conv_out128', h, w, b, Bn, H, W)
            _lib.check(rc)
            assert bool(torch.isfinite(out).all())
            ratio = float(((out.double() - ref).abs() / bound).max())
            print(f'[conv_out128 {Cin}->{Cout} {H}x{W} B{Bn}] max-abs {float((out.double() - ref).abs().max()):.3e}, worst err / bound {ratio:.4f}',
                  flush=True)
            worst = max(worst, ratio)
    assert worst <= 1.0, worst


@pytest.mark.parametrize('Cout', [8, 32])
def test_conv_out_up_to_32_channels_same_bits_through_both_entries(Cout):
    for Cin in (64, 512):
        for H, W in ((3, 5), (4, 8)):
            h, w, b, ref, bound = _conv_out_case(Cin, Cout, H, W, 2)
            rc_old, old = _conv_out('sdmi_k_conv_out32', h, w, b, 2, H, W)
            rc_new, new = _conv_out('sdmi_k_conv_out128', h, w, b, 2, H, W)
            assert rc_old == 0 and rc_new == 0 and torch.equal(old, new), (Cin, Cout, H, W)
            assert float(((new.double() - ref).abs() / bound).max()) <= 1.0


def test_conv_out_129_channels_is_refused():
    h, w, b, _, _ = _conv_out_case(64, 129, 4, 8, 1)
    rc, out = _conv_out('sdmi_k_conv_out128', h, w, b, 1, 4, 8)
    assert rc != 0 and b'out_channels <= 128' in _lib.load().sdmi_last_error()
    assert bool(torch.isnan(out).all())          # (nothing was launched: the output keeps its poison)


# ---- pointwise --------------------------------------------------------------------------------------------------------------------------
def _pointwise(entry, x, w, b, in_scale):
    Bn, Cin, HW = x.shape
    Cout = w.shape[0]
    lib = _lib.load()
    P = guard.Pool(DEV)
    x_d, w_d, b_d = P.put('x', x), P.put('w', w), P.put('bias', b)
    out = P.new('out', (Bn, Cout, HW), torch.float32)
    rc = getattr(lib, entry)(x_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), Bn, Cin, Cout, HW, in_scale, _lib.stream_ptr())
    torch.cuda.synchronize()
    tag = f'{entry} {Cin}->{Cout} HW{HW} scale {in_scale:.4f}'
    P.check(tag)
    assert torch.equal(x_d, x) and torch.equal(w_d, w) and torch.equal(b_d, b), f'{tag}: an input was modified'
    return rc, out


def _pointwise_case(Cin, Cout, HW, in_scale):
    g = _g(Cin, Cout, HW, int(in_scale * 1000))
    x = torch.randn((2, Cin, HW), generator=g, device=DEV)
    w = torch.randn((Cout, Cin), generator=g, device=DEV) / Cin ** 0.5
    b = 0.1 * torch.randn((Cout,), generator=g, device=DEV)
    s64 = float(torch.tensor(in_scale, dtype=torch.float32))       # (the scale as the kernel receives it)
    xs = x.double() * s64
    ref = torch.einsum('oc,bcp->bop', w.double(), xs) + b.double()[None, :, None]
    bound = Cin * U * (torch.einsum('oc,bcp->bop', w.double().abs(), xs.abs()) + b.double().abs()[None, :, None])
    return x, w, b, ref, bound


@pytest.mark.parametrize('Cout', [64, 128])
@pytest.mark.parametrize('Cin', [33, 64, 65, 128])
def test_pointwise_33_to_128_channels_vs_fp64(Cin, Cout):
    worst = 0.0
    for HW in (15, 256, 257):
        for in_scale in (1.0, 1.0 / 0.22765929):
            x, w, b, ref, bound = _pointwise_case(Cin, Cout, HW, in_scale)
            rc, out = _pointwise('sdmi_k_pointwise_nchw128', x, w, b, in_scale)
            _lib.check(rc)
            assert bool(torch.isfinite(out).all())
            ratio = float(((out.double() - ref).abs() / bound).max())
            print(f'[pointwise128 {Cin}->{Cout} HW{HW} scale {in_scale:.4f}] max-abs {float((out.double() - ref).abs().max()):.3e}, '
                  f'worst err / bound {ratio:.4f}', flush=True)
            worst = max(worst, ratio)
    assert worst <= 1.0, worst


@pytest.mark.parametrize('Cin', [16, 32])
def test_pointwise_up_to_32_channels_same_bits_through_both_entries(Cin):
    for Cout in (16, 64):
        for HW in (15, 257):
            for in_scale in (1.0, 1.0 / 0.22765929):
                x, w, b, ref, bound = _pointwise_case(Cin, Cout, HW, in_scale)
                rc_old, old = _pointwise('sdmi_k_pointwise_nchw', x, w, b, in_scale)
                rc_new, new = _pointwise('sdmi_k_pointwise_nchw128', x, w, b, in_scale)
                assert rc_old == 0 and rc_new == 0 and torch.equal(old, new), (Cin, Cout, HW, in_scale)
                assert float(((new.double() - ref).abs() / bound).max()) <= 1.0


def test_pointwise_limits_are_refused():
    x, w, b, _, _ = _pointwise_case(129, 64, 256, 1.0)
    rc, out = _pointwise('sdmi_k_pointwise_nchw128', x, w, b, 1.0)
    assert rc != 0 and b'Cin <= 128' in _lib.load().sdmi_last_error()
    assert bool(torch.isnan(out).all())          # (nothing was launched: the output keeps its poison)
    x, w, b, _, _ = _pointwise_case(33, 64, 256, 1.0)
    rc, out = _pointwise('sdmi_k_pointwise_nchw', x, w, b, 1.0)          # the old entry keeps its limit
    assert rc != 0 and b'Cin <= 32' in _lib.load().sdmi_last_error()
    assert bool(torch.isnan(out).all())


# ---- attention at the token counts of KL-f32's lowest levels ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [6, 15, 16, 24])
@pytest.mark.parametrize('d', [512, 256])
def test_attention_probe_few_keys(d, n, monkeypatch):
    """one head of d = 512 (ch 128) / 256 (the thin stand-ins) over the n = H W tokens of the 8 x 8 and 16 x 16 levels of KL-f32 at 2 x 3,
    3 x 5 and 4 x 4 latents (attn_wide.hip): far below one key tile; the pad columns n .. round_up(n, 8) of V^T hold NaN (TAP._run fills
    them so for d > 160) and must not reach the output"""
    TAP._run('wide', d, n, n, monkeypatch)


# ---- the codebooks of VQ-f16, VQ-f8 and VQ-f8-n256 -------------------------------------------------------------------------------------------
def _quantize_gpu(z, e):
    lib = _lib.load()
    zc, ec = z.cuda().contiguous(), e.cuda().contiguous()
    zq = torch.empty_like(zc)
    idx = torch.empty(z.shape[0], z.shape[2], z.shape[3], dtype=torch.int32, device='cuda')
    norms = torch.empty(e.shape[0], device='cuda')
    _lib.check(lib.sdmi_k_vq_quantize(zc.data_ptr(), 1.0, ec.data_ptr(), norms.data_ptr(), e.shape[0], e.shape[1], zq.data_ptr(),
                                      idx.data_ptr(), z.shape[0], z.shape[2] * z.shape[3], _lib.stream_ptr()))
    torch.cuda.synchronize()
    return zq.cpu(), idx.long().cpu()


@pytest.mark.parametrize('kind', ['gaussian', 'near_codes', 'ties'])
@pytest.mark.parametrize('n_embed,D', [(16384, 8), (16384, 4), (256, 4)])
def test_quantizer_at_the_zoo_codebooks(kind, n_embed, D):
    """tests/test_inpaint_gpu.py test_quantizer_vs_restatement at the codebook shapes of VQ-f16 / VQ-f8 / VQ-f8-n256 (D = 8 had no test)"""
    g = torch.Generator().manual_seed(n_embed + D)
    e = torch.randn(n_embed, D, generator=g)
    B, H, W = 2, 32, 32
    if kind == 'gaussian':
        z = torch.randn(B, D, H, W, generator=g)
    else:
        pick = torch.randint(0, n_embed, (B, H, W), generator=g)
        z = e[pick].permute(0, 3, 1, 2).contiguous()
        if kind == 'near_codes':
            z = z + 1e-3 * torch.randn(z.shape, generator=g)
        else:
            e = torch.cat([e, e[: n_embed // 2]])       # duplicated rows: exact ties, the first index must win
    zq, idx = _quantize_gpu(z, e)
    _, ref_idx = vq_ref.quantize(z, e)
    d = vq_ref.distances(z, e).double()
    best = d.gather(1, ref_idx.view(-1, 1)).squeeze(1)
    second = d.scatter(1, ref_idx.view(-1, 1), float('inf')).min(1).values
    clear = (second - best) > 1e-5 * best.abs().clamp_min(1e-30)
    mine = idx.view(-1)
    assert torch.equal(mine[clear], ref_idx.view(-1)[clear]), int((mine[clear] != ref_idx.view(-1)[clear]).sum())
    # elsewhere: any (near-)tied code is accepted -- its distance is within the tie band of the best one
    db = d.gather(1, mine.view(-1, 1)).squeeze(1)
    assert bool(((db - best) <= 1e-5 * best.abs().clamp_min(1e-30) + 1e-6).all())
    if kind == 'ties':
        assert bool((mine < n_embed).all())          # the first of two equal rows
    assert torch.equal(zq, vq_ref.straight_through(z, e, idx))
    print(f'[quantize {kind} n={n_embed} D={D}] clear-gap pixels {int(clear.sum())} / {clear.numel()}', flush=True)
