"""The kernels the KL-f16 first stage added or widened, against fp64 in guarded buffers (tests/guard.py):

* the 3x3 output convolution for 17 .. 32 outputs (sdmi_k_conv_out32: grid.y = 3 or 4 slices of eight outputs), on the 4-pixel form
  ((4, 8): W % 4 == 0) and the one-pixel form ((3, 5)), Cin 64 (one channel pass) and 512 (both), B 1 and 2, per output within the fp32
  bound 9 Cin 2^-24 sum |w x| (+ |bias|) -- the worst case of one fp32 accumulator chain over the 9 Cin products;
* 8 and 16 outputs through the new entry and through sdmi_k_conv_out give the same bits (they still take the launches they always
  took: checked through the outputs; sdmi_k_conv_out itself keeps refusing more than 16, tests/test_rdm_gpu.py);
* the 1x1 NCHW convolution for 16 (the instantiation that always was), 17, 24 and 32 input channels, per output within
  Cin 2^-24 (|bias| + sum |w x|), with and without the input scale of decode_first_stage;
* the flash attention at d = 512 over 60 / 64 / 120 keys (below one key tile, exactly one, one and a partial one) with the probe V of
  tests/attn_probes.py: every softmax weight against fp64, the pad columns of V^T filled with NaN."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import test_attention_probes_gpu as TAP  # noqa: E402  (its _run: the probe cases of one shape, guarded, judged per element)
from stable_diffusion_amd import _lib  # noqa: E402

DEV = 'cuda'
U = 2.0 ** -24


def _g(*xs):
    return torch.Generator(device=DEV).manual_seed(sum((i + 1) * 7919 * int(x) for i, x in enumerate(xs)) % (2 ** 31))


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


def _conv_case(Cin, Cout, H, W, Bn):
    g = _g(Cin, Cout, H, W, Bn)
    h = torch.randn((Bn, H, W, Cin), generator=g, device=DEV)
    w = torch.randn((Cout, Cin, 3, 3), generator=g, device=DEV) / (9 * Cin) ** 0.5
    b = 0.1 * torch.randn((Cout,), generator=g, device=DEV)
    x64 = h.double().permute(0, 3, 1, 2)
    ref = F.conv2d(x64, w.double(), b.double(), padding=1)
    bound = 9 * Cin * U * (F.conv2d(x64.abs(), w.double().abs(), b.double().abs(), padding=1))
    return h, w, b, ref, bound


@pytest.mark.parametrize('Cin', [64, 512])
@pytest.mark.parametrize('Cout', [17, 24, 31, 32])
def test_conv_out_17_to_32_channels_vs_fp64(Cout, Cin):
    worst = 0.0
    for H, W in ((3, 5), (4, 8)):
        for Bn in (1, 2):
            h, w, b, ref, bound = _conv_case(Cin, Cout, H, W, Bn)
            rc, out = _conv_out('sdmi_k_conv_out32', h, w, b, Bn, H, W)
            _lib.check(rc)
            assert bool(torch.isfinite(out).all())
            ratio = float(((out.double() - ref).abs() / bound).max())
            print(f'[conv_out32 {Cin}->{Cout} {H}x{W} B{Bn}] max-abs {float((out.double() - ref).abs().max()):.3e}, worst err / bound {ratio:.4f}',
                  flush=True)
            worst = max(worst, ratio)
    assert worst <= 1.0, worst


@pytest.mark.parametrize('Cout', [8, 16])
def test_conv_out_up_to_16_channels_same_bits_through_both_entries(Cout):
    for Cin in (64, 512):
        for H, W in ((3, 5), (4, 8)):
            h, w, b, ref, bound = _conv_case(Cin, Cout, H, W, 2)
            rc_old, old = _conv_out('sdmi_k_conv_out', h, w, b, 2, H, W)
            rc_new, new = _conv_out('sdmi_k_conv_out32', h, w, b, 2, H, W)
            assert rc_old == 0 and rc_new == 0 and torch.equal(old, new), (Cin, Cout, H, W)
            assert float(((new.double() - ref).abs() / bound).max()) <= 1.0


def test_conv_out_33_channels_is_refused():
    h, w, b, _, _ = _conv_case(64, 33, 4, 8, 1)
    rc, out = _conv_out('sdmi_k_conv_out32', h, w, b, 1, 4, 8)
    assert rc != 0 and b'out_channels <= 32' in _lib.load().sdmi_last_error()
    assert bool(torch.isnan(out).all())          # (nothing was launched: the output keeps its poison)


@pytest.mark.parametrize('Cout', [16, 32])
@pytest.mark.parametrize('Cin', [16, 17, 24, 32])
def test_pointwise_nchw_vs_fp64(Cin, Cout):
    lib = _lib.load()
    worst = 0.0
    for HW in (60, 256, 257):
        for in_scale in (1.0, 1.0 / 0.22765929):
            g = _g(Cin, Cout, HW, int(in_scale * 1000))
            x = torch.randn((2, Cin, HW), generator=g, device=DEV)
            w = torch.randn((Cout, Cin), generator=g, device=DEV) / Cin ** 0.5
            b = 0.1 * torch.randn((Cout,), generator=g, device=DEV)
            P = guard.Pool(DEV)
            x_d, w_d, b_d = P.put('x', x), P.put('w', w), P.put('bias', b)
            out = P.new('out', (2, Cout, HW), torch.float32)
            _lib.check(lib.sdmi_k_pointwise_nchw(x_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), 2, Cin, Cout, HW, in_scale,
                                                 _lib.stream_ptr()))
            torch.cuda.synchronize()
            tag = f'pointwise {Cin}->{Cout} HW{HW} scale {in_scale:.4f}'
            P.check(tag)
            assert torch.equal(x_d, x) and torch.equal(w_d, w) and torch.equal(b_d, b), f'{tag}: an input was modified'
            s64 = float(torch.tensor(in_scale, dtype=torch.float32))       # (the scale as the kernel receives it)
            xs = x.double() * s64
            ref = torch.einsum('oc,bcp->bop', w.double(), xs) + b.double()[None, :, None]
            bound = Cin * U * (torch.einsum('oc,bcp->bop', w.double().abs(), xs.abs()) + b.double().abs()[None, :, None])
            ratio = float(((out.double() - ref).abs() / bound).max())
            print(f'[{tag}] max-abs {float((out.double() - ref).abs().max()):.3e}, worst err / bound {ratio:.4f}', flush=True)
            assert bool(torch.isfinite(out).all())
            worst = max(worst, ratio)
    assert worst <= 1.0, worst


@pytest.mark.parametrize('n', [60, 64, 120])
def test_attention_d512_probe(n, monkeypatch):
    """the AttnBlocks of KL-f16: one head of d = 512 over the n = H W tokens of a 6 x 10 / 8 x 8 / 10 x 12 latent (attn_wide.hip); the pad
    columns n .. round_up(n, 8) of V^T hold NaN (TAP._run fills them so for d > 160) and must not reach the output"""
    TAP._run('wide', 512, n, n, monkeypatch)
