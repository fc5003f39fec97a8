"""The two entry points of csrc/rescale.hip (SpatialRescaler: bilinear halvings and the 1x1 channel map) in guarded buffers (tests/guard.py):

* sdmi_k_spatial_rescale against fp64 of the whole expression, per element within (Cin + 1 + 3 n) 2^-24 (|bias| + sum_c |w| pool(|x|)) -- the
  worst case of any summation order: gamma_3 per stage (three additions and an exact scaling), Cin products and Cin additions of the
  map and the bias -- and (3 n + 1) 2^-24 pool(|x|) without the channel map; on the 16-byte path, the element path (odd sizes; the same
  input one float off alignment), every n, and Cin one below / at / one above the kernel's channel boundaries: the chunk of 8 channels
  per wave (7 8 9, 15 16 17), the wrap of the 8 waves (63 64 65, 71 72 73) and the 4 channels in flight (3 4 5);
* an odd last row / column is never read (NaN there, finite output); a one-hot map through the no-map mode is count / 4^n exactly; two
  runs give equal bits; the aligned and the misaligned path give equal bits;
* sdmi_k_spatial_rescale_labels is bit-equal to sdmi_k_spatial_rescale(one_hot(labels)) on every mapped case, on a map that uses 3 of the
  182 classes and on a map of one class;
* every refusal returns -1 with the guarded output untouched;
* a 9.2 GB input whose last sample straddles element 2^31 (64-bit offsets)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
from stable_diffusion_amd import _lib  # noqa: E402

DEV = 'cuda'
U = 2.0 ** -24
# (Cin, Cout or None, n, B, H, W, bias)
CASES = [(182, 3, 2, 2, 16, 24, False),      # 16-byte path
         (182, 3, 2, 1, 13, 19, True),       # odd: element path, last row / column dropped
         (5, 8, 1, 2, 6, 10, True),
         (3, 3, 0, 1, 4, 4, True),
         (7, None, 2, 1, 12, 20, False),     # no map
         (1, 1, 2, 1, 4, 4, False)]          # smallest
BOUNDARY_CIN = [3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 71, 72, 73]
MAPPED = [c for c in CASES if c[1] is not None] + [(c, 3, 2, 1, 8, 12, True) for c in BOUNDARY_CIN] + [(9, 2, 1, 1, 5, 7, False)]


def _g(*xs):
    return torch.Generator(device=DEV).manual_seed(sum((i + 1) * 7919 * int(x) for i, x in enumerate(xs)) % (2 ** 31))


def _weights(Cin, Cout, bias, g):
    if Cout is None:
        return None, None
    w = torch.randn((Cout, Cin), generator=g, device=DEV) / Cin ** 0.5
    return w, (0.1 * torch.randn((Cout,), generator=g, device=DEV) if bias else None)


def _onehot(labels, Cin):
    return F.one_hot(labels.long(), Cin).permute(0, 3, 1, 2).float().contiguous()


def _run(inp, w, b, n, Cin, Cout, labels=False, offset=0, args=None, null=()):
    """inp: x fp32 [B, Cin, H, W] or labels int32 [B, H, W] -> (rc, out); `offset` floats of misalignment; `args` overrides (B, Cin, H, W, n,
    Cout) and `null` names pointers passed as NULL (refusals).  Guards are checked and the inputs must come back unchanged."""
    lib = _lib.load()
    P = guard.Pool(DEV)
    flat = P.new('in', (inp.numel() + offset,), inp.dtype)
    i_d = flat[offset:].view(inp.shape)
    i_d.copy_(inp)
    w_d = None if w is None else P.put('w', w)
    b_d = None if b is None else P.put('bias', b)
    B, H, W = inp.shape[0], inp.shape[-2], inp.shape[-1]
    out = P.new('out', (B, Cout if w is not None else Cin, H >> n if 0 <= n <= 2 else 1, W >> n if 0 <= n <= 2 else 1), torch.float32)
    a = list(args or (B, Cin, H, W, n, Cout or 0))
    ptrs = {'in': i_d.data_ptr(), 'w': _lib.ptr(w_d), 'bias': _lib.ptr(b_d), 'out': out.data_ptr()}
    for k in null:
        ptrs[k] = None
    fn = lib.sdmi_k_spatial_rescale_labels if labels else lib.sdmi_k_spatial_rescale
    rc = fn(ptrs['in'], ptrs['w'], ptrs['bias'], ptrs['out'], *a, _lib.stream_ptr())
    torch.cuda.synchronize()
    P.check(f'rescale Cin {Cin} Cout {Cout} n {n} {tuple(inp.shape)} labels={labels} offset={offset}')
    same_in = torch.equal(i_d.view(torch.int32), inp.contiguous().view(torch.int32))        # (as bits: the odd-row test puts NaN into it)
    assert same_in and (w is None or torch.equal(w_d, w)) and (b is None or torch.equal(b_d, b)), 'an input was modified'
    return rc, out


def _pool64(x, n):
    for _ in range(n):
        x = F.avg_pool2d(x, 2)           # (floor mode: an odd last row / column is dropped, as the definition has it)
    return x


def _ref_and_bound(x, w, b, n):
    Cin = x.shape[1]
    p, pa = _pool64(x.double(), n), _pool64(x.double().abs(), n)
    if w is None:
        return p, (3 * n + 1) * U * pa
    ref = torch.einsum('oc,bchw->bohw', w.double(), p)
    mag = torch.einsum('oc,bchw->bohw', w.double().abs(), pa)
    if b is not None:
        ref, mag = ref + b.double().view(1, -1, 1, 1), mag + b.double().abs().view(1, -1, 1, 1)
    return ref, (Cin + 1 + 3 * n) * U * mag


def _inputs(Cin, B, H, W, g):
    """3 * randn, and a one-hot map from a seeded randint"""
    x = 3.0 * torch.randn((B, Cin, H, W), generator=g, device=DEV)
    lab = torch.randint(0, Cin, (B, H, W), generator=g, device=DEV, dtype=torch.int32)
    return x, lab


def _judge(tag, out, ref, bound):
    assert out.shape == ref.shape and bool(torch.isfinite(out).all()), tag
    err = (out.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
    print(f'[{tag}] max-abs {float(err.max()):.3e}, worst err / bound {ratio:.4f}', flush=True)
    return ratio


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'Cin{}_Cout{}_n{}_B{}_{}x{}_bias{}'.format(*c))
def test_rescale_vs_fp64(case):
    Cin, Cout, n, B, H, W, bias = case
    g = _g(*[int(v or 0) for v in case])
    w, b = _weights(Cin, Cout, bias, g)
    x, lab = _inputs(Cin, B, H, W, g)
    worst = 0.0
    for kind, inp in (('randn', x), ('onehot', _onehot(lab, Cin))):
        rc, out = _run(inp, w, b, n, Cin, Cout)
        _lib.check(rc)
        ref, bound = _ref_and_bound(inp, w, b, n)
        worst = max(worst, _judge(f'rescale {case} {kind}', out, ref, bound))
        rc2, again = _run(inp, w, b, n, Cin, Cout)
        assert rc2 == 0 and torch.equal(out, again), 'two runs differ'
    assert worst <= 1.0, worst


@pytest.mark.parametrize('Cin', BOUNDARY_CIN)
def test_rescale_channel_boundaries_vs_fp64(Cin):
    """one below, at and one above: the 4 channels in flight, the chunk of 8 per wave, the wrap of the 8 waves at 64, the second chunk of a wave"""
    worst = 0.0
    for n, H, W in ((2, 8, 12), (1, 5, 7), (0, 3, 5)):
        g = _g(Cin, n, H, W)
        w, b = _weights(Cin, 3, True, g)
        x, _ = _inputs(Cin, 2, H, W, g)
        rc, out = _run(x, w, b, n, Cin, 3)
        _lib.check(rc)
        ref, bound = _ref_and_bound(x, w, b, n)
        worst = max(worst, _judge(f'rescale boundary Cin {Cin} n {n} {H}x{W}', out, ref, bound))
    assert worst <= 1.0, worst


def test_rescale_misaligned_pointer_takes_the_element_path():
    Cin, Cout, n, B, H, W, bias = CASES[0]
    g = _g(Cin, 1)
    w, b = _weights(Cin, Cout, bias, g)
    x, _ = _inputs(Cin, B, H, W, g)
    rc0, aligned = _run(x, w, b, n, Cin, Cout)
    rc1, off = _run(x, w, b, n, Cin, Cout, offset=1)
    assert rc0 == 0 and rc1 == 0
    ref, bound = _ref_and_bound(x, w, b, n)
    assert _judge('rescale 182->3 16x24 one float off alignment', off, ref, bound) <= 1.0
    assert torch.equal(aligned, off), 'the 16-byte path and the element path give different bits'
    for nn_, (h, ww) in ((1, (6, 10)), (2, (12, 20))):          # (the same for the 8-byte path and for the no-map kernel)
        x2 = 3.0 * torch.randn((2, 7, h, ww), generator=g, device=DEV)
        for wt, bs, co in ((None, None, None), _weights(7, 2, True, g) + (2,)):
            ra, a = _run(x2, wt, bs, nn_, 7, co)
            rb, o = _run(x2, wt, bs, nn_, 7, co, offset=1)
            assert ra == 0 and rb == 0 and torch.equal(a, o), (nn_, co)


def test_rescale_never_reads_the_odd_last_row_and_column():
    Cin, Cout, n, B, H, W, bias = CASES[1]
    g = _g(13, 19)
    w, b = _weights(Cin, Cout, bias, g)
    x, _ = _inputs(Cin, B, H, W, g)
    rc, clean = _run(x, w, b, n, Cin, Cout)
    x[:, :, H - 1, :] = float('nan')
    x[:, :, :, W - 1] = float('nan')
    rc2, out = _run(x, w, b, n, Cin, Cout)
    rc3, pooled = _run(x, None, None, n, Cin, None)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(pooled).all()) and torch.equal(out, clean)


@pytest.mark.parametrize('n', [0, 1, 2])
def test_rescale_one_hot_without_map_is_count_over_4_to_the_n(n):
    Cin, B, H, W = 7, 2, 12, 20
    lab = torch.randint(0, Cin, (B, H, W), generator=_g(n, 77), device=DEV, dtype=torch.int32)
    oh = _onehot(lab, Cin)
    rc, out = _run(oh, None, None, n, Cin, None)
    assert rc == 0
    s = 1 << n
    count = oh.view(B, Cin, H // s, s, W // s, s).sum(dim=(3, 5))
    assert torch.equal(out, count / float(s * s))


@pytest.mark.parametrize('case', MAPPED, ids=lambda c: 'Cin{}_Cout{}_n{}_B{}_{}x{}_bias{}'.format(*c))
def test_labels_entry_is_bit_equal_to_the_one_hot_entry(case):
    Cin, Cout, n, B, H, W, bias = case
    g = _g(*[int(v) for v in case], 5)
    w, b = _weights(Cin, Cout, bias, g)
    maps = [torch.randint(0, Cin, (B, H, W), generator=g, device=DEV, dtype=torch.int32),
            torch.full((B, H, W), Cin - 1, device=DEV, dtype=torch.int32)]                                    # one class
    if Cin >= 3:
        few = torch.tensor([0, Cin // 2, Cin - 1], device=DEV, dtype=torch.int32)                             # 3 of the Cin classes
        maps.append(few[torch.randint(0, 3, (B, H, W), generator=g, device=DEV)])
    for lab in maps:
        for offset in (0, 1):
            rc_l, from_labels = _run(lab, w, b, n, Cin, Cout, labels=True, offset=offset)
            rc_x, from_onehot = _run(_onehot(lab, Cin), w, b, n, Cin, Cout)
            assert rc_l == 0 and rc_x == 0
            assert bool(torch.isfinite(from_labels).all()) and torch.equal(from_labels, from_onehot), (case, offset)


def test_refusals_launch_nothing():
    Cin, Cout, n, B, H, W = 5, 3, 2, 1, 8, 8
    g = _g(99)
    w, b = _weights(Cin, Cout, True, g)
    x, lab = _inputs(Cin, B, H, W, g)
    w9 = torch.randn((9, Cin), generator=g, device=DEV)
    bad = [('n_stages 3', dict(args=(B, Cin, H, W, 3, Cout))), ('n_stages -1', dict(args=(B, Cin, H, W, -1, Cout))),
           ('Cout 0', dict(args=(B, Cin, H, W, n, 0))), ('Cout 9', dict(args=(B, Cin, H, W, n, 9), w=w9, b=None)),
           ('Cin 0', dict(args=(B, 0, H, W, n, Cout))), ('H below 2^n', dict(args=(B, Cin, 3, W, n, Cout))),
           ('W below 2^n', dict(args=(B, Cin, H, 3, n, Cout))), ('null input', dict(null=('in',))), ('null out', dict(null=('out',))),
           ('bias without w', dict(null=('w',)))]
    lib = _lib.load()
    for labels, inp in ((False, x), (True, lab)):
        for name, kw in bad:
            rc, out = _run(inp, kw.get('w', w), kw.get('b', b), n, Cin, Cout, labels=labels, args=kw.get('args'), null=kw.get('null', ()))
            assert rc == -1 and lib.sdmi_last_error(), (name, labels)
            assert bool(torch.isnan(out).all()), f'{name}: the output was written'         # (nothing was launched: it keeps its poison)


def test_offsets_past_2_to_the_31_elements():
    """[3, 182, 2048, 2048] is 2.29 G floats: the third sample straddles element 2^31.  The summation tree does not depend on B, so the
    last sample of the batched call equals a call on that sample alone bit for bit (map and no-map kernels); 64-bit offsets or not at all."""
    lib = _lib.load()
    B, Cin, H, W, n, Cout = 3, 182, 2048, 2048, 2, 3
    assert B * Cin * H * W > 2 ** 31 and (B - 1) * Cin * H * W < 2 ** 31
    g = _g(2048)
    w, b = _weights(Cin, Cout, True, g)
    x = torch.zeros((B, Cin, H, W), device=DEV)
    x[B - 1].normal_(generator=g)
    x[B - 1, :, H - 4:, W - 4:] = 7.0                     # (the very last block of the buffer is marked)
    last = x[B - 1:].clone()
    for wt, bs, co in ((w, b, Cout), (None, None, Cin)):
        P = guard.Pool(DEV)
        out = P.new('out', (B, co, H >> n, W >> n), torch.float32)
        alone = P.new('alone', (1, co, H >> n, W >> n), torch.float32)
        _lib.check(lib.sdmi_k_spatial_rescale(x.data_ptr(), _lib.ptr(wt), _lib.ptr(bs), out.data_ptr(), B, Cin, H, W, n, Cout if wt is not None else 0,
                                              _lib.stream_ptr()))
        _lib.check(lib.sdmi_k_spatial_rescale(last.data_ptr(), _lib.ptr(wt), _lib.ptr(bs), alone.data_ptr(), 1, Cin, H, W, n,
                                              Cout if wt is not None else 0, _lib.stream_ptr()))
        torch.cuda.synchronize()
        P.check(f'rescale past 2^31, Cout {co}')
        assert bool(torch.isfinite(out).all()) and torch.equal(out[B - 1:], alone)
        if wt is None:
            assert bool((out[:B - 1] == 0).all()) and bool((out[B - 1, :, -1, -1] == 7.0).all())
        else:
            assert torch.equal(out[0], (bs if bs is not None else torch.zeros(co, device=DEV)).view(-1, 1, 1).expand_as(out[0]))
    del x, last
    torch.cuda.empty_cache()
