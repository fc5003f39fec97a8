"""The Upsample conv (nearest x2, then conv3x3 pad 1) as four 2x2 phase convs (igemm KIND_2X2): the phase identity and the
weight derivation restated in torch (tests/up_phase.py), in fp64 against interpolate + conv2d, and the derived weights' K order against the
pack kernel's.  No GPU."""
import math

import pytest
import torch

import up_phase as P  # noqa: E402  (tests/ is on sys.path via conftest's rootdir insertion)


def _g(seed):
    return torch.Generator().manual_seed(seed)


# (2, 5, 7, 3, 5): the shape the identity was first checked at; 1 x 1 and one-row / one-column maps are all border
@pytest.mark.parametrize('B,C,N,H,W', [(2, 5, 7, 3, 5), (1, 3, 2, 1, 1), (2, 4, 3, 1, 6), (1, 2, 5, 4, 1), (2, 64, 8, 2, 3)])
def test_phase_identity_fp64(B, C, N, H, W):
    """the four padded 2x2 convs with summed taps, interleaved by parity, ARE conv3x3(interpolate(x, 2, 'nearest')): 1e-12 in fp64"""
    g = _g(100 * C + 10 * H + W)
    x = torch.randn((B, C, H, W), generator=g, dtype=torch.float64)
    w = torch.randn((N, C, 3, 3), generator=g, dtype=torch.float64) / math.sqrt(9 * C)
    got = P.phase_conv(x, P.phase_weights_oihw(w))
    ref = P.reference_conv(x, w)
    assert got.shape == ref.shape == (B, N, 2 * H, 2 * W)
    d = float((got - ref).abs().max())
    print(f'[up phase identity B{B} C{C} N{N} {H}x{W}] max |phase form - interpolate + conv2d| = {d:.2e}')
    assert d <= 1e-12


def test_taps_cover_the_window_once_per_parity():
    """per axis and parity the two 2x2 taps partition the three 3x3 taps: [w0, w1 + w2] for parity 0, [w0 + w1, w2] for parity 1"""
    assert [P.taps(0, 0), P.taps(0, 1)] == [[0], [1, 2]]
    assert [P.taps(1, 0), P.taps(1, 1)] == [[0, 1], [2]]


@pytest.mark.parametrize('C', [64, 128, 320])
def test_derived_weights_keep_the_kernel_k_order(C):
    """deriving on the packed layout = packing the derived OIHW weights: 64-channel chunk major, the four taps (2 dy + dx) of a chunk adjacent --
    the 3x3 pack order of tests/kernels.py's pack_conv_weight (k = ((i / 64) * 9 + 3 ky + kx) * 64 + i % 64) with a 2x2 window"""
    N = 6
    g = _g(C)
    w = torch.randn((N, C, 3, 3), generator=g, dtype=torch.float64)
    wp = P.pack_k(w)
    # the 3x3 pack order, element by element
    for (n, i, ky, kx) in [(0, 0, 0, 0), (1, 63, 2, 1), (2, C - 1, 1, 2), (5, 64 % C, 0, 1), (3, C // 2 + 5, 2, 2)]:
        assert wp[n, ((i // 64) * 9 + 3 * ky + kx) * 64 + i % 64] == w[n, i, ky, kx]
    assert torch.equal(P.unpack_k(wp, 3, 3), w)
    got = P.derive_packed(wp)
    want = P.phase_weights_oihw(w)
    assert got.shape == (4, N, 4 * C)
    for ph in range(4):
        assert torch.equal(got[ph], P.pack_k(want[ph]))
        for (n, i, dy, dx) in [(0, 0, 0, 0), (4, C - 1, 1, 1), (2, C // 2 + 1, 0, 1), (1, 63, 1, 0)]:
            assert got[ph, n, ((i // 64) * 4 + 2 * dy + dx) * 64 + i % 64] == want[ph, n, i, dy, dx]


def test_fp16_derivation_rounds_once():
    """fp16 weights: the taps are added in fp32 and the sum is rounded once, to nearest-even -- never fp16 additions.  The sum of up to four fp16
    values is not always an fp32 number, so the order of the additions is part of the definition: (ky, kx) ascending"""
    g = _g(7)
    w = (torch.randn((8, 64, 3, 3), generator=g) / 24.0).half()
    w.view(-1)[::5] *= 2.0 ** -9                # wide exponent spread inside a sum
    got = P.phase_weights_oihw(w, torch.float32)
    exact = P.phase_weights_oihw(w.double())
    # within half an fp16 ulp (<= |v| 2^-11, subnormal spacing 2^-24) of the fp32 sum, which is within 3 fp32 roundings of the exact one
    mag = P.phase_weights_oihw(w.double().abs())
    half_ulp = torch.maximum(exact.abs() * 2.0 ** -11, torch.tensor(2.0 ** -25, dtype=torch.float64))
    assert bool(((got.double() - exact).abs() <= half_ulp + 4 * 2.0 ** -24 * mag).all())
    naive = P.phase_weights_oihw(w)            # fp16 additions: a rounding per addition
    assert not torch.equal(naive, got)
    assert torch.equal(P.derive_packed(P.pack_k(w), torch.float32), torch.stack([P.pack_k(got[ph]) for ph in range(4)]))


def test_committed_phase_table_is_well_formed_and_loaded():
    """stable-diffusion_amd/tune_up_phase_gfx950.txt (the rows of the phase kind, key ksize 2, beside the main table): unsplit launches on generic
    tiles, K = 4 Cin of whole 64-channel chunks, unique keys -- and the library's tuner finds them"""
    import ctypes as C
    import os
    from stable_diffusion_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [ln.split() for ln in open(os.path.join(root, 'stable-diffusion_amd', 'tune_up_phase_gfx950.txt')) if ln.strip() and not ln.startswith('#')]
    assert len(rows) >= 6
    seen = set()
    lib = _lib.load()
    for r in rows:
        assert len(r) == 11, r
        M, N, K, ksize, stride, up, mode, req, tile, splitk = (int(v) for v in r[:10])
        assert M > 0 and N > 0 and K > 0 and K % 256 == 0 and (ksize, stride, up, mode, req, splitk) == (2, 1, 1, 0, 0, 1) and float(r[10]) > 0, r
        assert 0 <= tile < 22 and not 14 <= tile <= 17, r
        assert tuple(r[:8]) not in seen
        seen.add(tuple(r[:8]))
        t, s = C.c_int(-1), C.c_int(-1)
        assert lib.sdmi_tune_lookup(M, N, K, 2, 1, 1, 0, 0, 0, C.byref(t), C.byref(s)) == 0 and (t.value, s.value) == (tile, 1)
    main = open(os.path.join(root, 'stable-diffusion_amd', 'tune_gfx950.txt')).read().splitlines()
    assert not any(ln.split()[3] == '2' for ln in main if ln and not ln.startswith('#'))


def test_entry_points_are_declared():
    from stable_diffusion_amd import _lib
    assert 'sdmi_k_igemm_up_phase' in _lib.exported_symbols() and 'sdmi_k_up_phase_weights' in _lib.exported_symbols()
