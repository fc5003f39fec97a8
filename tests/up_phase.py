"""The Upsample conv as four 2x2 phase convs, restated in torch (shared by tests/test_up_phase_host.py and tests/test_up_phase_gpu.py).

conv3x3(pad 1) of a nearest-x2 upsampled map: output pixel (2i + a, 2j + c) reads upsampled rows 2i + a + ky - 1, i.e. source rows
floor((2i + a + ky - 1) / 2) -- {i - 1, i, i} for a = 0 and {i, i, i + 1} for a = 1 (ky = 0, 1, 2); columns alike.  So each parity class
(a, c) is a 2x2 conv on the SOURCE map with taps [w0, w1 + w2] (a = 0) or [w0 + w1, w2] (a = 1) per axis and zero pad top / left = 1 - a /
1 - c, bottom / right = a / c."""
import torch
import torch.nn.functional as F


def taps(par, d):
    """3x3 tap indices that fall on tap d (0, 1) of the 2x2 window of parity class `par` (0, 1), along one axis"""
    return list(range(1 + par if d else 0, (2 if d else par) + 1))


def phase_weights_oihw(w, acc_dtype=None):
    """[N, C, 3, 3] -> [4 phases = 2 a + c, N, C, 2, 2]: the contributing taps added in (ky, kx) order in acc_dtype, returned in w's dtype
    (fp16 weights: acc_dtype = float32, one rounding to nearest-even at the end)"""
    acc = w.dtype if acc_dtype is None else acc_dtype
    N, C_ = w.shape[:2]
    out = torch.empty((4, N, C_, 2, 2), dtype=w.dtype, device=w.device)
    for a in (0, 1):
        for c in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    s = None
                    for ky in taps(a, dy):
                        for kx in taps(c, dx):
                            v = w[:, :, ky, kx].to(acc)
                            s = v if s is None else s + v
                    out[2 * a + c, :, :, dy, dx] = s.to(w.dtype)
    return out


def pack_k(w):
    """the GEMM kernels' K order of a conv weight: [N, C, KH, KW] -> [N, KH KW C], k = ((i / 64) * KH KW + ky * KW + kx) * 64 + i % 64
    (64-channel chunk major, tap fastest; C % 64 == 0)"""
    N, C_, KH, KW = w.shape
    return w.reshape(N, C_ // 64, 64, KH, KW).permute(0, 1, 3, 4, 2).reshape(N, KH * KW * C_)


def unpack_k(wp, KH, KW):
    """inverse of pack_k: [N, KH KW C] -> [N, C, KH, KW]"""
    N, K_ = wp.shape
    C_ = K_ // (KH * KW)
    return wp.reshape(N, C_ // 64, KH, KW, 64).permute(0, 1, 4, 2, 3).reshape(N, C_, KH, KW)


def derive_packed(wp, acc_dtype=None):
    """packed 3x3 weights [N, 9 C] -> the derived [4, N, 4 C] of the phase launch, working on the PACKED layout as the device kernel does:
    chunk-major both ways, the 2x2 taps numbered 2 dy + dx"""
    acc = wp.dtype if acc_dtype is None else acc_dtype
    N, K9 = wp.shape
    C_ = K9 // 9
    w9 = wp.reshape(N, C_ // 64, 9, 64)
    out = torch.empty((4, N, C_ // 64, 4, 64), dtype=wp.dtype, device=wp.device)
    for a in (0, 1):
        for c in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    s = None
                    for ky in taps(a, dy):
                        for kx in taps(c, dx):
                            v = w9[:, :, ky * 3 + kx, :].to(acc)
                            s = v if s is None else s + v
                    out[2 * a + c, :, :, 2 * dy + dx, :] = s.to(wp.dtype)
    return out.reshape(4, N, 4 * C_)


def phase_conv(x, wph):
    """x [B, C, H, W], wph [4, N, C, 2, 2] -> [B, N, 2H, 2W]: the four padded 2x2 convs, interleaved by parity"""
    B, _, H, W = x.shape
    out = torch.empty((B, wph.shape[1], 2 * H, 2 * W), dtype=x.dtype, device=x.device)
    for a in (0, 1):
        for c in (0, 1):
            out[:, :, a::2, c::2] = F.conv2d(F.pad(x, (1 - c, c, 1 - a, a)), wph[2 * a + c])
    return out


def reference_conv(x, w):
    """the op itself: conv3x3(pad 1) of the nearest-x2 upsampled map"""
    return F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
