"""fp64 numpy restatements for the CLIP vision tower's tests (test_vit_host.py, test_vit_gpu.py): the safety checker's concept head, the
image embedder's bicubic preprocess, the patch unfold.  Written from the contract in include/sdmi.h, not from the kernels."""
import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def round3(x):
    """three decimals, half to even (numpy's round: rint(x * 1000) / 1000)"""
    return np.rint(np.asarray(x, dtype=np.float64) * 1000.0) / 1000.0


def cosines(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    an = a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)
    bn = b / np.maximum(np.linalg.norm(b, axis=1, keepdims=True), 1e-12)
    return an @ bn.T


def safety_head(image_embeds, concept_embeds, special_care_embeds, concept_thr, special_thr):
    """-> has_nsfw bool [B], rounded concept scores [B, Nc], rounded special-care scores [B, Ns], and the scores BEFORE rounding (for the
    tests' distance-to-a-rounding-boundary conditions)"""
    B, Nc, Ns = len(image_embeds), len(concept_embeds), len(special_care_embeds)
    cc = cosines(image_embeds, concept_embeds)
    sc = cosines(image_embeds, special_care_embeds) if Ns else np.zeros((B, 0))
    has = np.zeros(B, dtype=bool)
    cs, ss = np.zeros((B, Nc)), np.zeros((B, Ns))
    raw_c, raw_s = np.zeros((B, Nc)), np.zeros((B, Ns))
    for b in range(B):
        adjustment = 0.0
        for j in range(Ns):
            raw_s[b, j] = sc[b, j] - float(special_thr[j]) + adjustment
            ss[b, j] = round3(raw_s[b, j])
            if ss[b, j] > 0:
                adjustment = 0.01
        for j in range(Nc):
            raw_c[b, j] = cc[b, j] - float(concept_thr[j]) + adjustment
            cs[b, j] = round3(raw_c[b, j])
            if cs[b, j] > 0:
                has[b] = True
    return has, cs, ss, raw_c, raw_s


def boundary_distance(raw):
    """distance of every un-rounded score to the nearest rounding boundary (an odd multiple of 0.0005)"""
    t = np.asarray(raw, dtype=np.float64) * 1000.0
    return np.abs(t - np.floor(t) - 0.5) / 1000.0


def _cubic(t, A=-0.75):
    def c1(x):
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def c2(x):
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return np.stack([c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)], -1)


def bicubic_align_corners(x, S):
    """[B, C, H, W] -> [B, C, S, S], fp64: cubic convolution (A = -0.75), align_corners=True, border indices clamped, no antialiasing"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]

    def taps(n_in):
        src = np.arange(S, dtype=np.float64) * ((n_in - 1) / (S - 1) if S > 1 else 0.0)
        i0 = np.floor(src)
        idx = np.clip(i0[:, None].astype(np.int64) + np.arange(-1, 3)[None], 0, n_in - 1)
        return idx, _cubic(src - i0)
    iy, wy = taps(H)
    ix, wx = taps(W)
    rows = (x[:, :, iy, :] * wy[None, None, :, :, None]).sum(3)              # [B, C, S, W]
    return (rows[:, :, :, ix] * wx[None, None, None]).sum(4)


def preprocess(x, S):
    """FrozenClipImageEmbedder.preprocess in fp64"""
    y = (bicubic_align_corners(x, S) + 1.0) / 2.0
    mean, std = np.asarray(CLIP_MEAN)[None, :, None, None], np.asarray(CLIP_STD)[None, :, None, None]
    return (y - mean) / std


def patchify(px, p, Kp):
    """[B, 3, S, S] fp32 -> fp16 [B P^2, Kp]: column (c, ky, kx) of patch (py, px), pad columns zero"""
    B, Cc, S, _ = px.shape
    P = S // p
    cols = px.reshape(B, Cc, P, p, P, p).transpose(0, 2, 4, 1, 3, 5).reshape(B * P * P, Cc * p * p)
    out = np.zeros((B * P * P, Kp), dtype=np.float16)
    out[:, :Cc * p * p] = cols.astype(np.float16)
    return out
