"""Probe inputs for the attention kernels: softmax weights read back through an indicator V, held per element against fp64.

Attention is linear in V.  With V an indicator matrix (entries 0 or 1) an output element is the sum of the softmax weights of the keys coded
into its column, so a kernel's weights themselves can be held to a RELATIVE bar -- which random V and a max-abs bar cannot do: there the
output is an average of nkv values and a proportional error of a few per cent disappears under the bar.

Score regimes (`REGIMES`): q, k ~ N(0, 1) from a seeded generator (fp16-rounded for the mixed kernels, fp32 for the split-fp16 ones), another
draw for every (batch, head) pair; then dimension 0 is overwritten with fp16-exact values q[..., 0] = 8, k[:, j, 0] = fp16(b_j sqrt(d) / 8),
which shifts key j's score by b_j natural units at scale = d^-1/2.
V codings (`codings`): which column of V key j sets, rotated by the (batch, head) index.
Reference (`softmax_ref` / `coded`): fp64 softmax of the operands as the kernel receives them, summed per column.
Tolerance (`tolerance`), liveness (`live`), the comparison (`judge`), the list of GPU cases (`gpu_cases`) that the host suite checks for
liveness before a GPU sees them, and a plain-torch restatement of the kernels' loop with switchable defects (`emulate`).

torch only; importing this needs no GPU."""
import math

import torch

REGIMES = ('diffuse', 'negative', 'rising', 'falling', 'first_half', 'second_half')
R_MIXED = 2.0 ** -9      # three fp16 roundings of 2^-11 on a weight (P, the denominator summed from the rounded P, the stored output) + one spare
R_SPLIT = 1e-5           # the project's bar for split-fp16 attention (BAR in test_attention_wide_split16_gpu.py), per element here
SUB = 2.0 ** -24         # fp16 subnormal spacing
KVT = 64                 # keys per tile, every attention kernel
MUTANTS = ('nomask', 'droptile', 'perm', 'merge_swapped', 'merge_unit', 'merge_l')


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def shift(regime, nkv):
    """b_j [nkv] float64, or None for `diffuse`"""
    j = torch.arange(nkv, dtype=torch.float64)
    if regime == 'diffuse':
        return None
    if regime == 'negative':
        return torch.full((nkv,), -20.0, dtype=torch.float64)
    if regime == 'rising':
        return 20.0 * j / nkv
    if regime == 'falling':
        return -20.0 * j / nkv
    if regime == 'first_half':
        return torch.where(2 * j < nkv, 8.0, 0.0).double()
    if regime == 'second_half':
        return torch.where(2 * j >= nkv, 8.0, 0.0).double()
    raise ValueError(regime)


def make_qk(regime, BH, nq, nkv, d, seed, split=False):
    """q [BH, nq, d], k [BH, nkv, d] on the CPU: fp16 for the mixed kernels, fp32 (to be split into hi / lo) when `split`"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((BH, nq, d), generator=g)
    k = torch.randn((BH, nkv, d), generator=g)
    if not split:
        q, k = q.half(), k.half()
    b = shift(regime, nkv)
    if b is not None:
        q[..., 0] = 8.0
        k[..., 0] = (b * math.sqrt(d) / 8.0).half().to(k.dtype)      # fp16-exact in either type
    return q, k


def split16(x):
    """hi = fp16(x), lo = fp16(x - hi): what sdmi_k_cast_f16 writes"""
    hi = x.half()
    return hi, (x.float() - hi.float()).half()


def codings(regime, nkv, d):
    """the V codings of one regime: (name, column of key j [nkv] int64, -1 = key coded nowhere)"""
    j = torch.arange(nkv)
    out = [('segments', j * d // nkv), ('stride', j % d)]
    if regime in ('diffuse', 'negative'):
        seen = set()
        for name, j0 in (('window0', 0), ('window_end', nkv - d), ('window_seam', nkv // 2 - d // 2)):
            j0 = max(j0, 0)
            if j0 in seen:
                continue
            seen.add(j0)
            c = j - j0
            out.append((f'{name}@{j0}', torch.where((c >= 0) & (c < d), c, torch.full_like(c, -1))))
    return out


def dense_v(col, BH, d, dtype=torch.float16):
    """V [BH, nkv, d]: key j sets column (col[j] + bh) mod d"""
    nkv = col.numel()
    v = torch.zeros((BH, nkv, d), dtype=dtype)
    keys = (col >= 0).nonzero().flatten()
    for bh in range(BH):
        v[bh, keys, (col[keys] + bh) % d] = 1
    return v


def vt_padded(v, pad_fill):
    """V^T [BH, d, nkv_pad] with the pad columns nkv .. nkv_pad set to `pad_fill`"""
    BH, nkv, d = v.shape
    vt = torch.full((BH, d, (nkv + 7) // 8 * 8), pad_fill, dtype=v.dtype)
    vt[:, :, :nkv] = v.transpose(1, 2)
    return vt


def heads_first(out, heads):
    """the kernels' output [B, nq, heads * d] -> [BH, nq, d]"""
    B, nq, hd = out.shape
    return out.reshape(B, nq, heads, hd // heads).permute(0, 2, 1, 3).reshape(B * heads, nq, hd // heads)


# ---- reference, tolerance, liveness -------------------------------------------------------------------------------------------------------
def softmax_ref(q, k, scale, causal=False):
    """P = softmax(q k^T scale) in fp64, [BH, nq, nkv], on the operands' device (q, k: anything .double() takes, e.g. hi + lo already summed),
    and each row's largest |q k_j| before the scale, [BH, nq, 1] (see `score_rounding`)"""
    P, smax = [], []
    for i in range(q.shape[0]):
        s = q[i].double() @ k[i].double().t()
        if causal:
            s = s.masked_fill(torch.ones_like(s, dtype=torch.bool).triu(1), float('-inf'))
        smax.append(torch.where(torch.isinf(s), torch.zeros_like(s), s.abs()).max(dim=-1, keepdim=True).values)
        P.append(torch.softmax(s * scale, dim=-1))
    return torch.stack(P), torch.stack(smax)


def score_rounding(family, d, scale, smax):
    """The split-fp16 kernels' extra relative term, from their arithmetic.  R = 1e-5 leaves room for the fp32 exp and sums, not for the fp32
    rounding of the SCORE: q k_j is accumulated in fp32 over n_acc MFMA passes -- three products per 16-wide k-step, 3 ceil(d / 16) in
    attn_split16.hip; in attn_wide_split16.hip a wave runs 3 d / 64 of them over its quarter of d and three more additions join the four
    partials -- and each pass rounds a partial sum of magnitude up to S = max_j |q k_j| by at most 2^-24 S.  Independent roundings add in
    quadrature, and an error ds of a score is a relative error scale * ds of its weight: scale * 2^-24 * S * sqrt(n_acc).  The regimes make S
    large on purpose (q_0 k_j0 = b_j sqrt(d), up to 20 sqrt(d): 253 at d = 160, 640 at d = 1024), so the term is 0.4 .. 2e-5 there and a few
    1e-7 under `diffuse`.  A CPU restatement of exactly that accumulation (`emulate_split_weights`: fp64 products, one fp32 rounding per pass,
    exact exp, no fp16) is up to 1.3e-5 (d = 160) and 1.7e-5 (d = 1024) away from fp64 on a weight under `negative` and `rising`
    (test_attention_probes_host.py::test_split_score_rounding_term); the kernels add the fp16 floors to that.  The factor 2 is set from the
    GPU measurement (module docstring of test_attention_probes_gpu.py): without the term the worst weight is at 1.43 (d = 160) and 2.01
    (d = 1024) of the bar, with it at 0.69 and 0.80.
    The mixed kernels need no such term: their R = 2^-9 is 200 times larger."""
    if family == 'split16':
        n_acc = 3 * ((d + 15) // 16)
    elif family == 'wide_split16':
        n_acc = 3 * (d // 64) + 3
    else:
        return 0.0
    return 2.0 * scale * SUB * smax * math.sqrt(n_acc)


def coded(P, col, d):
    """P @ V for the indicator V of `col` (dense_v), without the matrix: [BH, nq, d] float64"""
    BH, nq, nkv = P.shape
    col = col.to(P.device)
    keys = (col >= 0).nonzero().flatten()
    base = torch.zeros((BH, nq, d), dtype=torch.float64, device=P.device)
    base.index_add_(2, col[keys], P[:, :, keys])
    return torch.stack([base[bh].roll(bh, dims=1) for bh in range(BH)])


def key_counts(col, BH, nq, d, causal=False, device='cpu'):
    """n_c [BH, nq, d]: how many keys that the query row sees are coded into the column"""
    nkv = col.numel()
    vis = torch.ones((1, nq, nkv), dtype=torch.float64, device=device)
    if causal:
        vis = vis.tril()
    return coded(vis.expand(BH, nq, nkv), col, d)


def tolerance(ref, rowmax, n_c, R):
    """R ref + the fp16-subnormal spacing of a P stored against the running maximum, once per key of the column, + the output's own"""
    return R * ref + SUB * n_c * rowmax + SUB


def live(ref, rowmax, n_c):
    """Outputs large enough that a weight is measured and not fp16's subnormal grid: 2^-9 ref > 8 x the floor terms.  For the mixed kernels
    this says that the relative term of their tolerance decides.  For the split-fp16 kernels the same outputs are taken: their R = 1e-5 can
    exceed 8 x the floor only on a weight above 8 x 2^-24 / 1e-5 = 0.048, because P_lo and out_lo are fp16 as well, which no softmax over
    65 or more keys has in 10 % of its columns; on a live output their whole tolerance is below (1e-5 + 2^-12) ref, i.e. a proportional
    error of 0.026 % shows."""
    return R_MIXED * ref > 8 * (SUB * n_c * rowmax + SUB)


def judge(got, P, col, R, causal=False, extra=0.0):
    """got [BH, nq, d] (float64) against the weights P coded by `col`.  Returns a dict: worst err / tol, the share of live outputs among the
    non-empty ones, whether every row that sees a coded key has a live output, and whether the empty outputs are exactly 0.  `extra`: a relative term beside R,
    per row (score_rounding)."""
    BH, nq, d = got.shape
    ref = coded(P, col, d)
    rowmax = P.max(dim=-1, keepdim=True).values
    n_c = key_counts(col, BH, nq, d, causal, P.device)
    tol = tolerance(ref, rowmax, n_c, R) + extra * ref
    err = (got - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / tol, torch.full_like(err, float('inf')))
    full = n_c > 0
    lv = live(ref, rowmax, n_c) & full
    rows = full.any(dim=-1)                       # (causal: a row before the window sees no coded key, and all of it must be 0)
    own = (R * ref > 8 * (SUB * n_c * rowmax + SUB)) & full          # (printed for the split-fp16 kernels, not asserted: see `live`)
    return dict(worst=float(ratio.max()), at=int(ratio.flatten().argmax()), share=float(lv.sum()) / max(1, int(full.sum())),
                share_own=float(own.sum()) / max(1, int(full.sum())), rows_live=bool(lv.any(dim=-1)[rows].all()),
                zeros_exact=bool((got[~full] == 0).all()))


def liveness(P, col, d, causal=False):
    """the two liveness figures of `judge` from the reference alone"""
    BH, nq, _ = P.shape
    ref = coded(P, col, d)
    rowmax = P.max(dim=-1, keepdim=True).values
    n_c = key_counts(col, BH, nq, d, causal, P.device)
    full = n_c > 0
    lv = live(ref, rowmax, n_c) & full
    return float(lv.sum()) / max(1, int(full.sum())), bool(lv.any(dim=-1)[full.any(dim=-1)].all())


# ---- the GPU cases ------------------------------------------------------------------------------------------------------------------------
DMA_SHAPES = [(33, 1), (33, 64), (40, 65), (96, 203), (130, 129), (130, 337), (1000, 1000), (1030, 449)]
DMA_D = [24, 32, 40, 48, 64, 80, 96, 128, 160]
KVSPLIT_SHAPES = [(1030, 2048), (1062, 2176), (1030, 4096), (1030, 2112)]
CAUSAL_D = [32, 64, 128]
CAUSAL_N = [1, 40, 64, 65, 77, 130]
WIDE_SHAPES = {192: [(33, 1), (64, 65), (40, 203), (1290, 203)], 448: [(33, 1), (64, 65), (40, 203), (520, 203)],
               1024: [(33, 1), (64, 65), (40, 203), (260, 520)]}
SPLIT_D = [24, 40, 64, 160]
SPLIT_SHAPES = [(33, 1), (40, 65), (130, 203), (64, 337)]
WIDE_SPLIT_D = [192, 1024]
WIDE_SPLIT_SHAPES = [(33, 1), (64, 65), (129, 203)]


def gpu_cases():
    """(family, d, nq, nkv) of tests/test_attention_probes_gpu.py"""
    out = [('dma', d, nq, nkv) for d in DMA_D for nq, nkv in DMA_SHAPES]
    out += [('kvsplit', 40, nq, nkv) for nq, nkv in KVSPLIT_SHAPES]
    out += [('causal', d, n, n) for d in CAUSAL_D for n in CAUSAL_N]
    out += [('wide', d, nq, nkv) for d in WIDE_SHAPES for nq, nkv in WIDE_SHAPES[d]]
    out += [('split16', d, nq, nkv) for d in SPLIT_D for nq, nkv in SPLIT_SHAPES]
    out += [('wide_split16', d, nq, nkv) for d in WIDE_SPLIT_D for nq, nkv in WIDE_SPLIT_SHAPES]
    return out


def batch_heads(family, nq, nkv):
    """(B, heads): 2 x 2, except for the one largest shape (the 4096-key split), which runs one batch of two heads"""
    return (1, 2) if nq * nkv > 4_000_000 else (2, 2)


def case_seed(family, d, nq, nkv, regime):
    return 1009 * d + 31 * nq + 7 * nkv + 100003 * REGIMES.index(regime) + (17 if family in ('split16', 'wide_split16') else 0)


def case_R(family):
    return R_SPLIT if family in ('split16', 'wide_split16') else R_MIXED


# ---- the kernels' loop in plain torch ------------------------------------------------------------------------------------------------------
def emulate(q, k, v, scale, kvs=1, ones=True, causal=False, mutant=None):
    """The arithmetic of attn_dma_kernel restated: tiles of 64 keys, fp32 scores, a running maximum in log2 units, alpha = exp2(m_old - m_new),
    P rounded to fp16 for the P V product, the denominator summed from the rounded P (`ones`: the ONES row of V^T) or from the fp32 P, fp32
    accumulation, and for kvs = 2 two key groups of nt / 2 tiles merged as O = 2^(m0 - m) O0 + 2^(m1 - m) O1.  q [BH, nq, d], k, v [BH, nkv, d]
    -> fp16 [BH, nq, d].  Rows of K and V past nkv are zeros, as the kernels stage them.
    `mutant` plants one defect: nomask (no tail mask), droptile (the last tile skipped), perm (keys 4..7 <-> 8..11 of every tile swapped on the
    V side), merge_swapped (the two merge weights exchanged), merge_unit (both 1), merge_l (the denominators added without weights)."""
    assert mutant is None or mutant in MUTANTS
    BH, nq, d = q.shape
    nkv = k.shape[1]
    nt_all = (nkv + KVT - 1) // KVT
    assert nt_all % kvs == 0
    pad = nt_all * KVT - nkv
    kf = torch.cat([k.float(), torch.zeros((BH, pad, d))], dim=1)
    vf = torch.cat([v.float(), torch.zeros((BH, pad, d))], dim=1)
    if mutant == 'perm':
        idx = torch.arange(nt_all * KVT)
        r = idx % KVT
        idx = torch.where((r >= 4) & (r < 8), idx + 4, torch.where((r >= 8) & (r < 12), idx - 4, idx))
        vf = vf[:, idx]
    s_all = q.float() @ kf.transpose(1, 2)                      # fp32, [BH, nq, nt_all * 64]
    sc = torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    kv = torch.arange(nt_all * KVT)
    dead = torch.zeros((nq, nt_all * KVT), dtype=torch.bool)
    if mutant != 'nomask':
        dead |= (kv >= nkv)[None, :]
    if causal:
        dead |= kv[None, :] > torch.arange(nq)[:, None]
    s_all = s_all.masked_fill(dead[None], -1e30)
    nt = nt_all // kvs
    parts = []
    for g in range(kvs):
        o = torch.zeros((BH, nq, d))
        l_run = torch.zeros((BH, nq, 1))
        m_run = torch.full((BH, nq, 1), -1e30)
        for t in range(g * nt, (g + 1) * nt):
            if mutant == 'droptile' and t == nt_all - 1:
                continue
            s = s_all[:, :, t * KVT:(t + 1) * KVT]
            m_new = torch.maximum(m_run, s.max(dim=-1, keepdim=True).values * sc)
            alpha = torch.exp2(m_run - m_new)
            m_run = m_new
            p = torch.exp2(s * sc - m_run)
            p16 = p.half().float()
            o = o * alpha + p16 @ vf[:, t * KVT:(t + 1) * KVT]
            l_run = l_run * alpha + (p16 if ones else p).sum(dim=-1, keepdim=True)
        parts.append((o, m_run, l_run))
    o, m_run, l_run = parts[0]
    if kvs == 2:
        o1, m1, l1 = parts[1]
        m = torch.maximum(m_run, m1)
        a0, a1 = torch.exp2(m_run - m), torch.exp2(m1 - m)
        if mutant == 'merge_swapped':
            a0, a1 = a1, a0
        if mutant == 'merge_unit':
            a0, a1 = torch.ones_like(a0), torch.ones_like(a1)
        o = a0 * o + a1 * o1
        l_run = l_run + l1 if mutant == 'merge_l' else a0 * l_run + a1 * l1
    return (o * (1.0 / l_run)).half()


def emulate_split_weights(q, k, scale, family):
    """The split-fp16 kernels' SCORE arithmetic restated, everything after it exact: q k_j accumulated in fp32, one rounding per MFMA pass (three
    products per 16-wide k-step; `wide_split16`: four quarters of d, then ((w0 + w1) + w2) + w3), the exponent argument rounded to fp32, the exp
    and the normalisation in fp64.  q, k fp32 [BH, n, d] -> weights [BH, nq, nkv] float64.  What `score_rounding` is about."""
    (qh, ql), (kh, kl) = split16(q), split16(k)
    BH, nq, d = q.shape

    def accumulate(d0, d1):
        s = torch.zeros((BH, nq, k.shape[1]), dtype=torch.float32)
        for c in range(d0, d1, 16):
            sl = slice(c, min(c + 16, d1))
            for a, b in ((kl, qh), (kh, ql), (kh, qh)):
                s = (s.double() + b[:, :, sl].double() @ a[:, :, sl].double().transpose(1, 2)).float()
        return s

    if family == 'wide_split16':
        w = [accumulate(i * d // 4, (i + 1) * d // 4) for i in range(4)]
        s = ((w[0] + w[1]) + w[2]) + w[3]
    else:
        s = accumulate(0, d)
    sc = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    m = s.max(dim=-1, keepdim=True).values * sc
    e = (s.double() * sc.double() - m.double()).float()
    p = torch.exp2(e.double())
    return p / p.sum(dim=-1, keepdim=True)
