"""The LayerNorm fold of the transformer blocks (csrc/unet.cpp attn_block: C % 64 == 0, C <= 1280, rows per sample and M multiples of
64) through the C ABI, in guarded buffers (tests/guard.py), against fp64 torch on the device -- at every transformer width of the committed
configs, at the row shapes where the producer's tile rule bites, with every tile pinned, and on inputs a one-pass fp32 variance dislikes.

The fold has two halves.  The PRODUCER (the GEMM that writes the token stream x = residual + a Wo^T + b) also stores fp16(gamma * x) and,
per row and 32-column block, {sum, sum of squares} of the fp32 values it stored (IGemmParams::f16_scale + lnp_out; 16-byte epilogue only:
launch_igemm replaces a tile that is not full in M, N and inside one sample by tile 5, pinned or not).  The CONSUMER (q | k | v head
scatter, GEGLU, a plain projection) fetches the partials of its rows in two halves (blocks 0..19 always, 20..39 for C > 640:
lnf_request), folds them in fp32 (one pass: var = q / C - mu^2, clamped at 0: lnf_finish) and turns its accumulators into
rstd * (acc - mu * cs) + d, with the column terms cs = sum_k gamma_k w_nk, d = sum_k beta_k w_nk + bias of ln_fold_prep.

Every operand and output lives in a guard.Pool buffer, outputs 0xFF-poisoned (a partial that was never written is NaN and comes out of
the consumer as NaN); after every launch all guards are checked and the inputs must be unchanged bits.  No library LayerNorm on the
reference path; the reference works from the fp32 stream the producer STORED, so each stage's error is its own.

Comparisons
  1  producer   x against fp64 residual + a Wo^T + b: 3e-4 (fp16 operands), _tol_split of test_model_shapes_gpu (split-fp16 operands: 3e-5),
                also on the outlier channels, whose values reach 300.  fp16 copy == (x * gamma).half() of the stored x, bit for bit.
                Partials against fp64 sums over the stored x:
                rtol 1e-5, atol 1e-4 (sum) / 1e-3 (sum of squares) as in test_layernorm_folded_into_consumer, scaled by the block's
                sum |x| / 43 and sum x^2 / 91 where those exceed the benign block's (32 values of std 1.66, mean 0.3: E sum |x| = 43,
                E sum x^2 = 91).  In place (residual == out_f32, as the executor runs it) == out of place, bit for bit.
  2  consumer against the TRUE operation Linear(LayerNorm_fp64(x)) (+ GEGLU / head scatter), benign inputs only: 6e-3 plain and heads,
                8e-3 GEGLU, and e_fold <= 1.5 e_two_launch + 5e-4 against the layernorm kernel + GEMM path (not under test here) -- the
                bars of test_layernorm_folded_into_consumer, unchanged.  On the adverse inputs both errors are printed, nothing asserted:
                the fold rounds its operand relative to |gamma x|, the two-launch path relative to |x - mu| / sigma, so the fold loses
                by about A_m = rms(x_m) / sigma_m there.  That is the design.
  3  consumer against the FOLD IN EXACT ARITHMETIC, y3 = rstd64 * (a16 w^T - mu64 cs64) + d64 in fp64 from the stored fp16 operand, the fp16
                weights and fp64 statistics of the stored x: the operand rounding is in the reference, what is left is the kernel's arithmetic.
                Bar per element of y:  3e-4 A_m + 2^-20 A_m^2 |y3_mn|  (the fp32-accumulation bar at unit scale, amplified by the
                cancellation in acc - mu cs; 16 fp32 ulps of the one-pass variance).  Derived, not measured.  Two corrections of the
                derivation, both written into _out / _bar_y and both measured next to the uncorrected bar's figure (printed per case):
                  a) the bar is for the fp32 value.  q | k | v^T and the GEGLU output are STORED as fp16: + 2^-11 (|ref| + bar), half an ulp
                     of the format (a q of 4.0 moves by up to 9.8e-4 in the store alone).  GEGLU = value * gelu(gate) propagates the two
                     bars: bar_v |gelu(g)| + |v| (1.13 bar_g + 0.75e-7 |g|) + 1.13 bar_v bar_g  (1.13 = sup |gelu'|; 1.5e-7 = the erf
                     approximation of gelu_erf).  The plain consumer stores fp32 and keeps the bar as derived.
                  b) constant rows (variance exactly 0: A_m has no meaning).  The |cs_n| form: finite, within sqrt(1 / eps) 2^-22 |mu| |cs_n|
                     of d.  acc and mu * cs are two fp32 sums of the SAME K products in different orders; their difference scales with
                     sum_k |gamma_k w_nk| (about 0.8 sqrt(K)), not with the sum's value |cs_n|, which is arbitrarily close to 0 for some
                     column.  Asserted: sqrt(1 / eps) 2^-22 |mu| sum_k |gamma_k w_nk|; the |cs_n| form is measured and printed.  Three
                     constant rows are built where the operand does not round (gamma fp16-representable in this distribution, x a power
                     of two: 4, -8, 0.5), so y3 = d as that derivation assumes, and s, q, mu are nearly exact: there the negative side of
                     the clamp fmaxf(q / C - mu^2, 0) is reached, if at all, through the rounding of 1 / C.  A fourth row is 3.7: gamma * x
                     rounds, E_mn = a16 w^T - mu cs is about 2^-12 |mu| instead of 0, the sums round, and the one-pass variance is rounding
                     noise of either sign next to eps.  Its bar adds what that noise does to rstd: with the variance off by up to the
                     16 ulps of the bar above, 2^-20 mu^2, rstd lies in [R / sqrt(1 + 2^-20 mu^2 / eps), R], R = sqrt(1 / eps), so
                     + R |E_mn| (1 - 1 / sqrt(1 + 2^-20 mu^2 / eps)), 0.35 R |E_mn| at 3.7 and 0 on the other three rows.  Against the
                     TRUE operation that row is off by order 1 (printed with comparison 2): 2^-12 |mu| of operand rounding against a
                     sigma of 0, times rstd = 316 -- the fold cannot normalise a constant row.  No token stream has one; it is the limit
                     of the offset rows.
Controls: one partial {sum, sum of squares} of one row, in the LAST block of the width, off by 1 % -> comparison 3 fails on that row and holds
on every other (at C = 1280: block 39, so the second half of lnf_request is read); cs, d prepared with gamma = 1 -> comparison 2 fails.

Axes.  Widths 192 .. 1280 (every transformer width of the committed configs with C % 64 == 0; 640 | 704 = the two sides of lnf_npart > 20).
Row shapes (B, rows per sample): (1, 64) M below every tile but the 64-row ones; (2, 64) (3, 64) 128- / 256-row tiles straddle samples and
192 is no multiple of 128; (3, 128); (2, 256); (1, 576) the 24 x 24 level; (8, 64) the smallest shape the executor folds.  Producers: fp16
dense out-projection with bias + residual out of place and in place, split-fp16 proj_in form (hi | lo from K.cast_f16; with the residual,
a superset of proj_in's epilogue, so that the four distributions are built the same way).  Consumers: q | k | v at every head dim of the
models that divides C, GEGLU N = 8C, plain N = C without bias.  Every width x row shape x distribution x consumer runs at the dispatch
request (tile -1); at C = 320 / 640 / 1280 on (2, 64) and (1, 576) the producers sweep every generic dense tile
(0..13, 18..21; split-fp16: the ids of test_gemm_split16) and the consumers every generic tile of their mode (GEGLU: even TN), on all four
distributions.  Nothing thinned.

Measured on an MI355X, worst over all cases of the file (from the `comparison 1 / 2 / 3` line every case prints); ratio = error / bar:
                                                      benign      offset rows  outlier ch.  constant rows
  1  x, fp16 operands          max-abs (bar 3e-4)     2.2e-6      2.5e-6       1.3e-5       2.2e-6
     x, split-fp16 operands    max-abs (bar 3e-5)     1.07e-5     1.15e-5      1.57e-5      1.05e-5
     partials                  ratio                  0.037       0.015        0.027        0.027
     fp16 copy, in place == out of place: bit-equal in every case
  2  plain   fold | two-launch max-abs (bar 6e-3)     1.27e-3 | 1.21e-3   9.9e-3 | 1.29e-3   2.35e-3 | 2.51e-3   0.98 | 1.13e-3
     heads   fold | two-launch max-abs (bar 6e-3)     2.50e-3 | 2.54e-3   1.09e-2 | 2.54e-3  4.14e-3 | 4.31e-3   1.02 | 2.62e-3
     GEGLU   fold | two-launch max-abs (bar 8e-3)     7.05e-3 | 6.57e-3   3.30e-2 | 7.13e-3  1.24e-2 | 1.48e-2   0.49 | 8.31e-3
     (asserted on benign only.  The GEGLU figures are the fp16 store of outputs beyond 8, half an ulp = 3.9e-3, on both paths.  Offset rows:
     the fold loses by 4.6 .. 7.7 at A_m = 8, as designed; outlier channels: no loss, A_m is 1; constant rows: the fold's figure is the
     3.7 row's, correction b)
  3  plain   ratio (bar as derived)                   0.010       0.035        0.012        0.885  (|cs_n| form: 4.2e3)
     heads   ratio (correction a)                     0.861       0.619        0.861        0.889  (without a: 6.4, 1.7, 6.4; |cs_n| form: 4.3e4)
     GEGLU   ratio (correction a)                     0.672       0.211        0.677        0.759  (without a: 2.1, 0.27, 2.5; |cs_n| form: 43)
     The fp32 output sits a factor 30 .. 100 inside the derived bar; with an fp16 store the half ulp of the format is what is seen
     (a ratio near 1 is an output just above a power of two, not a kernel error: the term is a strict bound).  Constant rows: the
     power-of-two rows reach 0.28 of their bar; 0.885 is the 3.7 row, whose one-pass variance noise uses most of the 16 ulps allowed.
  controls  wrong partial: ratio 27 .. 57 on the corrupted row (the one whose last block holds most of its sum of squares), <= 0.010 on
            every other; missing gamma: fold 0.16 .. 0.23 against a two-launch error of 1e-3 at every width
No case failed: launch_igemm's tile rule and the 16-byte epilogue's condition agree on every pinned tile, and both halves of lnf_request are read.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import kernels as K  # noqa: E402
from test_model_shapes_gpu import _tol_split  # noqa: E402  (the split-fp16 bar: 3e-5 at every K of this file)

DEV = 'cuda'
EPS = 1e-5
WIDTHS = [192, 256, 320, 384, 512, 576, 640, 704, 768, 960, 1024, 1280]
ROWS = [(1, 64), (2, 64), (3, 64), (3, 128), (2, 256), (1, 576), (8, 64)]
DISTS = ['benign', 'offset', 'outlier', 'const']
HEAD_DIMS = [32, 40, 64, 80, 96, 160]
# id: (BM, BN, waves M, waves N) of the generic dense tiles (kTiles of csrc/igemm.hip; 14..17 are the halo-staged 3x3 conv)
TILES = {0: (128, 128, 2, 2), 1: (128, 64, 2, 2), 2: (64, 64, 2, 2), 3: (256, 128, 4, 2), 4: (128, 64, 2, 2), 5: (64, 64, 2, 2),
         6: (256, 128, 4, 2), 7: (128, 128, 2, 2), 8: (64, 128, 2, 2), 9: (128, 128, 4, 2), 10: (64, 64, 2, 2), 11: (128, 256, 2, 4),
         12: (64, 256, 1, 4), 13: (256, 64, 4, 1), 18: (64, 64, 2, 2), 19: (64, 128, 2, 2), 20: (128, 64, 2, 2), 21: (128, 128, 4, 2)}
GENERIC = sorted(TILES)
GEGLU_TILES = [t for t in GENERIC if (TILES[t][1] // TILES[t][3] // 32) % 2 == 0]
SPLIT16_TILES = [0, 1, 2, 4, 5, 8, 10]
CONST_VALUES = (4.0, -8.0, 0.5, 3.7)    # three where gamma * x does not round in fp16, one where it does (module docstring, correction b)


def _g(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, device=DEV) * scale


def _worst(name, got, ref, bar):
    """(max |got - ref| / bar, max |got - ref|); bar a number or a tensor like ref.  Prints K.report for the row that holds the worst
    ratio (the tensors stay on the device); a non-finite output is reported as inf."""
    got2 = got.reshape(-1, got.shape[-1]).double()
    ref2 = ref.reshape(-1, ref.shape[-1]).double()
    if not bool(torch.isfinite(got2).all()):
        bad = (~torch.isfinite(got2)).nonzero()[0].tolist()
        print(f'[{name}] non-finite output at row {bad[0]} col {bad[1]} of {tuple(got2.shape)}', flush=True)
        return float('inf'), float('inf')
    d = (got2 - ref2).abs()
    bar_t = bar.reshape(d.shape).double() if torch.is_tensor(bar) else torch.full_like(d, float(bar))
    ratio = d / bar_t
    r = int(ratio.max(1).values.argmax())
    c = int(ratio[r].argmax())
    K.report(name, got2[r], ref2[r], float(bar_t[r, c]))
    return float(ratio[r, c]), float(d.max())


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


class _Weights:
    """what depends on the width alone: LayerNorm affine, the three consumers' weights, their column terms (ln_fold_prep) and fp64 twins"""

    def __init__(self, C, g16):
        self.C = C
        g = _g(1000 + C + (7 if g16 else 0))
        self.P = P = guard.Pool(DEV)
        gamma = 1 + _randn((C,), g, 0.2)
        if g16:         # the constant rows' gamma: fp16-representable (module docstring, correction b)
            gamma = gamma.half().float()
        self.gamma, self.beta = P.put('ln_gamma', gamma), P.put('ln_beta', _randn((C,), g, 0.1))
        s = 1.0 / math.sqrt(C)
        self.w = {'heads': P.put('w_qkv', _randn((3 * C, C), g, s).half()), 'plain': P.put('w_q', _randn((C, C), g, s).half())}
        wg, bg = _randn((8 * C, C), g, s), _randn((8 * C,), g, 0.1)
        wp, bp = K.pack_geglu(wg, bg)
        self.w['geglu'] = P.put('w_geglu_packed', wp)
        self.bp = P.put('b_geglu_packed', bp)
        self.w64 = {'heads': self.w['heads'].double(), 'plain': self.w['plain'].double(), 'geglu': wg.half().double()}
        self.b64 = {'heads': None, 'plain': None, 'geglu': bg.double()}
        self.ones = P.put('ones', torch.ones(C, device=DEV))
        self.cs, self.dn, self.cs64, self.d64, self.acs64 = {}, {}, {}, {}, {}
        for kind in ('heads', 'plain', 'geglu'):
            N = self.w[kind].shape[0]       # (written straight into poisoned, guarded buffers: a column the prep kernel skips is NaN)
            self.cs[kind], self.dn[kind] = P.new(f'cs_{kind}', (N,), torch.float32), P.new(f'd_{kind}', (N,), torch.float32)
            K.ln_fold_prep(self.w[kind], C, self.gamma, self.beta, self.bp if kind == 'geglu' else None, out=(self.cs[kind], self.dn[kind]))
            w64 = self.w64[kind]
            self.cs64[kind] = (w64 * self.gamma.double()[None]).sum(1)
            self.acs64[kind] = (w64 * self.gamma.double()[None]).abs().sum(1)
            self.d64[kind] = (w64 * self.beta.double()[None]).sum(1) + (0.0 if self.b64[kind] is None else self.b64[kind])
        # (the packed GEGLU order is a permutation of the columns: compare the prepared terms as sorted multisets would hide a wrong
        # pairing, so the GEGLU terms are checked through the consumer's output; the unpermuted two directly, fp32 chain of K / 64 fmas
        # per lane + a 6-step butterfly)
        tol = (C / 64 + 6) * 2.0 ** -24
        for kind in ('heads', 'plain'):
            assert bool(((self.cs[kind].double() - self.cs64[kind]).abs() <= tol * self.acs64[kind] + 1e-30).all()), kind
            ab = (self.w64[kind] * self.beta.double()[None]).abs().sum(1)
            assert bool(((self.dn[kind].double() - self.d64[kind]).abs() <= tol * ab + 1e-30).all()), kind
        torch.cuda.synchronize()
        self.inputs = [(v, v.clone()) for _, gb in P.bufs for v in (gb.view,)]
        P.check(f'C{C} weights')

    def unchanged(self, tag):
        self.P.check(tag)
        for v, keep in self.inputs:
            assert torch.equal(v, keep), f'{tag}: a weight / column-term operand was modified'


@functools.lru_cache(maxsize=2)
def _weights(C, g16):
    return _Weights(C, g16)


class _Stream:
    """one (width, row shape, distribution): the producers' operands in guarded buffers and the fp64 reference of the token stream"""

    def __init__(self, C, B, ntok, dist):
        self.C, self.B, self.ntok, self.dist, self.M = C, B, ntok, dist, B * ntok
        M = self.M
        self.W = _weights(C, dist == 'const')
        self.tag = f'C{C} B{B} n{ntok} {dist}'
        g = _g((C * 131 + B * 17 + ntok) * 4 + DISTS.index(dist))
        self.P = P = guard.Pool(DEV)
        s = 1.0 / math.sqrt(C)
        a = _randn((M, C), g, 0.7).half()
        a32 = _randn((M, C), g, 2.0)                              # N(0, 4): the operands _tol_split is stated for
        bo = _randn((C,), g, 0.1)
        self.const_rows = None
        if dist == 'benign':            # test_layernorm_folded_into_consumer's
            resid = _randn((M, C), g, 1.5) + 0.3
        elif dist == 'offset':          # every row: mean +-8, unit std (the product adds 0.7^2 of variance: the residual brings the rest)
            sign = (torch.rand((M, 1), generator=g, device=DEV) < 0.5).float() * 2 - 1
            resid = _randn((M, C), g, math.sqrt(1 - 0.49)) + 8.0 * sign
        elif dist == 'outlier':         # four channels at 40 x: one in the last block, for C >= 704 one in block 20
            resid = _randn((M, C), g, 1.5) + 0.3
            ch = [5, C // 3, 2 * C // 3 + 1, C - 9]
            if C >= 704:
                ch[1] = 20 * 32 + 7
            assert len(set(ch)) == 4 and ch[3] // 32 == C // 32 - 1
            resid[:, ch] *= 40.0
        else:                           # a few rows constant over the channels: zero `a` row, zero bias, constant residual row
            resid = _randn((M, C), g, 1.5) + 0.3
            rows = sorted({0, 5, M // 2 + 1, M - 1})
            self.const_rows = torch.tensor(rows, device=DEV)
            self.const_val = torch.tensor([CONST_VALUES[i % len(CONST_VALUES)] for i in range(len(rows))], device=DEV)
            a[rows] = 0
            a32[rows] = 0
            bo.zero_()
            resid[rows] = self.const_val[:, None].expand(-1, C)
        self.resid0 = resid
        wo = _randn((C, C), g, s).half()
        w32 = _randn((C, C), g, s)
        hi, lo = K.cast_f16(a32, want_lo=True)
        self.a, self.wo, self.bo = P.put('a', a), P.put('wo', wo), P.put('bo', bo)
        self.hi, self.lo, self.w3 = P.put('a_hi', hi), P.put('a_lo', lo), P.put('wo_split3', K.pack_split3(w32))
        self.resid = P.put('residual', resid)
        self.ref = {'f16': resid.double() + a.double() @ wo.double().t() + bo.double()[None],
                    'split16': resid.double() + a32.double() @ w32.double().t() + bo.double()[None]}
        torch.cuda.synchronize()
        self.inputs = [(v, v.clone()) for v in (self.a, self.wo, self.bo, self.hi, self.lo, self.w3, self.resid)]
        self.stored = []        # the consumers' own inputs (the stored x, fp16 copy and partials): prepare()
        self.two = {}

    def unchanged(self, tag):
        for v, keep in self.inputs + self.stored:
            assert torch.equal(v, keep), f'{tag}: an input operand was modified'
        self.W.unchanged(tag)

    # ---- producer ---------------------------------------------------------------------------------------------------------------
    def produce(self, kind, tile, keep=True):
        """kind: 'f16' (dense out-projection), 'f16-inplace' (residual == out_f32), 'split16'.  Comparison 1 on what it stored."""
        P, M, C, B, ntok, W = self.P, self.M, self.C, self.B, self.ntok, self.W
        tag = f'{self.tag} producer {kind} tile{tile}'
        n0 = len(P.bufs)
        x = P.new('x', (M, C), torch.float32)
        a16 = P.new('ln16', (M, C), torch.float16)
        part = P.new('lnp', (C // 32, M, 2), torch.float32, row_bytes=8 * M)
        if kind == 'f16-inplace':
            x.copy_(self.resid0)
            res = x
        else:
            res = self.resid
        if kind == 'split16':
            K.igemm(self.hi, self.w3, C, B, ntok, 1, ntok, 1, a1=self.lo, bias=self.bo, residual=res, out_f32=x, out_f16=a16, tile=tile,
                    f16_scale=W.gamma, lnp_out=part, split16=True)
            ref, tol = self.ref['split16'], _tol_split(C)
        else:
            K.igemm(self.a, self.wo, C, B, ntok, 1, ntok, 1, bias=self.bo, residual=res, out_f32=x, out_f16=a16, tile=tile,
                    f16_scale=W.gamma, lnp_out=part)
            ref, tol = self.ref['f16'], 3e-4
        torch.cuda.synchronize()
        r1, e1 = _worst(f'{tag} x', x, ref, tol)
        assert r1 < 1.0, (tag, r1, e1)
        assert torch.equal(a16, (x * W.gamma[None]).half()), f'{tag}: fp16 copy != (x * gamma).half()'
        xs = x.double().reshape(M, C // 32, 32)
        s1, s2, sa = xs.sum(-1).t(), (xs * xs).sum(-1).t(), xs.abs().sum(-1).t()
        adverse = self.dist != 'benign'
        bar1 = 1e-5 * s1.abs() + 1e-4 * (torch.clamp(sa / 43.0, min=1.0) if adverse else 1.0)
        bar2 = 1e-5 * s2 + 1e-3 * (torch.clamp(s2 / 91.0, min=1.0) if adverse else 1.0)
        rs, es = _worst(f'{tag} partial sums', part[..., 0], s1, bar1)
        rq, eq = _worst(f'{tag} partial sums of squares', part[..., 1], s2, bar2)
        print(f'[{tag}] comparison 1: x max-abs {e1:.3e} (bar {tol:.0e}); partials ratio {max(rs, rq):.3f} of the bar', flush=True)
        assert rs < 1.0 and rq < 1.0, (tag, rs, rq)
        P.check(tag)
        self.unchanged(tag)
        if not keep:
            del P.bufs[n0:]         # (the tensors outlive their pool entry)
        return x, a16, part

    # ---- consumer ---------------------------------------------------------------------------------------------------------------
    def prepare(self, x, a16, part, kinds=('heads', 'plain', 'geglu')):
        """fp64 statistics of the STORED stream and the two references of y = Linear(LayerNorm(x)) per consumer kind; from here on the
        stored x, its fp16 copy and the partials are inputs (of the consumers) and must stay unchanged bits"""
        W = self.W
        self.stored = [(v, v.clone()) for v in (x, a16, part)]
        xd = x.double()
        mu = xd.mean(1)
        var = (xd - mu[:, None]).pow(2).mean(1)
        self.mu = mu
        A = (xd.pow(2).mean(1) / var).sqrt()
        if self.const_rows is not None:
            var[self.const_rows] = 0.0                   # (exactly: the stored rows ARE constant, asserted here)
            assert bool((x[self.const_rows] == self.const_val[:, None]).all())
            A[self.const_rows] = 1.0                     # (placeholder: these rows take their own bar, _bar_y)
        self.A = A
        rstd = 1.0 / (var + EPS).sqrt()
        xn = (xd - mu[:, None]) * rstd[:, None] * W.gamma.double()[None] + W.beta.double()[None]
        a64 = a16.double()
        self.y_true, self.y3, self.E = {}, {}, {}
        for kind in kinds:
            w64, b = W.w64[kind], W.b64[kind]
            self.y_true[kind] = xn @ w64.t() + (0.0 if b is None else b[None])
            e = a64 @ w64.t() - mu[:, None] * W.cs64[kind][None]
            self.y3[kind] = rstd[:, None] * e + W.d64[kind][None]
            if self.const_rows is not None:         # what the operand rounding leaves of acc - mu cs on a constant row (0 where it does not round)
                self.E[kind] = e[self.const_rows].abs()
        self.two = {}

    def _bar_y(self, kind, cs_form=False):
        """comparison 3's bar per element of y (module docstring); constant rows: correction b, or with |cs_n| for sum_k |gamma_k w_nk|"""
        A = self.A[:, None]
        bar = 3e-4 * A + 2.0 ** -20 * A * A * self.y3[kind].abs()
        if self.const_rows is not None:
            col = self.W.cs64[kind].abs() if cs_form else self.W.acs64[kind]
            mu = self.mu[self.const_rows].abs()[:, None]
            rstd_slack = 1.0 - 1.0 / (1.0 + 2.0 ** -20 * mu * mu / EPS).sqrt()
            bar[self.const_rows] = math.sqrt(1.0 / EPS) * (2.0 ** -22 * mu * col[None] + self.E[kind] * rstd_slack)
        return bar

    def _out(self, kind, y, bar_y=None, stored_bar=True):
        """y [M, N] fp64 -> the consumer's output (GEGLU: value * gelu(gate)); with bar_y also the propagated bar (correction a)"""
        if kind == 'geglu':
            v, gt = y.chunk(2, dim=1)
            out = v * _gelu64(gt)
            if bar_y is None:
                return out
            bv, bg = bar_y.chunk(2, dim=1)
            bar = bv * _gelu64(gt).abs() + v.abs() * (1.13 * bg + 0.75e-7 * gt.abs()) + 1.13 * bv * bg
        else:
            out = y
            if bar_y is None:
                return out
            bar = bar_y
        if kind != 'plain' and stored_bar:
            bar = bar + 2.0 ** -11 * (out.abs() + bar)
        return out, bar

    def _launch(self, kind, src, tile, dh, fold, part=None, cs=None, dn=None):
        """one consumer launch into fresh poisoned outputs; returns its output as [M, N'] (heads: q | k | v gathered back to token order)"""
        P, M, C, B, ntok, W = self.P, self.M, self.C, self.B, self.ntok, self.W
        n0 = len(P.bufs)
        extra = dict(lnf=(part, EPS, W.cs[kind] if cs is None else cs, W.dn[kind] if dn is None else dn)) if fold else {}
        if kind == 'plain':
            out = P.new('out_plain', (M, C), torch.float32)
            K.igemm(src, W.w[kind], C, B, ntok, 1, ntok, 1, out_f32=out, tile=tile, **extra)
            torch.cuda.synchronize()
            got = out.double()
        elif kind == 'geglu':
            out = P.new('out_geglu', (M, 4 * C), torch.float16)
            K.igemm(src, W.w[kind], 8 * C, B, ntok, 1, ntok, 1, out_f16=out, mode=1, tile=tile, bias=None if fold else W.bp, **extra)
            torch.cuda.synchronize()
            got = out.double()
        else:
            heads = C // dh
            q = P.new('q', (B * heads, ntok, dh), torch.float16)
            k = P.new('k', (B * heads, ntok, dh), torch.float16)
            vt = P.new('vt', (B * heads, dh, ntok), torch.float16)
            K.igemm(src, W.w[kind], 3 * C, B, ntok, 1, ntok, 1, mode=2, tile=tile,
                    heads=dict(segs=[(q, 0), (k, 0), (vt, 1)], heads=heads, dh=dh, ntok=ntok, ntok_pad=ntok, segC=C), **extra)
            torch.cuda.synchronize()
            qq = q.double().reshape(B, heads, ntok, dh).permute(0, 2, 1, 3).reshape(M, C)
            kk = k.double().reshape(B, heads, ntok, dh).permute(0, 2, 1, 3).reshape(M, C)
            vv = vt.double().reshape(B, heads, dh, ntok).permute(0, 3, 1, 2).reshape(M, C)
            got = torch.cat([qq, kk, vv], dim=1)
        P.check(f'{self.tag} consumer {kind} tile{tile} dh{dh} fold{int(fold)}')
        del P.bufs[n0:]
        return got

    def two_launch_error(self, kind, x, dh):
        """max error of the layernorm kernel + GEMM path against the true operation (dispatch tile; once per kind and head dim)"""
        if (kind, dh) not in self.two:
            if 'ln16' not in self.two:
                self.two['ln16'] = K.layernorm(x, self.W.gamma, self.W.beta, EPS)
            got = self._launch(kind, self.two['ln16'], -1, dh, fold=False)
            self.two[(kind, dh)] = float((got - self._out(kind, self.y_true[kind])).abs().max())
        return self.two[(kind, dh)]

    def consume(self, kind, x, a16, part, tile=-1, dh=None, src='f16'):
        """one folding consumer launch: comparison 3 always, comparison 2 on the benign inputs (figures only on the adverse ones)"""
        tag = f'{self.tag} {src}->{kind}' + (f' dh{dh}' if dh else '') + f' tile{tile}'
        got = self._launch(kind, a16, tile, dh, fold=True, part=part)
        ref3, bar3 = self._out(kind, self.y3[kind], self._bar_y(kind))
        r3, e3 = _worst(f'{tag} vs exact fold', got, ref3, bar3)
        # the uncorrected bar (no fp16-store term, |cs_n| on the constant rows): measured for the docstring, not asserted
        _, bar3u = self._out(kind, self.y3[kind], self._bar_y(kind, cs_form=True), stored_bar=False)
        r3u = float(((got - ref3).abs() / bar3u).max())
        print(f'[{tag}] comparison 3: ratio {r3:.3f} of the bar (max-abs {e3:.3e}); of the uncorrected bar {r3u:.3f}', flush=True)
        assert r3 < 1.0, (tag, r3, e3)
        true = self._out(kind, self.y_true[kind])
        bar2 = 8e-3 if kind == 'geglu' else 6e-3
        _, e_fold = _worst(f'{tag} vs true op', got, true, bar2)
        e_two = self.two_launch_error(kind, x, dh)
        print(f'[{tag}] comparison 2: fold {e_fold:.3e} two-launch {e_two:.3e} (bar {bar2:.0e}, 1.5 x + 5e-4'
              f'{"" if self.dist == "benign" else "; not asserted on this distribution"})', flush=True)
        if self.dist == 'benign':
            assert e_fold < bar2 and e_fold <= 1.5 * e_two + 5e-4, (tag, e_fold, e_two)
        self.unchanged(tag)
        return got


def _head_dims(C):
    return [dh for dh in HEAD_DIMS if C % dh == 0]


@pytest.mark.parametrize('B,ntok', ROWS, ids=[f'B{b}x{n}' for b, n in ROWS])
@pytest.mark.parametrize('C', WIDTHS)
def test_fold_at_the_dispatch_request(C, B, ntok):
    """every width x row shape x distribution: the three producers and every consumer as launch_igemm configures them by itself (tile -1)"""
    for dist in DISTS:
        s = _Stream(C, B, ntok, dist)
        x, a16, part = s.produce('f16', -1)
        xi, a16i, parti = s.produce('f16-inplace', -1)
        assert torch.equal(x, xi) and torch.equal(a16, a16i) and torch.equal(part, parti), f'{s.tag}: in place != out of place'
        s.prepare(x, a16, part)
        for dh in _head_dims(C):
            s.consume('heads', x, a16, part, dh=dh)
        s.consume('geglu', x, a16, part)
        s.consume('plain', x, a16, part)
        xs, a16s, parts = s.produce('split16', -1)              # proj_in's form feeds norm1 -> q | k | v
        s.prepare(xs, a16s, parts, kinds=('heads',))
        s.consume('heads', xs, a16s, parts, dh=_head_dims(C)[0], src='split16')


@pytest.mark.parametrize('B,ntok', [(2, 64), (1, 576)], ids=['B2x64', 'B1x576'])
@pytest.mark.parametrize('C', [320, 640, 1280])
def test_fold_with_every_tile_pinned(C, B, ntok):
    """npart 10 / 20 / 40 on the two fallback triggers (a 128- or 256-row tile straddles two samples of 64 rows; 576 rows and N = 320 are no
    multiples of 128 / 256): a pinned tile the launcher has to replace must still give correct partials and the gamma-scaled copy"""
    for dist in DISTS:
        s = _Stream(C, B, ntok, dist)
        for t in GENERIC:
            o = s.produce('f16', t, keep=False)
            i = s.produce('f16-inplace', t, keep=False)
            assert all(torch.equal(u, v) for u, v in zip(o, i)), f'{s.tag} tile{t}: in place != out of place'
        for t in SPLIT16_TILES:
            s.produce('split16', t, keep=False)
        x, a16, part = s.produce('f16', -1)
        s.prepare(x, a16, part)
        dh = 64 if C % 64 == 0 else _head_dims(C)[0]
        for t in GENERIC:
            s.consume('plain', x, a16, part, tile=t)
            s.consume('heads', x, a16, part, tile=t, dh=dh)
        for t in GEGLU_TILES:
            s.consume('geglu', x, a16, part, tile=t)


@pytest.mark.parametrize('C', WIDTHS)
def test_control_a_wrong_partial_is_seen_on_its_row_only(C):
    """{sum, sum of squares} of ONE row in the LAST block off by 1 % (outlier inputs: that block holds one of the four 40 x channels, a
    fifth of the row's sum of squares): comparison 3 must fail on that row and hold on every other.  At C > 640 the block is one of 20..39."""
    B, ntok = 2, 64
    s = _Stream(C, B, ntok, 'outlier')
    x, a16, part = s.produce('f16', -1)
    s.prepare(x, a16, part)
    # the row whose last block holds the largest share of its sum of squares (where the outlier channel drew its largest value): 1 % of
    # that share moves rstd by half as much, relative -- the most visible single partial of the case, so the control does not hang on
    # one random draw
    share = part[C // 32 - 1, :, 1] / part[..., 1].sum(0)
    row = int(share.argmax())
    bad = s.P.put('lnp_corrupt', part)
    bad[C // 32 - 1, row] *= 1.01
    s.stored.append((bad, bad.clone()))
    got = s._launch('plain', a16, -1, None, fold=True, part=bad)
    ref3, bar3 = s._out('plain', s.y3['plain'], s._bar_y('plain'))
    ratio = ((got - ref3).abs() / bar3).max(1).values
    others = float(torch.cat([ratio[:row], ratio[row + 1:]]).max())
    print(f'[C{C} wrong partial] row {row} (last block: {float(share[row]):.2f} of the sum of squares): ratio {float(ratio[row]):.2f}; '
          f'worst other row {others:.3f}', flush=True)
    assert float(ratio[row]) > 1.0, 'comparison 3 did not notice a partial that is off by 1 %'
    ratio[row] = 0
    assert float(ratio.max()) < 1.0
    s.unchanged(f'C{C} wrong partial')


@pytest.mark.parametrize('C', WIDTHS)
def test_control_missing_gamma_fails_the_true_operation(C):
    """column terms prepared with gamma = 1 (what a producer that lost f16_scale's partner would pair with): comparison 2 must fail"""
    B, ntok = 2, 64
    s = _Stream(C, B, ntok, 'benign')
    x, a16, part = s.produce('f16', -1)
    s.prepare(x, a16, part)
    W = s.W
    cs1, d1 = s.P.new('cs_gamma1', (C,), torch.float32), s.P.new('d_gamma1', (C,), torch.float32)
    K.ln_fold_prep(W.w['plain'], C, W.ones, W.beta, out=(cs1, d1))
    got = s._launch('plain', a16, -1, None, fold=True, part=part, cs=cs1, dn=d1)
    e_fold = float((got - s.y_true['plain']).abs().max())
    e_two = s.two_launch_error('plain', x, None)
    print(f'[C{C} missing gamma] fold {e_fold:.3e} two-launch {e_two:.3e}', flush=True)
    assert not (e_fold < 6e-3 and e_fold <= 1.5 * e_two + 5e-4), 'comparison 2 did not notice column terms without gamma'
    s.unchanged(f'C{C} missing gamma')
