"""A pure-Python walk of the first stage's Encoder.__init__ / Decoder.__init__ (ldm/modules/diffusionmodules/model.py:368-425, 462-526, with
the quant convs and the codebook of ldm/models/autoencoder.py) over the committed first-stage configs.

It yields (1) every state_dict key with its shape and (2) every kernel launch site of the mixed-precision executor (csrc/vae.cpp, Vae::decode /
Vae::encode with SDMI_PRECISION_MIXED) with its geometry and epilogue role, per image: the test that runs them chooses the batch.
tests/test_first_stage_shapes_host.py pins (1) against the recorded state_dict keys of the reference first stages, which makes (2) a derived
fact and not a hand-typed table; tests/test_first_stage_shapes_gpu.py runs (2).

Launch kinds and what their dicts hold (`hw` is a map side, maps are square here):
  pointwise     post_quant_conv / quant_conv on NCHW fp32: cin, N, hw, in_scale (the latent's 1 / scale_factor folded into the launch)
  vq_quantize   nearest codebook row: n_embed, D, hw
  conv_in       3x3 fp32 NCHW -> NHWC: cin, N, hw
  gn            GroupNorm(32, eps 1e-6): C, hw, silu, outs = which of f16 / f32 / raw / raw_lo are written
  conv3         3x3 implicit GEMM on the fp16 GroupNorm output: role conv1 (bias) / conv2 (bias + residual) / up (nearest x2 folded, bias) /
                down (stride 2, zero pad right and bottom only: asym_pad), C, N, hin, hout, stride, up, asym_pad; splitk 0 (the heuristic)
  nin           nin_shortcut as the split-fp16 GEMM (raw hi | lo against [w_hi | w_hi | w_lo]): K, N, hw; bias; splitk 0
  cast          the fp16 copy of the stream in front of a resampling conv: C, hw
  dense         the attention block's GEMMs, role q / k (fp16 out, bias), vt (v^T = Wv xn_b^T per image: the weights are the A operand, the
                activation is `w`, ldo = ntok), scores (fp32 S = q_chunk k^T, `w` = k, ldo = ntok), pv (P v^T, K = ntok, the V bias, fp16 out),
                proj_out (bias + residual, fp32 out): M, K, N, ldo, splitk, out ('f16' / 'f32'), bias, resid, per_image (launched once per
                image, M rows are not multiplied by the batch), and for scores / pv the chunk (r0, rows)
  softmax       softmax_rows on one chunk: rows, cols, r0
  conv_out      3x3 fp32 NHWC -> NCHW: cin, N, hw"""
import json
import math
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
QC_MAX = 2048        # query rows per chunk (VFwd::attn_block)

# name -> (config, recorded state_dict keys or None, latent side of the product size)
MODELS = {
    'kl_f8': ('txt2img_1p4B_eval.json', None, 64),
    'vq_f4': ('cin256_v2_config.json', 'cin_vq_state_dict_keys.json', 64),
    'vq_f4_noattn': ('inpainting_big_config.json', 'inpaint_vq_state_dict_keys.json', 64),
}


def first_stage_params(name):
    with open(os.path.join(GOLDEN, MODELS[name][0])) as f:
        return json.load(f)['model']['params']['first_stage_config']['params']


def recorded_keys(name):
    with open(os.path.join(GOLDEN, MODELS[name][1])) as f:
        return json.load(f)['keys']


def chunks(ntok):
    """the query chunks (r0, rows) of one image"""
    qc = min(ntok, QC_MAX)
    return [(r0, min(qc, ntok - r0)) for r0 in range(0, ntok, qc)]


def walk(p, latent):
    """p: the params of a first_stage_config (embed_dim, optional n_embed, ddconfig) -> (W: key -> shape, dec: launches of a decode of a
    `latent`-sided code, enc: launches of the encode that produces one); launches are (kind, dict)"""
    dd = p['ddconfig']
    ch, mult, nrb, zc, ed = dd['ch'], dd['ch_mult'], dd['num_res_blocks'], dd['z_channels'], p['embed_dim']
    n_embed = p.get('n_embed', 0)
    mid_attn = dd.get('attn_type', 'vanilla') != 'none'
    enc_zc = 2 * zc if dd['double_z'] else zc
    enc_ed = 2 * ed if dd['double_z'] else ed
    assert not dd['attn_resolutions']          # the executor has the mid-block attention only
    n = len(mult)
    W = {}

    def conv(k, o, i, ks):
        W[k + '.weight'] = [o, i, ks, ks]
        W[k + '.bias'] = [o]

    def norm(k, c):
        W[k + '.weight'] = [c]
        W[k + '.bias'] = [c]

    def res(L, k, ci, co, hw):
        norm(k + '.norm1', ci); conv(k + '.conv1', co, ci, 3); norm(k + '.norm2', co); conv(k + '.conv2', co, co, 3)
        nin = ci != co
        L.append(('gn', dict(C=ci, hw=hw, silu=1, outs=('f16', 'raw', 'raw_lo') if nin else ('f16',))))
        L.append(('conv3', dict(role='conv1', C=ci, N=co, hin=hw, hout=hw, stride=1, up=0, asym_pad=0)))
        if nin:
            conv(k + '.nin_shortcut', co, ci, 1)
            L.append(('nin', dict(K=ci, N=co, hw=hw)))
        L.append(('gn', dict(C=co, hw=hw, silu=1, outs=('f16',))))
        L.append(('conv3', dict(role='conv2', C=co, N=co, hin=hw, hout=hw, stride=1, up=0, asym_pad=0)))

    def attn(L, k, c, hw):
        if not mid_attn:          # attn_type 'none': make_attn returns nn.Identity, no parameters and no launch
            return
        norm(k + '.norm', c)
        for nm in ('q', 'k', 'v', 'proj_out'):
            conv(f'{k}.{nm}', c, c, 1)
        nt = hw * hw
        L.append(('gn', dict(C=c, hw=hw, silu=0, outs=('f16',))))
        for role in ('q', 'k'):
            L.append(('dense', dict(role=role, M=nt, K=c, N=c, ldo=c, splitk=1, out='f16', bias=True, resid=False, per_image=False)))
        L.append(('dense', dict(role='vt', M=c, K=c, N=nt, ldo=nt, splitk=1, out='f16', bias=False, resid=False, per_image=True)))
        for r0, rows in chunks(nt):
            L.append(('dense', dict(role='scores', M=rows, K=c, N=nt, ldo=nt, splitk=1, out='f32', bias=False, resid=False, per_image=True,
                                    r0=r0)))
            L.append(('softmax', dict(rows=rows, cols=nt, r0=r0)))
            L.append(('dense', dict(role='pv', M=rows, K=nt, N=c, ldo=c, splitk=1, out='f16', bias=True, resid=False, per_image=True, r0=r0)))
        L.append(('dense', dict(role='proj_out', M=nt, K=c, N=c, ldo=c, splitk=0, out='f32', bias=True, resid=True, per_image=False)))

    def resample(L, k, c, hw, up):
        conv(k + '.conv', c, c, 3)
        L.append(('cast', dict(C=c, hw=hw)))
        if up:
            L.append(('conv3', dict(role='up', C=c, N=c, hin=hw, hout=2 * hw, stride=1, up=1, asym_pad=0)))
        else:
            L.append(('conv3', dict(role='down', C=c, N=c, hin=hw, hout=hw // 2, stride=2, up=0, asym_pad=1)))

    # ---- encoder (model.py:368-425), then quant_conv ----
    enc = []
    hw = latent * 2 ** (n - 1)
    conv('encoder.conv_in', ch, dd['in_channels'], 3)
    enc.append(('conv_in', dict(cin=dd['in_channels'], N=ch, hw=hw)))
    bi = ch
    for lvl in range(n):
        bo = ch * mult[lvl]
        for i in range(nrb):
            res(enc, f'encoder.down.{lvl}.block.{i}', bi, bo, hw)
            bi = bo
        if lvl != n - 1:
            resample(enc, f'encoder.down.{lvl}.downsample', bi, hw, False)
            hw //= 2
    res(enc, 'encoder.mid.block_1', bi, bi, hw); attn(enc, 'encoder.mid.attn_1', bi, hw); res(enc, 'encoder.mid.block_2', bi, bi, hw)
    norm('encoder.norm_out', bi); conv('encoder.conv_out', enc_zc, bi, 3)
    enc.append(('gn', dict(C=bi, hw=hw, silu=1, outs=('f32',))))
    enc.append(('conv_out', dict(cin=bi, N=enc_zc, hw=hw)))
    conv('quant_conv', enc_ed, enc_zc, 1)
    enc.append(('pointwise', dict(cin=enc_zc, N=enc_ed, hw=hw, in_scale=False)))
    assert hw == latent

    # ---- the codebook, post_quant_conv, decoder (model.py:462-526) ----
    dec = []
    if n_embed:
        W['quantize.embedding.weight'] = [n_embed, ed]
        dec.append(('vq_quantize', dict(n_embed=n_embed, D=ed, hw=latent)))
    conv('post_quant_conv', zc, ed, 1)
    dec.append(('pointwise', dict(cin=ed, N=zc, hw=latent, in_scale=not n_embed)))       # (Vae::decode: the scale goes into the quantizer if there is one)
    bi = ch * mult[n - 1]
    hw = latent
    conv('decoder.conv_in', bi, zc, 3)
    dec.append(('conv_in', dict(cin=zc, N=bi, hw=hw)))
    res(dec, 'decoder.mid.block_1', bi, bi, hw); attn(dec, 'decoder.mid.attn_1', bi, hw); res(dec, 'decoder.mid.block_2', bi, bi, hw)
    for lvl in reversed(range(n)):
        bo = ch * mult[lvl]
        for i in range(nrb + 1):
            res(dec, f'decoder.up.{lvl}.block.{i}', bi, bo, hw)
            bi = bo
        if lvl != 0:
            resample(dec, f'decoder.up.{lvl}.upsample', bi, hw, True)
            hw *= 2
    norm('decoder.norm_out', bi); conv('decoder.conv_out', dd['out_ch'], bi, 3)
    dec.append(('gn', dict(C=bi, hw=hw, silu=1, outs=('f32',))))
    dec.append(('conv_out', dict(cin=bi, N=dd['out_ch'], hw=hw)))
    return W, dec, enc


def model_walk(name):
    return walk(first_stage_params(name), MODELS[name][2])


def _freeze(d):
    return tuple(sorted(d.items()))


def distinct(names=None, kinds=None):
    """the distinct launch geometries of the named first stages (all three by default) at their product sizes, decode then encode, in
    first-appearance order: [(kind, dict)]"""
    seen, out = set(), []
    for name in (names or MODELS):
        _, dec, enc = model_walk(name)
        for kind, d in dec + enc:
            if kinds is not None and kind not in kinds:
                continue
            key = (kind, _freeze(d))
            if key not in seen:
                seen.add(key)
                out.append((kind, dict(d)))
    return out


def case_id(kind, d):
    return kind + ''.join(f'-{k}{"+".join(v) if isinstance(v, tuple) else v}' for k, v in d.items())


# ---- an fp64 restatement of the decoder, with the mixed path's fp16 operand roundings and with planted attention defects -----------------
# (torch is imported inside: the walk above needs none.  NHWC, convolutions as nine shifted matmuls -- no library convolution -- so the same
# code runs on the CPU and on the device.)
PEAKED = {'decoder.mid.attn_1.q.weight': 2.0, 'decoder.mid.attn_1.k.weight': 2.0, 'decoder.mid.attn_1.v.bias': 25.0}
ATTN_MUTANTS = ('tail', 'nobias', 'flush')
FLUSH_BELOW = 5e-4


def peaked_state_dict(cfg, seed):
    """oracle.vae_ref's synthetic decoder weights with the mid attention's q / k weights doubled (scores x 4: a peaked softmax) and its V bias
    x 25 (so that the bias added behind P v carries weight in the image)"""
    from oracle import vae_ref
    sd = vae_ref.make_vae_state_dict(cfg, seed)
    for k, f in PEAKED.items():
        sd[k] = sd[k] * f
    return sd


def decode64(sd, cfg, z, r16=False, mutant=None, info=None):
    """AutoencoderKL.decode in fp64: z [B, embed_dim, h, w] -> image [B, out_ch, H, W] (float64, on z's device).
    r16: the fp16-operand floor of the mixed executor -- every operand csrc/vae.cpp rounds to fp16 is rounded once: activations and weights of
    the 3x3 convs on the stream (ResnetBlock convs, Upsample conv) and of q / k / v / proj_out, the stored q, k, v^T, P and attention output;
    post_quant_conv, conv_in, nin_shortcut (split-fp16) and conv_out stay exact.
    mutant: one defect of the attention block -- `tail`: the rows of a last query chunk shorter than QC_MAX take their neighbour row's weights
    (row r gets row r - 1's); `nobias`: the V bias is dropped; `flush`: weights below FLUSH_BELOW become 0.
    info: a dict that receives the softmax's row maxima (`rowmax` [B, N])."""
    import torch
    assert mutant is None or mutant in ATTN_MUTANTS
    dev = z.device
    P = {k: v.to(dev).double() for k, v in sd.items()}
    R = (lambda t: t.half().double()) if r16 else (lambda t: t)

    def gn(p, x, silu):
        B, H, W, C = x.shape
        g = x.reshape(B, H * W, 32, C // 32)
        mean = g.mean((1, 3), keepdim=True)
        var = ((g - mean) ** 2).mean((1, 3), keepdim=True)
        y = ((g - mean) / torch.sqrt(var + 1e-6)).reshape(B, H, W, C) * P[p + '.weight'] + P[p + '.bias']
        return y * torch.sigmoid(y) if silu else y

    def conv3(p, x, rounded):
        w = P[p + '.weight']
        if rounded:
            x, w = R(x), R(w)
        B, H, W, C = x.shape
        xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
        out = torch.zeros((B, H, W, w.shape[0]), dtype=torch.float64, device=dev)
        for ky in range(3):
            for kx in range(3):
                out += xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
        return out + P[p + '.bias']

    def lin(p, x, rounded, bias=True):
        w = P[p + '.weight'].reshape(P[p + '.weight'].shape[0], -1)
        if rounded:
            x, w = R(x), R(w)
        y = x @ w.t()
        return y + P[p + '.bias'] if bias else y

    def res(p, x):
        h = conv3(p + '.conv1', gn(p + '.norm1', x, True), True)
        h = conv3(p + '.conv2', gn(p + '.norm2', h, True), True)
        if p + '.nin_shortcut.weight' in P:
            x = lin(p + '.nin_shortcut', x, False)
        return x + h

    def attn(p, x):
        B, H, W, C = x.shape
        N = H * W
        a = gn(p + '.norm', x, False).reshape(B, N, C)
        q, k = R(lin(p + '.q', a, True)), R(lin(p + '.k', a, True))
        v = R(lin(p + '.v', a, True, bias=False))
        w_ = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=2)
        if info is not None:
            info['rowmax'] = w_.max(dim=2).values
        r0, rows = chunks(N)[-1]
        if mutant == 'tail' and rows < min(N, QC_MAX):
            w_ = torch.cat([w_[:, :r0], w_[:, r0 - 1:N - 1]], dim=1)
        if mutant == 'flush':
            w_ = torch.where(w_ < FLUSH_BELOW, torch.zeros_like(w_), w_)
        ao = R(w_) @ v
        if mutant != 'nobias':
            ao = ao + P[p + '.v.bias']
        return x + lin(p + '.proj_out', R(ao), True).reshape(B, H, W, C)

    zc = z.double().permute(0, 2, 3, 1)
    h = lin('post_quant_conv', zc, False)
    h = conv3('decoder.conv_in', h, False)
    h = res('decoder.mid.block_1', h); h = attn('decoder.mid.attn_1', h); h = res('decoder.mid.block_2', h)
    for lvl in reversed(range(len(cfg.ch_mult))):
        for i in range(cfg.num_res_blocks + 1):
            h = res(f'decoder.up.{lvl}.block.{i}', h)
        if lvl != 0:
            h = h.repeat_interleave(2, 1).repeat_interleave(2, 2)
            h = conv3(f'decoder.up.{lvl}.upsample.conv', h, True)
    return conv3('decoder.conv_out', gn('decoder.norm_out', h, True), False).permute(0, 3, 1, 2)


# ---- the materialised attention chain on probe operands (tests/attn_probes.py) -------------------------------------------------------------
# (ntok, the chunks launched): the smallest shapes that reach each code path of S = q k^T, softmax_rows (256 threads x 4 columns = 1024 columns
# per pass) and P v^T, each chunk at its row offset r0 as VFwd::attn_block launches it
CHAIN_SHAPES = [
    (64, chunks(64)),                # one partial pass of the 1024-column loop
    (192, chunks(192)),              # no multiple of a 128-wide tile
    (576, chunks(576)),
    (1024, chunks(1024)),            # exactly one pass
    (1088, chunks(1088)),            # a second pass with 16 active lanes
    (2304, chunks(2304)),            # a 48 x 48 latent: one chunk of 2048 rows and a tail of 256
    (4096, chunks(4096)),            # a 64 x 64 latent: two full chunks
    (9216, chunks(9216)[-1:]),       # the last chunk of a 768 x 768 decode: 1024 rows at r0 = 8192
]
CHAIN_C = (512, 128)                 # the mid width of the three product first stages, and of the tiny one
R_CHAIN = 2.0 ** -9                  # attn_probes.R_MIXED: P, the fp32 sum's reciprocal applied before the rounding, the stored output, one spare
SOFTMAX_REL, SOFTMAX_ABS = 2.0 ** -10, 2.0 ** -24
# a NORMALISED weight stored as fp16 is off by at most 2^-25 below 2^-14 (half the subnormal spacing): attn_probes.tolerance / .live with
# rowmax = 1 / 2 are exactly  R ref + 2^-25 n_c + 2^-24  and  2^-9 ref > 8 (2^-25 n_c + 2^-24)
CHAIN_ROWMAX = 0.5


def must_be_live(coding, ntok):
    """Whether the liveness rule (every row has a live output, >= 10 % of the non-empty outputs are live) is asserted for a coding.  A `window`
    coding puts ONE key into a column, so its outputs are single weights, and a single normalised weight is live only above 8 (2^-25 + 2^-24)
    2^9 = 1.5 x 2^-12 = 3.7e-4.  Windows exist under `diffuse` and `negative` only, where the scaled scores are N(0, 1) (unit-variance
    operands, scale d^-1/2; `negative` shifts every key alike), so a weight is exp(x) / (ntok e^1/2) with x ~ N(0, 1) and the live share is
    Phi(-ln(1.5 x 2^-12 ntok e^1/2)): 18.3 % at 4096 keys, 4.3 % at 9216 (the restatement's weights give 17.8 .. 18.6 % and 4.1 .. 4.4 %).
    The rule is asserted while that prediction is at least 10 %, i.e. up to 5900 keys; beyond, fp16 itself stores most single weights as
    subnormals and no kernel decides that.  Those cases still run and are held to the bar and to exact zeros; their share is printed."""
    if not coding.startswith('window'):
        return True
    x = math.log(1.5 * 2.0 ** -12 * ntok * math.exp(0.5))
    return 0.5 * math.erfc(x / math.sqrt(2.0)) >= 0.10


def chain_seed(C, ntok, regime_index):
    return 7001 * C + 13 * ntok + 100003 * regime_index


def softmax_tol(ref):
    """softmax_rows stores fp16(exp * inv): 2^-11 relative above 2^-14, 2^-25 absolute below; the fp32 exp, sum and reciprocal add relative
    terms of order |argument| 2^-24, at most 5e-6.  Twice the fp16 rounding and nothing else."""
    return SOFTMAX_REL * ref + SOFTMAX_ABS


def chain_restate(q, k, v, bias, scale):
    """The chain's arithmetic in plain torch: fp16 q / k, fp32 scores, softmax_rows_kernel's order (row maximum of the raw scores times the
    scale, exp(s scale - max), the fp32 sum, one reciprocal), P rounded to fp16 AFTER the normalisation, fp32 accumulation of P v, the bias,
    the fp16 output.  q [rows, C], k, v [ntok, C] fp16, bias [C] fp32 -> (P fp16 [rows, ntok], out fp16 [rows, C])"""
    import torch
    s = q.float() @ k.float().t()
    sc = torch.tensor(scale, dtype=torch.float32)
    mx = s.max(dim=1, keepdim=True).values * sc
    e = torch.exp(s * sc - mx)
    inv = 1.0 / e.sum(dim=1, keepdim=True)
    p16 = (e * inv).half()
    return p16, (p16.float() @ v.float() + bias.float()).half()


def chain_judge(got, P, col, d):
    """got [rows, d] (float64) against the fp64 weights P [rows, ntok] coded by `col`: worst err / tol, the live share among the non-empty
    outputs, whether every row has a live output, whether the empty outputs are exactly 0 (as attn_probes.judge, with the floor terms of
    normalised weights)"""
    import torch
    import attn_probes as A
    ref = A.coded(P[None], col, d)[0]
    n_c = A.key_counts(col, 1, P.shape[0], d, False, P.device)[0]
    tol = A.tolerance(ref, CHAIN_ROWMAX, n_c, R_CHAIN)
    err = (got - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / tol, torch.full_like(err, float('inf')))
    full = n_c > 0
    lv = A.live(ref, CHAIN_ROWMAX, n_c) & full
    return dict(worst=float(ratio.max()), at=int(ratio.flatten().argmax()), share=float(lv.sum()) / max(1, int(full.sum())),
                rows_live=bool(lv.any(dim=-1)[full.any(dim=-1)].all()), zeros_exact=bool((got[~full] == 0).all()))
