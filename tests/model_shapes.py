"""A pure-Python walk of UNetModel.__init__ (ldm/modules/diffusionmodules/openaimodel.py:443-692) over the committed model configs.

It yields (1) every state_dict key with its shape and (2) every kernel launch site of the executor (csrc/unet.cpp) with its geometry:
GroupNorms, 3x3 convs, 1x1 skip convs, resample2, the transformer / legacy-attention GEMMs with their epilogue mode, attention, the
context K / V projection.  Launches whose output feeds GroupNorms carry the (cpg, cbase) statistics targets of their real consumers --
the next block's norm and, through the skip stack, the concat norm of an output block -- i.e. what FwdBase::attach_gn_targets attaches.
A ResBlock with a skip convolution also yields a 'conv2_tail' entry: conv2 as the executor launches it where it folds the skip convolution
into conv2's halo-staged launch (tail channels, passes, what excludes the block); folds() is the executor's decision restated over the
committed tuning table, and tests/test_model_shapes_host.py pins it against sdmi_unet_skip_fold_plan.
tests/test_model_shapes_host.py pins (1) against the recorded state_dict keys of the reference models, which makes (2) a derived fact
and not a hand-typed table; tests/test_model_shapes_gpu.py runs (2)."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# name -> (config, recorded state_dict keys or None, latent side of the product size, context tokens)
MODELS = {
    'cin': ('cin256_v2_config.json', 'cin_unet_state_dict_keys.json', 64, 1),
    'inpaint': ('inpainting_big_config.json', 'inpaint_unet_state_dict_keys.json', 128, 0),
    'laion': ('txt2img_1p4B_eval.json', None, 32, 77),
    # SD v1 and the tiny plan: the params are the oracle's own configs (oracle/plan.py, the ones tests/test_unet_gpu.py builds its models
    # from), not a file under golden/
    'sdv1': ('oracle.plan:SD_V1', None, 64, 77),
    'tiny': ('oracle.plan:TINY', None, 64, 77),
}
HALO_TILES = (14, 15, 16, 17)      # include/sdmi.h: the halo-staged 3x3 conv tiles, the only ones that run a 1x1 tail
PRECISE_1X1_MAX_DS = 4             # csrc/unet.h precise_1x1_max_ds_: stream 1x1 convs are three-pass split-fp16 below this downsample factor


def unet_params(name):
    cfg = MODELS[name][0]
    if cfg.startswith('oracle.plan:'):
        import oracle.plan
        return getattr(oracle.plan, cfg.split(':')[1]).ref_kwargs()
    with open(os.path.join(GOLDEN, cfg)) as f:
        return json.load(f)['model']['params']['unet_config']['params']


class Act:
    """an fp32 activation: `prod` is the launch whose epilogue can emit GroupNorm statistics for it (None: no such producer), FwdBase::make_act"""

    def __init__(self, C, hw, prod):
        self.C, self.hw, self.prod = C, hw, prod
        self.stats = prod is not None and (hw * hw) % 32 == 0 and hw * hw >= 1024 // C + 2 and C % 4 == 0 and C // 32 >= 2


def walk(p, latent, nctx):
    """-> (W: key -> shape, L: list of (kind, dict)); dicts of statistics-capable launches hold 'gn': [(cpg, cbase), ...]"""
    mc, mult, nrb, ar = p['model_channels'], p['channel_mult'], p['num_res_blocks'], p['attention_resolutions']
    st, heads, updown = p.get('use_spatial_transformer', False), p.get('num_heads', -1), p.get('resblock_updown', False)
    ctx, te = p.get('context_dim'), 4 * mc
    scale_shift = p.get('use_scale_shift_norm', False)
    W, L = {}, []

    def lin(k, o, i, b=True):
        W[k + '.weight'] = [o, i]
        if b:
            W[k + '.bias'] = [o]

    def conv(k, o, i, ks):
        W[k + '.weight'] = [o, i, ks, ks]
        W[k + '.bias'] = [o]

    def vec2(k, c):
        W[k + '.weight'] = [c]
        W[k + '.bias'] = [c]

    def launch(kind, **d):
        L.append((kind, d))
        return d

    def gn(srcs, hw):
        """GroupNorm32 over the channel concat of `srcs`; fused statistics iff every source has a statistics-capable producer (FwdBase::groupnorm)"""
        C = sum(a.C for a in srcs)
        launch('gn', C=C, c0=srcs[0].C, c1=C - srcs[0].C, hw=hw)
        if all(a.stats for a in srcs):
            cbase = 0
            for a in srcs:
                a.prod['gn'].append((C // 32, cbase))
                cbase += a.C

    def res(k, srcs, cout, ud=0, p3=False):
        cin, hw = sum(a.C for a in srcs), srcs[0].hw
        c0, c1 = srcs[0].C, cin - srcs[0].C
        vec2(k + '.in_layers.0', cin); conv(k + '.in_layers.2', cout, cin, 3); lin(k + '.emb_layers.1', cout, te)
        vec2(k + '.out_layers.0', cout); conv(k + '.out_layers.3', cout, cout, 3)
        hw2 = hw // 2 if ud == 1 else hw * 2 if ud == -1 else hw
        gn(srcs, hw)
        if ud:
            launch('resample', hw=hw, C=cin, dir=ud)
        launch('small_linear', K=te, N=cout)
        # p3: the last ResBlock, whose two 3x3 convs the executor runs as 3-pass split-fp16 products (Layer::precise3, csrc/unet.cpp)
        extra = dict(p3=True) if p3 else {}
        l1 = launch('conv3', role='conv1', c0=c0, c1=c1, N=cout, hin=hw2, hout=hw2, stride=1, up=0, gn=[], **extra)
        hact = Act(cout, hw2, l1)
        gn([hact], hw2)
        if cin != cout:
            conv(k + '.skip_connection', cout, cin, 1)
            launch('conv1x1', role='skip', K=cin, N=cout, hw=hw2)
        l2 = launch('conv3', role='conv2', c0=cout, c1=0, N=cout, hin=hw2, hout=hw2, stride=1, up=0, gn=[], **extra)
        if cin != cout:
            # conv2 with the skip convolution as its 1x1 tail (csrc/unet.cpp res_block): tail_c = cin channels, three passes where the layer's
            # p1x1 rule makes the 1x1 split-fp16 (ds < PRECISE_1X1_MAX_DS), the statistics targets of conv2 (the same list: filled later).
            # `excluded`: what keeps the executor from folding whatever the tuning table says -- the split-fp16 last block, scale-shift
            # blocks, a source that is no multiple of 64 channels, a map wider than skip_fold_max_w = 64.  Whether an admitted block folds is
            # the table's decision (folds()).
            why = [w for w, on in (('p3', p3), ('scale_shift', scale_shift), ('tail_c % 64', cin % 64 != 0), ('width > 64', hw2 > 64)) if on]
            launch('conv2_tail', N=cout, hw=hw2, tail_c=cin, passes=3 if ds < PRECISE_1X1_MAX_DS else 1, excluded='+'.join(why), gn=l2['gn'])
        return Act(cout, hw2, l2)

    def attn(k, x):
        c, hw = x.C, x.hw
        n = hw * hw
        vec2(k + '.norm', c)
        gn([x], hw)
        if st:
            d = c // heads
            conv(k + '.proj_in', c, c, 1); conv(k + '.proj_out', c, c, 1)
            t = k + '.transformer_blocks.0'
            for a, cd in (('attn1', c), ('attn2', ctx)):
                lin(t + f'.{a}.to_q', c, c, False); lin(t + f'.{a}.to_k', c, cd, False); lin(t + f'.{a}.to_v', c, cd, False)
                lin(t + f'.{a}.to_out.0', c, c)
            lin(t + '.ff.net.0.proj', 8 * c, c); lin(t + '.ff.net.2', c, 4 * c)
            for nm in ('norm1', 'norm2', 'norm3'):
                vec2(t + '.' + nm, c)
            launch('dense', role='proj_in', M=n, K=c, N=c, mode='plain')
            launch('dense', role='qkv', M=n, K=c, N=3 * c, mode='heads', heads=heads, dh=d)
            launch('attn', d=d, heads=heads, nq=n, nkv=n)
            launch('dense', role='attn_out', M=n, K=c, N=c, mode='plain')          # to_out.0 of attn1 / attn2: bias, residual in place
            launch('dense', role='to_q', M=n, K=c, N=c, mode='heads', heads=heads, dh=d)
            launch('kv', K=ctx, N=2 * c, heads=heads, dh=d, ntok=nctx)
            launch('attn', d=d, heads=heads, nq=n, nkv=nctx)
            launch('dense', role='geglu', M=n, K=c, N=8 * c, mode='geglu')
            launch('dense', role='ff2', M=n, K=4 * c, N=c, mode='plain')
        else:
            d = c // heads
            W[k + '.qkv.weight'] = [3 * c, c, 1]; W[k + '.qkv.bias'] = [3 * c]
            W[k + '.proj_out.weight'] = [c, c, 1]; W[k + '.proj_out.bias'] = [c]
            launch('dense', role='qkv_legacy', M=n, K=c, N=3 * c, mode='plain')
            launch('attn', d=d, heads=heads, nq=n, nkv=n)
        po = launch('dense', role='proj_out', M=n, K=c, N=c, mode='plain', gn=[])
        return Act(c, hw, po)

    lin('time_embed.0', te, mc); lin('time_embed.2', te, te)
    launch('timestep_embedding', dim=mc)
    launch('small_linear', K=mc, N=te)
    launch('small_linear', K=te, N=te)
    conv('input_blocks.0.0', mc, p['in_channels'], 3)
    # conv_in emits the statistics of its own output (csrc/unet.cpp: make_act(..., (H * W) % 16 == 0) and attach_gn_targets on its carrier):
    # the targets are input_blocks.1.0's norm and, through the skip stack, the (mc | mc) concat norm of the last output block
    h = Act(mc, latent, launch('conv_in', cin=p['in_channels'], N=mc, hw=latent, gn=[]) if (latent * latent) % 16 == 0 else None)
    hs, ch, ds, ib = [h], mc, 1, 1
    for lv, m in enumerate(mult):
        for _ in range(nrb):
            h = res(f'input_blocks.{ib}.0', [h], m * mc); ch = m * mc
            if ds in ar:
                h = attn(f'input_blocks.{ib}.1', h)
            hs.append(h); ib += 1
        if lv != len(mult) - 1:
            if updown:
                h = res(f'input_blocks.{ib}.0', [h], ch, ud=1)
            else:
                conv(f'input_blocks.{ib}.0.op', ch, ch, 3)
                h = Act(ch, h.hw // 2, launch('conv3', role='down', c0=ch, c1=0, N=ch, hin=h.hw, hout=h.hw // 2, stride=2, up=0, gn=[]))
            hs.append(h); ib += 1; ds *= 2
    h = res('middle_block.0', [h], ch); h = attn('middle_block.1', h); h = res('middle_block.2', [h], ch)
    ob = 0
    for lv, m in list(enumerate(mult))[::-1]:
        for i in range(nrb + 1):
            h = res(f'output_blocks.{ob}.0', [h, hs.pop()], m * mc, p3=(lv == 0 and i == nrb)); ch = m * mc; j = 1
            if ds in ar:
                h = attn(f'output_blocks.{ob}.{j}', h); j += 1
            if lv and i == nrb:
                if updown:
                    h = res(f'output_blocks.{ob}.{j}', [h], ch, ud=-1)
                else:
                    conv(f'output_blocks.{ob}.{j}.conv', ch, ch, 3)
                    h = Act(ch, h.hw * 2, launch('conv3', role='up', c0=ch, c1=0, N=ch, hin=h.hw, hout=h.hw * 2, stride=1, up=1, gn=[]))
                ds //= 2
            ob += 1
    vec2('out.0', ch); conv('out.2', p['out_channels'], mc, 3)
    gn([h], h.hw)
    launch('conv_out', cin=mc, N=p['out_channels'], hw=h.hw)
    return W, L


def model_walk(name, latent=None):
    _, _, lat, nctx = MODELS[name]
    return walk(unet_params(name), lat if latent is None else latent, nctx)


def tune_lookup(M, N, Kd, ksize, up, kt=0):
    """the committed tuning table's (tile, split-K) for the executor's request (stride 1, plain mode, split-K 0) of a conv, or None
    (sdmi_tune_lookup: host arithmetic, no GPU)"""
    import ctypes as C
    from stable_diffusion_amd import _lib
    t, s = C.c_int(-1), C.c_int(-1)
    rc = _lib.load().sdmi_tune_lookup(M, N, Kd, ksize, 1, up, 0, 0, kt, C.byref(t), C.byref(s))
    return (t.value, s.value) if rc == 0 else None


def folds(d, B):
    """the walk's fold decision for a 'conv2_tail' entry at batch B: not excluded, and the table's row for conv2 with that tail (the row keyed
    with the tail's K where there is one, else the plain conv's) is a halo-staged tile"""
    if d['excluded']:
        return False
    row = tune_lookup(B * d['hw'] ** 2, d['N'], 9 * d['N'], 3, 0, d['passes'] * d['tail_c'])
    return row is not None and row[0] in HALO_TILES


def _freeze(d):
    return tuple(sorted((k, tuple(sorted(set(v))) if isinstance(v, list) else v) for k, v in d.items()))


def distinct(name, kinds=None):
    """the distinct launch geometries of a model at its product size, in first-appearance order: [(kind, dict)].  ('conv2_tail' is another
    form of a conv2 + skip pair already listed, not one more launch: it is returned only when asked for by kind.)"""
    seen, out = set(), []
    for kind, d in model_walk(name)[1]:
        if (kinds is not None and kind not in kinds) or (kinds is None and kind == 'conv2_tail'):
            continue
        key = (kind, _freeze(d))
        if key not in seen:
            seen.add(key)
            e = dict(d)
            if 'gn' in e:
                e['gn'] = sorted(set(e['gn']))
            out.append((kind, e))
    return out


def case_id(kind, d):
    s = kind + ''.join(f'-{k}{v}' for k, v in d.items() if k != 'gn')
    if d.get('gn'):
        s += '-gn' + '+'.join(f'{c}@{b}' for c, b in d['gn'])
    return s
