"""What tools/record_fp32_ends_bits.py and tests/test_fp32_ends_bits_gpu.py share: the cases of tests/golden/fp32_ends_parent_bits.json, their
inputs and the one function that runs a case -- one definition, so that the recorder and the test cannot drift apart.

The fp32 "ends" of csrc/small.hip (output head, input conv, 1x1 quant convs, conv weight packers, GELUs) at small shapes on every edge of
their launch rules, through the public C entries.  A case is one row of CASES: a handful of launches whose return codes, refusal messages
and output bytes are hashed together.  An output buffer is filled with 0xFF bytes before the launch, so what a launch leaves unwritten (or a
refusal leaves untouched) is part of the digest too.

The inputs are a closed-form integer hash in numpy uint64 arithmetic: no library random generator, the same bytes on every machine."""
import hashlib
import os

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def hash_f32(n, seed, scale=1.0):
    """n fp32 values in [-scale, scale): h(i) = (i * 2654435761 + 40503 * seed) mod 2^32, two xor-shift / multiply rounds, / 2^31 - 1"""
    i = np.arange(int(n), dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(40503) * np.uint64(seed)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & M32
    h ^= h >> np.uint64(13)
    v = (h.astype(np.float64) / 2147483648.0 - 1.0).astype(np.float32)      # (a 32-bit integer / 2^31 is exact in fp64; one rounding to fp32)
    return v * np.float32(scale)


HEAD_COUT = (1, 3, 4, 5, 8, 9, 16, 17, 24, 32, 33, 127, 128)
CASES = {}
# output head, 4-pixel form (W % 4 == 0, aligned buffers): 1 x 4 puts every tap row partly out of the image; Cin 4 = one lane live, 256 = the
# first channel pass exactly full, 260 = one lane of the second pass, 512 = both passes full
for _n in HEAD_COUT:
    CASES[f'head4_cout{_n}'] = dict(kind='head', Cout=_n, Cin=(4, 256, 260, 512), HW=((1, 4), (3, 4), (2, 8)))
# ... and the 1-pixel form (W % 4 != 0); Cin 516 is past the 4-pixel form's 512 and, above 32 outputs, refused
for _n in HEAD_COUT:
    CASES[f'head1_cout{_n}'] = dict(kind='head', Cout=_n, Cin=(4, 260, 516), HW=((3, 5), (2, 6)))
CASES['head1_knob_cout_le8'] = dict(kind='head', Cout=(1, 3, 4, 5, 8), Cin=(4, 260, 516), HW=((3, 4),), env={'SDMI_CONV_OUT4': '0'})
# input conv: 320 outputs = two passes of the <= 16-channel form; 3 x 7 (B = 2: 42 pixels) ends in a partial block of 16 pixels
for _c in (1, 4, 16, 17, 63, 64):
    CASES[f'conv_in_cin{_c}'] = dict(kind='conv_in', Cin=_c, Cout=(255, 256, 320, 512), HW=((1, 2), (4, 4), (3, 7)))
for _c in (1, 16, 17, 32, 33, 65, 128):
    CASES[f'pointwise_cin{_c}'] = dict(kind='pointwise', Cin=_c, Cout=(1, 16, 17), HW=(1, 257), in_scale=(1.0, 1.0 / 0.18215))
CASES['pack_conv_weight_3x3'] = dict(kind='pack', entry='sdmi_k_pack_conv_weight', O=5, k=3, I=(64, 96, 128, 160))
CASES['pack_conv_weight_1x1'] = dict(kind='pack', entry='sdmi_k_pack_conv_weight', O=5, k=1, I=(4, 77, 768))
CASES['pack_conv_weight_src'] = dict(kind='pack', entry='sdmi_k_pack_conv_weight_src', O=5, k=3, split=((64, 32, 0), (96, 64, 32)))
CASES['pack_conv_split3'] = dict(kind='pack', entry='sdmi_k_pack_conv_split3', O=5, k=3, I=(64, 96))
CASES['pack_conv_out'] = dict(kind='pack', entry='sdmi_k_pack_conv_out', O=9, k=3, I=(20,))
for _e in ('sdmi_k_quick_gelu', 'sdmi_k_gelu_erf'):
    CASES[_e[7:]] = dict(kind='gelu', entry=_e, n=(4, 1028))


def case_seed(name):
    return 1 + sorted(CASES).index(name)


def _many(v):
    return v if isinstance(v, tuple) else (v,)


def head_entry(Cout):
    """the narrowest entry that takes Cout outputs"""
    return 'sdmi_k_conv_out' if Cout <= 16 else ('sdmi_k_conv_out32' if Cout <= 32 else 'sdmi_k_conv_out128')


def launches(name):
    """the launches of a case: (entry, {argument name: fp32 numpy array}, output shape, output dtype, call) with call(lib, ptrs, out_ptr,
    stream) -> rc.  The inputs of launch j come from seed 1000 * case_seed + 10 * j + argument index."""
    c, seed, out = CASES[name], 1000 * case_seed(name), []

    def add(entry, shapes, out_shape, out_dtype, call, scale=1.0):
        j = len(out)
        args = {k: hash_f32(int(np.prod(s)), seed + 10 * j + a, scale).reshape(s) for a, (k, s) in enumerate(shapes.items())}
        out.append((entry, args, out_shape, out_dtype, call))

    if c['kind'] == 'head':                    # h NHWC, w packed [Cout][3][3][Cin]
        for Cout in _many(c['Cout']):
            for Cin in c['Cin']:
                for H, W in c['HW']:
                    add(head_entry(Cout), dict(h=(2, H, W, Cin), w=(Cout, 3, 3, Cin), bias=(Cout,)), (2, Cout, H, W), np.float32,
                        lambda fn, p, o, s, H=H, W=W, Cin=Cin, Cout=Cout: fn(p['h'], p['w'], p['bias'], o, 2, H, W, Cin, Cout, s))
    elif c['kind'] == 'conv_in':               # x NCHW, w OIHW -> NHWC
        Cin = c['Cin']
        for Cout in c['Cout']:
            for H, W in c['HW']:
                add('sdmi_k_conv_in' if Cin <= 16 else 'sdmi_k_conv_in64', dict(x=(2, Cin, H, W), w=(Cout, Cin, 3, 3), bias=(Cout,)),
                    (2, H, W, Cout), np.float32,
                    lambda fn, p, o, s, H=H, W=W, Cout=Cout: fn(p['x'], p['w'], p['bias'], o, 2, Cin, H, W, Cout, s))
    elif c['kind'] == 'pointwise':
        Cin = c['Cin']
        for Cout in c['Cout']:
            for HW in c['HW']:
                for sc in c['in_scale']:
                    add('sdmi_k_pointwise_nchw' if Cin <= 32 else 'sdmi_k_pointwise_nchw128', dict(x=(2, Cin, HW), w=(Cout, Cin), bias=(Cout,)),
                        (2, Cout, HW), np.float32,
                        lambda fn, p, o, s, Cout=Cout, HW=HW, sc=sc: fn(p['x'], p['w'], p['bias'], o, 2, Cin, Cout, HW, sc, s))
    elif c['kind'] == 'pack':
        O, k, e = c['O'], c['k'], c['entry']
        for I in c.get('I', ()):
            if e == 'sdmi_k_pack_conv_out':
                add(e, dict(w=(O, I, 3, 3)), (O, 3, 3, I), np.float32, lambda fn, p, o, s, I=I: fn(p['w'], o, O, I, s))
            else:
                K = (3 if e == 'sdmi_k_pack_conv_split3' else 1) * I * k * k
                add(e, dict(w=(O, I, k, k)), (O, K), np.float16, lambda fn, p, o, s, I=I: fn(p['w'], o, O, I, k, k, s))
        for c0, c1, c2 in c.get('split', ()):
            I = c0 + c1 + c2
            add(e, dict(w=(O, I, k, k)), (O, I * k * k), np.float16,
                lambda fn, p, o, s, I=I, c0=c0, c1=c1, c2=c2: fn(p['w'], o, O, I, k, k, c0, c1, c2, s))
    else:                                      # gelu: inputs spanning [-6, 6)
        for n in c['n']:
            add(c['entry'], dict(x=(n,)), (n,), np.float16, lambda fn, p, o, s, n=n: fn(p['x'], o, n, s), scale=6.0)
    return out


def input_digest(name):
    h = hashlib.sha256()
    for _, args, _, _, _ in launches(name):
        for a in args.values():
            h.update(a.tobytes())
    return h.hexdigest()


def run_case(name):
    """run the case on the GPU through the loaded library -> SHA-256 over (rc, refusal message, output bytes) of its launches"""
    import torch
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    env = CASES[name].get('env', {})
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                     # (the knobs are read per launch)
    h = hashlib.sha256()
    try:
        for entry, args, out_shape, out_dtype, call in launches(name):
            dev = {k: torch.from_numpy(a).cuda() for k, a in args.items()}
            nbytes = int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize
            out = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device='cuda')
            rc = call(getattr(lib, entry), {k: t.data_ptr() for k, t in dev.items()}, out.data_ptr(), _lib.stream_ptr())
            torch.cuda.synchronize()
            h.update(str(int(rc)).encode())
            if rc != 0:
                h.update(lib.sdmi_last_error().split(b' -- ', 1)[-1])      # (the message, not the source text of the condition)
            h.update(out.cpu().numpy().tobytes())
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return h.hexdigest()
