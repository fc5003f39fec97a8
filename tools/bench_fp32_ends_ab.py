"""Time the fp32 ends (csrc/small.hip) of two builds of libsdmi against each other on one MI355X, in one process.

    SDMI_LIB_OUT=libsdmi_parent.so python stable-diffusion_amd/build.py        # at the commit to compare with
    python tools/bench_fp32_ends_ab.py --parent stable-diffusion_amd/libsdmi_parent.so [--new stable-diffusion_amd/libsdmi.so]
                                       [--rounds 40] [--iters 50] [--repeats 3] [--out profiles/fp32_ends_refactor_ab.txt]

Three libraries are loaded side by side: the parent, a byte copy of the parent, and the new one.  Per launch they alternate, `rounds` times
`iters` back-to-back calls between two device events after a warm-up of every library; the median round -- and that `repeats` times.  The
first table is the parent against its own copy: the spread of this way of measuring, per launch the largest of |copy / parent - 1| over
the repeats and of the parent's own drift between repeats.  The second is the new library against the parent (the median of the repeats'
ratios); a launch passes if its difference is within the spread measured for it.  Warm caches (the same buffers every call),
launch-to-launch time including the launch gap.

Launches: the UNet `out` head (B = 2, 64 x 64, 320 -> 4), KL-f8's decoder.conv_out (512 x 512, 128 -> 3), the 16-output head (B = 2,
48 x 48, 448 -> 16), the wide ends at KL-f32's shapes (tools/bench_first_stages.py: B = 2, 16 x 16), conv_in (B = 2, 64 x 64, 4 -> 320)."""
import argparse
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, I, F = C.c_void_p, C.c_int, C.c_float
CONV = [P, P, P, P, I, I, I, I, I, P]
SIGS = {'sdmi_k_conv_in': CONV, 'sdmi_k_conv_in64': CONV, 'sdmi_k_conv_out': CONV, 'sdmi_k_conv_out128': CONV,
        'sdmi_k_pointwise_nchw128': [P, P, P, P, I, I, I, I, F, P], 'sdmi_k_pack_conv_out': [P, P, I, I, P]}


def load(path):
    lib = C.CDLL(path)
    for name, args in SIGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True)
    ap.add_argument('--new', default=os.path.join(ROOT, 'stable-diffusion_amd', 'libsdmi.so'))
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    copy = shutil.copy(args.parent, os.path.join(tmp, 'libsdmi_parent_copy.so'))
    libs = [load(os.path.abspath(p)) for p in (args.parent, copy, args.new)]
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=g)
    cases = []

    def head(name, entry, B, H, W, Cin, Cout):
        h, w, b = rnd(B, H, W, Cin), rnd(Cout, Cin, 3, 3) / (9 * Cin) ** 0.5, rnd(Cout)
        wp, o = torch.empty(Cout, 3, 3, Cin, device='cuda'), torch.empty(B, Cout, H, W, device='cuda')
        assert libs[0].sdmi_k_pack_conv_out(w.data_ptr(), wp.data_ptr(), Cout, Cin, s) == 0
        cases.append((name, o, lambda lib: getattr(lib, entry)(h.data_ptr(), wp.data_ptr(), b.data_ptr(), o.data_ptr(), B, H, W, Cin, Cout, s), (h, wp, b)))

    def conv_in(name, entry, B, H, W, Cin, Cout):
        x, w, b = rnd(B, Cin, H, W), rnd(Cout, Cin, 3, 3) / (9 * Cin) ** 0.5, rnd(Cout)
        o = torch.empty(B, H, W, Cout, device='cuda')
        cases.append((name, o, lambda lib: getattr(lib, entry)(x.data_ptr(), w.data_ptr(), b.data_ptr(), o.data_ptr(), B, Cin, H, W, Cout, s), (x, w, b)))

    def pointwise(name, B, HW, c):
        x, w, b = rnd(B, c, HW), rnd(c, c) / c ** 0.5, rnd(c)
        o = torch.empty(B, c, HW, device='cuda')
        cases.append((name, o, lambda lib: lib.sdmi_k_pointwise_nchw128(x.data_ptr(), w.data_ptr(), b.data_ptr(), o.data_ptr(), B, c, c, HW, 1.0, s), (x, w, b)))

    head('UNet out head B2 64x64 320->4', 'sdmi_k_conv_out', 2, 64, 64, 320, 4)
    head('KL-f8 decoder.conv_out 512x512 128->3', 'sdmi_k_conv_out', 1, 512, 512, 128, 3)
    head('16-output head B2 48x48 448->16', 'sdmi_k_conv_out', 2, 48, 48, 448, 16)
    conv_in('conv_in64 B2 16x16 64->512', 'sdmi_k_conv_in64', 2, 16, 16, 64, 512)
    head('conv_out128 B2 16x16 512->128', 'sdmi_k_conv_out128', 2, 16, 16, 512, 128)
    pointwise('pointwise128 B2 16x16 128->128', 2, 256, 128)
    pointwise('pointwise128 B2 16x16 64->64', 2, 256, 64)
    conv_in('conv_in B2 64x64 4->320', 'sdmi_k_conv_in', 2, 64, 64, 4, 320)

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    rows = []
    for name, o, call, _keep in cases:
        outs = []
        for lib in libs:                       # warm-up, and the three libraries must agree bit for bit
            for _ in range(20):
                assert call(lib) == 0, name
            torch.cuda.synchronize()
            outs.append(o.clone())
        same = torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        meds = []                              # per repeat: the median round of (parent, copy, new)
        for _ in range(args.repeats):
            acc = [[] for _ in libs]
            for _ in range(args.rounds):
                for lib, a in zip(libs, acc):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        call(lib)
                    e1.record()
                    torch.cuda.synchronize()
                    a.append(1e3 * e0.elapsed_time(e1) / args.iters)
            meds.append([statistics.median(a) for a in acc])
        parent = [m[0] for m in meds]
        spread = max(max(abs(m[1] / m[0] - 1) for m in meds), max(parent) / min(parent) - 1)
        rows.append((name, meds, spread, statistics.median(m[2] / m[0] for m in meds), same))
    fmt = lambda xs: ' '.join(f'{x:7.2f}' for x in xs)
    say(f'# {torch.cuda.get_device_name(0)}; us per call, median of {args.rounds} rounds x {args.iters} calls, {args.repeats} repeats; parent, its copy '
        'and the new library alternate')
    say('# (1) the spread: the parent against a byte copy of itself')
    say(f'# {"launch":40s} {"parent (per repeat)":>24s} {"parent copy":>24s}  spread')
    for name, meds, spread, _, _ in rows:
        say(f'{name:42s} {fmt(m[0] for m in meds):>24s} {fmt(m[1] for m in meds):>24s}  {100 * spread:5.2f} %')
    say('# (2) the new library against the parent')
    say(f'# {"launch":40s} {"parent (per repeat)":>24s} {"new":>24s}  new/parent  same bits  within the spread')
    for name, meds, spread, ratio, same in rows:
        say(f'{name:42s} {fmt(m[0] for m in meds):>24s} {fmt(m[2] for m in meds):>24s}  {100 * (ratio - 1):+6.2f} %   {"yes" if same else "NO":9s}'
            f'  {"yes" if abs(ratio - 1) <= spread else "NO"}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
