"""In-situ tuning of the implicit-GEMM tile / split-K choice on the MI355X (writes stable-diffusion_amd/tune_gfx950.txt).

    python tools/tune.py [--out PATH] [--rounds 64] [--reps 2] [--workloads unet64,unet96,...] [--append-new]

Every auto-configured GEMM launch of the real executors (UNet, first stage, text encoder) runs candidate
(round mod #candidates) of its shape while the library times it with HIP events on the launch stream
(sdmi_tune_begin / _round / _end, include/sdmi.h).  A candidate is therefore measured inside the real call: weights cold
in HBM (1.7 GB of them stream through per UNet call), activations warm from the producing kernel -- the conditions a
stand-alone sweep of one shape does not reproduce.  The resulting table is committed, so the choice (and with it the
split-K summation order, i.e. the exact output bits) is fixed.

--append-new: the table at --out keeps every row it has; only shapes whose key is not in it yet are appended (a model added
later brings its own shapes and changes no other model's tiles): `--workloads churches32b8,churches32b2 --append-new`,
`--workloads faces64b8,faces64b2,bsr64b8,bsr64b2 --append-new`, `--workloads bsr128b8,bsr128b1 --append-new` (bsr_sr's 128 x 128
windows, nine of them as 8 + 1 rows; profiles/tune_candidates_bsr128.txt).

The 2x2 phase convs of the Upsample convs (key ksize 2) are a family of their own, measured in a run restricted to it -- the executors take
the phase form during a collection only then -- and kept in tune_up_phase_gfx950.txt beside the table:
`SDMI_TUNE_ONLY_KSIZE=2 python tools/tune.py --workloads unet64,unet96,vaedec64,vaedec96 --append-new` (the shapes of the three bench
workloads and the first stage; profiles/tune_candidates_up_phase.txt).
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'stable-diffusion_amd', 'tune_gfx950.txt'))
    ap.add_argument('--dump', default=None, help='also write the per-candidate timings here')
    ap.add_argument('--rounds', type=int, default=72)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--workloads', default='unet64,unet96,unet32,unet64b4,unet64b6,unet64b8,vaedec64,vaedec96,vaeenc512,clip')
    ap.add_argument('--append-new', action='store_true', help='keep every row of the table at --out; append the shapes it does not have')
    args = ap.parse_args()
    from stable_diffusion_amd import AutoencoderKLHIP, FrozenCLIPEmbedderHIP, UNetModelHIP, _lib
    from stable_diffusion_amd.synthetic import (SD_V1_UNET_KWARGS, SD_V1_VAE_DDCONFIG, randomize_, randomize_vae_,
                                                synthetic_clip_state_dict)
    lib = _lib.load()
    dev = torch.device('cuda')
    unet = UNetModelHIP(**SD_V1_UNET_KWARGS).to(dev).eval()
    randomize_(unet, 0)
    vae = AutoencoderKLHIP(SD_V1_VAE_DDCONFIG, None, 4).to(dev).eval()
    randomize_vae_(vae, 0)
    clip = None
    g = torch.Generator().manual_seed(0)

    def unet_fn(B, H):
        x = torch.randn(B, 4, H, H, generator=g).to(dev)
        ctx = (0.1 * torch.randn(B, 77, 768, generator=g)).to(dev)
        t = torch.full((B,), 481, device=dev)

        def fn():
            unet(x, t, context=ctx * 1.0)        # a fresh context object: the cross-attention K/V GEMMs run too
        return fn

    def vaedec_fn(H):
        z = torch.randn(1, 4, H, H, generator=g).to(dev)
        return lambda: vae.decode(z)

    def vaeenc_fn(S):
        img = torch.randn(1, 3, S, S, generator=g).to(dev)
        return lambda: vae.encode(img)

    def clip_fn():
        nonlocal clip
        if clip is None:
            clip = FrozenCLIPEmbedderHIP(tokenizer=object()).to(dev)
            clip.load_state_dict(synthetic_clip_state_dict(None, 0), strict=False)
            clip = clip.to(dev)
        ids = torch.randint(0, 49408, (2, 77), generator=g).to(dev)
        return lambda: clip.encode_ids(ids)

    churches = None

    def churches_fn(B):              # the unconditional LSUN-Churches UNet at its native 32 x 32 latent (8 + 2 rows of a batch of 10)
        nonlocal churches
        from stable_diffusion_amd.synthetic import CHURCHES_UNET_KWARGS
        if churches is None:
            churches = randomize_(UNetModelHIP(**CHURCHES_UNET_KWARGS).to(dev).eval(), 0)
        x = torch.randn(B, 4, 32, 32, generator=g).to(dev)
        t = torch.full((B,), 481, device=dev)
        return lambda: churches(x, t)

    lowwidth = {}

    def faces_fn(which, B, H=64):    # the face / bedroom UNet (224 wide) and bsr_sr's (160) at their native 64 x 64 latent: half k-tiles
        from stable_diffusion_amd.synthetic import BSR_UNET_KWARGS, FACES_UNET_KWARGS
        kw = FACES_UNET_KWARGS if which == 'faces' else BSR_UNET_KWARGS
        if which not in lowwidth:
            lowwidth[which] = randomize_(UNetModelHIP(**kw).to(dev).eval(), 0)
        m = lowwidth[which]
        x = torch.randn(B, kw['in_channels'], H, H, generator=g).to(dev)
        t = torch.full((B,), 481, device=dev)
        return lambda: m(x, t)

    makers = {
        'faces64b8': lambda: faces_fn('faces', 8), 'faces64b2': lambda: faces_fn('faces', 2),
        'bsr64b8': lambda: faces_fn('bsr', 8), 'bsr64b2': lambda: faces_fn('bsr', 2),
        'bsr128b8': lambda: faces_fn('bsr', 8, 128), 'bsr128b1': lambda: faces_fn('bsr', 1, 128),
        'churches32b8': lambda: churches_fn(8), 'churches32b2': lambda: churches_fn(2),
        'unet64': lambda: unet_fn(2, 64), 'unet96': lambda: unet_fn(2, 96), 'unet32': lambda: unet_fn(2, 32),
        'unet64b4': lambda: unet_fn(4, 64), 'unet64b6': lambda: unet_fn(6, 64), 'unet64b8': lambda: unet_fn(8, 64),
        'vaedec64': lambda: vaedec_fn(64), 'vaedec96': lambda: vaedec_fn(96), 'vaeenc512': lambda: vaeenc_fn(512),
        'clip': clip_fn,
    }
    fns = []
    for name in args.workloads.split(','):
        try:
            fn = makers[name]()
            fn()                                 # warm up outside the collection (packs weights, sizes workspaces)
            torch.cuda.synchronize()
            fns.append((name, fn))
        except Exception as e:                    # a workload that does not exist in this build is skipped, not fatal
            print(f'[tune] workload {name} skipped: {type(e).__name__}: {e}', flush=True)
    _lib.check(lib.sdmi_tune_begin())
    t0 = time.time()
    for rep in range(args.reps):
        for r in range(args.rounds):
            _lib.check(lib.sdmi_tune_round(r))
            for name, fn in fns:
                fn()
        torch.cuda.synchronize()
    n = C.c_int(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = args.out + '.new' if args.append_new else args.out
    _lib.check(lib.sdmi_tune_end(out.encode(), C.byref(n)))
    if args.append_new:
        key = lambda ln: tuple(ln.split()[:8])
        rows = lambda path: [ln for ln in open(path).read().splitlines() if ln and not ln.startswith('#')]

        def phase_path(p):      # the rows of the 2x2 phase kind (ksize 2) live beside the table (csrc/igemm.hip Tuner::phase_path_of)
            return p[:-len('tune_gfx950.txt')] + 'tune_up_phase_gfx950.txt' if p.endswith('tune_gfx950.txt') else p + '.up_phase'
        for dst, new in ((args.out, out), (phase_path(args.out), phase_path(out))):
            if not os.path.exists(new):
                continue
            have = {key(ln) for ln in rows(dst)} if os.path.exists(dst) else set()
            fresh = [ln for ln in rows(new) if key(ln) not in have]
            head = '' if os.path.exists(dst) else open(new).read().splitlines()[0] + '\n'
            with open(dst, 'a') as f:
                f.write(head + ''.join(ln + '\n' for ln in fresh))
            os.remove(new)
            print(f'[tune] --append-new: {len(fresh)} new rows appended to {os.path.basename(dst)}, {len(have)} kept as they were', flush=True)
    print(f'[tune] {n.value} shapes tuned over {args.reps} x {args.rounds} rounds of {[w for w, _ in fns]} in '
          f'{time.time() - t0:.1f} s -> {args.out}', flush=True)
    if args.dump:
        buf = C.create_string_buffer(8 << 20)
        _lib.check(lib.sdmi_tune_dump(buf, len(buf)))
        open(args.dump, 'w').write('# M N K ksize stride up mode splitk_req | tile splitk median_us min_us samples\n' + buf.value.decode())


if __name__ == '__main__':
    main()
