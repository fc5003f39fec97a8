"""Run the retrieval-augmented UNet (configs/retrieval-augmented-diffusion/768x768.yaml: 1 335 480 400 parameters, model_channels 448,
num_head_channels 32, 16 latent channels) on one MI355X with seeded synthetic weights: parity against the reference golden of the full
configuration (tests/golden/rdm_unet_8x8_b2.npz, tools/make_golden_rdm.py) and the time of one call on the native 48 x 48 latent.

    python tools/bench_rdm.py [--precision mixed] [--knn 10] [--calls 200] [--rounds 5] [--out profiles/bench_rdm.txt]

Prints (and writes to --out, replacing it) one parity line -- max-abs / rms against the golden eps -- and one JSON line: the size of the packed handle,
ms per UNet call for B = 1 and for the classifier-free-guidance pair B = 2 (knn2img.py evaluates cat([uc, c]) as one batch): the median
over --rounds windows of --calls replayed calls each, device events around every window, with the min .. max of the windows' means.  A
timestep table and a pinned context, as inside DDIMSamplerHIP's loop.  There is no earlier build of this model to compare against:
the numbers are reported, nothing is asserted."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precision', default='mixed', choices=['mixed', 'full'])
    ap.add_argument('--knn', type=int, default=10)
    ap.add_argument('--calls', type=int, default=200)        # (a window of about a second)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_rdm.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_rdm.py needs the MI355X'
    from stable_diffusion_amd import UNetModelHIP, synthetic
    kw = synthetic.RDM_UNET_KWARGS
    dev = 'cuda'
    unet = UNetModelHIP(**kw, hip_precision=args.precision)
    unet.load_state_dict(synthetic.synthetic_named_state_dict([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], 0), strict=True)
    n_params = sum(v.numel() for v in unet.state_dict().values())
    unet = unet.to(dev)
    lines = []

    # ---- parity: the full configuration against the reference's own eps ----
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rdm_unet_8x8_b2.npz'))
    b, h, w = int(z['batch']), int(z['h']), int(z['w'])
    x = torch.randn(b, kw['in_channels'], h, w, generator=torch.Generator().manual_seed(int(z['input_seed'])))
    c = torch.randn(b, int(z['ctx_tokens']), kw['context_dim'], generator=torch.Generator().manual_seed(int(z['ctx_seed'])))
    t = torch.tensor([int(v) for v in z['t']], dtype=torch.int64)
    eps = unet(x.to(dev), t.to(dev), context=c.to(dev))
    torch.cuda.synchronize()
    err = (eps.float().cpu() - torch.from_numpy(z['eps'])).abs()
    lines.append(f'[rdm unet 8x8_b2 {args.precision}] {n_params} parameters; max-abs {float(err.max()):.3e} rms {float(err.pow(2).mean().sqrt()):.3e} '
                 f'against the reference golden (|eps| max {float(np.abs(z["eps"]).max()):.3f}); finite {bool(torch.isfinite(eps).all())}')
    print(lines[-1], flush=True)

    # ---- one call on the native latent, as inside the sampling loop ----
    lat, L = kw['image_size'], 1 + args.knn
    g = torch.Generator().manual_seed(0)
    res = {'metric': 'rdm768_unet', 'precision': args.precision, 'latent': lat, 'context_tokens': L, 'calls_per_window': args.calls,
           'windows': args.rounds, 'packed_handle_gb': round(int(unet._handle.lib.sdmi_unet_packed_bytes(unet._handle.h)) / 1e9, 3)}
    unet.cache_timesteps([501])
    for rows in (1, 2):
        xr = torch.randn(rows, kw['in_channels'], lat, lat, generator=g).to(dev)
        cr = torch.randn(rows, L, kw['context_dim'], generator=g).to(dev)
        if rows == 2:
            cr[0] = 0                       # (the pair of knn2img.py: uc = zeros_like(c) in front)
        tr = torch.full((rows,), 501, dtype=torch.long, device=dev)
        unet.pin_context(cr)

        def call():
            unet.hint_timestep(501)
            return unet(xr, tr, context=cr)
        for _ in range(3):                  # (every shape of the timed window is warm: the tape is recorded, the code objects loaded)
            out = call()
        torch.cuda.synchronize()
        ms = [_window(call, args.calls) for _ in range(args.rounds)]
        res[f'ms_per_unet_call_b{rows}'] = round(statistics.median(ms), 3)
        res[f'ms_min_max_b{rows}'] = [round(min(ms), 3), round(max(ms), 3)]
        res[f'finite_b{rows}'] = bool(torch.isfinite(out).all())
        unet.unpin_context()
    unet.cache_timesteps([])
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        head = ('Retrieval-augmented UNet (configs/retrieval-augmented-diffusion/768x768.yaml), seeded synthetic weights, one MI355X, one process, one run:\n'
                f'python tools/bench_rdm.py --precision {args.precision} --knn {args.knn} --calls {args.calls} --rounds {args.rounds}\n'
                'parity line, then one JSON line: per batch size the median over the windows of the mean ms per replayed call (device events around\n'
                'every window), min .. max of the windows; timestep table and pinned context as in the sampling loop.  Reported, not asserted.\n\n')
        with open(args.out, 'w') as f:
            f.write(head + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
