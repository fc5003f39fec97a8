"""Requests that arrive one after another: SamplerPoolHIP against the same requests one after another through DDIMSamplerHIP.

    python tools/bench_sampler_pool.py [--requests 8] [--steps 50] [--gaps 0,5,25] [--runs 3] [--out profiles/bench_sampler_pool.txt]

SD-v1 UNet (seeded synthetic weights, as bench.py), a 4 x 64 x 64 latent, guided DDIM requests (scale 7.5) that arrive k steps apart, a
pool of 8 rows (four guided requests at a time).  One "step" of the arrival clock is the measured time of one step of a lone request
(a 2-row UNet call and its update), so k = 50 would be the rate at which a lone sampler just keeps up.

  pool      every request is submitted when its arrival time has come; the driver synchronises after a step only while arrivals are still
            outstanding (it needs the device's clock to admit them on time) and when a request finishes (to take its finish time)
  baseline  what the library did before the pool, in the same process: the requests in arrival order, each alone through
            DDIMSamplerHIP.sample (hinted timesteps, pinned context), started when it has arrived and its predecessor is done

Reported per k, for each of `--runs` alternating runs: latents per second from the first arrival to the last finish, and the mean
latency arrival -> finish.  Then the launches of one steady pool step against one bare UNet call of the same rows (the library's own
profile scope), and the cost of the unhinted timestep path per 8-row call.  ONE BOX: the runs show the spread, not a confidence interval."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--requests', type=int, default=8)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--gaps', default='0,5,25')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from stable_diffusion_amd import DDIMSamplerHIP, LatentDiffusionHIP, SamplerPoolHIP, UNetModelHIP, _lib
    from stable_diffusion_amd.synthetic import SD_V1_UNET_KWARGS, randomize_
    dev = 'cuda'
    unet = UNetModelHIP(**SD_V1_UNET_KWARGS)
    ld = LatentDiffusionHIP(unet).to(dev).eval()
    randomize_(unet, 0)
    lib = _lib.load()
    shape, S, scale, N = (4, 64, 64), args.steps, 7.5, args.requests
    g = torch.Generator().manual_seed(0)
    reqs = [((torch.randn((1,) + shape, generator=g)).to(dev), (0.1 * torch.randn(1, 77, 768, generator=g)).to(dev),
             (0.1 * torch.randn(1, 77, 768, generator=g)).to(dev)) for _ in range(N)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def alone(i):
        x_T, c, uc = reqs[i]
        return DDIMSamplerHIP(ld).sample(S=S, batch_size=1, shape=list(shape), conditioning=c, verbose=False, x_T=x_T,
                                         unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=0.)[0]

    def run_baseline(arrival):
        torch.cuda.synchronize()
        t0, fin = time.perf_counter(), []
        for i in range(N):
            while time.perf_counter() - t0 < arrival[i]:
                pass
            alone(i)
            torch.cuda.synchronize()
            fin.append(time.perf_counter() - t0)
        return fin

    def run_pool(arrival):
        pool = SamplerPoolHIP(ld, shape)
        torch.cuda.synchronize()
        t0, fin, tickets, nxt = time.perf_counter(), {}, {}, 0
        while len(fin) < N:
            now = time.perf_counter() - t0
            while nxt < N and arrival[nxt] <= now:
                x_T, c, uc = reqs[nxt]
                tickets[nxt] = pool.submit(S=S, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=scale, x_T=x_T)
                nxt += 1
            if not pool.step():
                continue                      # idle until the next arrival
            newly = [i for i, t in tickets.items() if i not in fin and pool.done(t)]
            if newly or nxt < N:
                torch.cuda.synchronize()
            for i in newly:
                fin[i] = time.perf_counter() - t0
                pool.result(tickets[i])
        return [fin[i] for i in range(N)]

    # warm every row count the runs meet: tapes, workspaces, the allocator; then the arrival clock's step
    run_pool([0.0] * N)
    run_pool([0.05 * i for i in range(N)])
    alone(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    alone(0)
    torch.cuda.synchronize()
    tau = (time.perf_counter() - t0) / S
    say(f'bench_sampler_pool: {torch.cuda.get_device_name(0)}; SD-v1 UNet, 4 x 64 x 64, {N} guided DDIM-{S} requests, pool of 8 rows; '
        f'{args.runs} alternating runs each')
    say(f'one step of a lone request (the arrival clock\'s unit): {tau * 1e3:.3f} ms')
    for k in [int(v) for v in args.gaps.split(',')]:
        arrival = [i * k * tau for i in range(N)]
        res = {'pool': [], 'baseline': []}
        for _ in range(args.runs):
            for name, fn in (('pool', run_pool), ('baseline', run_baseline)):
                fin = fn(arrival)
                res[name].append((N / (max(fin) - arrival[0]), sum(f - a for f, a in zip(fin, arrival)) / N * 1e3))
        for name in ('pool', 'baseline'):
            say(f'[k = {k:2d}] {name:8s} latents/s ' + ' / '.join(f'{r[0]:.3f}' for r in res[name]) + '   mean latency ms ' +
                ' / '.join(f'{r[1]:.1f}' for r in res[name]))
        med = lambda v: sorted(v)[len(v) // 2]
        tp, tb = med([r[0] for r in res['pool']]), med([r[0] for r in res['baseline']])
        lp, lb = med([r[1] for r in res['pool']]), med([r[1] for r in res['baseline']])
        say(f'[k = {k:2d}] medians: throughput pool / baseline = {tp / tb:.3f}x, mean latency pool / baseline = {lp / lb:.3f}x'
            + ('   ** the pool is slower here **' if tp < tb or lp > lb else ''))

    # launches of one steady pool step against one bare UNet call of the same 8 rows
    def profiled(fn):
        torch.cuda.synchronize()
        _lib.check(lib.sdmi_profile_begin())
        fn()
        buf = ctypes.create_string_buffer(1 << 16)
        _lib.check(lib.sdmi_profile_end(buf, 1 << 16))
        return json.loads(buf.value.decode())

    pool = SamplerPoolHIP(ld, shape)
    for x_T, c, uc in reqs[:4]:
        pool.submit(S=S, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=scale, x_T=x_T)
    for _ in range(3):
        pool.step()
    x_in, t_in, c_in = pool._views
    bare = profiled(lambda: ld.apply_model(x_in, t_in, c_in))
    step = profiled(pool.step)
    count = lambda p: sum(e['launches'] for e in p)
    rows_launches = sum(e['launches'] for e in step if e['name'] == 'sampler_step_rows')
    rows_ms = sum(e['ms'] for e in step if e['name'] == 'sampler_step_rows')
    say(f'launches in the library\'s profile scope: one steady pool step (8 rows, 4 slots) {count(step)}, one bare UNet call of the same rows '
        f'{count(bare)}: {count(step) - count(bare)} more, of which sdmi_sampler_step_rows {rows_launches} ({rows_ms * 1e3:.1f} us)')
    pool.run_until_idle()

    # the unhinted timestep path: 8-row calls with and without the scalar hint, same timestep, same pinned context
    t_same = torch.full((8,), 481, device=dev, dtype=torch.long)
    x8, c8 = x_in.clone(), c_in.clone()
    unet.pin_context(c8)
    unet.cache_timesteps([481])

    def calls(n, hint):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            if hint:
                unet.hint_timestep(481)
            ld.apply_model(x8, t_same, c8)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    calls(5, True), calls(5, False)
    th, tu = [], []
    for _ in range(args.runs):
        th.append(calls(40, True))
        tu.append(calls(40, False))
    unet.unpin_context()
    say('8-row UNet call, ms: hinted ' + ' / '.join(f'{t:.4f}' for t in th) + '   unhinted ' + ' / '.join(f'{t:.4f}' for t in tu) +
        f'   unhinted - hinted (best of each): {(min(tu) - min(th)) * 1e3:.1f} us per call')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
