"""DPM-Solver requests that arrive one after another: SamplerPoolHIP(timesteps='float32') against the same requests one after another
through DPMSolverSamplerHIP, and what the fp32-timestep launch costs on the workload the pool already had.

    python tools/bench_sampler_pool_dpm.py [--requests 8] [--S 20] [--ddim_S 50] [--gaps 0,5,25] [--runs 3] [--out profiles/bench_sampler_pool_dpm.txt]

The setup of tools/bench_sampler_pool.py: SD-v1 UNet (seeded synthetic weights, as bench.py), a 4 x 64 x 64 latent, guided requests
(scale 7.5) that arrive k steps apart, a pool of 8 rows.  One "step" of the arrival clock is the measured time of one evaluation of a
lone request of the kind measured.

  dpm       default sampler='dpm' requests (DPM-Solver++(2M), S evaluations) through a float pool, against the baseline: the requests in
            arrival order, each alone through DPMSolverSamplerHIP.sample (its fused step), started when it has arrived and its
            predecessor is done
  ddim      DDIM requests through a float pool (sdmi_sampler_plan_rows, kind 0 slots) against an int pool (sdmi_sampler_step_rows)

Reported per k, for each of `--runs` alternating runs: latents per second from the first arrival to the last finish, and the mean
latency arrival -> finish.  Then the two launches' times in the library's own profile scope.  ONE BOX: the runs show the spread, not a
confidence interval."""
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
    ap.add_argument('--S', type=int, default=20)
    ap.add_argument('--ddim_S', type=int, default=50)
    ap.add_argument('--gaps', default='0,5,25')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from stable_diffusion_amd import DDIMSamplerHIP, DPMSolverSamplerHIP, LatentDiffusionHIP, SamplerPoolHIP, UNetModelHIP, _lib
    from stable_diffusion_amd.synthetic import SD_V1_UNET_KWARGS, randomize_
    dev = 'cuda'
    unet = UNetModelHIP(**SD_V1_UNET_KWARGS)
    ld = LatentDiffusionHIP(unet).to(dev).eval()
    randomize_(unet, 0)
    lib = _lib.load()
    shape, scale, N = (4, 64, 64), 7.5, args.requests
    g = torch.Generator().manual_seed(0)
    reqs = [((torch.randn((1,) + shape, generator=g)).to(dev), (0.1 * torch.randn(1, 77, 768, generator=g)).to(dev),
             (0.1 * torch.randn(1, 77, 768, generator=g)).to(dev)) for _ in range(N)]
    gaps = [int(v) for v in args.gaps.split(',')]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def alone_dpm(i):
        x_T, c, uc = reqs[i]
        return DPMSolverSamplerHIP(ld).sample(S=args.S, batch_size=1, shape=list(shape), conditioning=c, verbose=False, x_T=x_T,
                                              unconditional_guidance_scale=scale, unconditional_conditioning=uc)[0]

    def run_sequential(arrival):
        torch.cuda.synchronize()
        t0, fin = time.perf_counter(), []
        for i in range(N):
            while time.perf_counter() - t0 < arrival[i]:
                pass
            alone_dpm(i)
            torch.cuda.synchronize()
            fin.append(time.perf_counter() - t0)
        return fin

    def pool_runner(timesteps, **submit):
        def run(arrival):
            pool = SamplerPoolHIP(ld, shape, timesteps=timesteps)
            torch.cuda.synchronize()
            t0, fin, tickets, nxt = time.perf_counter(), {}, {}, 0
            while len(fin) < N:
                now = time.perf_counter() - t0
                while nxt < N and arrival[nxt] <= now:
                    x_T, c, uc = reqs[nxt]
                    tickets[nxt] = pool.submit(conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=scale, x_T=x_T, **submit)
                    nxt += 1
                if not pool.step():
                    continue                      # idle until the next arrival
                newly = [i for i, t in tickets.items() if i not in fin and pool.done(t)]
                if newly or nxt < N:              # (the device's clock admits arrivals on time and stamps a finish)
                    torch.cuda.synchronize()
                for i in newly:
                    fin[i] = time.perf_counter() - t0
                    pool.result(tickets[i])
            return [fin[i] for i in range(N)]
        return run

    def compare(title, tau, a_name, a_run, b_name, b_run):
        """alternating runs of a (the candidate) and b (what it is held against) at every arrival rate"""
        for k in gaps:
            arrival = [i * k * tau for i in range(N)]
            res = {a_name: [], b_name: []}
            for _ in range(args.runs):
                for name, fn in ((a_name, a_run), (b_name, b_run)):
                    fin = fn(arrival)
                    res[name].append((N / (max(fin) - arrival[0]), sum(f - a for f, a in zip(fin, arrival)) / N * 1e3))
            for name in (a_name, b_name):
                say(f'[{title}, k = {k:2d}] {name:10s} latents/s ' + ' / '.join(f'{r[0]:.3f}' for r in res[name]) + '   mean latency ms ' +
                    ' / '.join(f'{r[1]:.1f}' for r in res[name]))
            med = lambda v: sorted(v)[len(v) // 2]
            spread = max((max(v) - min(v)) / med(v) for v in ([r[0] for r in res[n]] for n in res))
            ta, tb = med([r[0] for r in res[a_name]]), med([r[0] for r in res[b_name]])
            la, lb = med([r[1] for r in res[a_name]]), med([r[1] for r in res[b_name]])
            # slower beyond the runs' own spread: every run of a behind every run of b, in throughput or in latency
            slower = (max(r[0] for r in res[a_name]) < min(r[0] for r in res[b_name]) or
                      min(r[1] for r in res[a_name]) > max(r[1] for r in res[b_name]))
            say(f'[{title}, k = {k:2d}] medians: throughput {a_name} / {b_name} = {ta / tb:.3f}x, mean latency {a_name} / {b_name} = {la / lb:.3f}x, '
                f'largest throughput spread of the runs {spread * 100:.1f} %' + (f'   ** {a_name} is slower here, beyond the runs\' spread **' if slower else ''))

    def lone_step(fn, steps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    dpm_pool = pool_runner('float32', S=args.S, sampler='dpm')
    ddim_f32, ddim_i64 = pool_runner('float32', S=args.ddim_S), pool_runner('int64', S=args.ddim_S)
    say(f'bench_sampler_pool_dpm: {torch.cuda.get_device_name(0)}; SD-v1 UNet, 4 x 64 x 64, {N} guided requests, pools of 8 rows; '
        f'{args.runs} alternating runs each')

    # warm every row count the runs meet: tapes of both timestep dtypes, workspaces, the allocator
    for run in (dpm_pool, ddim_f32, ddim_i64):
        run([0.0] * N)
        run([0.05 * i for i in range(N)])
    tau = lone_step(lambda: alone_dpm(0), args.S)
    say(f'one evaluation of a lone DPM-Solver++(2M)-{args.S} request (the arrival clock\'s unit): {tau * 1e3:.3f} ms')
    compare(f'DPM-{args.S}', tau, 'float pool', dpm_pool, 'sequential', run_sequential)

    # a request that has the machine to itself, timed end to end with ONE synchronisation: what the pool's host work per step costs when
    # nothing hides it is the difference between this and the k >= S rows above, where the driver synchronises after every step
    def lone_pool():
        pool = SamplerPoolHIP(ld, shape, timesteps='float32')
        x_T, c, uc = reqs[0]
        t = pool.submit(S=args.S, sampler='dpm', conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=scale, x_T=x_T)
        pool.run_until_idle()
        return pool.result(t)[0]
    ms = {'float pool': [], 'sampler': []}
    for _ in range(args.runs):
        for name, fn in (('float pool', lone_pool), ('sampler', lambda: alone_dpm(0))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    say(f'one lone DPM-{args.S} request, one synchronisation at its end, ms: float pool ' + ' / '.join(f'{v:.2f}' for v in ms['float pool']) +
        '   DPMSolverSamplerHIP ' + ' / '.join(f'{v:.2f}' for v in ms['sampler']))

    x_T, c, uc = reqs[0]
    tau = lone_step(lambda: DDIMSamplerHIP(ld).sample(S=args.ddim_S, batch_size=1, shape=list(shape), conditioning=c, verbose=False, x_T=x_T,
                                                      unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=0.), args.ddim_S)
    say(f'one step of a lone DDIM-{args.ddim_S} request (the arrival clock\'s unit): {tau * 1e3:.3f} ms')
    compare(f'DDIM-{args.ddim_S}', tau, 'float pool', ddim_f32, 'int pool', ddim_i64)

    # the two launches in the library's own profile scope: one steady step of four guided DDIM requests in each pool
    def profiled(fn):
        torch.cuda.synchronize()
        _lib.check(lib.sdmi_profile_begin())
        fn()
        buf = ctypes.create_string_buffer(1 << 16)
        _lib.check(lib.sdmi_profile_end(buf, 1 << 16))
        return json.loads(buf.value.decode())

    for timesteps, sampler, S, name in (('int64', 'ddim', args.ddim_S, 'sampler_step_rows'), ('float32', 'ddim', args.ddim_S, 'sampler_plan_rows'),
                                        ('float32', 'dpm', args.S, 'sampler_plan_rows')):
        pool = SamplerPoolHIP(ld, shape, timesteps=timesteps)
        for x_T, c, uc in reqs[:4]:
            pool.submit(S=S, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=scale, x_T=x_T, sampler=sampler)
        for _ in range(4):
            pool.step()
        us = []
        for _ in range(5):
            step = profiled(pool.step)
            us.append(sum(e['ms'] for e in step if e['name'] == name) * 1e3)
        say(f'{timesteps} pool, four guided {sampler} requests (8 rows, 4 slots): sdmi_{name} ' + ' / '.join(f'{u:.1f}' for u in us) + ' us per step')
        pool.run_until_idle()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
