"""SamplerPoolHIP(timesteps='float32') on the GPU.

With the exactly rounded, per-row stub model of tests/dpm_cases.py: nine DPM-Solver requests -- each one or two samples of a case of
tests/golden/dpm_variants.npz, on its recorded plan -- with a DDIM and a PLMS request among them through one pool of 8 rows, submitted
at staggered call counts.  Rows are independent, so a request made of sample j of a case must equal the reference's end point for that
sample bit for bit, and the DDIM / PLMS requests must equal DDIMSamplerHIP / PLMSSamplerHIP alone and the same requests in an 'int64'
pool.  Portability: a DPMPlan's scalars pass through the CPU's exp / log; the recorded plans take that out of the fixture comparisons,
and the default-path test computes both of its sides on the same host.

With UNetModelHIP (tiny configuration, 8 x 8 latent): a float pool with a default DPM request and a DDIM request against an explicit
loop that issues plan_calls' calls with fp32 timesteps to the same handle and does every update in torch expressions, bit for bit; and a
lone DDIM request through a float pool against an int pool: an integer timestep handed over as fp32 gives the same embedding bits."""
import os

import numpy as np
import pytest
import torch

import dpm_cases as DC
from stable_diffusion_amd import DDIMSamplerHIP, DPMSolverSamplerHIP, PLMSSamplerHIP, SamplerPoolHIP, plan_calls
from stable_diffusion_amd.sampler_pool import dpm_plan_pairs, dpm_request_plan
from stable_diffusion_amd.samplers import make_ddim_timesteps, make_tables

pytestmark = pytest.mark.gpu
SHAPE = DC.SHAPE[1:]
TOKENS = (3, 5)
MAX_ROWS = 8

# name -> (case of the fixture, its samples, the number of UNet calls the pool has made at submit).  Between them: multistep orders 1-3,
# singlestep orders 2 and 3 in both solver types, denoise_to_zero, data and noise prediction, guided and unguided, one two-sample request
DPM = {
    'ms1': ('ms1_eps', (0,), 0),                     # guided, noise prediction: form 0 throughout
    'ms2': ('ms2_t06_x0', (1,), 0),                  # guided, t_start = 0.6: forms 0, 1
    'ms3': ('ms3_s16_eps', (2,), 0),                 # guided, 16 evaluations: forms 0, 1, 3
    'ss2': ('ss2_s5_x0', (0,), 1),                   # guided; finds the pool full and waits
    'ss3': ('ss3_s6_eps', (1,), 1),                  # unguided; would fit later but waits behind 'ss2'
    'taylor': ('ss3_s6_taylor_x0', (2,), 2),         # guided: form 2
    'zero_x0': ('ssf3_uniform_x0', (0,), 3),         # unguided, denoise_to_zero: its last slot has no update
    'zero_eps': ('ssf3_uniform_eps', (1,), 5),       # guided, denoise_to_zero: the last evaluation is the data prediction of a noise-prediction run
    'pair': ('ms1_x0', (0, 1), 6),                   # unguided, two samples
}
STEP = {'ddim': dict(sampler='ddim', S=8, eta=0.5, scale=5.0, arrival=0, seed=91), 'plms': dict(sampler='plms', S=5, eta=0., scale=3.0, arrival=4, seed=92)}
NAMES = list(DPM) + list(STEP)


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'dpm_variants.npz'))


class StubLD:
    """the samplers' view of a LatentDiffusion over dpm_cases' stub: a row's conditioning number is c[row, 0, 0] (0 for an unconditional row)"""

    def __init__(self):
        self.num_timesteps = 1000
        self.alphas_cumprod = DC.alphas_cumprod().cuda()
        self.betas = torch.zeros(1000, device='cuda')
        self.device = torch.device('cuda')
        self.calls = []                  # the timesteps of every call, as they were when it was made

    def apply_model(self, x, t, c):
        self.calls.append(t.clone())
        return DC.MODELS['stub'](x, t.float(), c[:, 0, 0].contiguous())


def _context(values):
    c = torch.zeros((len(values),) + TOKENS)
    c[:, 0, 0] = torch.tensor(values)
    return c.cuda()


def _step_inputs(name):
    r = STEP[name]
    g = torch.Generator().manual_seed(r['seed'])
    x_T = torch.randn((1,) + SHAPE, generator=g)
    draws = [torch.randn((1,) + SHAPE, generator=g) for _ in range(r['S'] + 1)]
    return x_T.cuda(), _context([0.75]), _context([0.0]), [d.cuda() for d in draws]


def _submit(pool, G, name, seqs):
    if name in STEP:
        r = STEP[name]
        x_T, c, uc, draws = _step_inputs(name)
        t = pool.submit(S=r['S'], conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=r['scale'], eta=r['eta'], x_T=x_T,
                        sampler=r['sampler'], log_every_t=3)
        seqs[t] = draws
        return t
    case_name, samples, _ = DPM[name]
    case = DC.CASES[case_name]
    x = DC.case_x(int(G[f'{case_name}_seed']))[list(samples)].cuda()
    guided = case['scale'] is not None
    return pool.submit(S=case['sample']['steps'], conditioning=_context([DC.COND[j] for j in samples]),
                       unconditional_conditioning=_context([0.0] * len(samples)) if guided else None,
                       unconditional_guidance_scale=case['scale'] if guided else 1., x_T=x, sampler='dpm', plan=DC.load_plan(G, case_name),
                       predict_x0=case['predict_x0'])


def _arrival(name):
    return STEP[name]['arrival'] if name in STEP else DPM[name][2]


def _run(G, names, timesteps, at_once=False):
    """the requests through one pool, each submitted at its call count (or all at the start) -> (results by name, trace, timesteps per call)"""
    model = StubLD()
    pool = SamplerPoolHIP(model, SHAPE, max_rows=MAX_ROWS, timesteps=timesteps)
    pool.trace = []
    seqs, tickets = {}, {}
    pool._noise_like = lambda shape, device, generator=None, ticket=None: seqs[ticket].pop(0)
    while True:
        for name in names:
            if name not in tickets and (at_once or _arrival(name) <= pool.calls):
                tickets[name] = _submit(pool, G, name, seqs)
        if not pool.step():
            break
    assert all(pool.done(t) for t in tickets.values()) and pool.pending() == 0
    results = {name: pool.result(tickets[name]) for name in names}
    torch.cuda.synchronize()
    by_ticket = {t: name for name, t in tickets.items()}
    trace = [[(by_ticket[row[0]],) + row[1:] for row in call] for call in pool.trace]
    return results, trace, [t.cpu() for t in model.calls]


@pytest.fixture(scope='module')
def pool_run(G):
    return _run(G, NAMES, 'float32')


def _plan_request(G, name):
    if name in STEP:
        r = STEP[name]
        return dict(ticket=name, S=r['S'], sampler=r['sampler'], guided=True, arrival=r['arrival'])
    case_name, samples, arrival = DPM[name]
    return dict(ticket=name, sampler='dpm', plan=DC.load_plan(G, case_name), samples=len(samples),
                guided=DC.CASES[case_name]['scale'] is not None, arrival=arrival)


def test_float_pool_executes_the_plan(G, pool_run):
    results, trace, times = pool_run
    plan = plan_calls([_plan_request(G, n) for n in NAMES], MAX_ROWS, 1000)
    assert trace == plan and [int(t.shape[0]) for t in times] == [len(c) for c in plan]
    assert all(t.dtype == torch.float32 for t in times)
    first = {n: min(k for k, c in enumerate(trace) if any(row[0] == n for row in c)) for n in NAMES}
    assert first['ss2'] > _arrival('ss2') and first['ss3'] > _arrival('ss3')                # both waited in the queue
    assert max(len(c) for c in plan) == MAX_ROWS
    own = sum(len(G[f'{DPM[n][0]}_calls']) for n in DPM) + STEP['ddim']['S'] + STEP['plms']['S'] + 1
    print(f'[float pool, stub] {len(plan)} UNet calls where the {len(NAMES)} requests alone make {own}')
    assert len(plan) < own
    # every row of every call carried the time its request's plan names
    for call, t in zip(plan, times):
        assert t.tolist() == [float(np.float32(row[2])) for row in call]


@pytest.mark.parametrize('name', list(DPM))
def test_dpm_request_equals_the_reference_run(G, pool_run, name):
    """the reference's end point of the request's samples, bit for bit, and the model called at the reference's times"""
    results, trace, times = pool_run
    case_name, samples, _ = DPM[name]
    out, none = results[name]
    assert none is None
    want = torch.from_numpy(G[f'{case_name}_out'])[list(samples)]
    print(f'[{name}: {case_name}{list(samples)}] max-abs {float((out.cpu() - want).abs().max()):.3e} (|x| max {float(want.abs().max()):.2f})')
    assert torch.equal(out.cpu(), want)
    seen = [float(t[[row[0] for row in call].index(name)]) for call, t in zip(trace, times) if any(row[0] == name for row in call)]
    assert np.array_equal(np.asarray(seen, dtype=np.float32), G[f'{case_name}_calls'])


@pytest.mark.parametrize('name', list(STEP))
def test_step_request_equals_the_sampler_alone_and_the_int_pool(G, pool_run, name):
    r = STEP[name]
    out, inter = pool_run[0][name]
    x_T, c, uc, draws = _step_inputs(name)
    smp = (DDIMSamplerHIP if r['sampler'] == 'ddim' else PLMSSamplerHIP)(StubLD())
    smp._noise_like = lambda shape, device: draws.pop(0)
    alone, alone_inter = smp.sample(S=r['S'], batch_size=1, shape=list(SHAPE), conditioning=c, verbose=False, x_T=x_T, eta=r['eta'], log_every_t=3,
                                    unconditional_guidance_scale=r['scale'], unconditional_conditioning=uc)
    assert torch.equal(out, alone)
    for key in ('pred_x0', 'x_inter'):
        assert len(inter[key]) == len(alone_inter[key]) and all(torch.equal(a, b) for a, b in zip(inter[key], alone_inter[key])), key
    int_results, int_trace, int_times = _run(G, [name], 'int64', at_once=True)
    assert all(t.dtype == torch.int64 for t in int_times)
    assert torch.equal(out, int_results[name][0])
    for key in ('pred_x0', 'x_inter'):
        assert all(torch.equal(a, b) for a, b in zip(inter[key], int_results[name][1][key])), key


def test_default_dpm_request_equals_the_sampler_class():
    """no keyword but S: DPM-Solver++(2M).  DPMSolverSamplerHIP's fused step and the pool's plan forms are both the reference's bits"""
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn((2,) + SHAPE, generator=g).cuda()
    c, uc = _context([0.5, -0.25]), _context([0.0, 0.0])
    seen = []
    alone, none = DPMSolverSamplerHIP(StubLD()).sample(S=10, batch_size=2, shape=list(SHAPE), conditioning=c, verbose=False, x_T=x_T,
                                                       unconditional_guidance_scale=3.0, unconditional_conditioning=uc,
                                                       img_callback=lambda m, k: seen.append((m, k)))
    pool = SamplerPoolHIP(StubLD(), SHAPE, timesteps='float32')
    got = []
    t = pool.submit(S=10, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=3.0, x_T=x_T, sampler='dpm',
                    img_callback=lambda m, k: got.append((m, k)))
    assert pool.run_until_idle() == 10
    out, none2 = pool.result(t)
    torch.cuda.synchronize()
    assert none is None and none2 is None and torch.equal(out, alone)
    assert [k for _, k in got] == [k for _, k in seen] == list(range(10)) and all(torch.equal(a, b) for (a, _), (b, _) in zip(got, seen))


# ---- through UNetModelHIP ---------------------------------------------------------------------------------------------------------------
E2E = [dict(ticket=0, sampler='dpm', S=4, scale=7.5, arrival=0), dict(ticket=1, sampler='ddim', S=5, scale=3.0, arrival=1)]


@pytest.fixture(scope='module')
def tiny():
    from oracle.plan import TINY
    from oracle.weights import make_inputs, make_state_dict
    from stable_diffusion_amd import LatentDiffusionHIP, UNetModelHIP
    unet = UNetModelHIP(**TINY.ref_kwargs())
    unet.load_state_dict(make_state_dict(TINY, 0), strict=True)
    ld = LatentDiffusionHIP(unet).cuda()
    inp = []
    for r in E2E:
        x_T, _, ctx = make_inputs(TINY, 1, 8, 8, seed=30 + r['ticket'], ctx_len=7)
        inp.append((x_T.cuda(), ctx.cuda(), (torch.zeros_like(ctx) + 0.1 * (r['ticket'] + 1)).cuda()))
    return unet, ld, inp


def test_float_pool_over_the_hip_unet_equals_the_explicit_loop(tiny):
    unet, ld, inp = tiny
    shape = (4, 8, 8)
    ac = ld.alphas_cumprod.detach().float().cpu()
    plan = plan_calls([dict(ticket=r['ticket'], sampler=r['sampler'], S=r['S'], guided=True, arrival=r['arrival']) for r in E2E], 8,
                      ld.num_timesteps, alphas_cumprod=ac)
    row_sets = [[row[0] for row in call] for call in plan]
    assert row_sets == [[0, 0]] + [[0, 0, 1, 1]] * 3 + [[1, 1]] * 2
    changes = [len(s) for k, s in enumerate(row_sets) if k == 0 or s != row_sets[k - 1]]

    # the pool; the K/V are computed by pin_context when the row set changes and by no forward()
    pins = []
    pin = unet.pin_context
    unet.pin_context = lambda context: (pins.append(int(context.shape[0])), pin(context))[1]
    pool = SamplerPoolHIP(ld, shape, timesteps='float32')
    pool.trace = []
    tickets = {}
    try:
        while True:
            for r, (x_T, c, uc) in zip(E2E, inp):
                if r['ticket'] not in tickets and r['arrival'] <= pool.calls:
                    tickets[r['ticket']] = pool.submit(S=r['S'], conditioning=c, unconditional_conditioning=uc, sampler=r['sampler'],
                                                       unconditional_guidance_scale=r['scale'], x_T=x_T, log_every_t=1)
            if not pool.step():
                break
            if pool.pending():
                assert unet._pinned == (len(pool.trace[-1]), 7), 'a forward() recomputed the K/V of an unchanged row set'
    finally:
        unet.pin_context = pin
    assert pool.trace == plan
    assert pins == changes == [2, 4, 2]
    got = [pool.result(tickets[r['ticket']]) for r in E2E]

    # the explicit loop: the same calls with fp32 timesteps to the same handle, every update in torch expressions on the device
    dplan, px0 = dpm_request_plan(ac, E2E[0]['S'])
    pairs = dpm_plan_pairs(dplan)
    buf = {0: inp[0][0].clone()}
    tab = make_tables(ac.numpy(), make_ddim_timesteps(E2E[1]['S'], ld.num_timesteps), 0.)
    state = inp[1][0].clone()
    full = lambda v: torch.full((1, 1, 1, 1), float(v), device='cuda')
    for call in plan:
        owners = [row[0] for row in call][0::2]
        x_of = {0: lambda: buf[int(dplan.ops[pairs[call[0][4]][0]][3])], 1: lambda: state}
        x_in = torch.cat([x_of[k]() for k in owners for _ in range(2)])
        t_in = torch.tensor([row[2] for row in call], device='cuda', dtype=torch.float32)
        c_in = torch.cat([t for k in owners for t in (inp[k][2], inp[k][1])])
        eps = ld.apply_model(x_in, t_in, c_in).float()
        for j, k in enumerate(owners):
            pair = eps[2 * j:2 * j + 2]
            if k == 0:
                ke, ku = pairs[call[2 * j][4]]
                sc = DC._scalars(dplan.coef[ke], 'cuda')
                op = dplan.ops[ke]
                buf[int(op[2])] = DC.torch_model_value(pair, buf[int(op[3])], True, E2E[0]['scale'], px0 or int(op[1]) == 1, sc[2], sc[3])
                if ku is not None:
                    op = dplan.ops[ku]
                    buf[int(op[2])] = DC.torch_update(int(op[1]), buf[int(op[3])], [buf[int(m)] for m in op[4:] if m >= 0],
                                                      DC._scalars(dplan.coef[ku], 'cuda'))
            else:
                index = call[2 * j][4]
                e_t = pair[0:1] + E2E[1]['scale'] * (pair[1:2] - pair[0:1])
                sqrt_at, sqrt_aprev = np.sqrt(np.float32(tab['alphas'][index])), np.sqrt(np.float32(tab['alphas_prev'][index]))
                dir_coef = np.sqrt(np.float32(1.0) - np.float32(tab['alphas_prev'][index]))
                pred = (state - full(tab['sqrt_one_minus_alphas'][index]) * e_t) / full(sqrt_at)
                state = full(sqrt_aprev) * pred + full(dir_coef) * e_t
    torch.cuda.synchronize()
    assert got[0][1] is None and torch.isfinite(got[0][0]).all()
    assert torch.equal(got[0][0], buf[dplan.result]), 'the DPM request'
    assert torch.equal(got[1][0], state), 'the DDIM request'


def test_lone_ddim_request_float_pool_equals_int_pool_over_the_hip_unet(tiny):
    """temb_kernel computes (float)t_i64[b] or t_f32[b]: an integer timestep handed over as fp32 gives the same embedding, so the same run"""
    unet, ld, inp = tiny
    x_T, c, uc = inp[1]
    outs = []
    for timesteps in ('int64', 'float32'):
        pool = SamplerPoolHIP(ld, (4, 8, 8), timesteps=timesteps)
        t = pool.submit(S=5, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=3.0, x_T=x_T, log_every_t=1)
        assert pool.run_until_idle() == 5
        outs.append(pool.result(t))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1]['pred_x0'], outs[1][1]['pred_x0']))
