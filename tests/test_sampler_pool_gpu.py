"""SamplerPoolHIP on the GPU.

With the exactly rounded stub model of tests/sampler_pool_cases.py: six staggered requests through a pool of 8 rows -- admissions and
retirements mid-flight, two requests waiting in the queue -- against the reference's own one-request-at-a-time CPU runs
(tests/golden/sampler_pool.npz, tools/make_golden_sampler_pool.py) and against the same request alone in DDIMSamplerHIP / PLMSSamplerHIP,
bit for bit.  Portability: the table scalars of a step pass through the CPU's sqrt in the reference run and through the host's sqrtf here;
the fixture's schedule was searched for timesteps at which torch's sqrt gave the correctly rounded value (the tool asserts it), as the
DDPM fixture's was.

With UNetModelHIP (tiny configuration, 8 x 8 latent): the pool against an explicit loop that issues plan_calls' calls to the same handle
and does every update in torch expressions, bit for bit; the cross-attention K/V recomputed exactly when the row set changes."""
import os

import numpy as np
import pytest
import torch

import sampler_pool_cases as PC
from stable_diffusion_amd import DDIMSamplerHIP, PLMSSamplerHIP, SamplerPoolHIP, plan_calls
from stable_diffusion_amd.samplers import make_ddim_timesteps, make_tables

pytestmark = pytest.mark.gpu
NAMES = list(PC.REQUESTS)


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'sampler_pool.npz'))


def _submit(pool, name, seqs):
    r = PC.REQUESTS[name]
    x_T, c, uc, draws = (v.cuda() if torch.is_tensor(v) else [d.cuda() for d in v] for v in PC.inputs(name))
    t = pool.submit(S=r['S'], conditioning=c, unconditional_conditioning=uc if PC.guided(name) else None,
                    unconditional_guidance_scale=r['scale'], eta=r.get('eta', 0.), x_T=x_T, sampler=r['sampler'], t_start=r.get('t_start'),
                    log_every_t=r['log_every_t'])
    seqs[t] = draws
    return t


@pytest.fixture(scope='module')
def pool_run(G):
    """the six requests through one pool, submitted at the call counts of PC.ARRIVAL -> (results by name, trace, rows per model call)"""
    model = PC.StubLD(G, 'cuda')
    pool = SamplerPoolHIP(model, PC.SHAPE, max_rows=PC.MAX_ROWS)
    pool.trace = []
    seqs, tickets = {}, {}
    pool._noise_like = lambda shape, device, generator=None, ticket=None: seqs[ticket].pop(0)
    while True:
        for name in NAMES:
            if name not in tickets and PC.ARRIVAL[name] <= pool.calls:
                tickets[name] = _submit(pool, name, seqs)
        if not pool.step():
            break
    assert all(pool.done(t) for t in tickets.values()) and pool.pending() == 0
    results = {name: pool.result(tickets[name]) for name in NAMES}
    torch.cuda.synchronize()
    left = {name: len(seqs[tickets[name]]) for name in NAMES}
    trace = [[(NAMES[row[0]],) + row[1:] for row in call] for call in pool.trace]
    return results, trace, model.calls, left


def test_pool_executes_the_plan(pool_run):
    results, trace, rows, left = pool_run
    plan = plan_calls([PC.plan_request(n) for n in NAMES], PC.MAX_ROWS, PC.TIMESTEPS)
    assert trace == plan and rows == [len(c) for c in plan]
    first = {n: min(k for k, c in enumerate(trace) if any(row[0] == n for row in c)) for n in NAMES}
    assert first['pair'] > PC.ARRIVAL['pair'] and first['decode'] > PC.ARRIVAL['decode']            # both waited in the queue
    assert len(plan) == 11 and sum(PC.n_draws(n) for n in NAMES) == 34                               # 11 UNet calls where 34 run alone
    # a request with eta > 0 took one draw per step, the others none
    assert left == {n: (0 if PC.REQUESTS[n].get('eta') else PC.n_draws(n)) for n in NAMES}


@pytest.mark.parametrize('name', NAMES)
def test_pool_equals_the_reference_run(G, pool_run, name):
    out, inter = pool_run[0][name]
    assert torch.equal(out.cpu(), torch.from_numpy(G[f'{name}_out'])), 'samples'
    assert inter['x_inter'][0].data_ptr() != out.data_ptr() and torch.equal(inter['x_inter'][0].cpu(), torch.from_numpy(G[f'{name}_x_T']))
    if f'{name}_pred_x0' in G.files:                # (DDIMSampler.decode returns no intermediates)
        for key in ('pred_x0', 'x_inter'):
            got = torch.stack(inter[key][1:]).cpu()
            assert torch.equal(got, torch.from_numpy(G[f'{name}_{key}'])), key
        assert inter['x_inter'][-1] is out


@pytest.mark.parametrize('name', NAMES)
def test_pool_equals_the_request_alone(G, pool_run, name):
    r = PC.REQUESTS[name]
    model = PC.StubLD(G, 'cuda')
    smp = (DDIMSamplerHIP if r['sampler'] == 'ddim' else PLMSSamplerHIP)(model)
    x_T, c, uc, draws = (v.cuda() if torch.is_tensor(v) else [d.cuda() for d in v] for v in PC.inputs(name))
    smp._noise_like = lambda shape, device: draws.pop(0)
    kw = dict(unconditional_guidance_scale=r['scale'], unconditional_conditioning=uc if PC.guided(name) else None)
    if r.get('t_start') is not None:
        smp.make_schedule(ddim_num_steps=r['S'], ddim_eta=0., verbose=False)
        alone, inter = smp.decode(x_T, c, r['t_start'], **kw), None
    else:
        alone, inter = smp.sample(S=r['S'], batch_size=r['samples'], shape=list(PC.SHAPE), conditioning=c, verbose=False, x_T=x_T,
                                  eta=r.get('eta', 0.), log_every_t=r['log_every_t'], **kw)
    out, pool_inter = pool_run[0][name]
    assert torch.equal(out, alone)
    if inter is not None:
        for key in ('pred_x0', 'x_inter'):
            assert len(inter[key]) == len(pool_inter[key]) and all(torch.equal(a, b) for a, b in zip(inter[key], pool_inter[key])), key


def test_neighbours_do_not_change_a_requests_draws(G):
    """eta > 0 with the request's own generator: the same bits alone and among other drawing requests"""
    x_T, c, uc, _ = (v.cuda() if torch.is_tensor(v) else v for v in PC.inputs('ddim8_eta'))

    def run(n_others):
        pool = SamplerPoolHIP(PC.StubLD(G, 'cuda'), PC.SHAPE, max_rows=PC.MAX_ROWS)
        for k in range(n_others):
            pool.submit(S=5, conditioning=c * (k + 2), eta=1.0, x_T=x_T + k)        # (a generator of their own each, seeded at submit)
        g = torch.Generator(device='cuda').manual_seed(77)
        t = pool.submit(S=8, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=5.0, eta=0.5, x_T=x_T, generator=g)
        pool.run_until_idle()
        return pool.result(t)[0]
    alone, shared = run(0), run(3)
    assert torch.equal(alone, shared)
    assert not torch.equal(alone.cpu(), torch.from_numpy(G['ddim8_eta_out']))      # (other draws than the recorded ones: the noise is live)


def test_token_count_and_shape_are_the_pools(G):
    pool = SamplerPoolHIP(PC.StubLD(G, 'cuda'), PC.SHAPE, max_rows=4)
    x_T, c, uc, _ = (v.cuda() if torch.is_tensor(v) else v for v in PC.inputs('ddim5'))
    pool.submit(S=5, conditioning=c, x_T=x_T)
    with pytest.raises(ValueError, match='token count'):
        pool.submit(S=5, conditioning=torch.zeros(1, PC.TOKENS[0] + 1, PC.TOKENS[1], device='cuda'))
    with pytest.raises(ValueError, match="is not the pool's"):
        pool.submit(S=5, conditioning=c, x_T=torch.zeros(1, 4, 8, 16, device='cuda'))
    with pytest.raises(RuntimeError, match='CPU tensors'):
        pool.submit(S=5, conditioning=c.cpu())
    assert pool.pending() == 1 and pool.run_until_idle() == 5


# ---- through UNetModelHIP ---------------------------------------------------------------------------------------------------------------
E2E = [dict(ticket=0, S=4, scale=7.5, arrival=0), dict(ticket=1, S=5, scale=3.0, arrival=1), dict(ticket=2, S=2, scale=5.0, arrival=3)]


def test_pool_over_the_hip_unet_equals_the_explicit_loop():
    from oracle.plan import TINY
    from oracle.weights import make_inputs, make_state_dict
    from stable_diffusion_amd import LatentDiffusionHIP, UNetModelHIP
    unet = UNetModelHIP(**TINY.ref_kwargs())
    unet.load_state_dict(make_state_dict(TINY, 0), strict=True)
    ld = LatentDiffusionHIP(unet).cuda()
    shape = (4, 8, 8)
    inp = []
    for r in E2E:
        x_T, _, ctx = make_inputs(TINY, 1, 8, 8, seed=20 + r['ticket'], ctx_len=7)
        inp.append((x_T.cuda(), ctx.cuda(), (torch.zeros_like(ctx) + 0.1 * (r['ticket'] + 1)).cuda()))
    plan = plan_calls([dict(ticket=r['ticket'], S=r['S'], guided=True, arrival=r['arrival']) for r in E2E], 8, ld.num_timesteps)
    row_sets = [[row[0] for row in call] for call in plan]
    changes = sum(1 for k, s in enumerate(row_sets) if k == 0 or s != row_sets[k - 1])
    assert changes == 5 and len(plan) == 6          # every admission and every retirement but the last changes the rows

    # the pool; the K/V are computed by pin_context when the row set changes and by no forward()
    pins = []
    pin = unet.pin_context
    unet.pin_context = lambda context: (pins.append(int(context.shape[0])), pin(context))[1]
    pool = SamplerPoolHIP(ld, shape)
    pool.trace = []
    tickets = {}
    try:
        while True:
            for r, (x_T, c, uc) in zip(E2E, inp):
                if r['ticket'] not in tickets and r['arrival'] <= pool.calls:
                    tickets[r['ticket']] = pool.submit(S=r['S'], conditioning=c, unconditional_conditioning=uc,
                                                       unconditional_guidance_scale=r['scale'], x_T=x_T, log_every_t=1)
            if not pool.step():
                break
            if pool.pending():
                assert unet._pinned == (len(pool.trace[-1]), 7), 'a forward() recomputed the K/V of an unchanged row set'
    finally:
        unet.pin_context = pin
    assert pool.trace == plan
    assert pins == [len(s) for k, s in enumerate(row_sets) if k == 0 or s != row_sets[k - 1]] and len(pins) == changes
    got = [pool.result(tickets[r['ticket']]) for r in E2E]

    # the explicit loop: the same calls to the same handle, every update in torch expressions (ddim.py:165-204) on the device
    ac = ld.alphas_cumprod.detach().float().cpu().numpy()
    tabs = [make_tables(ac, make_ddim_timesteps(r['S'], ld.num_timesteps), 0.) for r in E2E]
    state = [x.clone() for x, _, _ in inp]
    preds = [[] for _ in E2E]
    full = lambda v: torch.full((1, 1, 1, 1), float(v), device='cuda')
    for call in plan:
        owners = [row[0] for row in call][0::2]
        x_in = torch.cat([state[k] for k in owners for _ in range(2)])
        t_in = torch.tensor([row[2] for row in call], device='cuda', dtype=torch.long)
        c_in = torch.cat([t for k in owners for t in (inp[k][2], inp[k][1])])
        eps = ld.apply_model(x_in, t_in, c_in).float()
        for j, k in enumerate(owners):
            index = call[2 * j][4]
            e_u, e_c = eps[2 * j:2 * j + 1], eps[2 * j + 1:2 * j + 2]
            e_t = e_u + E2E[k]['scale'] * (e_c - e_u)
            T = tabs[k]
            sqrt_at, sqrt_aprev = np.sqrt(np.float32(T['alphas'][index])), np.sqrt(np.float32(T['alphas_prev'][index]))
            dir_coef = np.sqrt(np.float32(1.0) - np.float32(T['alphas_prev'][index]))
            pred = (state[k] - full(T['sqrt_one_minus_alphas'][index]) * e_t) / full(sqrt_at)
            state[k] = full(sqrt_aprev) * pred + full(dir_coef) * e_t
            preds[k].append(pred)
    torch.cuda.synchronize()
    for k, (out, inter) in enumerate(got):
        assert torch.equal(out, state[k]), f'request {k}: samples'
        assert len(inter['pred_x0']) == len(preds[k]) + 1 and all(torch.equal(a, b) for a, b in zip(inter['pred_x0'][1:], preds[k])), f'request {k}: pred_x0'

    # each request alone: another row composition changes the UNet's tile and split-K choices, which is not the pool's to bound
    for r, (x_T, c, uc), (out, _) in zip(E2E, inp, got):
        alone, _ = DDIMSamplerHIP(ld).sample(S=r['S'], batch_size=1, shape=list(shape), conditioning=c, verbose=False, x_T=x_T,
                                             unconditional_guidance_scale=r['scale'], unconditional_conditioning=uc, eta=0.)
        d = (out - alone).abs().max().item()
        print(f'[pool vs alone, tiny UNet 8x8] request {r["ticket"]} (S={r["S"]}, scale {r["scale"]}): max-abs {d:.3e} at |x| max '
              f'{alone.abs().max().item():.3f}')
        assert np.isfinite(d)
