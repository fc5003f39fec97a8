"""The sampler pool's host side, without a GPU: the plan (`plan_calls`) per request and across the queue, the refusals of `submit` and of
`sdmi_sampler_step_rows` (its checks run before anything is launched), and the descriptor's layout against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import sampler_pool_cases as PC
from stable_diffusion_amd import SamplerPoolHIP, _lib, plan_calls
from stable_diffusion_amd.samplers import make_ddim_timesteps, plms_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan of one request ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,discretize,t_start', [(50, 'uniform', None), (30, 'uniform', None), (7, 'quad', None), (20, 'uniform', 6), (1, 'uniform', None)])
def test_ddim_plan_is_the_flipped_time_range(S, discretize, t_start):
    calls = plan_calls([dict(ticket='a', S=S, ddim_discretize=discretize, t_start=t_start, guided=True)])
    ts = make_ddim_timesteps(S, 1000, discretize)
    ts = ts if t_start is None else ts[:t_start]
    total = len(ts)
    assert total == (31 if S == 30 else (t_start or S))                 # range(0, 1000, 1000 // 30) has 31 entries: so has the reference's loop
    want = [[('a', 0, int(t), 0, total - i - 1, 0)] * 2 for i, t in enumerate(np.flip(ts))]
    assert calls == want


@pytest.mark.parametrize('S', [50, 30, 6, 3, 2])
def test_plms_plan_has_the_double_evaluation(S):
    calls = plan_calls([dict(ticket=7, S=S, sampler='plms', samples=2)])
    plan = plms_plan(make_ddim_timesteps(S, 1000))
    assert len(plan) == len(range(0, 1000, 1000 // S)) and len(calls) == len(plan) + 1          # (S = 30: 31 steps, 32 evaluations)
    rows = [c[0][2:] for c in calls]
    assert all(c == [(7, 0) + r, (7, 1) + r] for c, r in zip(calls, rows))          # two unguided samples: one row each, same step
    (i, index, t, t_next, mode) = plan[0]
    assert mode == 4 and rows[0] == (t, 0, index, 0) and rows[1] == (t_next, 4, index, 1)        # predictor at t, corrector at t_next
    assert rows[2:] == [(t, mode, index, 0) for (i, index, t, t_next, mode) in plan[1:]]
    assert [r[1] for r in rows[2:5]] == [1, 2, 3][:len(rows) - 2] and all(r[1] == 3 for r in rows[5:])
    assert rows[-1][2] == 0 and rows[-1][0] == 1


# ---- the queue --------------------------------------------------------------------------------------------------------------------------
def _tickets(call):
    out = []
    for row in call:
        if not out or out[-1] != row[0]:
            out.append(row[0])
    return out


def test_queue_is_fifo_and_the_head_is_never_overtaken():
    """4 rows: 'a' (2 rows, 3 calls) runs; 'big' (4 rows) has to wait for an empty pool; 'small' (1 row) would fit beside 'a' at once but
    came later: it waits behind 'big'"""
    reqs = [dict(ticket='a', S=3, guided=True), dict(ticket='big', S=2, samples=2, guided=True, arrival=1),
            dict(ticket='small', S=2, arrival=1), dict(ticket='late', S=1, arrival=2)]
    calls = plan_calls(reqs, max_rows=4, num_timesteps=600)
    assert [_tickets(c) for c in calls] == [['a'], ['a'], ['a'], ['big'], ['big'], ['small', 'late'], ['small']]
    assert [len(c) for c in calls] == [2, 2, 2, 4, 4, 2, 1]


def test_rows_close_up_and_freed_rows_are_reused():
    """mixed guided / unguided requests in 8 rows: the budget holds in every call, a request's rows are adjacent and in admission order,
    and the rows a finished request leaves are taken by the ones behind it and then by the queue"""
    names = list(PC.REQUESTS)
    calls = plan_calls([PC.plan_request(n) for n in names], PC.MAX_ROWS, PC.TIMESTEPS)
    assert [len(c) for c in calls] == [5, 7, 7, 7, 8, 8, 8, 8, 2, 2, 2]
    assert [_tickets(c) for c in calls][:6] == [names[:3], names[:4], names[:4], names[:4], ['ddim5', 'ddim8_eta', 'plms6', 'pair'],
                                                ['ddim8_eta', 'plms6', 'pair', 'decode']]
    first = {}
    for k, c in enumerate(calls):
        assert len(c) <= PC.MAX_ROWS
        order = _tickets(c)
        assert len(order) == len(set(order))                            # each request's rows are one adjacent run
        for t in order:
            first.setdefault(t, k)
            n = sum(1 for row in c if row[0] == t)
            assert n == PC.REQUESTS[t]['samples'] * (2 if PC.guided(t) else 1)
        assert order == sorted(order, key=lambda t: (first[t], names.index(t)))            # admission order
        for t in order:
            if PC.guided(t):
                rows = [row for row in c if row[0] == t]
                assert rows[0::2] == rows[1::2]                         # [uncond, cond] of the same sample at the same step
    assert first == {'ddim5': 0, 'ddim8_eta': 0, 'plms3': 0, 'plms6': 1, 'pair': 4, 'decode': 5}      # 'pair' and 'decode' waited
    # 'ddim8_eta' starts at rows 2-3, moves to 0-1 when 'ddim5' leaves; 'pair' enters on the rows 'plms3' and the shift freed
    start = lambda k, t: [row[0] for row in calls[k]].index(t)
    assert [start(k, 'ddim8_eta') for k in range(8)] == [2, 2, 2, 2, 2, 0, 0, 0]
    assert start(4, 'pair') == 6 and start(5, 'pair') == 4 and start(5, 'decode') == 6


def test_an_idle_pool_takes_the_next_request_at_once():
    calls = plan_calls([dict(ticket=0, S=2), dict(ticket=1, S=2, arrival=9)], num_timesteps=600)
    assert [_tickets(c) for c in calls] == [[0], [0], [1], [1]]
    with pytest.raises(ValueError, match='can never fit'):
        plan_calls([dict(ticket=0, S=2, samples=5, guided=True)])


# ---- submit's refusals: each by name, before the request touches a device ------------------------------------------------------------
class _CpuModel:
    num_timesteps = 1000
    betas = torch.zeros(1000)
    alphas_cumprod = torch.linspace(0.999, 0.01, 1000)

    def apply_model(self, x, t, c):
        raise AssertionError('no call')


@pytest.mark.parametrize('kw,exc,name', [
    (dict(mask=torch.ones(1, 1, 8, 8)), NotImplementedError, 'mask / x0'),
    (dict(x0=torch.ones(1, 4, 8, 8)), NotImplementedError, 'mask / x0'),
    (dict(quantize_x0=True), NotImplementedError, 'quantize_x0'),
    (dict(score_corrector=object()), NotImplementedError, 'score_corrector'),
    (dict(conditioning=dict(c_crossattn=[torch.zeros(1, 3, 5)])), NotImplementedError, 'dict conditioning'),
    (dict(sampler='dpm'), NotImplementedError, "sampler='dpm'"),
    (dict(sampler='plms', eta=0.5), ValueError, 'eta must be 0 for PLMS'),
    (dict(x_T=torch.zeros(1, 4, 8, 9)), ValueError, "is not the pool's"),
    (dict(conditioning=torch.zeros(1, 4, 5)), ValueError, 'token count'),
    (dict(conditioning=torch.zeros(3, 3, 5), unconditional_conditioning=torch.zeros(3, 3, 5), unconditional_guidance_scale=2.), ValueError,
     'can never fit'),
    (dict(), RuntimeError, 'CPU tensors'),
])
def test_submit_refuses_by_name(kw, exc, name):
    pool = SamplerPoolHIP(_CpuModel(), shape=(4, 8, 8), max_rows=4)
    pool._tokens = (3, 5)            # as after a first accepted request
    args = dict(S=10, conditioning=torch.zeros(1, 3, 5))
    args.update(kw)
    with pytest.raises(exc, match=name):
        pool.submit(**args)
    assert pool.pending() == 0 and pool.step() is False


def test_pool_defaults():
    from stable_diffusion_amd import UNetModelHIP
    pool = SamplerPoolHIP(_CpuModel(), shape=(4, 64, 64))
    assert pool.max_rows == UNetModelHIP.MAX_ROWS == _lib.SAMPLER_MAX_SLOTS and pool.n == 4 * 64 * 64
    assert not pool.done(0)
    with pytest.raises(KeyError, match='not done'):
        pool.result(0)


# ---- the entry point: additive, its descriptor laid out as the header's, its checks in front of the launch -----------------------------
FIELDS = [f[0] for f in _lib.SamplerSlot._fields_]


def test_descriptor_layout_equals_the_header():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    assert '#define SDMI_ABI_VERSION 17' in hdr and lib.sdmi_abi_version() == 17
    assert 'sdmi_sampler_step_rows' in _lib.exported_symbols() and 'sdmi_sampler_step_rows(' in hdr
    assert f'#define SDMI_SAMPLER_MAX_SLOTS {_lib.SAMPLER_MAX_SLOTS}\n' in hdr
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sdmi.h"\nint main(){ printf("%zu", sizeof(sdmi_sampler_slot));\n' + \
        ''.join(f'printf(" %zu", offsetof(sdmi_sampler_slot, {f}));\n' for f in FIELDS) + 'return 0; }\n'
    d = os.path.join(ROOT, 'stable-diffusion_amd', 'build')
    os.makedirs(d, exist_ok=True)
    c, exe = os.path.join(d, 'abi_probe_sampler_rows.c'), os.path.join(d, 'abi_probe_sampler_rows')
    open(c, 'w').write(src)
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.SamplerSlot)] + [getattr(_lib.SamplerSlot, f).offset for f in FIELDS]
    assert got[0] == 152 and got[0] < 200


def _slot(**kw):
    s = _lib.SamplerSlot()
    s.eps_u, s.x, s.x_state_out = 256, 512, 512           # never dereferenced: every case below fails its check before the launch
    s.a_t, s.a_prev, s.scale = 0.5, 0.6, 1.0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize('slots,n,name', [
    ([_slot()] * 9, 64, 'more than SDMI_SAMPLER_MAX_SLOTS'),
    ([_slot()], 0, 'sampler_step_rows: n'),
    ([_slot()], -4, 'sampler_step_rows: n'),
    ([_slot(x=None)], 64, 'missing pointer'),
    ([_slot(eps_u=None)], 64, 'missing pointer'),
    ([_slot(cfg=1)], 64, 'missing pointer'),                           # guided without eps_c
    ([_slot(x_state_out=None)], 64, 'missing pointer: no output'),
    ([_slot(), _slot(mode=5)], 64, r'sampler_step_rows: mode \(slot 1\)'),
    ([_slot(mode=-1)], 64, 'sampler_step_rows: mode'),
    ([_slot(mode=1)], 64, 'history missing'),
    ([_slot(mode=4)], 64, 'history missing'),
    ([_slot(mode=2, old0=768)], 64, 'history missing'),
    ([_slot(mode=3, old0=768, old1=1024)], 64, 'history missing'),
])
def test_entry_refuses_by_name_before_the_launch(slots, n, name):
    import re
    lib = _lib.load()
    arr = (_lib.SamplerSlot * len(slots))(*slots)
    assert lib.sdmi_sampler_step_rows(arr, len(slots), n, None) != 0
    assert re.search(name, lib.sdmi_last_error().decode())
    assert lib.sdmi_sampler_step_rows(None, 1, 64, None) != 0
