"""The fp32-timestep sampler pool's host side, without a GPU: DPM-Solver requests in `plan_calls` (a DPMPlan's evaluations are a request's
rows; arrivals, waiting and closing up as for DDIM), the alternation every plan of tests/dpm_cases.py keeps, the refusals of a float
pool's `submit` by name and the default pool's unchanged one, the refusals of `sdmi_sampler_plan_rows` (its checks run before anything is
launched), and the new descriptor's layout against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dpm_cases as DC
from stable_diffusion_amd import SamplerPoolHIP, _lib, plan_calls
from stable_diffusion_amd.sampler_pool import dpm_plan_pairs, dpm_request_plan, request_evals
from stable_diffusion_amd.samplers import DPMSolverHIP, _DiscreteVP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANNED = [n for n in DC.CASES if n != 'thresholding']


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'dpm_variants.npz'))


def _plan(name):
    case = DC.CASES[name]
    return DPMSolverHIP(None, _DiscreteVP(DC.alphas_cumprod()), predict_x0=case['predict_x0']).plan(**case['sample'])


# ---- the plan of one request ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', PLANNED)
def test_every_plan_alternates_evaluation_and_update(G, name):
    """computed here and as recorded by the reference run: EVAL, UPDATE, EVAL, ... -- ending in an EVAL exactly with denoise_to_zero --
    and every evaluation after the first is at the state the update before it wrote; a request's rows are its evaluations"""
    for plan in (_plan(name), DC.load_plan(G, name)):
        kinds = plan.ops[:, 0].tolist()
        assert kinds[0::2] == [0] * len(kinds[0::2]) and kinds[1::2] == [1] * len(kinds[1::2])
        assert (kinds[-1] == 0) == bool(DC.CASES[name]['sample'].get('denoise_to_zero'))
        pairs = dpm_plan_pairs(plan)
        assert [k for k, _ in pairs] == [k for k, kind in enumerate(kinds) if kind == 0]
        assert all(u == k + 1 for k, u in pairs[:-1]) and pairs[-1][1] == (None if kinds[-1] == 0 else pairs[-1][0] + 1)
        assert all(plan.ops[k][3] == plan.ops[k - 1][2] for k, _ in pairs[1:])
        evals = request_evals('dpm', None, plan)
        assert [e[0] for e in evals] == plan.model_times() and [e[2] for e in evals] == list(range(len(plan.model_times())))
        assert [e[1] for e in evals] == [-1 if u is None else int(plan.ops[u][1]) for _, u in pairs] and all(e[3] == 0 for e in evals)
    assert len(DC.load_plan(G, name).model_times()) == len(G[f'{name}_calls'])


def test_a_plan_that_does_not_alternate_is_refused():
    plan = _plan('ms1_x0')
    plan.ops = np.concatenate([plan.ops[:1], plan.ops])
    plan.coef = np.concatenate([plan.coef[:1], plan.coef])
    with pytest.raises(ValueError, match='does not alternate'):
        dpm_plan_pairs(plan)
    plan = _plan('ms1_x0')
    plan.ops[2][3] = 0                   # the second evaluation at the initial latent instead of the first update's state
    with pytest.raises(ValueError, match='not at the state'):
        dpm_plan_pairs(plan)


def test_default_request_is_dpm_solver_pp_2m():
    """no keyword: what DPMSolverSamplerHIP runs by default -- multistep, order 2, time_uniform, data prediction, S evaluations"""
    ac = DC.alphas_cumprod()
    plan, px0 = dpm_request_plan(ac, 10)
    want = DPMSolverHIP(None, _DiscreteVP(ac), predict_x0=True).plan(steps=10, order=2, skip_type='time_uniform', method='multistep',
                                                                     lower_order_final=True)
    assert px0 is True and np.array_equal(plan.ops, want.ops) and np.array_equal(plan.coef, want.coef)
    assert len(plan.model_times()) == 10 and plan.orders.tolist() == [1] + [2] * 8 + [1]
    calls = plan_calls([dict(ticket='d', S=10, sampler='dpm', guided=True)], alphas_cumprod=ac)
    forms = [1 if o == 2 else 0 for o in plan.orders]
    assert calls == [[('d', 0, t, f, k, 0)] * 2 for k, (t, f) in enumerate(zip(plan.model_times(), forms))]
    other, px0 = dpm_request_plan(ac, 6, predict_x0=False, method='singlestep', order=3, skip_type='logSNR')
    assert px0 is False and other.orders.tolist() == [3, 2, 1]
    ready, _ = dpm_request_plan(None, None, plan=other, predict_x0=False)
    assert ready is other


# ---- the queue: DPM requests beside DDIM / PLMS ones ----------------------------------------------------------------------------------
def _tickets(call):
    out = []
    for row in call:
        if not out or out[-1] != row[0]:
            out.append(row[0])
    return out


def test_dpm_requests_arrive_wait_and_close_up_as_ddim_ones(G):
    """4 rows: 'a' (guided DPM, 5 evaluations) and 'd' (DDIM, 3 steps) run; 'big' (two guided samples) waits for an empty pool and
    'late' waits behind it though it would fit; when 'd' leaves nothing moves ('a' came first), when 'a' leaves 'big' enters"""
    ms1, ss2 = DC.load_plan(G, 'ms1_x0'), DC.load_plan(G, 'ss2_s5_x0')
    assert len(ms1.model_times()) == 5 and len(ss2.model_times()) == 5
    reqs = [dict(ticket='a', sampler='dpm', plan=ms1, guided=True), dict(ticket='d', S=3, guided=True),
            dict(ticket='big', sampler='dpm', plan=ss2, samples=2, guided=True, arrival=1), dict(ticket='late', sampler='dpm', plan=ms1, arrival=2)]
    calls = plan_calls(reqs, max_rows=4, num_timesteps=600)
    assert [_tickets(c) for c in calls] == [['a', 'd']] * 3 + [['a']] * 2 + [['big']] * 5 + [['late']] * 5
    assert [len(c) for c in calls] == [4] * 3 + [2] * 2 + [4] * 5 + [1] * 5
    a_rows = [c[0] for c in calls[:5]]
    assert a_rows == [('a', 0, t, 0, k, 0) for k, t in enumerate(ms1.model_times())]          # order 1 throughout: form 0 after each
    assert calls[0][2] == ('d', 0, 401, 0, 2, 0)
    big = [c[2] for c in calls[5:10]]                # the second sample's unconditional row
    assert [r[:2] for r in big] == [('big', 1)] * 5 and [r[2] for r in big] == ss2.model_times() and [r[4] for r in big] == list(range(5))
    # an idle pool takes the next request at once; one that can never fit is refused
    assert [_tickets(c) for c in plan_calls([dict(ticket=0, sampler='dpm', plan=ms1, arrival=7)])] == [[0]] * 5
    with pytest.raises(ValueError, match='can never fit'):
        plan_calls([dict(ticket=0, sampler='dpm', plan=ms1, samples=5, guided=True)])
    with pytest.raises(ValueError, match='needs the schedule'):
        plan_calls([dict(ticket=0, sampler='dpm', S=5)])


# ---- submit's refusals: each by name, before the request touches a device ------------------------------------------------------------
class _CpuModel:
    num_timesteps = 1000
    betas = torch.zeros(1000)
    alphas_cumprod = DC.alphas_cumprod()

    def apply_model(self, x, t, c):
        raise AssertionError('no call')


@pytest.mark.parametrize('kw,exc,name', [
    (dict(sampler='dpm', method='adaptive'), NotImplementedError, "method='adaptive'"),
    (dict(sampler='dpm', thresholding=True), NotImplementedError, 'thresholding=True'),
    (dict(sampler='dpm', eta=0.5), ValueError, 'eta must be 0 for DPM-Solver'),
    (dict(sampler='dpm', method='singlestep', order=3), ValueError, "skip_type='time_uniform' raises in the reference"),     # DPMSolverHIP.plan's own
    (dict(sampler='dpm', method='multistep', order=3), ValueError, '4 <= steps < 15 raises in the reference'),
    (dict(sampler='dpm', method='euler'), ValueError, "method 'euler'"),
    (dict(sampler='dpm', atol=0.1), TypeError, "sampler='dpm' takes"),
    (dict(sampler='ddim', order=2), TypeError, "keywords of sampler='dpm'"),
    (dict(sampler='heun'), NotImplementedError, "'ddim' or 'plms' or 'dpm'"),
    (dict(sampler='dpm', mask=torch.ones(1, 1, 8, 8)), NotImplementedError, 'mask / x0'),
    (dict(sampler='dpm', quantize_x0=True), NotImplementedError, 'quantize_x0'),
    (dict(sampler='dpm', conditioning=dict(c_crossattn=[torch.zeros(1, 3, 5)])), NotImplementedError, 'dict conditioning'),
    (dict(sampler='plms', eta=0.5), ValueError, 'eta must be 0 for PLMS'),
    (dict(sampler='dpm', x_T=torch.zeros(1, 4, 8, 9)), ValueError, "is not the pool's"),
    (dict(sampler='dpm', conditioning=torch.zeros(1, 4, 5)), ValueError, 'token count'),
    (dict(sampler='dpm'), RuntimeError, 'CPU tensors'),                  # (everything else is in order: the next check is the device's)
    (dict(), RuntimeError, 'CPU tensors'),
])
def test_float_pool_submit_refuses_by_name(kw, exc, name):
    pool = SamplerPoolHIP(_CpuModel(), shape=(4, 8, 8), max_rows=4, timesteps='float32')
    pool._tokens = (3, 5)            # as after a first accepted request
    args = dict(S=10, conditioning=torch.zeros(1, 3, 5))
    args.update(kw)
    with pytest.raises(exc, match=name):
        pool.submit(**args)
    assert pool.pending() == 0 and pool.step() is False


def test_default_pool_still_refuses_dpm_with_its_text():
    for kw in (dict(), dict(timesteps='int64')):
        pool = SamplerPoolHIP(_CpuModel(), shape=(4, 8, 8), max_rows=4, **kw)
        assert pool.timesteps == 'int64'
        with pytest.raises(NotImplementedError, match=re.escape("sampler='dpm': DPM-Solver's float timesteps cannot share a call with integer ones")):
            pool.submit(S=10, conditioning=torch.zeros(1, 3, 5), sampler='dpm')
        with pytest.raises(NotImplementedError, match="sampler='heun': 'ddim' or 'plms'$"):
            pool.submit(S=10, conditioning=torch.zeros(1, 3, 5), sampler='heun')
        assert pool.pending() == 0
    with pytest.raises(ValueError, match="'int64' or 'float32'"):
        SamplerPoolHIP(_CpuModel(), shape=(4, 8, 8), timesteps='float16')


# ---- the entry point: additive, its descriptor laid out as the header's, its checks in front of the launch -----------------------------
FIELDS = [f[0] for f in _lib.SamplerPlanSlot._fields_]


def test_plan_descriptor_layout_equals_the_header():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    assert '#define SDMI_ABI_VERSION 17' in hdr and lib.sdmi_abi_version() == 17
    assert 'sdmi_sampler_plan_rows' in _lib.exported_symbols() and 'sdmi_sampler_plan_rows(' in hdr
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sdmi.h"\nint main(){ printf("%zu", sizeof(sdmi_sampler_plan_slot));\n' + \
        ''.join(f'printf(" %zu", offsetof(sdmi_sampler_plan_slot, {f}));\n' for f in FIELDS) + \
        'printf(" %zu", sizeof(sdmi_sampler_slot)); return 0; }\n'
    d = os.path.join(ROOT, 'stable-diffusion_amd', 'build')
    os.makedirs(d, exist_ok=True)
    c, exe = os.path.join(d, 'abi_probe_sampler_plan_rows.c'), os.path.join(d, 'abi_probe_sampler_plan_rows')
    open(c, 'w').write(src)
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:-1] == [C.sizeof(_lib.SamplerPlanSlot)] + [getattr(_lib.SamplerPlanSlot, f).offset for f in FIELDS]
    assert got[0] == 248
    assert (got[0] + 16) * _lib.SAMPLER_MAX_SLOTS + 8 <= 4096            # with the launcher's derived scalars: within HIP's kernel arguments
    assert got[-1] == C.sizeof(_lib.SamplerSlot) == 152                  # the existing descriptor is as it was


def _slot(**kw):
    """a kind 1 slot in order (form 0 on the value just computed); never dereferenced: every case below fails its check before the launch"""
    s = _lib.SamplerPlanSlot()
    s.kind, s.eps_u, s.x, s.x_base, s.x_state_out, s.data_prediction, s.m_self = 1, 256, 512, 768, 1024, 1, 1
    s.alpha_t, s.sigma_t, s.scale = 0.5, 0.6, 1.0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _step(**kw):
    return _slot(kind=0, a_t=0.5, a_prev=0.6, **kw)


@pytest.mark.parametrize('slots,n,name', [
    ([_slot()] * 9, 64, 'more than SDMI_SAMPLER_MAX_SLOTS'),
    ([_slot()], 0, 'sampler_plan_rows: n'),
    ([_slot()], -4, 'sampler_plan_rows: n'),
    ([_slot(kind=2)], 64, 'sampler_plan_rows: kind'),
    ([_slot(eps_u=None)], 64, 'missing pointer'),
    ([_slot(cfg=1)], 64, 'missing pointer'),                             # guided without eps_c
    ([_slot(x=None)], 64, 'the data prediction needs x'),
    ([_slot(x_base=None)], 64, 'missing pointer: x_base'),
    ([_slot(m_self=0)], 64, 'a model value of the update'),              # form 0 reads m0: neither given nor the value just computed
    ([_slot(form=1, m1=1280)], 64, 'a model value of the update'),       # m2 missing
    ([_slot(form=3, m_self=0, m0=1280, m2=1536)], 64, 'a model value of the update'),
    ([_slot(x_state_out=None)], 64, 'missing pointer: no output'),
    ([_slot(form=-1, m_self=0, x_base=None, x_state_out=None, tf_dst0=2048)], 64, 'missing pointer: no output'),
    ([_slot(), _slot(form=4)], 64, r'sampler_plan_rows: form \(slot 1\)'),
    ([_slot(form=-2)], 64, 'sampler_plan_rows: form'),
    ([_slot(form=-1)], 64, 'm_self names an operand'),                   # no update reads nothing
    ([_slot(m_self=3)], 64, 'm_self names an operand'),                  # form 0 reads m0 alone
    ([_slot(form=2, m_self=8)], 64, 'm_self names an operand'),
    ([_step(x=None)], 64, 'missing pointer'),
    ([_step(x_state_out=None)], 64, 'missing pointer: no output'),
    ([_step(), _step(mode=5)], 64, r'sampler_plan_rows: mode \(slot 1\)'),
    ([_step(mode=-1)], 64, 'sampler_plan_rows: mode'),
    ([_step(mode=1)], 64, 'history missing'),
    ([_step(mode=2, old0=1280)], 64, 'history missing'),
    ([_step(mode=3, old0=1280, old1=1536)], 64, 'history missing'),
])
def test_plan_entry_refuses_by_name_before_the_launch(slots, n, name):
    lib = _lib.load()
    arr = (_lib.SamplerPlanSlot * len(slots))(*slots)
    assert lib.sdmi_sampler_plan_rows(arr, len(slots), n, None) != 0
    assert re.search(name, lib.sdmi_last_error().decode()), lib.sdmi_last_error()
    assert lib.sdmi_sampler_plan_rows(None, 1, 64, None) != 0
