"""The DPM-Solver variants, host side (no GPU): the plans of DPMSolverHIP -- time grids, orders, model-input times, every coefficient --
against what tools/make_golden_dpm_variants.py recorded next to the reference runs (tests/golden/dpm_variants.npz), inverse_lambda
and the singlestep order lists against the reference's, the refusals, and DPMSolverHIP's own loops with the launches replaced by the
torch expressions of tests/dpm_cases.py.

Non-portability: the scalars pass through torch's CPU exp / log / sqrt / expm1 / logaddexp, whose last bit depends on the CPU model
(tests/test_ddpm_host.py saw 23 of 1000 values differ between two hosts with one torch build).  The bit-for-bit comparisons of scalars
below therefore hold on the CPU model the fixture was recorded on; the GPU trajectory tests replay the recorded scalars instead."""
import os

import numpy as np
import pytest
import torch

import dpm_cases as DC


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'dpm_variants.npz'))


def solver_of(case, calls=None, device='cpu'):
    from stable_diffusion_amd.samplers import DPMSolverHIP, _DiscreteVP
    scale = case['scale']
    return DPMSolverHIP(DC.eps_fn_of(DC.MODELS[case.get('model', 'stub')], scale, calls, device), _DiscreteVP(DC.alphas_cumprod()),
                        predict_x0=case['predict_x0'], thresholding=case.get('thresholding', False), max_val=case.get('max_val', 1.),
                        cfg=scale is not None, scale=1. if scale is None else scale)


def emulate(solver):
    """the two launches of DPMSolverHIP in torch (dpm_cases.torch_model_value / torch_update): the loops run on the CPU"""
    def model_value(x, t_input, alpha_t, sigma_t, data_prediction):
        solver.model_times.append(float(t_input))
        a, s = DC._scalars([alpha_t, sigma_t], x.device)
        return DC.torch_model_value(solver.eps_fn(x, t_input), x, solver.cfg, solver.scale, data_prediction, a, s,
                                    solver.thresholding and data_prediction, solver.max_val)
    solver._model_value = model_value
    solver._update = lambda form, x, ms, coef: DC.torch_update(form, x, list(ms), DC._scalars(
        [v if not torch.is_tensor(v) else float(v.reshape(-1)[0]) for v in coef] + [0.0] * (9 - len(coef)), x.device))

    def error(x_higher, x_lower, x_prev, atol, rtol):           # :952-954
        delta = torch.max(torch.ones_like(x_lower) * atol, rtol * torch.max(torch.abs(x_lower), torch.abs(x_prev)))
        norm_fn = lambda v: torch.sqrt(torch.square(v.reshape((v.shape[0], -1))).mean(dim=-1, keepdim=True))
        return norm_fn((x_higher - x_lower) / delta).max().cpu()
    solver._error = error
    return solver


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('name', list(DC.CASES))
def test_host_plan_equals_the_recorded_plan(G, name):
    """timesteps, orders, the op list and every coefficient, bit for bit (on the recording CPU model: see the module docstring); the
    cases cover logSNR, time_uniform and time_quadratic grids"""
    case = DC.CASES[name]
    plan = solver_of(case).plan(**case['sample'])
    want = DC.load_plan(G, name)
    assert np.array_equal(plan.ops, want.ops) and plan.result == want.result
    assert np.array_equal(plan.orders, want.orders)
    assert np.array_equal(bits(plan.timesteps), bits(want.timesteps))
    assert np.array_equal(bits(plan.coef), bits(want.coef))
    assert np.array_equal(bits(plan.model_times()), bits(G[f'{name}_calls']))


@pytest.mark.parametrize('name', list(DC.CASES))
def test_plan_loop_reaches_the_reference_end_point(G, name):
    """DPMSolverHIP.run_plan over the recorded plan, launches emulated in torch: the reference's end point bit for bit, its model calls"""
    case = DC.CASES[name]
    calls = []
    solver = emulate(solver_of(case, calls))
    out = solver.run_plan(DC.case_x(int(G[f'{name}_seed'])), DC.load_plan(G, name))
    assert torch.equal(out, torch.from_numpy(G[f'{name}_out']))
    assert np.array_equal(bits(calls), bits(G[f'{name}_calls'])) and solver.model_times == calls


@pytest.mark.parametrize('name', list(DC.ADAPTIVE))
def test_adaptive_loop_makes_the_reference_decisions(G, name):
    """DPMSolverHIP.dpm_solver_adaptive on the CPU with emulated launches and the error norm in torch: the reference's accept / reject
    sequence and evaluation count (GAP keeps every decision away from rounding), its end point to 2e-4"""
    case = DC.ADAPTIVE[name]
    solver = emulate(solver_of(case))
    x = DC.case_x(int(G[f'{name}_seed']))
    got = solver.sample(x, **case['sample'])
    log, times = solver.adaptive_log, solver.model_times
    assert [a for _, a in log] == G[f'{name}_accept'].tolist() and len(times) == len(G[f'{name}_calls'])
    assert np.allclose([e for e, _ in log], G[f'{name}_E'], rtol=1e-4)
    assert float((got - torch.from_numpy(G[f'{name}_out'])).abs().max()) <= 2e-4
    got2, log2, times2 = DC.torch_adaptive_loop(solver_of(case), x, case['sample']['order'])       # the restatement the GPU tests compare with
    assert torch.equal(got2, got) and log2 == log and times2 == times
    assert min(abs(float(e) - 1.) for e in G[f'{name}_E']) >= DC.GAP
    assert any(not a for n in DC.ADAPTIVE for a in G[f'{n}_accept'])


def test_inverse_lambda_equals_the_reference(G):
    from stable_diffusion_amd.samplers import _DiscreteVP
    ns = _DiscreteVP(DC.alphas_cumprod())
    t = ns.inverse_lambda(torch.from_numpy(G['il_lambda']))
    assert np.array_equal(bits(t.numpy()), bits(G['il_t']))
    back = ns.lam(t)                       # and it inverts marginal_lambda inside the table
    assert np.allclose(back.numpy()[1:-1], G['il_lambda'][1:-1], rtol=0, atol=2e-3)


@pytest.mark.parametrize('steps', DC.SINGLESTEP_STEPS)
def test_singlestep_orders_and_outer_timesteps(G, steps):
    ts, orders = solver_of(DC.CASES['ss3_s3_eps']).get_orders_and_timesteps_for_singlestep_solver(steps, 3, 'logSNR', 1., 1e-3)
    assert orders == G[f'ss_orders_{steps}'].tolist() and sum(orders) == steps
    assert np.array_equal(bits(ts.numpy()), bits(G[f'ss_timesteps_{steps}']))


def test_the_refusals_name_their_reference_line():
    s = solver_of(DC.CASES['ss3_s3_eps'])
    for skip in ('time_uniform', 'time_quadratic'):
        with pytest.raises(ValueError, match=r'dpm_solver\.py:495'):
            s.plan(steps=6, order=3, method='singlestep', skip_type=skip)
    for steps in (4, 7, 14):
        with pytest.raises(ValueError, match=r'dpm_solver\.py:773'):
            s.plan(steps=steps, order=3, method='multistep', lower_order_final=True)
    with pytest.raises(ValueError, match=r'dpm_solver\.py:1114'):
        s.plan(steps=4, order=1, method='singlestep', skip_type='logSNR')
    # what the reference does run next to them
    assert s.plan(steps=15, order=3, method='multistep').orders.tolist() == [1, 2] + [3] * 13
    assert s.plan(steps=7, order=3, method='multistep', lower_order_final=False).orders.tolist() == [1, 2, 3, 3, 3, 3, 3]
    assert s.plan(steps=3, order=3, method='multistep').orders.tolist() == [1, 2, 1]        # (the history is never unpacked at order 2 here)
    assert s.plan(steps=1, order=1, method='singlestep', skip_type='logSNR').orders.tolist() == [1]
    with pytest.raises(ValueError):
        s.plan(steps=4, method='heun')
    with pytest.raises(ValueError):
        s.plan(steps=4, order=2, method='multistep', skip_type='cosine')


def test_sampler_without_new_keywords_builds_todays_plan():
    """DPMSolverSamplerHIP.sample(S) without a DPM-Solver keyword runs dpm_plan through sdmi_dpm_solver_step, as before; and the
    general plan of the same configuration carries the same scalars (c1 = -a, c2 = -(0.5 a) -- the kernel halves a itself)"""
    from stable_diffusion_amd.samplers import DPMSolverHIP, DPMSolverSamplerHIP, _DiscreteVP, dpm_plan
    model = type('M', (), dict(num_timesteps=1000, alphas_cumprod=DC.alphas_cumprod()))()
    smp = DPMSolverSamplerHIP(model)
    for S in (2, 7, 20):
        old = dpm_plan(_DiscreteVP(DC.alphas_cumprod()), S)
        assert smp.plan(S) == old
        new = DPMSolverHIP(None, _DiscreteVP(DC.alphas_cumprod()), predict_x0=True).plan(steps=S, order=2, skip_type='time_uniform',
                                                                                         method='multistep')
        evals = [c for o, c in zip(new.ops, new.coef) if o[0] == 0]
        upds = [(o, c) for o, c in zip(new.ops, new.coef) if o[0] == 1]
        assert len(evals) == len(upds) == S
        for (t_input, alpha_s, sigma_s, order, cx, a, inv_r0), e, (o, c) in zip(old, evals, upds):
            assert (np.float32(t_input), np.float32(alpha_s), np.float32(sigma_s)) == (e[1], e[2], e[3])
            assert int(o[1]) == order - 1 and c[0] == np.float32(cx) and c[1] == -np.float32(a)
            if order == 2:
                assert c[2] == -(np.float32(0.5) * np.float32(a)) and c[3] == np.float32(inv_r0)


def test_abi_is_additive():
    from stable_diffusion_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sdmi.h')).read()
    for name in ('sdmi_dpm_model_value', 'sdmi_dpm_update', 'sdmi_dpm_threshold_scale', 'sdmi_dpm_adaptive_error',
                 'sdmi_dpm_adaptive_error_ws_floats', 'sdmi_dpm_solver_step'):
        assert name in _lib.exported_symbols() and name + '(' in hdr and hasattr(lib, name)
    assert '#define SDMI_ABI_VERSION 17' in hdr and lib.sdmi_abi_version() == 17
    assert lib.sdmi_dpm_adaptive_error_ws_floats(3, 891) == 3 and lib.sdmi_dpm_adaptive_error_ws_floats(3, 65537) == 3 * 65
