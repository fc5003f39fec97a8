"""Reference-run goldens for the DPM-Solver variants (needs the reference checkout; CPU only):

    python tools/make_golden_dpm_variants.py [--reference DIR]

Runs the reference's own, unmodified `NoiseScheduleVP`, `model_wrapper` and `DPM_Solver` (ldm/models/diffusion/dpm_solver/dpm_solver.py)
on the cases of tests/dpm_cases.py over its stub models, and writes tests/golden/dpm_variants.npz:
  * per non-adaptive case: the end point, the model-input time of every model call, and the host plan (ops, coefficients, timesteps,
    orders) of `DPMSolverHIP.plan` AS COMPUTED ON THIS MACHINE -- the last bit of torch's CPU exp / log / sqrt depends on the CPU model,
    so a trajectory recorded here can only be replayed bit for bit through the scalars computed here.  Before anything is written a
    CPU loop over that plan, in torch expressions (dpm_cases.torch_plan_loop), must equal the reference run bit for bit;
  * per adaptive case: the end point, the E of every iteration with its accept / reject flag, the model-input times.  Asserted: at
    least one case rejects a step, and every E keeps |E - 1| >= GAP (a seed is searched until it does);
  * `inverse_lambda` of the reference on a grid, and its order lists and outer timesteps of method='singlestep' for steps 3..9.
The only stand-in is a recording wrapper around torch.float_power (called once per adaptive iteration with E)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import dpm_cases as DC  # noqa: E402
from stable_diffusion_amd.samplers import DPMSolverHIP, _DiscreteVP  # noqa: E402


def reference_solver(ref, case, calls):
    """(DPM_Solver, NoiseScheduleVP) of the reference over the case's stub"""
    ns = ref.NoiseScheduleVP('discrete', alphas_cumprod=DC.alphas_cumprod())
    model = DC.MODELS[case.get('model', 'stub')]
    c = torch.tensor(DC.COND)

    def apply(x, t, cond):
        calls.append(float(t[0]))
        assert bool((t == t[0]).all())
        return model(x, t, cond)
    scale = case['scale']
    fn = ref.model_wrapper(apply, ns, model_type='noise', guidance_type='classifier-free', condition=c,
                           unconditional_condition=torch.zeros_like(c), guidance_scale=1. if scale is None else scale)
    return ref.DPM_Solver(fn, ns, predict_x0=case['predict_x0'], thresholding=case.get('thresholding', False),
                          max_val=case.get('max_val', 1.)), ns


def mine(case, calls=None):
    scale = case['scale']
    return DPMSolverHIP(DC.eps_fn_of(DC.MODELS[case.get('model', 'stub')], scale, calls), _DiscreteVP(DC.alphas_cumprod()),
                        predict_x0=case['predict_x0'], thresholding=case.get('thresholding', False), max_val=case.get('max_val', 1.),
                        cfg=scale is not None, scale=1. if scale is None else scale)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', default=os.environ.get('SD_REFERENCE', '/root/reference'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    import ldm.models.diffusion.dpm_solver.dpm_solver as ref
    torch.set_grad_enabled(False)
    out = {}

    # ---- the non-adaptive cases -----------------------------------------------------------------------------------------------------
    for name, case in DC.CASES.items():
        seed = DC.case_seed(name)
        x = DC.case_x(seed)
        calls = []
        solver, _ = reference_solver(ref, case, calls)
        if case.get('thresholding'):            # how the quantile sits against max_val at every (sample, evaluation) of the reference run
            qs, orig_q = [], torch.quantile
            torch.quantile = lambda *a, **k: (lambda v: (qs.append(v.clone()), v)[1])(orig_q(*a, **k))
        try:
            want = solver.sample(x, **case['sample'])
        finally:
            if case.get('thresholding'):
                torch.quantile = orig_q
        my_calls = []
        m = mine(case, my_calls)
        plan = m.plan(**case['sample'])
        got = DC.torch_plan_loop(plan, x, m.eps_fn, m.predict_x0, m.cfg, m.scale, m.thresholding, m.max_val)
        same = torch.equal(got, want)
        print(f'[{name}] {len(calls)} model calls, orders {plan.orders.tolist()}, |x| max {float(want.abs().max()):.3f}; '
              f'CPU loop over the plan == reference: {same}')
        assert same, (name, float((got - want).abs().max()))
        assert my_calls == calls and plan.model_times() == calls, name
        if case.get('thresholding'):
            q = torch.stack(qs)
            above, below = int((q > case['max_val']).sum()), int((q < case['max_val']).sum())
            print(f'[{name}] quantile above max_val at {above}, below at {below} of {q.numel()} (sample, evaluation) pairs; '
                  f'range {float(q.min()):.3f} .. {float(q.max()):.3f}')
            assert above > 0 and below > 0, 'choose max_val inside the range of the quantiles'
        out.update({f'{name}_out': want.numpy(), f'{name}_seed': np.int64(seed), f'{name}_calls': np.asarray(calls, dtype=np.float32),
                    f'{name}_ops': plan.ops, f'{name}_coef': plan.coef, f'{name}_timesteps': plan.timesteps, f'{name}_orders': plan.orders,
                    f'{name}_result': np.int64(plan.result)})

    # ---- the adaptive cases: a seed at which every E of the reference run keeps GAP ---------------------------------------------------
    def run_adaptive(name, case, seed):
        x = DC.case_x(seed)
        calls, es = [], []
        solver, _ = reference_solver(ref, case, calls)
        orig = torch.float_power
        torch.float_power = lambda E, p: (es.append(float(E)), orig(E, p))[1]
        try:
            want = solver.sample(x, **case['sample'])
        finally:
            torch.float_power = orig
        return x, want, calls, es
    rejected = 0
    for name, case in DC.ADAPTIVE.items():
        for seed in range(DC.case_seed(name), DC.case_seed(name) + 4000, 100):
            x, want, calls, es = run_adaptive(name, case, seed)
            gap = min(abs(e - 1.) for e in es)
            if gap >= DC.GAP and all(np.isfinite(es)):
                break
        else:
            raise SystemExit(f'[{name}] no seed keeps |E - 1| >= {DC.GAP}')
        accept = [e <= 1. for e in es]
        m = mine(case)
        got, log, times = DC.torch_adaptive_loop(m, x, case['sample']['order'])
        print(f'[{name}] seed {seed}: {len(es)} iterations, {accept.count(False)} rejected, {len(calls)} model calls, min |E - 1| {gap:.3g}; '
              f'CPU restatement: same decisions {[a for _, a in log] == accept}, max |E diff| '
              f'{max(abs(a - b) for (a, _), b in zip(log, es)):.2e}, end point max-abs {float((got - want).abs().max()):.2e}')
        assert [a for _, a in log] == accept and len(times) == len(calls)
        rejected += accept.count(False)
        out.update({f'{name}_out': want.numpy(), f'{name}_seed': np.int64(seed), f'{name}_calls': np.asarray(calls, dtype=np.float32),
                    f'{name}_E': np.asarray(es, dtype=np.float32), f'{name}_accept': np.asarray(accept, dtype=np.bool_)})
    assert rejected > 0, 'no adaptive case rejects a step: the stub needs a sharper kink'

    # ---- inverse_lambda, and the singlestep order lists / outer timesteps ------------------------------------------------------------
    solver, ns = reference_solver(ref, DC.CASES['ss3_s3_eps'], [])
    lam = torch.linspace(float(ns.marginal_lambda(torch.tensor([1.]))), float(ns.marginal_lambda(torch.tensor([1e-3]))), 57)
    out['il_lambda'], out['il_t'] = lam.numpy(), ns.inverse_lambda(lam).numpy()
    for steps in DC.SINGLESTEP_STEPS:
        ts, orders = solver.get_orders_and_timesteps_for_singlestep_solver(steps, 3, 'logSNR', 1., 1e-3, 'cpu')
        out[f'ss_orders_{steps}'], out[f'ss_timesteps_{steps}'] = np.asarray(orders, dtype=np.int32), ts.numpy()
        print(f'[singlestep order 3, steps {steps}] orders {orders}')

    path = os.path.join(ROOT, 'tests', 'golden', 'dpm_variants.npz')
    np.savez_compressed(path, **out)
    print('written', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
