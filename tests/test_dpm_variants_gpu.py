"""The DPM-Solver variants on the MI355X (csrc/dpm.hip, DPMSolverHIP): every update form and the model value against the reference's
torch expression on the device (torch.equal), the thresholding scale against torch.sort / torch.quantile, the adaptive error against
fp64, the trajectories of tests/golden/dpm_variants.npz (tools/make_golden_dpm_variants.py: reference runs on the CPU), and two runs
end to end through UNetModelHIP."""
import os

import numpy as np
import pytest
import torch

import dpm_cases as DC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = (891, 1)            # three full blocks and a tail; a single element


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'dpm_variants.npz'))


@pytest.fixture(scope='module')
def ns():
    from stable_diffusion_amd.samplers import _DiscreteVP
    return _DiscreteVP(DC.alphas_cumprod())


def same(a, b):
    """torch.equal, with a NaN equal to a NaN"""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def D(v):
    """a host scalar (one-element CPU tensor) as the 0-dim device tensor the reference multiplies with"""
    return v.reshape(()).to(DEV)


def tensors(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    out = [(torch.randn(n, generator=g) * (2.0 if i == 0 else 1.0)).to(DEV) for i in range(k)]
    if n > 100:
        out[0][5], out[1][700] = float('nan'), float('inf')
    return out


def solver_of(ns, predict_x0, **kw):
    from stable_diffusion_amd.samplers import DPMSolverHIP
    return DPMSolverHIP(None, ns, predict_x0=predict_x0, **kw)


T = lambda v: torch.tensor([v], dtype=torch.float32)       # noqa: E731


# ---- update forms: the reference's expressions, written out with their own signs, scalars from the host ---------------------------
def ref_first(ns, px0, x, model_s, s, t):
    """dpm_solver.py:518-545"""
    h = ns.lam(t) - ns.lam(s)
    if px0:
        return D(ns.sigma(t) / ns.sigma(s)) * x - D(ns.alpha(t) * torch.expm1(-h)) * model_s
    return D(torch.exp(ns.log_alpha(t) - ns.log_alpha(s))) * x - D(ns.sigma(t) * torch.expm1(h)) * model_s


def ref_ss2(ns, px0, st, x, model_s, model_s1, s, t, r1):
    """dpm_solver.py:572-627 -> (x_s1, x_t)"""
    lambda_s, lambda_t = ns.lam(s), ns.lam(t)
    h = lambda_t - lambda_s
    s1 = ns.inverse_lambda(lambda_s + r1 * h)
    sigma_s, sigma_s1, sigma_t = ns.sigma(s), ns.sigma(s1), ns.sigma(t)
    alpha_s1, alpha_t = ns.alpha(s1), ns.alpha(t)
    if px0:
        phi_11, phi_1 = torch.expm1(-r1 * h), torch.expm1(-h)
        x_s1 = D(sigma_s1 / sigma_s) * x - D(alpha_s1 * phi_11) * model_s
        if st == 'dpm_solver':
            x_t = D(sigma_t / sigma_s) * x - D(alpha_t * phi_1) * model_s - D((0.5 / r1) * (alpha_t * phi_1)) * (model_s1 - model_s)
        else:
            x_t = (D(sigma_t / sigma_s) * x - D(alpha_t * phi_1) * model_s
                   + D((1. / r1) * (alpha_t * ((torch.exp(-h) - 1.) / h + 1.))) * (model_s1 - model_s))
    else:
        phi_11, phi_1 = torch.expm1(r1 * h), torch.expm1(h)
        la_s, la_s1, la_t = ns.log_alpha(s), ns.log_alpha(s1), ns.log_alpha(t)
        x_s1 = D(torch.exp(la_s1 - la_s)) * x - D(sigma_s1 * phi_11) * model_s
        if st == 'dpm_solver':
            x_t = D(torch.exp(la_t - la_s)) * x - D(sigma_t * phi_1) * model_s - D((0.5 / r1) * (sigma_t * phi_1)) * (model_s1 - model_s)
        else:
            x_t = (D(torch.exp(la_t - la_s)) * x - D(sigma_t * phi_1) * model_s
                   - D((1. / r1) * (sigma_t * ((torch.exp(h) - 1.) / h - 1.))) * (model_s1 - model_s))
    return x_s1, x_t


def ref_ss3(ns, px0, st, x, model_s, model_s1, model_s2, s, t, r1, r2):
    """dpm_solver.py:659-748 -> (x_s1, x_s2, x_t)"""
    lambda_s, lambda_t = ns.lam(s), ns.lam(t)
    h = lambda_t - lambda_s
    s1, s2 = ns.inverse_lambda(lambda_s + r1 * h), ns.inverse_lambda(lambda_s + r2 * h)
    sigma_s, sigma_s1, sigma_s2, sigma_t = ns.sigma(s), ns.sigma(s1), ns.sigma(s2), ns.sigma(t)
    alpha_s1, alpha_s2, alpha_t = ns.alpha(s1), ns.alpha(s2), ns.alpha(t)
    D1_0 = D(1. / r1) * (model_s1 - model_s)
    D1_1 = D(1. / r2) * (model_s2 - model_s)
    D1 = (D(r2) * D1_0 - D(r1) * D1_1) / D(r2 - r1)
    D2 = 2. * (D1_1 - D1_0) / D(r2 - r1)
    if px0:
        phi_11, phi_12, phi_1 = torch.expm1(-r1 * h), torch.expm1(-r2 * h), torch.expm1(-h)
        phi_22 = torch.expm1(-r2 * h) / (r2 * h) + 1.
        phi_2 = phi_1 / h + 1.
        phi_3 = phi_2 / h - 0.5
        x_s1 = D(sigma_s1 / sigma_s) * x - D(alpha_s1 * phi_11) * model_s
        x_s2 = D(sigma_s2 / sigma_s) * x - D(alpha_s2 * phi_12) * model_s + D(r2 / r1 * (alpha_s2 * phi_22)) * (model_s1 - model_s)
        if st == 'dpm_solver':
            x_t = D(sigma_t / sigma_s) * x - D(alpha_t * phi_1) * model_s + D((1. / r2) * (alpha_t * phi_2)) * (model_s2 - model_s)
        else:
            x_t = D(sigma_t / sigma_s) * x - D(alpha_t * phi_1) * model_s + D(alpha_t * phi_2) * D1 - D(alpha_t * phi_3) * D2
    else:
        phi_11, phi_12, phi_1 = torch.expm1(r1 * h), torch.expm1(r2 * h), torch.expm1(h)
        phi_22 = torch.expm1(r2 * h) / (r2 * h) - 1.
        phi_2 = phi_1 / h - 1.
        phi_3 = phi_2 / h - 0.5
        la_s, la_s1, la_s2, la_t = ns.log_alpha(s), ns.log_alpha(s1), ns.log_alpha(s2), ns.log_alpha(t)
        x_s1 = D(torch.exp(la_s1 - la_s)) * x - D(sigma_s1 * phi_11) * model_s
        x_s2 = D(torch.exp(la_s2 - la_s)) * x - D(sigma_s2 * phi_12) * model_s - D(r2 / r1 * (sigma_s2 * phi_22)) * (model_s1 - model_s)
        if st == 'dpm_solver':
            x_t = D(torch.exp(la_t - la_s)) * x - D(sigma_t * phi_1) * model_s - D((1. / r2) * (sigma_t * phi_2)) * (model_s2 - model_s)
        else:
            x_t = D(torch.exp(la_t - la_s)) * x - D(sigma_t * phi_1) * model_s - D(sigma_t * phi_2) * D1 - D(sigma_t * phi_3) * D2
    return x_s1, x_s2, x_t


def ref_ms2(ns, px0, st, x, model_prev_1, model_prev_0, t_prev_1, t_prev_0, t):
    """dpm_solver.py:771-810"""
    lambda_prev_1, lambda_prev_0, lambda_t = ns.lam(t_prev_1), ns.lam(t_prev_0), ns.lam(t)
    h_0, h = lambda_prev_0 - lambda_prev_1, lambda_t - lambda_prev_0
    r0 = h_0 / h
    D1_0 = D(1. / r0) * (model_prev_0 - model_prev_1)
    sigma_prev_0, sigma_t, alpha_t = ns.sigma(t_prev_0), ns.sigma(t), ns.alpha(t)
    la0, la_t = ns.log_alpha(t_prev_0), ns.log_alpha(t)
    if px0:
        if st == 'dpm_solver':
            return (D(sigma_t / sigma_prev_0) * x - D(alpha_t * (torch.exp(-h) - 1.)) * model_prev_0
                    - 0.5 * D(alpha_t * (torch.exp(-h) - 1.)) * D1_0)
        return (D(sigma_t / sigma_prev_0) * x - D(alpha_t * (torch.exp(-h) - 1.)) * model_prev_0
                + D(alpha_t * ((torch.exp(-h) - 1.) / h + 1.)) * D1_0)
    if st == 'dpm_solver':
        return D(torch.exp(la_t - la0)) * x - D(sigma_t * (torch.exp(h) - 1.)) * model_prev_0 - 0.5 * D(sigma_t * (torch.exp(h) - 1.)) * D1_0
    return D(torch.exp(la_t - la0)) * x - D(sigma_t * (torch.exp(h) - 1.)) * model_prev_0 - D(sigma_t * ((torch.exp(h) - 1.) / h - 1.)) * D1_0


def ref_ms3(ns, px0, x, model_prev_2, model_prev_1, model_prev_0, t_prev_2, t_prev_1, t_prev_0, t):
    """dpm_solver.py:826-857"""
    l2, l1, l0, lt = ns.lam(t_prev_2), ns.lam(t_prev_1), ns.lam(t_prev_0), ns.lam(t)
    h_1, h_0, h = l1 - l2, l0 - l1, lt - l0
    r0, r1 = h_0 / h, h_1 / h
    D1_0 = D(1. / r0) * (model_prev_0 - model_prev_1)
    D1_1 = D(1. / r1) * (model_prev_1 - model_prev_2)
    D1 = D1_0 + D(r0 / (r0 + r1)) * (D1_0 - D1_1)
    D2 = D(1. / (r0 + r1)) * (D1_0 - D1_1)
    sigma_prev_0, sigma_t, alpha_t = ns.sigma(t_prev_0), ns.sigma(t), ns.alpha(t)
    if px0:
        return (D(sigma_t / sigma_prev_0) * x - D(alpha_t * (torch.exp(-h) - 1.)) * model_prev_0
                + D(alpha_t * ((torch.exp(-h) - 1.) / h + 1.)) * D1 - D(alpha_t * ((torch.exp(-h) - 1. + h) / h ** 2 - 0.5)) * D2)
    return (D(torch.exp(ns.log_alpha(t) - ns.log_alpha(t_prev_0))) * x - D(sigma_t * (torch.exp(h) - 1.)) * model_prev_0
            - D(sigma_t * ((torch.exp(h) - 1.) / h - 1.)) * D1 - D(sigma_t * ((torch.exp(h) - 1. - h) / h ** 2 - 0.5)) * D2)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('st', ['dpm_solver', 'taylor'])
@pytest.mark.parametrize('px0', [True, False])
def test_update_forms_bit_exact(ns, px0, st, n):
    """all five updates of the reference, intermediate states included, through sdmi_dpm_update: torch.equal with the reference's torch
    expression on the device (NaN and inf elements too).  r1, r2 are tensors, as the singlestep loop passes them (dpm_solver.py:1119-1120)"""
    sv = solver_of(ns, px0)
    x, m0, m1, m2 = tensors(n, 4, 11 + n)
    s, t, r1, r2 = T(0.73), T(0.41), T(0.31), T(0.64)
    assert same(sv._update(0, x, (m0,), sv._first(s, t)), ref_first(ns, px0, x, m0, s, t))
    _, a, c = sv._ss2(s, t, r1, st)
    want = ref_ss2(ns, px0, st, x, m0, m1, s, t, r1)
    assert same(sv._update(0, x, (m0,), a), want[0]) and same(sv._update(1, x, (m0, m1, m0), c), want[1])
    _, _, a, b, form, c = sv._ss3(s, t, r1, r2, st)
    want = ref_ss3(ns, px0, st, x, m0, m1, m2, s, t, r1, r2)
    assert form == (1 if st == 'dpm_solver' else 2)
    assert same(sv._update(0, x, (m0,), a), want[0]) and same(sv._update(1, x, (m0, m1, m0), b), want[1])
    assert same(sv._update(form, x, (m0, m2, m0) if form == 1 else (m0, m1, m2), c), want[2])
    tp2, tp1, tp0, tt = T(0.93), T(0.81), T(0.70), T(0.52)
    assert same(sv._update(1, x, (m0, m0, m1), sv._ms2(tp1, tp0, tt, st)), ref_ms2(ns, px0, st, x, m1, m0, tp1, tp0, tt))
    assert same(sv._update(3, x, (m0, m1, m2), sv._ms3(tp2, tp1, tp0, tt)), ref_ms3(ns, px0, x, m2, m1, m0, tp2, tp1, tp0, tt))
    torch.cuda.synchronize()


def test_update_with_python_float_r_as_the_adaptive_solver_passes_them(ns):
    """r1 = 1/3, r2 = 2/3 as Python floats (dpm_solver.py:943): the scalar products round to fp32 where torch rounds them"""
    for px0 in (True, False):
        sv = solver_of(ns, px0)
        x, m0, m1, m2 = tensors(891, 4, 5)
        s, t, r1, r2 = T(0.5), T(0.46), 1. / 3., 2. / 3.
        _, _, a, b, form, c = sv._ss3(s, t, r1, r2, 'dpm_solver')
        want = ref_ss3(ns, px0, 'dpm_solver', x, m0, m1, m2, s, t, T(r1), T(r2))          # (D() of the fp32 value; 1/r etc. differ below)
        h = ns.lam(t) - ns.lam(s)
        if px0:
            lit = D(ns.sigma(t) / ns.sigma(s)) * x - D(ns.alpha(t) * torch.expm1(-h)) * m0 + (1. / r2) * D(ns.alpha(t) * (torch.expm1(-h) / h + 1.)) * (m2 - m0)
        else:
            lit = (D(torch.exp(ns.log_alpha(t) - ns.log_alpha(s))) * x - D(ns.sigma(t) * torch.expm1(h)) * m0
                   - (1. / r2) * D(ns.sigma(t) * (torch.expm1(h) / h - 1.)) * (m2 - m0))
        assert same(sv._update(form, x, (m0, m2, m0), c), lit)
        assert same(sv._update(0, x, (m0,), a), want[0])


# ---- model value --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('px0', [True, False])
@pytest.mark.parametrize('cfg', [True, False])
def test_model_value_bit_exact(lib, cfg, px0, n):
    from stable_diffusion_amd import _lib
    B = 3 if n > 1 else 1
    x, e0, e1 = tensors(n, 3, 3 + n)
    eps = torch.cat([e0, e1]) if cfg else e1.clone()
    alpha, sigma, scale = 0.2871234, 0.9578123, 3.0
    a, s = torch.tensor(alpha, device=DEV), torch.tensor(sigma, device=DEV)
    want = DC.torch_model_value(eps.reshape((2 * B if cfg else B), -1), x.reshape(B, -1), cfg, scale, px0, a, s)
    out = torch.empty_like(x)
    call = lambda sp: _lib.check(lib.sdmi_dpm_model_value(eps.data_ptr(), int(cfg), scale, x.data_ptr(), int(px0), alpha, sigma, sp, n // B,
                                                          out.data_ptr(), n, _lib.stream_ptr()))
    call(None)
    assert same(out.reshape(B, -1), want)
    if px0:         # thresholding, given the same s: clamp(x0, -s, s) / s per sample (dpm_solver.py:397-398); one scale is NaN
        sc = torch.tensor([0.8, 2.5, float('nan')][:B], device=DEV)
        s4 = sc[:, None]
        call(sc.data_ptr())
        assert same(out.reshape(B, -1), torch.clamp(want, -s4, s4) / s4)
    torch.cuda.synchronize()


# ---- thresholding scale -------------------------------------------------------------------------------------------------------------
ROWS = (1, 2, 201, 256, 891, 16384, 65537)       # 201: rank 199.0 -- weight 0, the upper index at the end


def rows_of(kind, n):
    g = torch.Generator().manual_seed(n + len(kind))
    x = torch.randn(3, n, generator=g) * torch.tensor([[0.3], [1.0], [7.0]])
    if kind == 'equal':
        x = torch.tensor([[0.25], [-3.0], [1e-30]]).expand(3, n).clone()
    elif kind == 'ties':                # a handful of levels: hundreds of equal values around the selected rank
        x = torch.round(x * 2.0) / 2.0
    elif kind == 'zeros':               # +-0.0 everywhere but a few elements: the selected values are zeros of either sign
        z = torch.where(torch.rand(3, n, generator=g) > 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        x = torch.where(torch.rand(3, n, generator=g) > 0.002, z, x)
    elif kind == 'lowbyte':             # bit patterns that differ in the lowest byte only (and the sign)
        bits = torch.randint(0, 256, (3, n), generator=g, dtype=torch.int32) + torch.tensor([[0x3f800000], [0x40490f00], [0x00800000]],
                                                                                            dtype=torch.int32)
        x = bits.view(torch.float32) * torch.where(torch.rand(3, n, generator=g) > 0.5, 1.0, -1.0)
    elif kind == 'nan':
        x[1, n // 2] = float('nan')
    return x.to(DEV).contiguous()


@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('kind', ['normal', 'equal', 'ties', 'zeros', 'lowbyte', 'nan'])
def test_threshold_scale(lib, kind, n):
    """the two order statistics equal torch.sort's exactly; s against torch.quantile on the device: torch.equal is the target, 1 ulp
    the bound should the lerp round otherwise.  Observed on the MI355X: torch.equal (0 ulp) in all 42 cases, with max_val 0 and 1
    (profiles/dpm_variants_parity.txt).  Two launches give the same bits."""
    from stable_diffusion_amd import _lib
    x = rows_of(kind, n)
    s, s2, stats = torch.empty(3, device=DEV), torch.empty(3, device=DEV), torch.empty(3, 2, device=DEV)
    _lib.check(lib.sdmi_dpm_threshold_scale(x.data_ptr(), 3, n, 0.0, s.data_ptr(), stats.data_ptr(), _lib.stream_ptr()))
    _lib.check(lib.sdmi_dpm_threshold_scale(x.data_ptr(), 3, n, 1.0, s2.data_ptr(), None, _lib.stream_ptr()))
    a = x.abs()
    srt = torch.sort(a, dim=1).values
    rank = torch.tensor(0.995) * (n - 1)                           # torch.quantile: the fp32 q times the last index
    lo, hi = int(torch.floor(rank)), int(torch.ceil(rank))
    ok = ~torch.isnan(a).any(dim=1)
    assert ok.sum() == (2 if kind == 'nan' else 3)
    assert torch.equal(stats[ok, 0], srt[ok, lo]) and torch.equal(stats[ok, 1], srt[ok, hi])
    q = torch.quantile(a, 0.995, dim=1)
    want, want2 = torch.maximum(q, torch.zeros_like(q)), torch.maximum(q, 1.0 * torch.ones_like(q))
    assert torch.equal(torch.isnan(s), ~ok) and torch.equal(torch.isnan(s2), ~ok) and torch.equal(torch.isnan(want), ~ok)
    ulps = (s[ok].view(torch.int32).long() - want[ok].view(torch.int32).long()).abs().max()
    ulps2 = (s2[ok].view(torch.int32).long() - want2[ok].view(torch.int32).long()).abs().max()
    print(f'[threshold {kind} n={n}] s vs torch.quantile: {int(ulps)} ulp, with max_val 1: {int(ulps2)} ulp '
          f'({"torch.equal" if ulps == 0 and ulps2 == 0 else "lerp rounding differs"})')
    assert ulps <= 1 and ulps2 <= 1
    s3 = torch.empty(3, device=DEV)
    _lib.check(lib.sdmi_dpm_threshold_scale(x.data_ptr(), 3, n, 0.0, s3.data_ptr(), None, _lib.stream_ptr()))
    assert same(s3, s)
    torch.cuda.synchronize()


# ---- adaptive error -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [891, 65537])
def test_adaptive_error_against_fp64(lib, n):
    """E against the fp64 evaluation of the same expression on the same fp32 inputs (atol, rtol at their fp32 values, as torch's ops see
    them).  Bound, u = 2^-24: per element (x_higher - x_lower) u, rtol * max u, the quotient u -> v to 3u, v^2 to 7u; the fixed tree adds
    at most 3 (in a thread) + 8 (workgroup) + 0 (at most one chunk per thread of the finish: n <= 262144) + 8 levels = 19 roundings on
    non-negative terms -> the sum to 26u; the mean u more; the square root halves it and adds u: |E - E64| <= 14.5u E < 16u E ~ 9.6e-7 E,
    a hundredth of GAP / 100 at E ~ 1.  Two runs give the same bits."""
    from stable_diffusion_amd import _lib
    g = torch.Generator().manual_seed(n)
    xl = torch.randn(3, n, generator=g) * torch.tensor([[0.05], [1.0], [3.0]])
    xp = torch.randn(3, n, generator=g)
    xh = xl + torch.randn(3, n, generator=g) * 0.03 * torch.tensor([[1.0], [2.0], [0.5]])
    atol, rtol = DC.ATOL, DC.RTOL
    a64, r64 = float(np.float32(atol)), float(np.float32(rtol))
    d, l, p = xh.double(), xl.double(), xp.double()
    delta = torch.max(torch.ones_like(l) * a64, r64 * torch.max(l.abs(), p.abs()))
    E64 = float(torch.sqrt(torch.square((d - l) / delta).mean(dim=-1)).max())
    xh, xl, xp = xh.to(DEV), xl.to(DEV), xp.to(DEV)
    nws = lib.sdmi_dpm_adaptive_error_ws_floats(3, n)
    res = []
    for _ in range(2):
        ws = torch.full((nws,), float('nan'), device=DEV)
        E = torch.full((1,), float('nan'), device=DEV)
        _lib.check(lib.sdmi_dpm_adaptive_error(xh.data_ptr(), xl.data_ptr(), xp.data_ptr(), atol, rtol, 3, n, ws.data_ptr(), nws, E.data_ptr(),
                                               _lib.stream_ptr()))
        res.append(E.cpu())
    bound = 16 * 2.0 ** -24
    print(f'[adaptive error n={n}] E {float(res[0]):.7f} fp64 {E64:.9f} rel {abs(float(res[0]) - E64) / E64:.2e} (bound {bound:.2e})')
    assert 0.1 < E64 < 100 and bound * 100 < DC.GAP / 100
    assert abs(float(res[0]) - E64) <= bound * E64
    assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32))
    # the torch expression on the device, for the record only: another summation order
    delta = torch.max(torch.ones_like(xl) * atol, rtol * torch.max(xl.abs(), xp.abs()))
    Et = float(torch.sqrt(torch.square((xh - xl) / delta).mean(dim=-1)).max())
    print(f'[adaptive error n={n}] torch fp32 on the device {Et:.7f}: rel {abs(Et - E64) / E64:.2e} to fp64')


# ---- trajectories ---------------------------------------------------------------------------------------------------------------------
def hip_solver(case, calls):
    from stable_diffusion_amd.samplers import DPMSolverHIP, _DiscreteVP
    scale = case['scale']
    return DPMSolverHIP(DC.eps_fn_of(DC.MODELS[case.get('model', 'stub')], scale, calls, DEV), _DiscreteVP(DC.alphas_cumprod()),
                        predict_x0=case['predict_x0'], thresholding=case.get('thresholding', False), max_val=case.get('max_val', 1.),
                        cfg=scale is not None, scale=1. if scale is None else scale)


@pytest.mark.parametrize('name', list(DC.CASES))
def test_trajectory_equals_the_reference_run(G, name):
    """every non-adaptive case on the recorded plan: the reference's end point bit for bit, its model calls at its times.  The
    thresholding case too: its scale came out torch.equal to torch.quantile's (test_threshold_scale)."""
    case = DC.CASES[name]
    calls = []
    solver = hip_solver(case, calls)
    out = solver.run_plan(DC.case_x(int(G[f'{name}_seed'])).to(DEV), DC.load_plan(G, name))
    want = torch.from_numpy(G[f'{name}_out'])
    print(f'[{name}] {len(calls)} model calls, max-abs {float((out.cpu() - want).abs().max()):.3e} (|x| max {float(want.abs().max()):.2f})')
    assert np.array_equal(np.asarray(calls, dtype=np.float32), G[f'{name}_calls'])
    assert torch.equal(out.cpu(), want)


# max-abs of the adaptive end points against the reference goldens, measured on the MI355X (profiles/dpm_variants_parity.txt):
# ad2_x0 1.907e-05, ad2_eps 7.629e-06, ad3_x0 2.289e-05, ad3_eps 9.537e-06 at |x| max 25 .. 32 (an ulp there is 1.9e-06).  The bar is
# 4 x the largest, rounded up to one digit -- the margin is for last-bit differences of CPU transcendentals between machines -- and
# stays under the 2e-4 of tests/test_sampler_gpu.py; a value above that would be a finding, not a new bar.
ADAPTIVE_BAR = 1e-4


@pytest.mark.parametrize('name', list(DC.ADAPTIVE))
def test_adaptive_equals_the_reference_decisions(G, name):
    """the accept / reject sequence and the evaluation count of the reference run (hard: GAP keeps every recorded E 1e-2 away from 1),
    every E to 1e-4 relative.  The end point cannot be bit-equal -- the step sizes pass through host exp / log at run time and E has
    another summation order; max-abs against the reference golden, measured on the MI355X: 7.6e-06 .. 2.3e-05 (ADAPTIVE_BAR above)."""
    case = DC.ADAPTIVE[name]
    calls = []
    solver = hip_solver(case, calls)
    out = solver.sample(DC.case_x(int(G[f'{name}_seed'])).to(DEV), **case['sample'])
    want = torch.from_numpy(G[f'{name}_out'])
    err = float((out.cpu() - want).abs().max())
    Es = np.asarray([e for e, _ in solver.adaptive_log])
    print(f'[{name}] {len(Es)} iterations, {len(calls)} model calls, max-abs {err:.3e} (|x| max {float(want.abs().max()):.2f}), '
          f'max rel E diff {np.abs(Es / G[f"{name}_E"][:len(Es)] - 1).max() if len(Es) == len(G[f"{name}_E"]) else float("nan"):.2e}')
    assert [a for _, a in solver.adaptive_log] == G[f'{name}_accept'].tolist()
    assert len(calls) == len(G[f'{name}_calls'])
    assert np.abs(Es - G[f'{name}_E']).max() <= DC.GAP / 10         # (a tenth of what a decision has to spare)
    assert err <= ADAPTIVE_BAR


# ---- end to end through UNetModelHIP ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tiny():
    from oracle.plan import TINY
    from oracle.weights import make_inputs, make_state_dict
    from stable_diffusion_amd import LatentDiffusionHIP, UNetModelHIP
    unet = UNetModelHIP(**TINY.ref_kwargs())
    unet.load_state_dict(make_state_dict(TINY, 0), strict=True)
    ld = LatentDiffusionHIP(unet).to(DEV)
    x_T, _, ctx = make_inputs(TINY, 2, 8, 8, seed=21)
    _, _, uc = make_inputs(TINY, 2, 8, 8, seed=22)
    return ld, x_T.to(DEV), ctx.to(DEV), uc.to(DEV)


def torch_side(ld, ctx, uc, scale, predict_x0=True):
    from stable_diffusion_amd.samplers import DPMSolverHIP, _DiscreteVP
    c_in = torch.cat([uc, ctx])

    def eps_fn(x, t_input):
        t_in = torch.full((2 * x.shape[0],), t_input, device=x.device, dtype=torch.float32)
        return ld.apply_model(torch.cat([x] * 2), t_in, c_in).float().contiguous()
    return DPMSolverHIP(eps_fn, _DiscreteVP(ld.alphas_cumprod.detach().float().cpu()), predict_x0=predict_x0, cfg=True, scale=scale)


def test_end_to_end_singlestep_with_hip_unet(tiny):
    """DPMSolverSamplerHIP.sample(method='singlestep', order=3, skip_type='logSNR', S=6) over the tiny UNet at 8 x 8 against the same
    plan in torch expressions over the same handle: the same eps bits go in on both sides, so torch.equal"""
    from stable_diffusion_amd import DPMSolverSamplerHIP
    ld, x_T, ctx, uc = tiny
    smp = DPMSolverSamplerHIP(ld)
    out, none = smp.sample(S=6, batch_size=2, shape=[4, 8, 8], conditioning=ctx, verbose=False, x_T=x_T, unconditional_guidance_scale=3.0,
                           unconditional_conditioning=uc, method='singlestep', order=3, skip_type='logSNR')
    sv = torch_side(ld, ctx, uc, 3.0)
    plan = sv.plan(steps=6, order=3, skip_type='logSNR', method='singlestep')
    ref = DC.torch_plan_loop(plan, x_T, sv.eps_fn, True, True, 3.0)
    torch.cuda.synchronize()
    print(f'[e2e singlestep-3 S=6] |x| max {float(ref.abs().max()):.3f} max-abs {float((out - ref).abs().max()):.3e}')
    assert none is None and plan.orders.tolist() == [3, 2, 1] and smp.solver.model_times == plan.model_times()
    assert torch.isfinite(ref).all() and torch.equal(out, ref)


def test_end_to_end_adaptive_with_hip_unet(tiny):
    """method='adaptive' (order 2) against dpm_cases.torch_adaptive_loop over the same handle: the same decisions and evaluation count;
    the end point to the 2e-4 of tests/test_sampler_gpu.py (E has another summation order, so the step sizes may differ in their last
    bits; measured on the MI355X: 6 iterations, none rejected, min |E - 1| 0.65, max-abs 0.0 at |x| max 42)"""
    from stable_diffusion_amd import DPMSolverSamplerHIP
    ld, x_T, ctx, uc = tiny
    smp = DPMSolverSamplerHIP(ld)
    out, _ = smp.sample(S=0, batch_size=2, shape=[4, 8, 8], conditioning=ctx, verbose=False, x_T=x_T, unconditional_guidance_scale=3.0,
                        unconditional_conditioning=uc, method='adaptive', order=2, atol=0.05, rtol=0.2)
    ref, log, times = DC.torch_adaptive_loop(torch_side(ld, ctx, uc, 3.0), x_T, 2, atol=0.05, rtol=0.2)
    torch.cuda.synchronize()
    err, top = float((out - ref).abs().max()), float(ref.abs().max())
    gap = min(abs(e - 1.) for e, _ in log)
    print(f'[e2e adaptive-2] {len(log)} iterations, {sum(not a for _, a in log)} rejected, min |E - 1| {gap:.3g}, |x| max {top:.3f}, max-abs {err:.3e}')
    assert torch.isfinite(ref).all() and len(log) < 200
    assert [a for _, a in smp.solver.adaptive_log] == [a for _, a in log] and len(smp.solver.model_times) == len(times)
    assert err <= 2e-4
