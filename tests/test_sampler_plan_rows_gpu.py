"""sdmi_sampler_plan_rows in guarded buffers: one launch for up to eight latents of two kinds.  A kind 1 slot (one model evaluation of a
DPM-Solver plan and the update that follows it) is bit-equal to lone sdmi_dpm_model_value + sdmi_dpm_update calls on the same arguments
and to tests/dpm_cases.py's torch expressions on the CPU; a kind 0 slot (the PLMS / DDIM step) to sdmi_sampler_step_rows on the same slot.
Both write the next call's timestep as fp32, in exactly the rows named."""
import re

import numpy as np
import pytest
import torch

import dpm_cases as DC
from guard import Pool
from stable_diffusion_amd import _lib

pytestmark = pytest.mark.gpu

# 256 elements on the 16-byte path; 105: the scalar path, a tail inside one block; 1028: one full 256-lane block of float4 and one lane of a second
SHAPES = {'vec': (4, 8, 8), 'scalar': (3, 5, 7), 'vec2': (257, 4)}
# kind 1: guided, px = data_prediction, form, self = m_self mask, outs (m = m_out, s = state, i = state written over x_base, 0 / 1 = unet_dst0 / 1)
# kind 0: as tests/test_sampler_rows_gpu.py (e = e_t_out, p = pred_x0, i = state written over x)
SLOTS = [
    dict(kind=1, cfg=1, px=1, form=1, self=0b011, outs='mi01', scale=7.5),       # multistep second update: the new value is m0 and m1
    dict(kind=0, cfg=1, mode=0, sigma=0.21, noise=True, outs='ip01', a_t=0.4321, a_prev=0.5678, scale=7.5),      # guided DDIM, eta > 0
    dict(kind=1, cfg=0, px=0, form=0, self=0b001, outs='s0', scale=1.0),         # first update, noise prediction
    dict(kind=1, cfg=1, px=1, form=2, self=0b100, outs='ms', scale=3.0, misalign=True),      # singlestep third 'taylor'; a last op: no rows to feed
    dict(kind=0, cfg=0, mode=3, sigma=0.15, noise=True, outs='esp0', a_t=0.9123, a_prev=0.9456, scale=1.0),
    dict(kind=1, cfg=0, px=1, form=3, self=0b001, outs='ms0', scale=1.0),        # multistep third update
    dict(kind=1, cfg=1, px=1, form=-1, self=0, outs='ms', scale=5.0),            # the last evaluation of denoise_to_zero: the result is m
    dict(kind=1, cfg=1, px=0, form=1, self=0b010, outs='s01', scale=2.0),        # singlestep second update: (m, m1, m), m1 the new value
]
LAUNCHES = {1: [0], 3: [6, 1, 3], 8: list(range(8))}
ALPHA, SIGMA = 0.2871234, 0.9578123
C9 = [0.83, -0.41, 0.27, 1.7, 2.9, 1.45, 0.66, 0.33, 0.31]


def _normal(g, shape):
    return torch.randn(shape, generator=g)


def _f32(v):
    return float(np.float32(v))


@pytest.mark.parametrize('n_slots', [1, 3, 8])
@pytest.mark.parametrize('path', ['vec', 'scalar', 'vec2'])
def test_plan_rows_equal_the_lone_launches_and_the_reference(path, n_slots):
    lib = _lib.load()
    st = _lib.stream_ptr()
    shape = SHAPES[path]
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(1000 * n_slots + n)
    P = Pool()
    ROWS = 13                                       # rows of the "next call": more than the eight-slot launch fills
    eps = P.put('eps', _normal(g, (16, n)))                             # the UNet output: up to two rows per slot
    X_next = P.new('X_next', (ROWS, n), torch.float32)
    T_next = P.new('T_next', (ROWS,), torch.float32)
    T_i64 = torch.full((ROWS,), -1, device='cuda', dtype=torch.int64)   # where the sdmi_sampler_step_rows twin of a kind 0 slot writes
    slots, cases, row, d = [], [], 0, 0
    for k in LAUNCHES[n_slots]:
        s = SLOTS[k]
        c = dict(s=s, k=k)
        mis = 1 if (s.get('misalign') and path != 'scalar') else 0     # one slot of a 16-byte launch goes element by element
        put = lambda name, t: P.put(f'{name}{k}', torch.cat([torch.zeros(mis), t.reshape(-1)]))[mis:]
        new = lambda name: P.new(f'{name}{k}', (n,), torch.float32)
        c['eu'], c['ec'] = eps[row], (eps[row + 1] if s['cfg'] else None)
        row += 2 if s['cfg'] else 1
        o = s['outs']
        c['dst'] = []
        for flag in '01':
            if flag in o:
                c['dst'].append(d)
                d += 1
        sl = _lib.SamplerPlanSlot()
        sl.kind, sl.cfg, sl.scale = s['kind'], s['cfg'], s['scale']
        sl.eps_u, sl.eps_c = c['eu'].data_ptr(), _lib.ptr(c['ec'])
        c['x_cpu'] = _normal(g, (n,)) * 2
        c['x'] = put('x', c['x_cpu'])
        c['ins'] = [c['x']]
        if s['kind'] == 1:
            c['t_next'] = _f32(612.3457 - 40.25 * k)
            c['c9'] = [_f32(v + 0.01 * k) for v in C9]
            c['alpha'], c['sigma'] = _f32(ALPHA + 0.05 * k), _f32(SIGMA - 0.05 * k)
            c['xb_cpu'] = _normal(g, (n,)) * 2
            c['m_cpu'] = [_normal(g, (n,)) for _ in range(3)]
            reads = 0 if s['form'] < 0 else (1 if s['form'] == 0 else 7)
            c['xb'] = put('x_base', c['xb_cpu']) if s['form'] >= 0 else None
            # an operand that is the value just computed has no buffer; (m, m1, m) passes one buffer twice
            c['m'] = [put(f'm{j}_', c['m_cpu'][j]) if (reads & ~s['self']) >> j & 1 else None for j in range(3)]
            if k == 7:
                c['m'][2], c['m_cpu'][2] = c['m'][0], c['m_cpu'][0]
            c['ins'] += [t for t in [c['xb']] + c['m'] if t is not None]
            c['m_out'] = new('m_out') if 'm' in o else None
            c['state'] = c['xb'] if 'i' in o else (new('state') if 's' in o else None)
            sl.x, sl.data_prediction = (c['x'].data_ptr() if s['px'] else None), s['px']
            sl.alpha_t, sl.sigma_t, sl.form, sl.m_self = c['alpha'], c['sigma'], s['form'], s['self']
            sl.x_base, sl.m0, sl.m1, sl.m2 = (_lib.ptr(t) for t in [c['xb']] + c['m'])
            sl.c9 = (_lib.C.c_float * 9)(*c['c9'])
            sl.m_out, sl.x_state_out = _lib.ptr(c['m_out']), _lib.ptr(c['state'])
        else:
            c['t_next'] = 1000 * (k + 1) + 7
            n_old = {0: 0, 1: 1, 2: 2, 3: 3, 4: 1}[s['mode']]
            c['old'] = [put(f'old{j}_', _normal(g, (n,))) for j in range(n_old)]
            c['noise'] = put('noise', _normal(g, (n,))) if s['noise'] else None
            c['ins'] += c['old'] + ([c['noise']] if s['noise'] else [])
            c['e_out'] = new('e_t') if 'e' in o else None
            c['state'] = c['x'] if 'i' in o else (new('state') if 's' in o else None)
            c['pred'] = new('pred') if 'p' in o else None
            sl.mode = s['mode']
            sl.x = c['x'].data_ptr()
            sl.old0, sl.old1, sl.old2 = ([t.data_ptr() for t in c['old']] + [None] * 3)[:3]
            sl.noise = _lib.ptr(c['noise'])
            sl.a_t, sl.a_prev, sl.sigma = s['a_t'], s['a_prev'], s['sigma']
            sl.sqrt_1m_at = float(np.sqrt(np.float32(1.0) - np.float32(s['a_t'])))
            sl.e_t_out, sl.x_state_out, sl.pred_x0 = _lib.ptr(c['e_out']), _lib.ptr(c['state']), _lib.ptr(c['pred'])
        for j, r in enumerate(c['dst']):
            setattr(sl, f'unet_dst{j}', X_next[r].data_ptr())
            setattr(sl, f'tf_dst{j}', T_next[r:r + 1].data_ptr())
        sl.t_next = c['t_next']
        c['in_copies'] = [t.clone() for t in c['ins']]
        c['slot'] = sl
        slots.append(sl)
        cases.append(c)
    eps_copy = eps.clone()

    # the lone launches of every slot first (the launch below may write a state over an input)
    for c in cases:
        s, sl = c['s'], c['slot']
        if s['kind'] == 1:
            pair = (torch.stack([c['eu'], c['ec']]) if s['cfg'] else c['eu']).contiguous()
            m = torch.empty(n, device='cuda')
            xs = c['x'].contiguous()
            _lib.check(lib.sdmi_dpm_model_value(pair.data_ptr(), s['cfg'], s['scale'], xs.data_ptr() if s['px'] else None, s['px'], c['alpha'],
                                                c['sigma'], None, n, m.data_ptr(), n, st))
            c['lone_m'], c['lone_x'] = m, m
            if s['form'] >= 0:
                ms = [m if s['self'] >> j & 1 else (None if t is None else t.contiguous()) for j, t in enumerate(c['m'])]
                c['lone_x'] = torch.empty(n, device='cuda')
                _lib.check(lib.sdmi_dpm_update(s['form'], c['xb'].contiguous().data_ptr(), ms[0].data_ptr(), _lib.ptr(ms[1]), _lib.ptr(ms[2]),
                                               (_lib.C.c_float * 9)(*c['c9']), c['lone_x'].data_ptr(), n, st))
        else:                            # the same slot through sdmi_sampler_step_rows, its outputs into buffers of their own
            tw = _lib.SamplerSlot()
            for f in ('eps_u', 'eps_c', 'x', 'old0', 'old1', 'old2', 'noise', 'cfg', 'mode', 'scale', 'a_t', 'a_prev', 'sigma', 'sqrt_1m_at'):
                setattr(tw, f, getattr(sl, f))
            c['twin'] = [torch.full((n,), float('nan'), device='cuda') for _ in range(3)]
            tw.e_t_out, tw.pred_x0, tw.x_state_out = (t.data_ptr() for t in c['twin'])
            tw.t_next = c['t_next']
            if c['dst']:
                tw.t_dst0 = T_i64[c['dst'][0]:].data_ptr()
            _lib.check(lib.sdmi_sampler_step_rows((_lib.SamplerSlot * 1)(tw), 1, n, st))
    torch.cuda.synchronize()
    arr = (_lib.SamplerPlanSlot * len(slots))(*slots)
    _lib.check(lib.sdmi_sampler_plan_rows(arr, len(slots), n, st))
    torch.cuda.synchronize()

    written = set()
    for c in cases:
        s, k = c['s'], c['k']
        if s['kind'] == 1:
            eu, ec = c['eu'].cpu()[None], (None if c['ec'] is None else c['ec'].cpu()[None])
            e = torch.cat([eu, ec]) if s['cfg'] else eu
            m_ref = DC.torch_model_value(e, c['x_cpu'][None], bool(s['cfg']), s['scale'], bool(s['px']), torch.tensor(c['alpha']),
                                         torch.tensor(c['sigma']))
            x_ref = m_ref
            if s['form'] >= 0:
                ms = [m_ref if s['self'] >> j & 1 else c['m_cpu'][j][None] for j in range(3)]
                x_ref = DC.torch_update(s['form'], c['xb_cpu'][None], ms, [torch.tensor(v) for v in c['c9']])
            outs = (('m_out', c['m_out'], m_ref, c['lone_m']), ('state', c['state'], x_ref, c['lone_x']))
        else:
            x_ref = c['twin'][2].cpu()
            outs = (('e_t_out', c['e_out'], c['twin'][0].cpu(), c['twin'][0]), ('pred_x0', c['pred'], c['twin'][1].cpu(), c['twin'][1]),
                    ('state', c['state'], x_ref, c['twin'][2]))
            assert not bool(torch.isnan(c['twin'][2]).any())
        lone_x = outs[-1][3]
        for name, got, ref, lone in outs:
            if got is None:
                continue
            assert torch.equal(got.cpu(), ref.reshape(-1)), f'slot {k} {name}: not the reference\'s bits'
            assert torch.equal(got, lone), f'slot {k} {name}: not the lone launch\'s bits'
        for r in c['dst']:
            assert torch.equal(X_next[r].cpu(), x_ref.reshape(-1)), f'slot {k} unet_dst row {r}'
            assert torch.equal(X_next[r], lone_x)
            assert float(T_next[r]) == float(c['t_next']), f'slot {k} tf_dst row {r}'
            written.add(r)
        if s['kind'] == 0 and c['dst']:
            assert int(T_i64[c['dst'][0]]) == c['t_next'] and float(np.float32(c['t_next'])) == c['t_next']
        # inputs are untouched (a state written over x_base / x is an output)
        over = c.get('xb') if s['kind'] == 1 else c['x']
        for t, saved in zip(c['ins'], c['in_copies']):
            if 'i' in s['outs'] and t is over:
                continue
            assert torch.equal(t, saved), f'slot {k}: an input was written'
    assert torch.equal(eps, eps_copy)
    for r in range(ROWS):                           # rows of the next call that no slot feeds keep their fill
        if r not in written:
            assert bool(torch.isnan(X_next[r]).all()) and bool(torch.isnan(T_next[r])), f'row {r} of an unused destination was written'
    P.check(f'{path} x {n_slots} slots')


def test_refusals_launch_nothing():
    """each refusal by name; the destinations of the refused launch keep their fill"""
    lib = _lib.load()
    P = Pool()
    n = 64
    src = P.put('src', torch.ones(6 * n))
    out = P.new('out', (3 * n,), torch.float32)
    t_out = P.new('t', (2,), torch.float32)
    at = lambda j: src[j * n:].data_ptr()

    def slot(**kw):
        s = _lib.SamplerPlanSlot()
        s.kind, s.eps_u, s.x, s.x_base, s.data_prediction, s.m_self = 1, at(0), at(1), at(2), 1, 1
        s.x_state_out, s.unet_dst0, s.m_out, s.tf_dst0 = out.data_ptr(), out[n:].data_ptr(), out[2 * n:].data_ptr(), t_out.data_ptr()
        s.alpha_t, s.sigma_t, s.scale, s.t_next = 0.5, 0.6, 1.0, 5.5
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    step = lambda **kw: slot(kind=0, a_t=0.5, a_prev=0.6, **kw)
    none = dict(x_state_out=None, unet_dst0=None, m_out=None)
    cases = [([slot()] * 9, n, 'more than SDMI_SAMPLER_MAX_SLOTS'), ([slot()], 0, 'sampler_plan_rows: n'), ([slot()], -1, 'sampler_plan_rows: n'),
             ([slot(kind=3)], n, 'sampler_plan_rows: kind'), ([slot(eps_u=None)], n, 'missing pointer'), ([slot(cfg=1)], n, 'missing pointer'),
             ([slot(x=None)], n, 'the data prediction needs x'), ([slot(x_base=None)], n, 'missing pointer: x_base'),
             ([slot(m_self=0)], n, 'a model value of the update'), ([slot(form=1, m1=at(3))], n, 'a model value of the update'),
             ([slot(form=2, m_self=2, m0=at(3))], n, 'a model value of the update'), ([slot(**none)], n, 'missing pointer: no output'),
             ([slot(), slot(form=4)], n, r'sampler_plan_rows: form \(slot 1\)'), ([slot(form=-2)], n, 'sampler_plan_rows: form'),
             ([slot(form=-1)], n, 'm_self names an operand'), ([slot(m_self=2)], n, 'm_self names an operand'),
             ([slot(form=3, m_self=9, m1=at(3), m2=at(4))], n, 'm_self names an operand'),
             ([step(x=None)], n, 'missing pointer'), ([step(**none)], n, 'missing pointer: no output'),
             ([slot(), step(mode=5)], n, r'sampler_plan_rows: mode \(slot 1\)'), ([step(mode=-1)], n, 'sampler_plan_rows: mode'),
             ([step(mode=1)], n, 'history missing'), ([step(mode=2, old0=at(3))], n, 'history missing'),
             ([step(mode=3, old0=at(3), old1=at(4))], n, 'history missing')]
    for slots, nn, name in cases:
        arr = (_lib.SamplerPlanSlot * len(slots))(*slots)
        assert lib.sdmi_sampler_plan_rows(arr, len(slots), nn, _lib.stream_ptr()) != 0, name
        assert re.search(name, lib.sdmi_last_error().decode()), (name, lib.sdmi_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(t_out).all())
    P.check('refusals')
