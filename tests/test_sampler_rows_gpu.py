"""sdmi_sampler_step_rows in guarded buffers: one launch for up to eight latents at different steps, each slot bit-equal to the reference's
torch expressions (plms.py:178-236, ddim.py:165-204) evaluated op by op on the CPU, and to a lone sdmi_sampler_step call with its arguments.

Portability: the three table scalars of a step -- sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2) -- are one-element tensor ops in the
reference and host sqrtf calls in the library.  torch's CPU sqrt is not the correctly rounded one at every value on every CPU model
(tools/make_golden_ddpm.py), so the CPU expression below takes these three through numpy's fp32 sqrt, which is; every other op is torch's."""
import numpy as np
import pytest
import torch

from guard import Pool
from stable_diffusion_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = {'vec': (4, 8, 8), 'scalar': (3, 5, 7)}       # 256 elements on the 16-byte path; 105: the scalar path, a tail inside one block
# per slot: guided, mode, sigma, noise given, outputs (e = e_t_out, s = state, i = state in place, p = pred_x0, 0 / 1 = unet_dst0 / 1), a_t, a_prev
SLOTS = [
    dict(cfg=1, mode=0, sigma=0.21, noise=True, outs='ip01', a_t=0.4321, a_prev=0.5678, scale=7.5),      # guided DDIM, eta > 0
    dict(cfg=0, mode=1, sigma=0.0, noise=False, outs='esp0', a_t=0.731, a_prev=0.802, scale=1.0),
    dict(cfg=1, mode=2, sigma=0.0, noise=False, outs='ei01', a_t=0.055, a_prev=0.093, scale=3.0),
    dict(cfg=0, mode=3, sigma=0.15, noise=True, outs='esp', a_t=0.9123, a_prev=0.9456, scale=1.0, misalign=True),   # a last step: no rows to feed
    dict(cfg=1, mode=4, sigma=0.0, noise=False, outs='ip01', a_t=0.0047, a_prev=0.0212, scale=5.0),       # the PLMS corrector
    dict(cfg=0, mode=0, sigma=0.0, noise=False, outs='e0', a_t=0.0047, a_prev=0.0212, scale=1.0),         # the PLMS predictor: state left alone
    dict(cfg=1, mode=3, sigma=0.08, noise=True, outs='esp01', a_t=0.618, a_prev=0.667, scale=7.5),
    dict(cfg=0, mode=0, sigma=0.0, noise=True, outs='sp0', a_t=0.25, a_prev=0.3, scale=1.0),              # sigma = 0 with a noise pointer
]
LAUNCHES = {1: [5], 3: [2, 3, 0], 8: list(range(8))}


def _normal(g, shape):
    return torch.randn(shape, generator=g)


def reference_step(s, eu, ec, x, old, noise):
    """the reference's expressions on [1, C, H, W] CPU tensors -> e_t, pred_x0, x_prev"""
    e_t = eu + s['scale'] * (ec - eu) if s['cfg'] else eu
    m = s['mode']
    if m == 0: ep = e_t
    elif m == 1: ep = (3 * e_t - old[0]) / 2
    elif m == 2: ep = (23 * e_t - 16 * old[0] + 5 * old[1]) / 12
    elif m == 3: ep = (55 * e_t - 59 * old[0] + 37 * old[1] - 9 * old[2]) / 24
    else: ep = (old[0] + e_t) / 2
    full = lambda v: torch.full((1, 1, 1, 1), v)
    sqrt = lambda t: torch.from_numpy(np.sqrt(t.numpy()))              # (see the module docstring)
    at, ap, sg = full(s['a_t']), full(s['a_prev']), full(s['sigma'])
    sm = full(float(np.sqrt(np.float32(1.0) - np.float32(s['a_t']))))
    pred = (x - sm * ep) / sqrt(at)
    dir_xt = sqrt(1. - ap - sg ** 2) * ep
    xp = sqrt(ap) * pred + dir_xt + (sg * noise if noise is not None else 0.)
    return e_t, pred, xp, float(sm)


@pytest.mark.parametrize('n_slots', [1, 3, 8])
@pytest.mark.parametrize('path', ['vec', 'scalar'])
def test_rows_step_equals_the_reference_and_the_lone_step(path, n_slots):
    lib = _lib.load()
    shape = SHAPES[path]
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(100 * n_slots + n)
    P = Pool()
    ROWS = 13                                       # rows of the "next call": two more than the eight-slot launch fills
    eps = P.put('eps', _normal(g, (16,) + shape))                       # the UNet output: up to two rows per slot
    X_next = P.new('X_next', (ROWS,) + shape, torch.float32)
    T_next = P.new('T_next', (ROWS,), torch.int64)
    slots, cases, row, d = [], [], 0, 0
    for k in LAUNCHES[n_slots]:
        s = SLOTS[k]
        c = dict(s=s, k=k)
        mis = 1 if (s.get('misalign') and path == 'vec') else 0        # one slot of a 16-byte launch goes element by element
        put = lambda name, t: P.put(f'{name}{k}', torch.cat([torch.zeros(mis), t.reshape(-1)]))[mis:]
        new = lambda name: P.new(f'{name}{k}', (n,), torch.float32)
        c['x_cpu'] = _normal(g, (1,) + shape) * 2
        c['old_cpu'] = [_normal(g, (1,) + shape) for _ in range(3)]
        c['noise_cpu'] = _normal(g, (1,) + shape) if s['noise'] else None
        c['x'] = put('x', c['x_cpu'])
        n_old = {0: 0, 1: 1, 2: 2, 3: 3, 4: 1}[s['mode']]
        c['old'] = [put(f'old{j}_', c['old_cpu'][j]) for j in range(n_old)]
        c['noise'] = put('noise', c['noise_cpu']) if s['noise'] else None
        c['in_copies'] = [t.clone() for t in [c['x']] + c['old'] + ([c['noise']] if s['noise'] else [])]
        c['eu'], c['ec'] = eps[row], (eps[row + 1] if s['cfg'] else None)
        row += 2 if s['cfg'] else 1
        o = s['outs']
        c['e_out'] = new('e_t') if 'e' in o else None
        c['state'] = c['x'] if 'i' in o else (new('state') if 's' in o else None)
        c['pred'] = new('pred') if 'p' in o else None
        c['dst'] = []
        for flag in '01':
            if flag in o:
                c['dst'].append(d)
                d += 1
        c['t_next'] = 1000 * (k + 1) + 7 + (2 ** 33 if k == 6 else 0)   # (a value that needs all 64 bits too)
        sl = _lib.SamplerSlot()
        sl.eps_u, sl.eps_c = c['eu'].data_ptr(), _lib.ptr(c['ec'])
        sl.cfg, sl.scale, sl.mode = s['cfg'], s['scale'], s['mode']
        sl.x = c['x'].data_ptr()
        sl.old0, sl.old1, sl.old2 = ([t.data_ptr() for t in c['old']] + [None] * 3)[:3]
        sl.noise = _lib.ptr(c['noise'])
        c['s1m'] = float(np.sqrt(np.float32(1.0) - np.float32(s['a_t'])))
        sl.a_t, sl.a_prev, sl.sigma, sl.sqrt_1m_at = s['a_t'], s['a_prev'], s['sigma'], c['s1m']
        sl.e_t_out, sl.x_state_out, sl.pred_x0 = _lib.ptr(c['e_out']), _lib.ptr(c['state']), _lib.ptr(c['pred'])
        for j, r in enumerate(c['dst']):
            setattr(sl, f'unet_dst{j}', X_next[r].data_ptr())
            setattr(sl, f't_dst{j}', T_next[r:r + 1].data_ptr())
        sl.t_next = c['t_next']
        slots.append(sl)
        cases.append(c)
    eps_copy = eps.clone()
    # the lone step of every slot first (the launch below may update a state in place)
    for c in cases:
        s = c['s']
        if s['cfg']:
            pair = torch.stack([c['eu'], c['ec']]).contiguous()
        else:
            pair = c['eu'].contiguous()
        c['lone'] = [torch.empty(n, device='cuda') for _ in range(3)]
        o = [t.contiguous() for t in c['old']]
        xs, nz = c['x'].contiguous(), (None if c['noise'] is None else c['noise'].contiguous())
        _lib.check(lib.sdmi_sampler_step(pair.data_ptr(), s['cfg'], s['scale'], xs.data_ptr(), s['mode'], *([t.data_ptr() for t in o] + [None] * 3)[:3],
                                         s['a_t'], s['a_prev'], s['sigma'], c['s1m'], _lib.ptr(nz), c['lone'][0].data_ptr(),
                                         c['lone'][2].data_ptr(), c['lone'][1].data_ptr(), n, _lib.stream_ptr()))
    torch.cuda.synchronize()
    arr = (_lib.SamplerSlot * len(slots))(*slots)
    _lib.check(lib.sdmi_sampler_step_rows(arr, len(slots), n, _lib.stream_ptr()))
    torch.cuda.synchronize()

    written = set()
    for c in cases:
        s, k = c['s'], c['k']
        e_ref, p_ref, x_ref, _ = reference_step(s, c['eu'].cpu()[None], None if c['ec'] is None else c['ec'].cpu()[None], c['x_cpu'],
                                                c['old_cpu'], c['noise_cpu'])
        for name, got, ref, lone in (('e_t_out', c['e_out'], e_ref, c['lone'][0]), ('pred_x0', c['pred'], p_ref, c['lone'][1]),
                                     ('state', c['state'], x_ref, c['lone'][2])):
            if got is None:
                continue
            assert torch.equal(got.cpu(), ref.reshape(-1)), f'slot {k} {name}: not the reference\'s bits'
            assert torch.equal(got, lone), f'slot {k} {name}: not the lone step\'s bits'
        for r in c['dst']:
            assert torch.equal(X_next[r].reshape(-1).cpu(), x_ref.reshape(-1)), f'slot {k} unet_dst row {r}'
            assert torch.equal(X_next[r].reshape(-1), c['lone'][2])
            assert int(T_next[r]) == c['t_next'], f'slot {k} t_dst row {r}'
            written.add(r)
        # inputs are untouched (a state updated in place is an output)
        ins = [c['x']] + c['old'] + ([c['noise']] if c['noise'] is not None else [])
        for t, saved in list(zip(ins, c['in_copies']))[(1 if 'i' in s['outs'] else 0):]:
            assert torch.equal(t, saved), f'slot {k}: an input was written'
        if 'i' not in s['outs'] and c['state'] is None:
            assert torch.equal(c['x'], c['in_copies'][0])               # the predictor leaves the state alone
    assert torch.equal(eps, eps_copy)
    for r in range(ROWS):                           # rows of the next call that no slot feeds keep their fill
        if r not in written:
            assert bool(torch.isnan(X_next[r]).all()) and int(T_next[r]) == -1, f'row {r} of an unused destination was written'
    P.check(f'{path} x {n_slots} slots')


def test_refusals_launch_nothing():
    """each refusal by name; the destinations of the refused launch keep their fill"""
    import re
    lib = _lib.load()
    P = Pool()
    n = 64
    src = P.put('src', torch.ones(4 * n))
    out = P.new('out', (2 * n,), torch.float32)
    t_out = P.new('t', (2,), torch.int64)

    def slot(**kw):
        s = _lib.SamplerSlot()
        s.eps_u, s.x, s.x_state_out, s.unet_dst0, s.t_dst0 = src.data_ptr(), src[n:].data_ptr(), out.data_ptr(), out[n:].data_ptr(), t_out.data_ptr()
        s.a_t, s.a_prev, s.scale, s.t_next = 0.5, 0.6, 1.0, 5
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    cases = [([slot()] * 9, n, 'more than SDMI_SAMPLER_MAX_SLOTS'), ([slot()], 0, 'sampler_step_rows: n'), ([slot(x=None)], n, 'missing pointer'),
             ([slot(cfg=1)], n, 'missing pointer'), ([slot(x_state_out=None, unet_dst0=None)], n, 'missing pointer: no output'),
             ([slot(), slot(mode=5)], n, r'sampler_step_rows: mode \(slot 1\)'), ([slot(mode=1)], n, 'history missing'),
             ([slot(mode=2, old0=src[2 * n:].data_ptr())], n, 'history missing'),
             ([slot(mode=3, old0=src[2 * n:].data_ptr(), old1=src[3 * n:].data_ptr())], n, 'history missing')]
    for slots, nn, name in cases:
        arr = (_lib.SamplerSlot * len(slots))(*slots)
        assert lib.sdmi_sampler_step_rows(arr, len(slots), nn, _lib.stream_ptr()) != 0
        assert re.search(name, lib.sdmi_last_error().decode()), (name, lib.sdmi_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and t_out.tolist() == [-1, -1]
    P.check('refusals')
