"""`SamplerPoolHIP`: requests that arrive one after another share UNet calls.

`PLMSSamplerHIP` / `DDIMSamplerHIP` run one request, all of its samples in lock-step: one schedule, one history, host scalars per launch.
A larger UNet batch costs 1.3-1.6x less per prompt (profiles/unet_latency_vs_batch_r04.txt), but only a caller that holds all its prompts
at the start gets it.  The pool keeps the rows of every UNet call filled as requests come and go: each row of a call may stand at another
step of another schedule -- `UNetModelHIP.forward` takes a timestep and a context per row anyway -- and ONE launch
(`sdmi_sampler_step_rows`, csrc/sampler.hip) advances all of them, each slot with its own table entries, history and destinations.  The
launch writes every x_prev a second time, into the row(s) of the NEXT call's input, and that row's timestep beside it, so the steady state
is the UNet call plus one launch with no host-to-device copy; which rows the next call has is known before the launch, because the plan is
deterministic (`plan_calls`).

Per slot the arithmetic is `sdmi_sampler_step`'s, so a request's samples and intermediates are, with a model whose rows are independent
(every UNet here), the bits of the same request run alone -- up to what the UNet's own kernels make of another row count.

`SamplerPoolHIP(..., timesteps='float32')` is a pool whose calls carry fp32 timesteps -- the UNet embeds (float)t either way, so an integer
timestep handed over as fp32 gives the same bits -- and whose launch is `sdmi_sampler_plan_rows`: a slot is that PLMS / DDIM step, or one
model evaluation of a DPM-Solver plan (`DPMSolverHIP.plan`) with the update that follows it.  Such a pool also takes `sampler='dpm'`."""
import numpy as np
import torch

from . import _lib
from .samplers import DPMSolverHIP, _DiscreteVP, make_ddim_timesteps, make_tables, plms_plan


# ---- the plan: pure host code, no GPU and no library ------------------------------------------------------------------------------
def request_timesteps(S, num_timesteps=1000, ddim_discretize='uniform', t_start=None):
    """the DDIM timesteps a request walks (flipped by the loop): all of make_ddim_timesteps, or with t_start the first t_start of them
    (DDIMSampler.decode, ddim.py:222-241)"""
    ts = make_ddim_timesteps(S, num_timesteps, ddim_discretize)
    return ts if t_start is None else ts[:t_start]


DPM_POOL_KEYWORDS = ('method', 'order', 'skip_type', 'predict_x0', 't_start', 't_end', 'lower_order_final', 'denoise_to_zero', 'solver_type')


def dpm_request_plan(alphas_cumprod, S, plan=None, **kw):
    """-> (DPMPlan, predict_x0) of a sampler='dpm' request: the given `plan`, or DPMSolverHIP.plan with the keywords of
    DPMSolverSamplerHIP.sample and its values for the rest (steps = S, predict_x0 = True, 'multistep', order 2, 'time_uniform',
    lower_order_final).  Refused: what has no plan (adaptive), what sits between a model value and its update (thresholding), and whatever
    DPMSolverHIP.plan refuses."""
    if kw.get('method') == 'adaptive':
        raise NotImplementedError("method='adaptive': its number of evaluations depends on the data, so there is no plan to share calls by")
    if kw.pop('thresholding', False):
        raise NotImplementedError('thresholding=True: the per-sample quantile sits between the model value and the update of one slot')
    unknown = sorted(k for k in kw if k not in DPM_POOL_KEYWORDS)
    if unknown:
        raise TypeError(f"sampler='dpm' takes {', '.join(DPM_POOL_KEYWORDS)} and plan; got {', '.join(unknown)}")
    predict_x0 = bool(kw.pop('predict_x0', True))
    if plan is not None:
        if any(v is not None for v in kw.values()):
            raise TypeError(f'plan= is a whole run: it goes with predict_x0 alone, not with {", ".join(sorted(kw))}')
        return plan, predict_x0
    if alphas_cumprod is None:
        raise ValueError("a sampler='dpm' request without a plan needs the schedule: pass alphas_cumprod")
    opts = dict(steps=int(S), order=2, skip_type='time_uniform', method='multistep', lower_order_final=True)
    opts.update({k: v for k, v in kw.items() if not (k in ('t_start', 't_end') and v is None)})
    ac = alphas_cumprod if torch.is_tensor(alphas_cumprod) else torch.as_tensor(np.asarray(alphas_cumprod))
    return DPMSolverHIP(None, _DiscreteVP(ac), predict_x0=predict_x0).plan(**opts), predict_x0


def dpm_plan_pairs(plan):
    """[(k, k + 1 or None)]: every model evaluation of a DPMPlan with the index of the update that follows it (None after the last
    evaluation of denoise_to_zero).  A plan alternates evaluation, update, ...; each evaluation but the first is at the state the update
    before it wrote -- what lets one slot run the pair and feed the next call."""
    ops, pairs, k = plan.ops, [], 0
    while k < len(ops):
        upd = k + 1 if k + 1 < len(ops) else None
        if int(ops[k][0]) != 0 or (upd is not None and int(ops[upd][0]) != 1):
            raise ValueError(f'the plan does not alternate evaluation and update at op {k}')
        if pairs and int(ops[k][3]) != int(ops[k - 1][2]):
            raise ValueError(f'the evaluation at op {k} is not at the state the update before it wrote')
        pairs.append((k, upd))
        k += 2
    if not pairs:
        raise ValueError('the plan has no model evaluation')
    return pairs


def request_evals(sampler, timesteps, plan=None):
    """[(t, mode, index, phase)], one per UNet evaluation of a request: the DDIM time range (ddim.py:141-146, mode 0), or plms_plan with
    its first step as the two evaluations it is -- the Euler predictor (t, 0, index, 0), which only feeds the next call, and the corrector
    (t_next, 4, index, 1) (plms.py:218-226).  sampler='dpm' (timesteps unused): the evaluations of the DPMPlan `plan`, each
    (t_input, form of the update that follows or -1, evaluation number, 0)."""
    if sampler == 'dpm':
        return [(float(plan.coef[k][1]), -1 if u is None else int(plan.ops[u][1]), j, 0) for j, (k, u) in enumerate(dpm_plan_pairs(plan))]
    timesteps = np.asarray(timesteps)
    if sampler == 'plms':
        out = []
        for (i, index, t, t_next, mode) in plms_plan(timesteps):
            out += [(t, 0, index, 0), (t_next, 4, index, 1)] if mode == 4 else [(t, mode, index, 0)]
        return out
    if sampler != 'ddim':
        raise NotImplementedError(f"sampler={sampler!r}: 'ddim' or 'plms'")
    total = timesteps.shape[0]
    return [(int(t), 0, total - i - 1, 0) for i, t in enumerate(np.flip(timesteps))]


class _Entry:
    """what the queue knows of a request"""

    def __init__(self, ticket, samples, guided, evals):
        self.ticket, self.samples, self.guided, self.evals = ticket, int(samples), bool(guided), evals
        self.rows = self.samples * (2 if self.guided else 1)
        self.cursor = 0

    def call_rows(self):
        t, mode, index, phase = self.evals[self.cursor]
        return [(self.ticket, j, t, mode, index, phase) for j in range(self.samples) for _ in range(2 if self.guided else 1)]


class _Queue:
    """Strict FIFO over a row budget: the head enters when its rows are free and is never overtaken; rows are in admission order and close
    up when a request leaves.  plan_calls and SamplerPoolHIP.step both run on this, so the pool cannot execute another plan."""

    def __init__(self, max_rows):
        self.max_rows, self.waiting, self.active = int(max_rows), [], []

    def rows_used(self):
        return sum(e.rows for e in self.active)

    def admit(self):
        entered = []
        while self.waiting and self.rows_used() + self.waiting[0].rows <= self.max_rows:
            entered.append(self.waiting.pop(0))
            self.active.append(entered[-1])
        return entered

    def call_rows(self):
        return [row for e in self.active for row in e.call_rows()]

    def advance(self):
        """after a call: -> the requests that made their last evaluation in it"""
        for e in self.active:
            e.cursor += 1
        left = [e for e in self.active if e.cursor == len(e.evals)]
        self.active = [e for e in self.active if e.cursor < len(e.evals)]
        return left


def plan_calls(requests, max_rows=8, num_timesteps=1000, alphas_cumprod=None):
    """The UNet calls a pool of `max_rows` rows makes for `requests`, each a dict(ticket, S, sampler='ddim', samples=1, guided=False,
    ddim_discretize='uniform', t_start=None, arrival=0); `arrival` is the number of calls the pool had made when the request was
    submitted (a request submitted to an idle pool arrives at once).  -> one list per call of (ticket, sample, t, mode, index, phase), a
    guided sample's row twice ([uncond, cond]).  A sampler='dpm' request carries `plan` (a DPMPlan), or S and the keywords of
    dpm_request_plan over `alphas_cumprod`; its rows are (ticket, sample, t_input, form of the following update or -1, evaluation, 0)."""
    pending = sorted(((int(r.get('arrival', 0)), k, r) for k, r in enumerate(requests)), key=lambda a: a[:2])
    q, calls = _Queue(max_rows), []
    while pending or q.waiting or q.active:
        if not (q.waiting or q.active):
            pending[0] = (len(calls),) + pending[0][1:]           # the pool idles until the next request
        while pending and pending[0][0] <= len(calls):
            r = pending.pop(0)[2]
            if r.get('sampler', 'ddim') == 'dpm':
                plan = dpm_request_plan(alphas_cumprod, r.get('S'), r.get('plan'), **{k: r[k] for k in DPM_POOL_KEYWORDS + ('thresholding',) if k in r})[0]
                evals = request_evals('dpm', None, plan)
            else:
                ts = request_timesteps(r['S'], num_timesteps, r.get('ddim_discretize', 'uniform'), r.get('t_start'))
                evals = request_evals(r.get('sampler', 'ddim'), ts)
            e = _Entry(r['ticket'], r.get('samples', 1), r.get('guided', False), evals)
            if e.rows > max_rows:
                raise ValueError(f'request {e.ticket!r} needs {e.rows} rows, the pool has {max_rows}: it can never fit')
            q.waiting.append(e)
        q.admit()
        calls.append(q.call_rows())
        q.advance()
    return calls


# ---- the pool -------------------------------------------------------------------------------------------------------------------------
class SamplerPoolHIP(object):
    """SamplerPoolHIP(model, shape=(C, H, W), max_rows=UNetModelHIP.MAX_ROWS, timesteps='int64') over the `model` the samplers take
    (apply_model, alphas_cumprod, betas, num_timesteps).

        ticket = pool.submit(S=50, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=7.5)
        pool.step()                 # one UNet evaluation of every active request: one apply_model, one sdmi_sampler_step_rows launch
        pool.run_until_idle()
        samples, intermediates = pool.result(ticket)       # as sample() returns them

    A request without a `generator` gets one of its own, seeded from torch's default generator at submit: what its neighbours in a call
    draw never changes its draws.

    timesteps='float32': every call carries fp32 timesteps and every step is one sdmi_sampler_plan_rows launch; 'ddim' and 'plms' requests
    run as in the default pool, and sampler='dpm' is taken too -- S model evaluations of DPM-Solver++(2M) by default, or what the keywords of
    DPMSolverSamplerHIP.sample (DPM_POOL_KEYWORDS; t_start is DPM-Solver's float time there) or a ready `plan=` say; result() gives
    (x, None), an img_callback receives the model value and the evaluation number.  The dtype is the pool's for good, like its shape."""

    def __init__(self, model, shape, max_rows=None, timesteps='int64'):
        from .unet import UNetModelHIP
        self.model = model
        self.shape = tuple(int(s) for s in shape)
        if len(self.shape) != 3:
            raise ValueError(f'shape is (C, H, W), got {shape!r}')
        self.max_rows = int(UNetModelHIP.MAX_ROWS if max_rows is None else max_rows)
        if self.max_rows < 1:
            raise ValueError('max_rows must be at least 1')
        if timesteps not in ('int64', 'float32'):
            raise ValueError(f"timesteps={timesteps!r}: 'int64' or 'float32'")
        self.timesteps = timesteps
        self._float = timesteps == 'float32'
        self.n = int(np.prod(self.shape))
        self._q = _Queue(self.max_rows)
        self._ac = None
        self._tokens = None         # (tokens, width) of every context of this pool: the first accepted request's
        self._lib = None
        self._X = self._T = self._ctx = None
        self._views = None          # (x, t, context) of the current row set: the same objects from call to call while it stands
        self._layout = None         # [(ticket, first row)] the views were made for
        self._results = {}
        self._next_ticket = 0
        self.calls = 0              # UNet calls made
        self.trace = None           # set to [] to record every call's rows, as plan_calls lists them

    # ---- overridable draws, as the samplers have them ---------------------------------------------------------------------------------
    def _noise_like(self, shape, device, generator=None, ticket=None):
        """util.py noise_like (ddim.py:200): one draw per step of a request with eta > 0, from the request's own generator.  A method of
        its own so that a parity test can hand out the recorded draws of a reference run, by ticket."""
        return torch.randn(shape, device=device, generator=generator)

    def _hip_unet(self):
        from .unet import UNetModelHIP
        u = getattr(getattr(self.model, 'model', None), 'diffusion_model', None)
        return u if isinstance(u, UNetModelHIP) else None

    @staticmethod
    def _check_device(tensors):
        if not all(t.is_cuda for t in tensors):
            raise RuntimeError('CPU tensors: the sampler pool runs on MI355X device tensors only (no CPU fallback)')

    # ---- submit -------------------------------------------------------------------------------------------------------------------------
    def submit(self, S, conditioning, unconditional_conditioning=None, unconditional_guidance_scale=1., eta=0., x_T=None, sampler='ddim',
               ddim_discretize='uniform', t_start=None, generator=None, img_callback=None, log_every_t=100, mask=None, x0=None,
               quantize_x0=False, score_corrector=None, plan=None, **dpm_keywords):
        if mask is not None or x0 is not None:
            raise NotImplementedError('mask / x0 (the inpainting blend draws q_sample noise between the steps) is not implemented in the pool')
        if quantize_x0:
            raise NotImplementedError('quantize_x0 (the step split around the codebook quantizer) is not implemented in the pool')
        if score_corrector is not None:
            raise NotImplementedError('score_corrector is not implemented here (the reference ships no corrector)')
        if isinstance(conditioning, dict) or isinstance(unconditional_conditioning, dict):
            raise NotImplementedError('dict conditioning (hybrid models) is not implemented in the pool')
        if sampler == 'dpm' and not self._float:
            raise NotImplementedError("sampler='dpm': DPM-Solver's float timesteps cannot share a call with integer ones")
        if sampler not in ('ddim', 'plms', 'dpm'):
            raise NotImplementedError(f"sampler={sampler!r}: 'ddim' or 'plms'" + (" or 'dpm'" if self._float else ''))
        if sampler != 'dpm' and (plan is not None or dpm_keywords):
            raise TypeError(f"{', '.join(sorted(dpm_keywords) or ['plan'])}: keywords of sampler='dpm'")
        if sampler == 'dpm' and eta != 0:
            raise ValueError('eta must be 0 for DPM-Solver')
        dpm = None
        if sampler == 'dpm':             # (refuses adaptive, thresholding and what DPMSolverHIP.plan refuses: host code only)
            dpm = dpm_request_plan(self.model.alphas_cumprod, S, plan, t_start=t_start, **dpm_keywords)
        if sampler == 'plms' and eta != 0:
            raise ValueError('eta must be 0 for PLMS')
        if sampler == 'plms' and t_start is not None:
            raise NotImplementedError('t_start is DDIMSampler.decode: not defined for PLMS')
        if not torch.is_tensor(conditioning) or conditioning.dim() != 3:
            raise ValueError('conditioning is a [samples, tokens, width] tensor')
        b = int(conditioning.shape[0])
        uc, scale = unconditional_conditioning, float(unconditional_guidance_scale)
        guided = not (uc is None or scale == 1.)
        if guided and tuple(uc.shape) != tuple(conditioning.shape):
            raise ValueError(f'unconditional_conditioning {tuple(uc.shape)} does not match conditioning {tuple(conditioning.shape)}')
        if x_T is not None and tuple(x_T.shape) != (b,) + self.shape:
            raise ValueError(f'shape {tuple(x_T.shape)} is not the pool\'s: x_T must be [{b}, {", ".join(map(str, self.shape))}]')
        if t_start is not None and x_T is None and sampler != 'dpm':
            raise ValueError('t_start decodes a given latent: pass it as x_T')
        tokens = tuple(int(s) for s in conditioning.shape[1:])
        if self._tokens is not None and tokens != tuple(self._tokens):
            raise ValueError(f'token count: this pool\'s contexts are [{self._tokens[0]}, {self._tokens[1]}], got [{tokens[0]}, {tokens[1]}]')
        rows = b * (2 if guided else 1)
        if rows > self.max_rows:
            raise ValueError(f'the request needs {rows} rows, the pool has {self.max_rows}: it can never fit')
        if dpm is None:
            ddim_timesteps = make_ddim_timesteps(S, self.model.num_timesteps, ddim_discretize)
            timesteps = ddim_timesteps if t_start is None else ddim_timesteps[:t_start]
            if timesteps.shape[0] < 1:
                raise ValueError('the request has no steps')
            evals = request_evals(sampler, timesteps)
        else:
            evals = request_evals('dpm', None, dpm[0])
        self._check_device([conditioning, self.model.betas] + ([uc] if guided else []) + ([x_T] if x_T is not None else []))
        device = self.model.betas.device

        if self._ac is None:
            ac = self.model.alphas_cumprod
            assert ac.shape[0] == self.model.num_timesteps, 'alphas have to be defined for each timestep'
            self._ac = ac.detach().to(torch.float32).cpu().numpy()
        r = _Entry(self._next_ticket, b, guided, evals)
        self._next_ticket += 1
        r.sampler, r.scale, r.eta, r.total = sampler, scale, float(eta), len(evals)
        if dpm is None:
            r.total = int(timesteps.shape[0])
            r.tab = make_tables(self._ac, ddim_timesteps, eta)        # exactly the tables of _SamplerBase._tables
        if generator is None and (eta != 0 or x_T is None):
            generator = torch.Generator(device=device)
            generator.manual_seed(int(torch.randint(0, 2 ** 62, (1,)).item()))
        r.generator = generator
        img = torch.randn((b,) + self.shape, device=device, generator=generator) if x_T is None else x_T
        img = img.detach().float().contiguous()
        r.state = r.own = img.clone()        # unlogged steps write x_prev into `own`, in place or not: never a tensor the caller has seen
        r.intermediates = {'x_inter': [img], 'pred_x0': [img]}
        cond = conditioning.detach().float()
        # a guided sample is two adjacent rows [uncond, cond]
        r.c_rows = torch.stack([uc.detach().float(), cond], dim=1).reshape((2 * b,) + tokens).contiguous() if guided else cond.contiguous()
        r.img_callback, r.log_every_t = img_callback, int(log_every_t)
        r.old, r.ring, r.e_pred, r.noise = [], None, None, None
        if dpm is not None:              # the plan's tensor slots are the request's state; slot 0 is the initial latent
            r.plan, r.predict_x0 = dpm
            r.pairs = dpm_plan_pairs(r.plan)
            r.buf = {0: r.state}
            r.last_use = {}
            for k, op in enumerate(r.plan.ops):
                for slot in op[3:]:
                    r.last_use[int(slot)] = k
            r.last_use[r.plan.result] = len(r.plan.ops)
            r.intermediates = None
        self._tokens = tokens
        self._q.waiting.append(r)
        return r.ticket

    # ---- buffers --------------------------------------------------------------------------------------------------------------------------
    def _allocate(self, device):
        self._lib = _lib.load()
        self._X = torch.zeros((self.max_rows,) + self.shape, device=device, dtype=torch.float32)
        self._T = torch.zeros((self.max_rows,), device=device, dtype=torch.float32 if self._float else torch.long)
        self._ctx = torch.zeros((self.max_rows,) + tuple(self._tokens), device=device, dtype=torch.float32)

    def _row_starts(self, active):
        starts, r0 = [], 0
        for e in active:
            starts.append((e.ticket, r0))
            r0 += e.rows
        return starts

    def _set_rows(self, entered):
        """the row set changed: bring the persistent context in line (only rows whose owner changed are written), hand the UNet the new
        K/V, and make the views the calls pass until the next change"""
        layout = self._row_starts(self._q.active)
        old = dict(self._layout or [])
        for e, (_, r0) in zip(self._q.active, layout):
            if old.get(e.ticket) != r0 or e in entered:
                self._ctx[r0:r0 + e.rows].copy_(e.c_rows)
        B = self._q.rows_used()
        self._views = (self._X[:B], self._T[:B], self._ctx[:B])
        self._layout = layout
        unet = self._hip_unet()
        if unet is not None:
            unet.pin_context(self._views[2])

    def _admit(self):
        entered = self._q.admit()
        if entered and self._X is None:
            self._allocate(entered[0].state.device)
        starts = dict(self._row_starts(self._q.active))
        for e in entered:             # plain tensor copies: the request's latent and first timestep into its rows
            r0, per = starts[e.ticket], (2 if e.guided else 1)
            self._X[r0:r0 + e.rows].copy_(e.state.repeat_interleave(per, dim=0) if per == 2 else e.state)
            self._T[r0:r0 + e.rows].fill_(e.evals[0][0])
            if e.sampler == 'plms':
                e.ring = [torch.empty_like(e.state) for _ in range(4)]      # e_t history: three old ones and the one being written
        return entered

    def _dpm_slots(self, e, eps, nxt_row, after):
        """the kind 1 slots of a DPM request's current evaluation, one per sample: the model value at plan op k and the update at k + 1.
        eps: the request's first row of the UNet output; nxt_row: its first row in the next call, None after its last evaluation"""
        nb = self.n * 4
        X, T = self._X.data_ptr(), self._T.data_ptr()
        plan, per = e.plan, (2 if e.guided else 1)
        k, u = e.pairs[e.cursor]
        dst, xs = int(plan.ops[k][2]), int(plan.ops[k][3])
        data = e.predict_x0 or int(plan.ops[k][1]) == 1
        x_eval = e.buf[xs]
        new = torch.empty_like(x_eval)
        if u is None:                    # the slot's result is the model value itself
            form, m_self, operands, m = -1, 0, [None] * 4, new
            e.buf[dst] = new
        else:
            form, udst = int(plan.ops[u][1]), int(plan.ops[u][2])
            names = [int(v) for v in plan.ops[u][3:]]
            m_self = sum(1 << j for j, v in enumerate(names[1:]) if v == dst)
            operands = [None if (v < 0 or v == dst) else e.buf[v] for v in names]
            m = torch.empty_like(x_eval) if (e.last_use.get(dst, -1) > u or e.img_callback) else None
            if e.last_use.get(dst, -1) > u:
                e.buf[dst] = m
            e.buf[udst] = new
        out = []
        for j in range(e.samples):
            off = j * nb
            at = lambda t: None if t is None else t.data_ptr() + off
            s = _lib.SamplerPlanSlot()
            s.kind, s.cfg, s.scale = 1, int(e.guided), e.scale
            s.eps_u = eps + per * j * nb
            s.eps_c = eps + (per * j + 1) * nb if e.guided else None
            s.x, s.data_prediction = (at(x_eval) if data else None), int(data)
            s.alpha_t, s.sigma_t = float(plan.coef[k][2]), float(plan.coef[k][3])
            s.form, s.m_self = form, m_self
            s.x_base, s.m0, s.m1, s.m2 = (at(t) for t in operands)
            if u is not None:
                s.c9 = (_lib.C.c_float * 9)(*[float(v) for v in plan.coef[u]])
            s.m_out, s.x_state_out = at(None if m is new else m), at(new)
            if nxt_row is not None:
                d = nxt_row + per * j
                s.t_next = e.evals[e.cursor + 1][0]
                s.unet_dst0, s.tf_dst0 = X + d * nb, T + d * 4
                if e.guided:
                    s.unet_dst1, s.tf_dst1 = X + (d + 1) * nb, T + (d + 1) * 4
            out.append(s)
        ops = (k,) if u is None else (k, u)
        freed = [slot for slot, last in e.last_use.items() if last in ops and slot in e.buf]
        after.append((e, m, e.evals[e.cursor][2], freed))
        return out

    # ---- one UNet evaluation of every active request ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self):
        """-> False if there was nothing to do"""
        entered = self._admit()
        q = self._q
        if not q.active:
            return False
        if entered or self._layout != self._row_starts(q.active):
            self._set_rows(entered)
        x_in, t_in, c_in = self._views
        if self.trace is not None:
            self.trace.append(q.call_rows())
        out = self.model.apply_model(x_in, t_in, c_in)           # rows at different timesteps: no timestep hint
        out = out.float().contiguous()
        if out.data_ptr() == self._X.data_ptr():                 # (the launch below writes the next call's rows)
            out = out.clone()
        self.calls += 1

        # the next call's rows: the requests that go on, closed up in admission order (whoever enters then comes after them)
        nxt, r0 = {}, 0
        for e in q.active:
            if e.cursor + 1 < len(e.evals):
                nxt[e.ticket] = r0
                r0 += e.rows
        n, nb = self.n, self.n * 4
        X, T, o = self._X.data_ptr(), self._T.data_ptr(), out.data_ptr()
        Slot, t_bytes = (_lib.SamplerPlanSlot, 4) if self._float else (_lib.SamplerSlot, 8)
        t_dst0, t_dst1 = ('tf_dst0', 'tf_dst1') if self._float else ('t_dst0', 't_dst1')
        slots, after, after_dpm, row = [], [], [], 0
        for e in q.active:
            if e.sampler == 'dpm':
                slots += self._dpm_slots(e, o + row * nb, None if e.cursor + 1 == len(e.evals) else nxt[e.ticket], after_dpm)
                row += e.rows
                continue
            t, mode, index, phase = e.evals[e.cursor]
            per = 2 if e.guided else 1
            predictor = e.sampler == 'plms' and mode == 0
            last = e.cursor + 1 == len(e.evals)
            log = (not predictor) and (index % e.log_every_t == 0 or index == e.total - 1)
            tab = e.tab
            sigma = float(tab['sigmas'][index])
            noise = None
            if e.eta != 0:               # ddim.py:200: one draw per step
                noise = self._noise_like(tuple(e.state.shape), e.state.device, e.generator, e.ticket).float().contiguous()
                if sigma == 0.0:
                    noise = None
            e.noise = noise              # (kept until the next step: the launch reads it)
            e_out = None
            if e.sampler == 'plms' and mode != 4:
                e_out = next(b for b in e.ring if all(b is not h for h in e.old))
            old = ([e.e_pred] if mode == 4 else e.old) + [None, None, None]
            new_state = torch.empty_like(e.state) if log else e.own        # a logged x_prev is a tensor of its own
            pred = torch.empty_like(e.state) if (log or (e.img_callback and not predictor)) else None
            for j in range(e.samples):
                s = Slot()               # (a plan slot of kind 0 has these fields under these names)
                off = j * nb
                s.eps_u = o + (row + per * j) * nb
                s.eps_c = o + (row + per * j + 1) * nb if e.guided else None
                s.cfg, s.scale, s.mode = int(e.guided), e.scale, mode
                s.x = e.state.data_ptr() + off
                s.old0, s.old1, s.old2 = (None if h is None else h.data_ptr() + off for h in old[:3])
                s.noise = None if noise is None else noise.data_ptr() + off
                s.a_t, s.a_prev = float(tab['alphas'][index]), float(tab['alphas_prev'][index])
                s.sigma, s.sqrt_1m_at = sigma, float(tab['sqrt_one_minus_alphas'][index])
                s.e_t_out = None if e_out is None else e_out.data_ptr() + off
                s.x_state_out = None if predictor else new_state.data_ptr() + off
                s.pred_x0 = None if pred is None else pred.data_ptr() + off
                if not last:
                    d = nxt[e.ticket] + per * j
                    s.t_next = e.evals[e.cursor + 1][0]                   # (an fp32 pool: float(int), exact below 2^24)
                    s.unet_dst0 = X + d * nb
                    setattr(s, t_dst0, T + d * t_bytes)
                    if e.guided:
                        s.unet_dst1 = X + (d + 1) * nb
                        setattr(s, t_dst1, T + (d + 1) * t_bytes)
                slots.append(s)
            after.append((e, predictor, mode, index, log, new_state, pred, e_out))
            row += e.rows
        stream = _lib.stream_ptr()
        launch = self._lib.sdmi_sampler_plan_rows if self._float else self._lib.sdmi_sampler_step_rows
        for k in range(0, len(slots), _lib.SAMPLER_MAX_SLOTS):
            chunk = slots[k:k + _lib.SAMPLER_MAX_SLOTS]
            arr = (Slot * len(chunk))(*chunk)
            _lib.check(launch(arr, len(chunk), n, stream))

        for (e, predictor, mode, index, log, new_state, pred, e_out) in after:
            if predictor:
                e.e_pred = e_out
                continue
            e.state = new_state
            if e.sampler == 'plms':      # plms.py:233-235: newest first, three kept
                e.old.insert(0, e.e_pred if mode == 4 else e_out)
                del e.old[3:]
            if e.img_callback:
                e.img_callback(pred, e.total - index - 1)
            if log:
                e.intermediates['x_inter'].append(e.state)
                e.intermediates['pred_x0'].append(pred)
        for (e, m, number, freed) in after_dpm:
            if e.img_callback:
                e.img_callback(m, number)
            for slot in freed:           # by last use, as DPMSolverHIP.run_plan frees them (the launch is queued on this stream)
                del e.buf[slot]
        for e in q.advance():
            self._results[e.ticket] = (e.buf[e.plan.result], None) if e.sampler == 'dpm' else (e.state, e.intermediates)
            e.ring = e.old = e.e_pred = e.noise = e.buf = None
        if not q.active:                 # idle: the next request finds no pinned K/V of rows that are gone
            self._layout = self._views = None
            unet = self._hip_unet()
            if unet is not None:
                unet.unpin_context()
        return True

    def run_until_idle(self):
        """step() until every submitted request is done; -> the number of UNet calls made"""
        n = 0
        while self.step():
            n += 1
        return n

    def pending(self):
        """requests submitted and not yet done"""
        return len(self._q.waiting) + len(self._q.active)

    def done(self, ticket):
        return ticket in self._results

    def result(self, ticket):
        """(samples, intermediates) of a finished request, as sample() returns them; the pool forgets the request"""
        if ticket not in self._results:
            raise KeyError(f'request {ticket!r} is not done (or its result was already taken)')
        return self._results.pop(ticket)
