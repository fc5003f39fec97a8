"""What tools/make_golden_sampler_pool.py (the reference run), tests/test_sampler_pool_host.py and tests/test_sampler_pool_gpu.py share: the
schedule, the stub model, the six requests and when each is submitted -- one definition, so that the three cannot drift apart.

The stub UNet is built only of individually rounded fp32 ops on one row (scalar multiplies, adds, clamp, t.float(), one element of the
row's context; no reduction, no transcendental), so CPU and GPU torch evaluate it identically and a row's value does not depend on its
neighbours in the call: a pool run equals the reference's one-request-at-a-time CPU runs bit for bit.

600 timesteps: every S below divides it, so make_ddim_timesteps stays inside the table (with 1000, S = 3 asks for t = 1000)."""
import numpy as np
import torch

TIMESTEPS = 600
LINEAR_START = 0.0015
SHAPE = (4, 8, 8)
TOKENS = (3, 5)                   # [tokens, width] of a context
MAX_ROWS = 8

# name -> submit() keywords (tensors come from `inputs`); in the order of submission
REQUESTS = {
    'ddim5': dict(S=5, sampler='ddim', samples=1, scale=7.5, log_every_t=2),
    'ddim8_eta': dict(S=8, sampler='ddim', samples=1, scale=5.0, eta=0.5, log_every_t=3),
    'plms3': dict(S=3, sampler='plms', samples=1, scale=1.0, log_every_t=1),
    'plms6': dict(S=6, sampler='plms', samples=1, scale=3.0, log_every_t=2),
    'pair': dict(S=4, sampler='ddim', samples=2, scale=1.0, log_every_t=1),
    'decode': dict(S=10, sampler='ddim', samples=1, scale=5.0, t_start=6, log_every_t=2),
}
# the number of UNet calls the pool has made when each is submitted: 'pair' finds 7 of 8 rows taken and waits, 'decode' waits behind it
ARRIVAL = {'ddim5': 0, 'ddim8_eta': 0, 'plms3': 0, 'plms6': 1, 'pair': 2, 'decode': 3}


def guided(name):
    return REQUESTS[name]['scale'] != 1.0


def plan_request(name):
    r = REQUESTS[name]
    return dict(ticket=name, S=r['S'], sampler=r['sampler'], samples=r['samples'], guided=guided(name), t_start=r.get('t_start'),
                arrival=ARRIVAL[name])


def stub_unet(x, t, c):
    h = 0.7 * x + 0.001 * t.float()[:, None, None, None]
    h = torch.clamp(h - 0.4, -1.5, 1.5) * 0.9
    return h + 0.1 * x + 0.25 * c[:, 0, 0][:, None, None, None]


def _normals(rs, shape):
    """approximately normal draws out of exactly rounded operations alone (as tests/ddpm_cases.py): the same bits on every machine"""
    u = rs.random_sample((12,) + tuple(shape))
    acc = u[0]
    for k in range(1, 12):
        acc = acc + u[k]
    return torch.from_numpy((acc - 6.0).astype(np.float32))


def n_draws(name):
    """noise_like calls of the reference run: one per step, two in the first PLMS step"""
    r = REQUESTS[name]
    steps = r.get('t_start') or r['S']
    return steps + (1 if r['sampler'] == 'plms' else 0)


def inputs(name):
    """x_T, c, uc, [draws] of a request, from its position in REQUESTS"""
    k = list(REQUESTS).index(name)
    rs = np.random.RandomState(4242 + k)
    b = REQUESTS[name]['samples']
    x_T = _normals(rs, (b,) + SHAPE)
    c = _normals(rs, (b,) + TOKENS)
    uc = _normals(rs, (b,) + TOKENS) * 0.5
    draws = [_normals(rs, (b,) + SHAPE) for _ in range(n_draws(name))]
    return x_T, c, uc, draws


class StubLD:
    """the samplers' view of a LatentDiffusion over the stub UNet, on `device`"""

    def __init__(self, G, device):
        self.num_timesteps = TIMESTEPS
        self.betas = torch.from_numpy(G['betas']).to(device)
        self.alphas_cumprod = torch.from_numpy(G['alphas_cumprod']).to(device)
        self.device = torch.device(device)
        self.calls = []

    def apply_model(self, x, t, c):
        self.calls.append(int(x.shape[0]))           # rows of the call
        return stub_unet(x, t, c)
