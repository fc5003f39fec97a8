"""UNet call time of each precision mode at the bench shape (SD v1, 64x64 latent, CFG batch 2, 77-token context), in one process.

    python tools/unet_precision_cost.py [mixed] [full]
    rocprofv3 --kernel-trace --stats -d OUT -o full -- python tools/unet_precision_cost.py full

5 warm-up calls, then 3 windows of 20 calls between device events; seeded random weights (oracle.weights)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.plan import SD_V1
from oracle.weights import make_inputs, make_state_dict
from stable_diffusion_amd import UNetModelHIP

modes = sys.argv[1:] or ['mixed', 'full']
sd = make_state_dict(SD_V1, 0)
x, t, ctx = make_inputs(SD_V1, 2, 64, 64, seed=1, ctx_len=77)
x, t, ctx = x.cuda(), t.cuda(), ctx.cuda()
for mode in modes:
    m = UNetModelHIP(**SD_V1.ref_kwargs(), hip_precision=mode)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    for _ in range(5):
        m(x, t, context=ctx)
    torch.cuda.synchronize()
    res = []
    for rep in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            m(x, t, context=ctx)
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / 20)
    print(f'UNET_CALL mode={mode} ms_per_call {" ".join(f"{r:.3f}" for r in res)} (64x64 latent, B=2, 20 calls x 3 windows, device events)', flush=True)
    del m
    torch.cuda.empty_cache()
