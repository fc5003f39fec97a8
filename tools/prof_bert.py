"""Latency of the LAION-400M model's text encoder (BERTEmbedderHIP, 32 layers, dim 1280, 77 tokens) at B = 2 (the (uc, c)
pair of one image) and B = 8, and of one UNet call at context_dim 1280 against 768 (64 x 64 latent, B = 2), on HIP events,
with bench.py's box probe beside them.  Seeded random weights.  python tools/prof_bert.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from stable_diffusion_amd import BERTEmbedderHIP, UNetModelHIP  # noqa: E402
from stable_diffusion_amd.synthetic import (LAION_BERT_KWARGS, LAION_UNET_KWARGS, SD_V1_UNET_KWARGS, randomize_,  # noqa: E402
                                            synthetic_bert_state_dict)


def events_ms(fn, n=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(n):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    dev = torch.device('cuda')
    out = {}
    m = BERTEmbedderHIP(**LAION_BERT_KWARGS, use_tokenizer=False)
    m.load_state_dict(synthetic_bert_state_dict(**LAION_BERT_KWARGS, seed=0), strict=True)
    m = m.to(dev)
    g = torch.Generator().manual_seed(0)
    for B in (2, 8):
        ids = torch.randint(103, 30522, (B, 77), generator=g).to(dev)
        med, best = events_ms(lambda: m(ids))
        out[f'bert_b{B}_ms'] = round(med, 4)
        out[f'bert_b{B}_best_ms'] = round(best, 4)
        print(f'BERT encoder 32 x 1280, B = {B} x 77 tokens: median {med:.3f} ms (best {best:.3f})', flush=True)
    del m
    torch.cuda.empty_cache()
    x = torch.randn(2, 4, 64, 64, generator=g).to(dev)
    t = torch.tensor([981, 481], device=dev)
    for name, kw in (('ctx768', SD_V1_UNET_KWARGS), ('ctx1280', LAION_UNET_KWARGS)):
        u = UNetModelHIP(**kw).to(dev)
        randomize_(u, 0)
        ctx = torch.randn(2, 77, kw['context_dim'], generator=g).to(dev)
        med, best = events_ms(lambda: u(x, t, context=ctx))                 # cached context K/V after the first call, as in sampling
        out[f'unet_{name}_64x64_b2_ms'] = round(med, 4)
        print(f'UNet call, 64 x 64 latent, B = 2, context_dim {kw["context_dim"]}: median {med:.3f} ms (best {best:.3f})', flush=True)
        ctxs = [torch.randn(2, 77, kw['context_dim'], generator=g).to(dev) for _ in range(4)]
        it = iter(range(1 << 30))
        med2, _ = events_ms(lambda: u(x, t, context=ctxs[next(it) % 4]))     # a new context every call: K/V projected each time
        out[f'unet_{name}_64x64_b2_newctx_ms'] = round(med2, 4)
        print(f'  ... with a new context on every call: median {med2:.3f} ms', flush=True)
        del u
        torch.cuda.empty_cache()
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        out['box_probe'] = b.box_probe(dev)
    except Exception as e:      # noqa: BLE001
        out['box_probe_error'] = f'{type(e).__name__}: {e}'[:200]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
