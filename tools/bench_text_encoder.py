"""Time the text encoders in both precisions on one MI355X, and show what the encoder's precision does to a full-precision UNet.

    python tools/bench_text_encoder.py [--iters 20] [--rounds 7] [--eps] [--out profiles/...txt]

Encoders: FrozenCLIPEmbedderHIP with SD v1's text config and BERTEmbedderHIP with the LAION-400M config (1280 wide, 32 layers), seeded
random weights.  One timed call is what scripts/txt2img.py does per prompt batch: the (uc, c) pair, two encodes of [B, 77] token ids.
hip_precision='mixed' and 'full' live in one process and are timed alternately, `rounds` times `iters` pairs between two events; the
median round is reported with the spread.  There is no speed bar on the full mode: the numbers are reported, not promised.

--eps: a full-precision UNet is called twice on the same latent and timestep, once with the mixed encoder's context and once with the full
encoder's; the difference of the two eps predictions is what the mixed encoder's 3e-3 context error costs downstream.  UNet / encoder
pairs whose widths match: SD v1's UNet (context_dim 768) with SD's CLIP, and the 64-channel test UNet (context_dim 128) with the tiny
CLIP and the tiny BERT of the tests."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _time(fns, iters, rounds):
    """alternate the callables; (median, min, max) ms per call of each"""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    acc = [[] for _ in fns]
    for _ in range(rounds):
        for fn, a in zip(fns, acc):
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            a.append(e0.elapsed_time(e1) / iters)
    return [(statistics.median(a), min(a), max(a)) for a in acc]


def _clip_pair(cfg, seed, tok=None):
    from oracle import clip_ref
    from stable_diffusion_amd import FrozenCLIPEmbedderHIP
    tc = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
              num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads, max_position_embeddings=cfg.max_positions)
    sd = clip_ref.make_clip_state_dict(cfg, seed)
    out = {}
    for prec in ('mixed', 'full'):
        m = FrozenCLIPEmbedderHIP(text_config=tc, tokenizer=object(), hip_precision=prec)
        m.load_state_dict({'transformer.' + k: v for k, v in sd.items()}, strict=False)
        out[prec] = m.cuda()
    return out, lambda B, s: clip_ref.make_clip_ids(cfg, B, 77, seed=s).cuda()


def _bert_pair(cfg, seed):
    import bert_ref
    from stable_diffusion_amd import BERTEmbedderHIP
    sd = bert_ref.make_bert_state_dict(cfg, seed)
    out = {}
    for prec in ('mixed', 'full'):
        m = BERTEmbedderHIP(**cfg.embedder_kwargs(), use_tokenizer=False, hip_precision=prec)
        m.load_state_dict({'transformer.' + k: v for k, v in sd.items()}, strict=True)
        out[prec] = m.cuda()
    return out, lambda B, s: bert_ref.make_bert_ids(cfg, B, 77, seed=s).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--eps', action='store_true', help='also the eps difference of a full-precision UNet under the two contexts')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import bert_ref
    from oracle import clip_ref
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f'# {torch.cuda.get_device_name(0)}; median (min .. max) of {args.rounds} rounds x {args.iters} (uc, c) pairs, mixed and full '
        'alternating in one process')
    say('# encoder, two encodes of [B, 77]          mixed_ms                 full_ms                  full/mixed  max-abs(full - mixed)')
    for name, make, cfg in (('SD CLIP (768 wide, 12 layers)', _clip_pair, clip_ref.SD_CLIP),
                            ('LAION BERT (1280 wide, 32 layers)', _bert_pair, bert_ref.LAION_BERT)):
        models, ids_of = make(cfg, 0)
        for B in (1, 3):
            uc, c = ids_of(B, 1), ids_of(B, 2)
            fns = [lambda m=models[p]: (m.encode_ids(uc), m.encode_ids(c)) for p in ('mixed', 'full')]
            outs = [fn() for fn in fns]
            for fn in fns:
                fn()
            torch.cuda.synchronize()
            diff = max(float((a - b).abs().max()) for a, b in zip(*outs))
            (tm, m0, m1), (tf, f0, f1) = _time(fns, args.iters, args.rounds)
            say(f'{name + f", B = {B}":40s} {tm:7.3f} ({m0:.3f} .. {m1:.3f}) {tf:7.3f} ({f0:.3f} .. {f1:.3f}) {tf / tm:9.2f}  {diff:.2e}')
        del models
        torch.cuda.empty_cache()

    if args.eps:
        from oracle.plan import SD_V1, TINY
        from oracle.weights import make_inputs, make_state_dict
        from stable_diffusion_amd import UNetModelHIP
        say('# full-precision UNet, eps under the mixed encoder\'s context against eps under the full encoder\'s (same latent, same timesteps)')
        say('# UNet / encoder                         max|ctx diff|  max|eps diff|  rms eps diff   |eps|max')
        for uname, ucfg, hw, encs in (('test UNet (ctx 128)', TINY, 16, (('tiny CLIP', _clip_pair, clip_ref.TINY_CLIP),
                                                                          ('tiny BERT', _bert_pair, bert_ref.TINY_BERT))),
                                      ('SD v1 UNet (ctx 768)', SD_V1, 32, (('SD CLIP', _clip_pair, clip_ref.SD_CLIP),))):
            unet = UNetModelHIP(**ucfg.ref_kwargs(), hip_precision='full')
            unet.load_state_dict(make_state_dict(ucfg, 0), strict=True)
            unet = unet.cuda().eval()
            x, t, _ = make_inputs(ucfg, 2, hw, hw, seed=1)
            for ename, make, ecfg in encs:
                models, ids_of = make(ecfg, 0)
                ids = ids_of(2, 1)
                ctx = {p: models[p].encode_ids(ids) for p in ('mixed', 'full')}
                eps = {p: unet(x.cuda(), t.cuda(), context=ctx[p]).float().clone() for p in ('mixed', 'full')}
                torch.cuda.synchronize()
                d = eps['mixed'] - eps['full']
                say(f'{uname + " / " + ename:40s} {float((ctx["mixed"] - ctx["full"]).abs().max()):12.3e} {float(d.abs().max()):14.3e} '
                    f'{float(d.pow(2).mean().sqrt()):13.3e} {float(eps["full"].abs().max()):10.3f}')
                del models
            del unet
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
