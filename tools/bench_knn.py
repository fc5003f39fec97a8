"""Measure the exact k-NN search (SearcherHIP's kernels) on the MI355X: scan + merge + gather per call, the achieved database read rate,
and two comparisons in the same process on the same box:

  torch    torch.topk(q_hat @ db_hat.T, k) in fp32 on PyTorch-ROCm over a pre-normalised copy of the database (the obvious alternative)
  stream   a plain 16-byte read-only sweep of the same buffer (sdmi_k_knn_stream_read): the bandwidth ceiling of one pass

Device events around every call, `--calls` timed calls after `--warmup`; median and [min, max].  The database is generated on the device, so
nothing is uploaded inside the timed region.  Read rate = N D 4 bytes / time: the bytes one pass needs, whatever the kernel actually reads
(B > 16 takes one pass per 16 queries).

    python tools/bench_knn.py [--out profiles/knn_search.txt] [--rows 65536 1048576 4194304]
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stable_diffusion_amd import _lib  # noqa: E402


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def bench_text(a):
    """FrozenCLIPTextEmbedderHIP.encode_ids (tower + pooled, projected head) against FrozenCLIPEmbedderHIP.encode_ids (tower only) on the same
    ids, ViT-L/14 text shape, seeded random weights"""
    from stable_diffusion_amd import FrozenCLIPEmbedderHIP, FrozenCLIPTextEmbedderHIP
    from stable_diffusion_amd.clip import CLIP_VIT_L14_TEXT
    out = ['# text encoder, ViT-L/14 text shape (12 layers, W = 768, E = 768), L = 77; ms per call: median [min, max]',
           f'# {"precision":>9} {"B":>3} | {"tower only":>24} | {"tower + pooled head":>24} | {"head ms":>8}']
    print('\n'.join(out), flush=True)
    for precision in ('mixed', 'full'):
        torch.manual_seed(0)
        emb = FrozenCLIPTextEmbedderHIP(text_config=dict(CLIP_VIT_L14_TEXT, projection_dim=768), tokenizer=object(), hip_precision=precision)
        with torch.no_grad():
            for n_, p in emb.named_parameters():
                p.copy_(torch.randn_like(p) * (0.02 if p.dim() > 1 else 0.1) + (1.0 if 'norm' in n_ and n_.endswith('weight') else 0.0))
        tower = FrozenCLIPEmbedderHIP(text_config=CLIP_VIT_L14_TEXT, tokenizer=object(), hip_precision=precision)
        tower.load_state_dict({k: v for k, v in emb.state_dict().items() if 'text_projection' not in k})
        emb, tower = emb.cuda(), tower.cuda()
        for B in (1, 3):
            ids = torch.randint(1, 49000, (B, 77), device='cuda')
            ids[:, 40] = 49407
            t_t = timed(lambda: tower.encode_ids(ids), a.warmup, a.calls)
            t_e = timed(lambda: emb.encode_ids(ids), a.warmup, a.calls)
            line = (f'  {precision:>9} {B:>3} | {t_t[0]:8.3f} [{t_t[1]:6.3f}, {t_t[2]:6.3f}] | {t_e[0]:8.3f} [{t_e[1]:6.3f}, {t_e[2]:6.3f}] | '
                    f'{t_e[0] - t_t[0]:8.3f}')
            print(line, flush=True)
            out.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-text', action='store_true', help='skip the text-encoder timing')
    ap.add_argument('--rows', type=int, nargs='+', default=[1 << 16, 1 << 20, 1 << 22])
    ap.add_argument('--dim', type=int, default=768)
    ap.add_argument('--batch', type=int, nargs='+', default=[1, 3, 16, 64])
    ap.add_argument('--knn', type=int, nargs='+', default=[10, 64])
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_knn.py measures on the GPU; there is no CPU path'
    lib = _lib.load()
    dev, D = 'cuda', a.dim
    st = _lib.stream_ptr()
    lines = [f'# exact k-NN search, D = {D}, {torch.cuda.get_device_name(0)}; ms per call: median [min, max] of {a.calls} calls after {a.warmup} warm-up',
             '# search = scan + merge + gather (sdmi_knn_search); read rate = N D 4 bytes / search time; torch = topk(q_hat @ db_hat.T, k), fp32,',
             '# pre-normalised copy; stream = one plain 16-byte read-only sweep of the database (the ceiling of one pass)',
             f'# {"N":>8} {"B":>3} {"k":>3} | {"search ms":>24} {"TB/s":>6} {"of stream":>9} | {"torch ms":>24} {"torch/search":>12} | {"stream ms":>9} {"TB/s":>6}']
    print('\n'.join(lines), flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    sink = torch.zeros(4, dtype=torch.float32, device=dev)
    for N in a.rows:
        db = torch.empty((N, D), dtype=torch.float32, device=dev)
        for r0 in range(0, N, 1 << 18):
            n = min(1 << 18, N - r0)
            db[r0:r0 + n] = torch.randn((n, D), generator=g, device=dev) * (0.5 + 19.5 * torch.rand((n, 1), generator=g, device=dev))
        h = _lib.c_ptr()
        _lib.check(lib.sdmi_knn_create(D, N, C.byref(h)))
        _lib.check(lib.sdmi_knn_set_rows(h, 0, N, db.data_ptr(), st))
        _lib.check(lib.sdmi_knn_finalize(h, st))
        for r0 in range(0, N, 1 << 18):                    # the torch route's pre-normalised copy, in place of the raw one
            db[r0:r0 + (1 << 18)] = torch.nn.functional.normalize(db[r0:r0 + (1 << 18)], dim=1)
        nbytes = N * D * 4
        t_stream = timed(lambda: _lib.check(lib.sdmi_k_knn_stream_read(db.data_ptr(), N * D, sink.data_ptr(), st)), a.warmup, a.calls)
        for B in a.batch:
            q = torch.randn((B, D), generator=g, device=dev)
            qn = torch.nn.functional.normalize(q, dim=1)
            for k in a.knn:
                ws = torch.empty(int(lib.sdmi_knn_workspace_bytes(h, B, k)), dtype=torch.uint8, device=dev)
                idx = torch.empty((B, k), dtype=torch.int32, device=dev)
                sc = torch.empty((B, k), dtype=torch.float32, device=dev)
                nn = torch.empty((B, k, D), dtype=torch.float32, device=dev)
                t_s = timed(lambda: _lib.check(lib.sdmi_knn_search(h, q.data_ptr(), B, k, idx.data_ptr(), sc.data_ptr(), nn.data_ptr(),
                                                                   ws.data_ptr(), ws.numel(), st)), a.warmup, a.calls)
                t_t = timed(lambda: torch.topk(qn @ db.T, k), a.warmup, a.calls)
                ti = torch.topk(qn @ db.T, k).indices
                agree = float((ti == idx.long()).float().mean())          # (fp32 GEMM order differs: near-ties may swap)
                line = (f'  {N:>8} {B:>3} {k:>3} | {t_s[0]:8.3f} [{t_s[1]:6.3f}, {t_s[2]:6.3f}] {nbytes / t_s[0] / 1e9:6.2f} {t_stream[0] / t_s[0]:9.2f} | '
                        f'{t_t[0]:8.3f} [{t_t[1]:6.3f}, {t_t[2]:6.3f}] {t_t[0] / t_s[0]:12.2f} | {t_stream[0]:9.3f} {nbytes / t_stream[0] / 1e9:6.2f}'
                        f'   idx agreement with torch {agree:.4f}')
                print(line, flush=True)
                lines.append(line)
        lib.sdmi_knn_destroy(h)
        del db
        torch.cuda.empty_cache()
    if not a.no_text:
        lines += bench_text(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
