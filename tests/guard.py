"""Guarded device buffers for the kernel-level tests: what a kernel touches outside its operands becomes visible.

One flat allocation per buffer, laid out as [front guard | rows at pitch ld >= cols | back guard].  Every guard byte and every
pitch-gap byte is 0xFF: all-ones is NaN as fp16 and as fp32 and -1 as int32 / int64, so the one fill is a poison for reads (a read
outside the contract that reaches a stored result makes it NaN and fails the value check) and a sentinel for writes (`check`).
A guard is max(4096, 256 * pitch_bytes) bytes -- one full row block of the tallest GEMM tile, BM = 256 -- rounded up to 256 bytes,
which keeps the 16-byte alignment the kernels check.  Every stray access this can see lands inside the test's own allocation: no
fault is provoked."""
import math

import torch

FILL = 0xFF


class Guarded:
    def __init__(self, shape, dtype, ld=None, device='cuda', row_bytes=None):
        shape = tuple(int(s) for s in shape)
        self.cols = shape[-1]
        self.rows = int(math.prod(shape[:-1]))
        self.ld = self.cols if ld is None else int(ld)
        assert self.ld >= self.cols
        self.es = torch.empty((), dtype=dtype).element_size()
        self.pitch = self.ld * self.es
        # (a flat buffer has no pitch: `row_bytes` names the row its kernels address it by, e.g. one slab row of a split-K workspace)
        row = row_bytes if row_bytes is not None else (self.pitch if len(shape) > 1 else self.es)
        self.guard = (max(4096, 256 * row) + 255) // 256 * 256
        self.nbytes = self.rows * self.pitch
        self.raw = torch.full((2 * self.guard + self.nbytes,), FILL, dtype=torch.uint8, device=device)
        assert not self.raw.is_cuda or self.raw.data_ptr() % 256 == 0
        body = self.raw[self.guard:self.guard + self.nbytes].view(dtype).view(self.rows, self.ld)
        self.view = body[:, :self.cols].unflatten(0, shape[:-1]) if len(shape) > 1 else body[:, :self.cols].reshape(shape)

    def data_ptr(self):
        return self.view.data_ptr()

    def check(self, name='buffer'):
        """every guard byte and every pitch-gap byte still 0xFF; reports the first few offending bytes"""
        g, n = self.guard, self.nbytes
        bad = []
        f = (self.raw[:g] != FILL).nonzero().flatten()
        if f.numel():
            bad += [int(i) - g for i in f[:4].cpu()]
        if self.ld != self.cols:
            gap = self.raw[g:g + n].view(self.rows, self.pitch)[:, self.cols * self.es:]
            w = (gap != FILL).nonzero()
            bad += [int(r) * self.pitch + self.cols * self.es + int(c) for r, c in w[:4].cpu()]
        b = (self.raw[g + n:] != FILL).nonzero().flatten()
        if b.numel():
            bad += [n + int(i) for i in b[:4].cpu()]
        if bad:
            where = ', '.join(f'byte {o:+d} (row {o // self.pitch}, col {(o % self.pitch) // self.es})' for o in bad)
            total = int(f.numel()) + int(b.numel()) + (int(w.shape[0]) if self.ld != self.cols else 0)
            raise AssertionError(f'{name}: {total} byte(s) outside the payload [{self.rows} x {self.cols}, pitch {self.ld}] were written; '
                                 f'offsets relative to the payload: {where}')


def guarded(shape, dtype, ld=None, device='cuda', row_bytes=None):
    return Guarded(shape, dtype, ld, device, row_bytes)


class Pool:
    """the guarded buffers of one test case: `put` copies a tensor in, `new` makes an output (left 0xFF = NaN, or filled), `check` checks all"""

    def __init__(self, device='cuda'):
        self.device = device
        self.bufs = []

    def new(self, name, shape, dtype, ld=None, fill=None, row_bytes=None):
        g = Guarded(shape, dtype, ld, self.device, row_bytes)
        if fill is not None:
            g.view.fill_(fill)
        self.bufs.append((name, g))
        return g.view

    def put(self, name, t, ld=None):
        v = self.new(name, t.shape, t.dtype, ld)
        v.copy_(t)
        return v

    def check(self, case=''):
        for name, g in self.bufs:
            g.check(f'{case} {name}'.strip())
