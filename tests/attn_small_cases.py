"""The cases of the one-pass attention kernel (csrc/attn_small.hip), shared by tests/test_attn_small_host.py (liveness, on the CPU, before a
GPU sees them) and tests/test_attn_small_gpu.py.  The smallest shapes at which that kernel can go wrong: both instantiated head dims; two
batches of two heads; 32 queries (one wave), 96 (a partly filled workgroup at four waves) and 40 (ragged inside a 32-query slice); and every
edge of the 32-key score blocks up to the kernel's limit of 256 keys, with nkv_pad = round_up(nkv, 8)."""
import attn_probes as A

FAMILY = 'small'
D = [80, 160]
B, HEADS = 2, 2
NQ = [32, 96, 40]
NKV = [1, 31, 32, 33, 64, 65, 77, 128, 129, 255, 256]
NKV_LIMIT = 256


def cases():
    return [(d, nq, nkv) for d in D for nq in NQ for nkv in NKV]


def seed(d, nq, nkv, regime):
    return A.case_seed(FAMILY, d, nq, nkv, regime)
