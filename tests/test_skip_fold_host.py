"""Host logic of the ResBlock skip-convolution fold (the skip_connection as the 1x1 tail phase of conv2's halo-staged launch; DESIGN.md
section 4): how the tail's k-tiles are dealt over conv2's splits, how the tuning table is asked for a conv with a tail, and which ResBlocks
of the SD-v1 plan fold.  No GPU: arithmetic and dry passes only."""
import ctypes as C
import os

import pytest


def _lib():
    from stable_diffusion_amd import _lib
    return _lib, _lib.load()


@pytest.mark.parametrize('nkt', [0, 1, 2, 3, 5, 9, 30, 45, 90, 120])
@pytest.mark.parametrize('nsplit', [1, 2, 3, 4, 5, 6, 8, 10, 12, 16])
def test_tail_split_ranges_cover_every_k_tile_exactly_once(nkt, nsplit):
    """contiguous ranges in split order, every k-tile in exactly one, sizes within one of each other; more splits than k-tiles leaves
    empty ranges (those workgroups skip the phase)"""
    _, lib = _lib()
    seen = []
    prev_end = 0
    sizes = []
    for s in range(nsplit):
        b, e = C.c_int(-1), C.c_int(-1)
        assert lib.sdmi_k_tail_split_range(nkt, nsplit, s, C.byref(b), C.byref(e)) == 0
        assert b.value == prev_end and b.value <= e.value <= nkt
        prev_end = e.value
        seen += list(range(b.value, e.value))
        sizes.append(e.value - b.value)
    assert seen == list(range(nkt))
    assert max(sizes) - min(sizes) <= 1
    if nsplit > nkt:
        assert sizes.count(0) == nsplit - nkt
    assert lib.sdmi_k_tail_split_range(nkt, nsplit, nsplit, C.byref(C.c_int()), C.byref(C.c_int())) != 0


_TABLE = '''# test table
512 1280 11520 3 1 0 0 0 16 10 20.00
512 1280 11520 3 1 0 0 0 17 5 22.00 2560
2048 640 5760 3 1 0 0 0 14 1 30.00
8192 320 2880 3 1 0 0 0 15 1 41.00 1920
'''

_LOOKUPS = '''
import ctypes as C, sys
from stable_diffusion_amd import _lib
lib = _lib.load()
def look(M, N, K, kt):
    t, s = C.c_int(-1), C.c_int(-1)
    rc = lib.sdmi_tune_lookup(M, N, K, 3, 1, 0, 0, 0, kt, C.byref(t), C.byref(s))
    return (rc, t.value, s.value)
print(look(512, 1280, 11520, 0), look(512, 1280, 11520, 2560), look(512, 1280, 11520, 1920), look(2048, 640, 5760, 960),
      look(8192, 320, 2880, 1920), look(8192, 320, 2880, 0), look(8192, 320, 2880, 640))
'''


def test_table_key_falls_back_from_the_tail_key_to_the_plain_conv(tmp_path):
    """a conv with a tail takes the line that carries its Kt (the optional 12th column) where there is one, else the plain conv's line;
    a plain conv never takes a tail line; old 11-column lines keep parsing.  (Fresh process: the table is loaded once per process.)"""
    import subprocess
    import sys
    path = tmp_path / 'tune.txt'
    path.write_text(_TABLE)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SDMI_TUNE_FILE=str(path), PYTHONPATH=root)
    out = subprocess.run([sys.executable, '-c', _LOOKUPS], capture_output=True, text=True, env=env, cwd=root, check=True).stdout
    assert eval('[' + out.strip().replace(') (', '), (') + ']') == [
        (0, 16, 10),      # plain conv: its own line
        (0, 17, 5),       # tail Kt = 2560: the line keyed with it
        (0, 16, 10),      # another Kt: falls back to the plain line
        (0, 14, 1),       # only a plain line exists
        (0, 15, 1),       # only a tail line exists: the tail finds it ...
        (1, -1, -1),      # ... the plain conv does not
        (1, -1, -1),      # ... nor a tail of another Kt
    ]


def _sdv1_handle():
    from oracle.plan import SD_V1
    from stable_diffusion_amd import UNetModelHIP
    return UNetModelHIP(**SD_V1.ref_kwargs())._handle


def _plan(h, B, H, W, L=77):
    buf = (C.c_int32 * 64)()
    n = h.lib.sdmi_unet_skip_fold_plan(h.h, B, H, W, L, buf, 64)
    assert n >= 0, h.lib.sdmi_last_error()
    return list(buf[:n])


# The ResBlocks of SD v1 with a skip convolution, in execution order: input_blocks.4.0 (320 -> 640), input_blocks.7.0 (640 -> 1280), then the
# twelve output blocks (every one reads a skip concat).  The last of them (output_blocks.11.0) runs its 3x3 convs as three-pass split-fp16
# (Layer::precise3): those are no halo-staged launches, so it keeps its skip GEMM.
_SDV1_SITES = 14


def test_fold_predicate_per_block_of_the_sdv1_plan(monkeypatch):
    """which ResBlocks fold at the flagship shape (CFG batch 2, 64 x 64 latents), from the committed tuning table: every block with a skip
    convolution whose conv2 the table sends to a halo-staged tile, but for the split-fp16 last block; the knob and the width rule switch
    classes off; the full-precision handle never folds"""
    monkeypatch.delenv('SDMI_SKIP_FOLD', raising=False)
    monkeypatch.delenv('SDMI_SKIP_FOLD_MAX_W', raising=False)
    h = _sdv1_handle()
    plan = _plan(h, 2, 64, 64)
    assert len(plan) == _SDV1_SITES
    assert plan[-1] == 0                                   # output_blocks.11.0: precise3
    assert plan[:-1] == [1] * (_SDV1_SITES - 1), plan      # the table sends every other conv2 of this shape to a halo tile
    monkeypatch.setenv('SDMI_SKIP_FOLD', '0')
    assert _plan(h, 2, 64, 64) == [0] * _SDV1_SITES
    monkeypatch.setenv('SDMI_SKIP_FOLD', '1')
    monkeypatch.setenv('SDMI_SKIP_FOLD_MAX_W', '32')       # the width rule: the two foldable 64-wide blocks (output_blocks.9 / .10) drop out
    narrow = _plan(h, 2, 64, 64)
    assert narrow == [1] * 11 + [0, 0, 0], narrow
    monkeypatch.delenv('SDMI_SKIP_FOLD_MAX_W')
    from oracle.plan import SD_V1
    from stable_diffusion_amd import UNetModelHIP
    hf = UNetModelHIP(**SD_V1.ref_kwargs(), hip_precision='full')._handle
    assert _plan(hf, 2, 64, 64) == [0] * _SDV1_SITES
