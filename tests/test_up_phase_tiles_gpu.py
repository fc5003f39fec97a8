"""The four 2x2 phase convs of an Upsample conv (igemm KIND_2X2, sdmi_k_igemm_up_phase) on every generic tile the kernel is instantiated for
and at every row of the committed phase table -- what tests/test_up_phase_gpu.py (tiles 5 and 7, M' <= 128, K' <= 512, one statistics target)
stops short of.  Operands, the launch in guarded buffers (guards, operands bit-unchanged; the derived weights live there too) and the
per-element bound are that module's (_operands, _run).

Forced tiles: each of the 18 generic tile ids (0 .. 13, 18 .. 21), unsplit, on three source geometries --
  B = 1, 16 x 16   M' = 256   one full 256-row tile, four full 64-row tiles per phase
  B = 3, 8 x 8     M' = 192   three / one and a half / under one M tile per phase, sample boundaries inside tiles
  B = 2, 5 x 4     M' = 40    ragged everywhere (no statistics: H W % 32 != 0)
at Cin = 320 (K' = 1280: 20 k-tiles, more than two wraps of the 8-stage ring) and N = 96, 320 (ragged at BN = 128 and 256; 320 is five
full tiles at BN = 64), and once at Cin = 64 (4 k-tiles: a ring shorter than its stage count on the 6- and 8-stage tiles).
Table rows: every data row of tune_up_phase_gfx950.txt.  Rows up to M' = 4608 run at their own (M', N, Cin) with tile = -1, after
sdmi_tune_lookup has shown that the row is found (or the heuristic would be what is tested); the larger first-stage rows run their (N, Cin)
with the row's tile forced on a 32 x 32 source (the tile index depends on the tile count, not on which rows a tile holds); the 262 144-row
originals stay under the first-stage goldens.

Bars: per element (K' + 1 + 4) 2^-24 (sum |a w'| + |bias|) against fp64 on the derived fp16 weights; the fp32-output bar _tol32(K') of
tests/test_model_shapes_gpu.py, max-abs; out_f16 == out.half() bit for bit; statistics (where H W % 32 == 0) for two targets per launch --
(N / 32, 0) and a concat norm of the real consumer (quads straddle groups; one at cbase != 0 whose last touched group is 31) -- at the bounds
of tests/test_up_phase_gpu.py, per group (tests/kernels.py gn_stats_ratio).

Measured on an MI355X: DESIGN.md section 2, "The phase and skip-tail convs at the product's tiles"."""
import ctypes as C
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernels as K  # noqa: E402  (tests/ is on sys.path via conftest's rootdir insertion)
import model_shapes as MS  # noqa: E402
import test_model_shapes_gpu as TMS  # noqa: E402
import test_up_phase_gpu as UP  # noqa: E402
from test_kernels_gpu import ALL_TILES  # noqa: E402

EPS32 = UP.EPS32
GEOMS = [(1, 16, 16), (3, 8, 8), (2, 5, 4)]
NS = (96, 320)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table_rows():
    """[(M', N, K', tile)] of the committed phase table"""
    rows = []
    with open(os.path.join(ROOT, 'stable-diffusion_amd', 'tune_up_phase_gfx950.txt')) as f:
        for ln in f:
            if ln.strip() and not ln.startswith('#'):
                v = ln.split()
                rows.append((int(v[0]), int(v[1]), int(v[2]), int(v[8])))
    return rows


def second_target(N):
    """the concat norm a real consumer attaches beside (N / 32, 0).  N = 320: the (320 | 160) norm, cpg 15 at cbase 0.  N = 96 (no product
    width): the second half of a (96 | 96) concat, cpg 6 at cbase 96 -- groups 16 .. 31.  N = 1280, 640, 512, 256: from the walks -- the
    Upsample conv of SD v1 feeds the (1280 | 1280) / (1280 | 640) / (640 | 320) concat norms as the FIRST source; the first stages' Upsample
    convs feed a plain norm only, so there the second target is this output as the second half of an (N | N) concat: cpg N / 16 at cbase N,
    groups 16 .. 31."""
    if N == 320:
        return (15, 0)
    if N == 96:
        return (6, 96)
    walked = sorted({t for kind, d in MS.distinct('sdv1', ('conv3',)) if d['role'] == 'up' and d['N'] == N for t in d['gn'] if t != (N // 32, 0)})
    return walked[-1] if walked else (N // 16, N)


def check_launch(tag, c, tile, splitk=1, targets=None):
    """one phase launch on the operands `c` against every bar of the module docstring (targets: the statistics targets, by default the two
    named there)"""
    B, H, W, N, Cin = c['B'], c['H'], c['W'], c['N'], c['Cin']
    Kp = 4 * Cin
    targets = [(N // 32, 0), second_target(N)] if targets is None else list(targets)
    if (H * W) % 32:            # (the launcher takes statistics targets only where a sample holds a multiple of 32 source pixels)
        targets = []
    stats = len(targets) > 0
    out, o16, accs, wph = UP._run(c, tile, True, phase=True, targets=targets, splitk=splitk)       # (the fp16 copy always, with or without targets)
    assert torch.equal(wph.view(torch.int16), c['wph'].view(torch.int16))
    finite = bool(torch.isfinite(out).all())
    err = (out.double() - c['ref']).abs()
    r = float((err / ((Kp + 1 + 4) * EPS32 * c['mag'])).max()) if finite else float('inf')
    e, tol = (float(err.max()) if finite else float('inf')), TMS._tol32(Kp)
    st = [K.gn_stats_ratio(out, B, 4 * H * W, acc, cpg, cbase) for acc, (cpg, cbase) in zip(accs, targets)] if stats else []
    print(f'[up phase tiles {tag} B{B} {H}x{W} Cin{Cin} N{N} tile{tile}] worst |err| / bound {r:.2e}, max-abs {e:.2e} (bar {tol:.1e}, ratio '
          f'{e / tol:.3f})' + (''.join(f'; statistics cpg{t[0]}@{t[1]} (sum, sumsq) / bound {a:.2e} {b:.2e}' for t, (a, b) in zip(targets, st))), flush=True)
    assert finite, f'{tag}: an output row was not written (or a guard value was read)'
    assert r <= 1.0 and e <= tol
    assert torch.equal(o16, out.half())
    for a, b in st:
        assert a <= 1.0 and b <= 1.0


@pytest.mark.parametrize('tile', ALL_TILES)
def test_phase_launch_on_every_generic_tile(tile):
    for B, H, W in GEOMS:
        for N in NS:
            check_launch('forced', UP._operands(B, H, W, 320, N), tile)
    check_launch('forced, short ring', UP._operands(3, 8, 8, 64, 96), tile)


def _geometry(Mp):
    """B = 2 and a square source where M' / 2 is a square, else B = 1 (M' a square there)"""
    s = math.isqrt(Mp // 2)
    if Mp % 2 == 0 and s * s == Mp // 2:
        return 2, s, s
    s = math.isqrt(Mp)
    assert s * s == Mp, Mp
    return 1, s, s


def test_the_phase_table_has_rows():
    rows = table_rows()
    assert len(rows) >= 1
    assert {6, 18, 21} <= {t for _, _, _, t in rows}


_SMALL = [r for r in table_rows() if r[0] <= 4608]
_LARGE = sorted({(N, Kp, tile) for Mp, N, Kp, tile in table_rows() if Mp > 4608})


@pytest.mark.parametrize('Mp,N,Kp,tile', _SMALL, ids=[f'M{r[0]}-N{r[1]}-K{r[2]}-t{r[3]}' for r in _SMALL])
def test_phase_table_row_as_launched(Mp, N, Kp, tile):
    from stable_diffusion_amd import _lib
    t, s = C.c_int(-1), C.c_int(-1)
    assert _lib.load().sdmi_tune_lookup(Mp, N, Kp, 2, 1, 1, 0, 0, 0, C.byref(t), C.byref(s)) == 0 and (t.value, s.value) == (tile, 1)
    B, H, W = _geometry(Mp)
    assert B * H * W == Mp
    check_launch(f'table row -> tile{tile}', UP._operands(B, H, W, Kp // 4, N), -1, splitk=0)


@pytest.mark.parametrize('N,Kp,tile', _LARGE, ids=[f'N{r[0]}-K{r[1]}-t{r[2]}' for r in _LARGE])
def test_first_stage_phase_table_row_reduced(N, Kp, tile):
    check_launch('first-stage row, 32x32 source', UP._operands(1, 32, 32, Kp // 4, N), tile)
