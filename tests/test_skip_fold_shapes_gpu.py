"""The 1x1 tail phase of conv2's halo-staged launch (conv3halo.hip TAIL, sdmi_k_igemm_tail) at what the product launches and
tests/test_skip_fold_gpu.py stops short of: 32- and 64-wide maps (interior tiles), the split-K counts 4, 5 and 10 of the committed tuning
table, tails of 30 .. 90 k-tiles, Cout = 1280 (10 / 20 N tiles).  The cases are tables in tests/skip_fold_cases.py; operands, the launch in
guarded buffers (guards, split-K counters zero again, operands bit-unchanged) and the per-element bound are those of
tests/test_skip_fold_gpu.py (_operands, _run, _ratio), with conv2's input channels as a parameter.

Bars, per launch:
  per element   |got - ref| <= (9 CA + Kt + S + 4) 2^-24 (sum_k |a_k w_k| + |bias|) against the fp64 sum over the same fp16 operands
  max-abs       the project's split-fp16 bar _tol_split(9 CA + Cin) of tests/test_model_shapes_gpu.py: 3e-5 sqrt(K / 1920), on exactly the operand
                scales it is stated for.  tests/test_skip_fold_shapes_host.py shows on the CPU that a launch which dropped the tail's lo w_hi pass, or
                the conv's last 64-channel chunk, misses this bar at least fourfold in every case here (the per-element bound alone, about 1e-2 at
                these sizes, would let the former pass)
  fp16 copy     bit for bit the fp16 rounding of the stored fp32 value
  statistics    two targets per launch, (Cout / 32, 0) and a concat norm whose channels per group are no multiple of 4 (quads straddle groups;
                cbase != 0 where the layout has one): tests/kernels.py gn_stats_ratio
  two launches  the skip GEMM into fp32 and conv2 with that residual, on the same tile and split, at the per-element bound

Measured on an MI355X: DESIGN.md section 2, "The phase and skip-tail convs at the product's tiles"."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import skip_fold_cases as SC  # noqa: E402  (tests/ is on sys.path via conftest's rootdir insertion)
import kernels as K  # noqa: E402
import test_model_shapes_gpu as TMS  # noqa: E402
import test_skip_fold_gpu as SF  # noqa: E402

# Cout -> the second statistics target (cpg, cbase), channels per group no multiple of 4: this output as the second source of a (128 | 64),
# (640 | 320) or (320 | 1280) concat -- cbase != 0, the last touched group is 31 -- or as the first source of (640 | 320), groups 0 .. 21
SECOND_TARGET = {64: (6, 128), 320: (30, 640), 640: (30, 0), 1280: (50, 320)}


def lookup(M, N, Kd, kt):
    """(rc, tile, split-K) of the committed tuning table for a stride-1 3x3 conv with a tail of kt"""
    from stable_diffusion_amd import _lib
    t, s = C.c_int(-1), C.c_int(-1)
    rc = _lib.load().sdmi_tune_lookup(M, N, Kd, 3, 1, 0, 0, 0, kt, C.byref(t), C.byref(s))
    return rc, t.value, s.value


def check_case(tag, c, tile, splitk, targets, two_launches=True):
    """one (tile, split-K) request on the operands `c`, folded (and as two launches), against every bar of the module docstring"""
    ca, Cout, Cin = c['CA'], c['Cout'], c['Cin']
    nsplit = splitk
    if tile < 0:            # as launched: the committed table must send this conv to a halo-staged tile, or the tail could not run
        rc, tt, nsplit = lookup(c['M'], Cout, 9 * ca, c['Kt'])
        assert rc == 0 and tt in SC.HALO_TILES, f'{tag}: the tuning table has no halo-staged row for this conv (rc {rc}, tile {tt})'
        tag += f' -> table tile{tt} split{nsplit}'
    tol = TMS._tol_split(9 * ca + Cin)
    assert tol == SC.tol_split(9 * ca + Cin)          # (the CPU control's copy of the bar is this bar)
    out, o16, accs = SF._run(c, tile, splitk, True, folded=True, targets=targets)
    r = SF._ratio(c, out, nsplit)
    finite = bool(torch.isfinite(out).all())
    e = float((out.double() - c['ref']).abs().max()) if finite else float('inf')
    st = [K.gn_stats_ratio(out, c['B'], c['H'] * c['W'], acc, cpg, cbase) for acc, (cpg, cbase) in zip(accs, targets)]
    r2 = float('nan')
    if two_launches:
        two, _, _ = SF._run(c, tile, splitk, False, folded=False)
        r2 = SF._ratio(c, two, nsplit)
    print(f'[skip fold shapes {tag}] folded: worst |err| / bound {r:.2e}, max-abs {e:.2e} (bar {tol:.2e}, ratio {e / tol:.2f}); two launches '
          f'|err| / bound {r2:.2e}; statistics (sum, sumsq) / bound ' + ', '.join(f'cpg{t[0]}@{t[1]}: {a:.2e} {b:.2e}' for t, (a, b) in zip(targets, st)),
          flush=True)
    assert finite, f'{tag}: an output element was not written (or a guard value was read)'
    assert r <= 1.0 and e <= tol
    assert torch.equal(o16, out.half())
    for a, b in st:
        assert a <= 1.0 and b <= 1.0
    if two_launches:
        assert r2 <= 1.0


def _id(s, ca, tile, co, ci, ps):
    return f'{s[0]}-ca{ca}-t{tile}-n{co}-c{ci}-p{ps}'


@pytest.mark.parametrize('shape,ca,tile,Cout,Cin,passes,splits', SC.WIDTHS + SC.SPLITS, ids=[_id(*k[:6]) for k in SC.WIDTHS + SC.SPLITS])
def test_tail_on_wide_maps_and_at_the_tables_splits(shape, ca, tile, Cout, Cin, passes, splits):
    c = SF._operands(shape, Cout, Cin, passes, ca=ca)
    targets = [(Cout // 32, 0), SECOND_TARGET[Cout]]
    for splitk in splits:
        check_case(f'{_id(shape, ca, tile, Cout, Cin, passes)} split{splitk} (tail k-tiles {c["Kt"] // 64})', c, tile, splitk, targets)


@pytest.mark.parametrize('shape,ca,Cout,Cin,passes,requests', SC.SITES, ids=[k[0][0] for k in SC.SITES])
def test_tail_at_the_sdv1_sites(shape, ca, Cout, Cin, passes, requests):
    c = SF._operands(shape, Cout, Cin, passes, ca=ca)
    targets = [(Cout // 32, 0), SECOND_TARGET[Cout]]
    for tile, splitk in requests:
        if tile >= 0:       # a forced request of this table is "the committed tuning table's choice": hold it to that
            assert lookup(c['M'], Cout, 9 * ca, c['Kt']) == (0, tile, splitk), 'the forced (tile, split-K) is no longer the table row of this site'
        check_case(f'{shape[0]} ca{ca} n{Cout} c{Cin} x{passes} tile{tile} split{splitk} (tail k-tiles {c["Kt"] // 64})', c, tile, splitk, targets)
