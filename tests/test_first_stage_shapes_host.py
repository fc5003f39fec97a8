"""The first-stage walk (tests/first_stage_shapes.py) against the recorded state_dict keys, and the CPU side of the bars that
tests/test_first_stage_shapes_gpu.py applies: the softmax and chain bars are derived from the number formats and checked here against a
plain-torch restatement of the chain's arithmetic; the peaked-attention decode case is shown, on an fp64 restatement of the decoder, to be
peaked and to move by many fp16-operand floors under each of three planted defects.  No GPU."""
import os

import pytest
import torch

import attn_probes as A
import first_stage_shapes as FS
from oracle import vae_ref

TINY = vae_ref.VAEConfig(ch=64, ch_mult=(1, 2), num_res_blocks=1)


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['vq_f4', 'vq_f4_noattn'])
def test_walk_keys_equal_the_recorded_vq_state_dict(name):
    W, dec, enc = FS.model_walk(name)
    ref = sorted((k, list(s)) for k, s in FS.recorded_keys(name))
    assert sorted((k, list(s)) for k, s in W.items()) == ref
    assert any(kind == 'softmax' for kind, _ in dec) == (name == 'vq_f4')


def test_walk_keys_equal_the_kl_f8_parameter_list():
    """oracle.vae_ref.vae_param_specs(SD_VAE) is what oracle/make_golden_vae.py loads strictly into the reference AutoencoderKL; the committed
    LAION config carries the same ddconfig"""
    W, _, _ = FS.model_walk('kl_f8')
    assert vae_ref.SD_VAE.ddconfig() == {k: v for k, v in FS.first_stage_params('kl_f8')['ddconfig'].items()}
    assert sorted((k, list(s)) for k, s in W.items()) == sorted((k, list(s)) for k, s, _ in vae_ref.vae_param_specs(vae_ref.SD_VAE))


def test_walk_reaches_the_tuned_product_geometries():
    """the (M, N, K) the tuning table is keyed by, at batch 1 on the 256^2 / 512^2 levels: 262144 x 128 x 1152, 65536 x 256 x 4608, and the
    chunked attention of a 64 x 64 latent"""
    convs = {(d['hout'] ** 2, d['N'], 9 * d['C']) for k, d in FS.distinct(kinds=('conv3',))}
    assert {(262144, 128, 1152), (65536, 256, 4608), (262144, 128, 2304), (16384, 512, 4608)} <= convs
    assert FS.chunks(4096) == [(0, 2048), (2048, 2048)] and FS.chunks(2304) == [(0, 2048), (2048, 256)] and FS.chunks(9216)[-1] == (8192, 1024)
    # ... and the committed table has rows for them (M N K ksize stride up mode splitk_req ...), so tile -1 takes a tuned dispatch there
    tune = os.path.join(os.path.dirname(FS.GOLDEN), os.pardir, 'stable-diffusion_amd', 'tune_gfx950.txt')
    with open(tune) as f:
        keys = {tuple(int(v) for v in ln.split()[:8]) for ln in f if ln.strip() and not ln.startswith('#')}
    assert {(262144, 128, 1152, 3, 1, 0, 0, 0), (65536, 256, 4608, 3, 1, 0, 0, 0), (16384, 512, 4608, 3, 1, 1, 0, 0),
            (2048, 4096, 512, 1, 1, 0, 0, 1), (2048, 512, 4096, 1, 1, 0, 0, 1)} <= keys
    roles = {d['role'] for k, d in FS.distinct(kinds=('dense',))}
    assert roles == {'q', 'k', 'vt', 'scores', 'pv', 'proj_out'}
    assert all(d['splitk'] == 1 for k, d in FS.distinct(kinds=('dense',)) if d['role'] != 'proj_out')


# ---- the chain's bar ------------------------------------------------------------------------------------------------------------------------
def _host_chain_cases():
    """every regime and coding the GPU module uses, at every chain shape with C = 128 and at the shapes up to 1088 with C = 512 (the CPU cost
    of the larger ones buys nothing: the arithmetic restated does not depend on the shape)"""
    return [pytest.param(C, ntok, ch, id=f'C{C}-ntok{ntok}') for C in FS.CHAIN_C for ntok, ch in FS.CHAIN_SHAPES if C == 128 or ntok <= 1088]


@pytest.mark.parametrize('C,ntok,chunk_list', _host_chain_cases())
def test_chain_restatement_stays_below_the_bar_and_cases_are_live(C, ntok, chunk_list):
    scale = C ** -0.5
    worst, worst_sm, least = 0.0, 0.0, 1.0
    for ri, regime in enumerate(A.REGIMES):
        q, k = A.make_qk(regime, 1, ntok, ntok, C, FS.chain_seed(C, ntok, ri))
        for r0, rows in chunk_list:
            qc = q[0, r0:r0 + rows]
            P, _ = A.softmax_ref(qc[None], k, scale)
            P = P[0]
            for name, col in A.codings(regime, ntok, C):
                v = A.dense_v(col, 1, C)[0]
                p16, out = FS.chain_restate(qc, k[0], v, torch.zeros(C), scale)
                sm = float(((p16.double() - P).abs() / FS.softmax_tol(P)).max())
                j = FS.chain_judge(out.double(), P, col, C)
                worst, worst_sm = max(worst, j['worst']), max(worst_sm, sm)
                assert sm <= 1.0, (regime, name, sm)
                assert j['worst'] <= 1.0 and j['zeros_exact'], (regime, name, j)
                if FS.must_be_live(name, ntok):
                    least = min(least, j['share'])
                    assert j['rows_live'] and j['share'] >= 0.10, (regime, name, j)
                else:
                    print(f'[chain restatement C{C} ntok{ntok} {regime}/{name}] single weights of a {ntok}-key softmax: live share '
                          f'{100 * j["share"]:.1f} % (not asserted: FS.must_be_live)', flush=True)
    print(f'[chain restatement C{C} ntok{ntok}] worst err / tol: chain {worst:.3f}, softmax alone {worst_sm:.3f}; smallest live share '
          f'{100 * least:.1f} %', flush=True)


def test_chain_bar_sees_a_flushed_weight_and_a_shifted_row():
    """the bar bites: weights below 5e-4 flushed to zero, and a chunk's rows shifted by one, are far outside it"""
    C, ntok = 128, 1088
    q, k = A.make_qk('diffuse', 1, ntok, ntok, C, FS.chain_seed(C, ntok, 0))
    P, _ = A.softmax_ref(q, k, C ** -0.5)
    P = P[0]
    name, col = A.codings('diffuse', ntok, C)[0]
    _, out = FS.chain_restate(q[0], k[0], A.dense_v(col, 1, C)[0], torch.zeros(C), C ** -0.5)
    assert FS.chain_judge(out.double(), P, col, C)['worst'] <= 1.0
    assert FS.chain_judge(out.double().roll(1, 0), P, col, C)['worst'] > 10.0
    flushed = torch.where(P < FS.FLUSH_BELOW, torch.zeros_like(P), P)
    assert FS.chain_judge(A.coded(flushed[None], col, C)[0], P, col, C)['worst'] > 10.0
    assert float(((flushed - P).abs() / FS.softmax_tol(P)).max()) > 10.0


# ---- the peaked-attention decode case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_peaked_decode_case_is_peaked_and_its_mutants_stand_out(seed):
    """the tiny first stage, batch 2, a 48 x 48 latent (2304 tokens: a chunk of 2048 rows and a tail of 256), q / k weights x 2 and the V bias
    x 25: conditions measured on the CPU over weight seeds 0, 1, 2 -- mean row maximum 0.34 .. 0.38 (21 .. 26 % of the rows above 0.5), fp16-operand
    floor 1.1e-3 .. 1.3e-3 on an image of |max| about 3; tail rows with their neighbour's weights 400 .. 580 floors, V bias dropped 80 .. 120,
    weights below 5e-4 flushed 7.7 .. 9.9"""
    sd = FS.peaked_state_dict(TINY, seed)
    z = vae_ref.make_vae_inputs(TINY, 2, 48, 48, seed=1)
    info = {}
    ref = FS.decode64(sd, TINY, z, info=info)
    floor = float((FS.decode64(sd, TINY, z, r16=True) - ref).abs().max())
    rm = info['rowmax']
    print(f'[peaked decode seed {seed}] |img| max {float(ref.abs().max()):.3f}, fp16-operand floor {floor:.3e}, mean row maximum '
          f'{float(rm.mean()):.3f}, rows above 0.5: {100 * float((rm > 0.5).double().mean()):.1f} %', flush=True)
    assert float(rm.mean()) >= 0.3
    assert 1.05e-3 <= floor < 1.35e-3          # (1.1e-3 .. 1.3e-3 to two digits)
    for m in FS.ATTN_MUTANTS:
        moved = float((FS.decode64(sd, TINY, z, mutant=m) - ref).abs().max()) / floor
        print(f'[peaked decode seed {seed}] mutant {m}: {moved:.1f} floors', flush=True)
        assert moved >= 5.0, (m, moved)


def test_decode64_is_the_oracle_decoder():
    sd = vae_ref.make_vae_state_dict(TINY, 0)
    z = vae_ref.make_vae_inputs(TINY, 2, 8, 8, seed=1)
    assert float((FS.decode64(sd, TINY, z).float() - vae_ref.vae_decode(sd, TINY, z)).abs().max()) < 1e-5
