"""The walk of tests/model_shapes.py against the recorded state_dict keys of the reference models (so that the launch geometries
tests/test_model_shapes_gpu.py runs are derived from the configs, not typed), and the self-checks of tests/guard.py.  No GPU."""
import json
import os

import pytest
import torch

import guard
import model_shapes as MS


@pytest.mark.parametrize('name', ['cin', 'inpaint'])
def test_walk_matches_the_recorded_state_dict(name):
    W, _ = MS.model_walk(name)
    with open(os.path.join(MS.GOLDEN, MS.MODELS[name][1])) as f:
        ref = {k: list(s) for k, s in json.load(f)['keys']}
    assert sorted(k for k in ref if k not in W) == [], 'keys the walk misses'
    assert sorted(k for k in W if k not in ref) == [], 'keys the walk invents'
    assert {k: (W[k], ref[k]) for k in W if W[k] != ref[k]} == {}, 'shapes that differ'
    assert len(W) == len(ref) == {'cin': 688, 'inpaint': 416}[name]


def test_walk_finds_the_shapes_the_kernel_suite_never_ran():
    cin = MS.distinct('cin')
    inp = MS.distinct('inpaint')
    gn_cin = {(d['c0'], d['c1']) for k, d in cin if k == 'gn'}
    gn_inp = {(d['c0'], d['c1']) for k, d in inp if k == 'gn'}
    assert {(384, 192), (576, 384), (960, 576), (192, 0), (576, 0)} <= gn_cin
    assert {(768, 512), (1024, 768), (1024, 1024), (256, 256)} <= gn_inp
    assert {(d['C'] // 32) for k, d in cin + inp if k == 'gn'} >= {6, 12, 18, 24, 30, 36, 48, 56, 64}
    # the longest K: the (1024 | 1024) -> 1024 3x3 conv of the inpainting UNet, K = 9 * 2048
    assert max(9 * (d['c0'] + d['c1']) for k, d in inp if k == 'conv3') == 18432
    # 3x3 convs at or above 25 GFLOP at batch 2 (tile 3 by the heuristic of launch_igemm)
    big = [d for k, d in inp if k == 'conv3' and 2.0 * 2 * d['hout'] ** 2 * d['N'] * 9 * (d['c0'] + d['c1']) >= 25e9]
    assert len(big) >= 18
    assert {(d['d'], d['heads'], d['nq'], d['nkv']) for k, d in cin if k == 'attn'} == {(384, 1, 1024, 1024), (384, 1, 1024, 1), (576, 1, 256, 256),
                                                                                        (576, 1, 256, 1), (960, 1, 64, 64), (960, 1, 64, 1)}
    assert {(d['d'], d['heads'], d['nq'], d['nkv']) for k, d in inp if k == 'attn'} == {(64, 8, 4096, 4096), (96, 8, 1024, 1024), (128, 8, 256, 256)}
    assert {d['K'] for k, d in cin if k == 'kv'} == {512} and {d['K'] for k, d in MS.distinct('laion') if k == 'kv'} == {1280}
    assert 60 <= len(cin) <= 120 and 60 <= len(inp) <= 120


def test_walk_statistics_targets():
    """what attach_gn_targets attaches: the next norm over the output alone, and the concat norm of the output block that pops it"""
    cin = MS.distinct('cin')
    # input_blocks.4 (384 at 32 x 32, behind an attention block): its proj_out feeds input_blocks.5's norm (cpg 12, cbase 0) and, as the second
    # source, the (384 | 384) concat norm of the output block that pops it (cpg 24, cbase 384)
    assert any(k == 'dense' and d['role'] == 'proj_out' and d['N'] == 384 and d['gn'] == [(12, 0), (24, 384)] for k, d in cin)
    # the (384 | 192) seam, cpg 18: cbase 384 is inside group 21
    assert any(d.get('gn') and (18, 384) in d['gn'] and d['N'] == 192 for k, d in cin)
    assert 384 % 18 != 0
    # conv_in emits its own statistics: input_blocks.1.0's norm and the (mc | mc) concat norm of the last output block, which is therefore
    # fused too -- the conv2 in front of it carries (2 mc / 32, 0), and no statistics-capable 3x3 conv is left without a consumer
    assert [d['gn'] for k, d in cin if k == 'conv_in'] == [[(6, 0), (12, 192)]]
    assert [d['gn'] for k, d in MS.distinct('inpaint') if k == 'conv_in'] == [[(8, 0), (16, 256)]]
    assert all(d['gn'] for k, d in cin + MS.distinct('inpaint') if k == 'conv3')
    for name in ('cin', 'inpaint', 'laion'):
        for k, d in MS.distinct(name):
            for cpg, cbase in d.get('gn', []):
                assert len(d['gn']) <= 2 and cpg >= 2 and (cbase + d['N'] + cpg - 1) // cpg <= 32


@pytest.mark.parametrize('name', ['sdv1', 'tiny'])
def test_walk_fold_sites_match_the_executors_plan(name, monkeypatch):
    """the walk's ResBlocks with a skip convolution are the executor's (sdmi_unet_skip_fold_plan: a dry pass, no GPU) in number and order,
    and the walk's fold decision -- not excluded, and the committed table's row is a halo-staged tile -- is the plan's entry for every one of
    them, at batch 2 and 64 x 64 latents, where 13 of SD v1's 14 fold"""
    import ctypes as C
    import oracle.plan
    from stable_diffusion_amd import UNetModelHIP
    for k in ('SDMI_SKIP_FOLD', 'SDMI_SKIP_FOLD_MAX_W', 'SDMI_IGEMM_TILE', 'SDMI_SPLITK', 'SDMI_TUNE_FILE'):
        monkeypatch.delenv(k, raising=False)
    h = UNetModelHIP(**getattr(oracle.plan, MS.MODELS[name][0].split(':')[1]).ref_kwargs())._handle
    buf = (C.c_int32 * 64)()
    n = h.lib.sdmi_unet_skip_fold_plan(h.h, 2, 64, 64, 77, buf, 64)
    assert n >= 0, h.lib.sdmi_last_error()
    plan = list(buf[:n])
    sites = [d for k, d in MS.model_walk(name, latent=64)[1] if k == 'conv2_tail']
    assert len(sites) == len(plan) == 14
    mine = [int(MS.folds(d, 2)) for d in sites]
    print(f'[walk vs plan {name}] plan {plan}, walk {mine}; sites ' + ', '.join(f'{d["hw"]}x{d["hw"]} {d["tail_c"]}x{d["passes"]}->{d["N"]}' for d in sites))
    assert mine == plan
    assert sites[-1]['excluded'] == 'p3' and all(not d['excluded'] for d in sites[:-1])
    if name == 'sdv1':
        assert plan == [1] * 13 + [0]
        # the three sites tests/test_skip_fold_shapes_gpu.py runs are sites of this walk
        assert {(d['hw'], d['N'], d['tail_c'], d['passes']) for d in sites} >= {(8, 1280, 2560, 1), (16, 1280, 2560, 1), (32, 640, 1920, 3)}
        # the pass count per site, in execution order (the table has no rows keyed by the tail's K, so the plan above cannot see it): the
        # stream 1x1 convs are three-pass split-fp16 on the two upper levels (ds 1, 2: 64 x 64, 32 x 32) and single-pass below (README.md,
        # DESIGN.md section 2 "Precision design"; csrc/unet.cpp Layer::p1x1) -- input_blocks.4 (32 x 32), .7 (16 x 16), output_blocks.0-2
        # (8 x 8), .3-5 (16 x 16), .6-8 (32 x 32), .9-11 (64 x 64)
        assert [(d['hw'], d['passes']) for d in sites] == [(32, 3), (16, 1)] + [(8, 1)] * 3 + [(16, 1)] * 3 + [(32, 3)] * 3 + [(64, 3)] * 3


def test_walk_up_sites_of_sdv1():
    """the Upsample convs of SD v1 and the concat norms they feed as the first source: what tests/test_up_phase_tiles_gpu.py takes its second
    statistics target from"""
    ups = [(d['c0'], d['hin'], d['gn']) for k, d in MS.distinct('sdv1', ('conv3',)) if d['role'] == 'up']
    assert ups == [(1280, 8, [(80, 0)]), (1280, 16, [(60, 0)]), (640, 32, [(30, 0)])]


@pytest.mark.parametrize('shape,dtype,ld', [((5, 24), torch.float16, 32), ((3, 7, 10), torch.float32, None), ((33,), torch.int64, None),
                                            ((300, 200), torch.float32, 264), ((2, 32, 8, 16), torch.int64, None)])
def test_guard_selfcheck(shape, dtype, ld):
    """one byte poked (with torch) into each guard and into one pitch gap must make `check` raise; writes inside the payload must not"""
    g = guard.guarded(shape, dtype, ld, device='cpu')
    assert g.guard >= 4096 and g.guard % 256 == 0 and (len(shape) == 1 or g.guard >= 256 * g.pitch)
    assert tuple(g.view.shape) == tuple(shape)
    if dtype.is_floating_point:
        assert torch.isnan(g.view).all()
    else:
        assert (g.view == -1).all()
    g.view.zero_()
    g.check('payload writes')
    pokes = [('front', g.guard - 1), ('front far', 0), ('back', g.guard + g.nbytes), ('back far', g.raw.numel() - 1)]
    if g.ld != g.cols:
        pokes.append(('gap', g.guard + 2 * g.pitch + g.cols * g.es))
        pokes.append(('last gap', g.guard + g.nbytes - 1))
    for what, off in pokes:
        g.raw[off] = 0
        with pytest.raises(AssertionError, match='outside the payload'):
            g.check(what)
        g.raw[off] = guard.FILL
        g.check(what)
    g.raw[g.guard - 3] = 7
    with pytest.raises(AssertionError, match=r'byte -3 \(row -1'):
        g.check('offset report')
