"""CPU: the exact k-NN search's host side -- the C ABI surface, the `.npz` database layouts, the refusals.

The entry points are additive: no struct or existing call changes, so SDMI_ABI_VERSION keeps the value every other host test pins; what
this file pins is that the header, the ctypes table and the cross-compiled library agree on the new names.  The argument refusals are
checked through the kernel-level entry points, which refuse before any HIP call, so they run without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from stable_diffusion_amd import _lib, retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN_SYMBOLS = ['sdmi_knn_create', 'sdmi_knn_destroy', 'sdmi_knn_set_rows', 'sdmi_knn_finalize', 'sdmi_knn_rows', 'sdmi_knn_dim',
               'sdmi_knn_workspace_bytes', 'sdmi_knn_search', 'sdmi_knn_condition', 'sdmi_k_knn_inv_norm', 'sdmi_k_knn_scan',
               'sdmi_k_knn_merge', 'sdmi_k_knn_gather', 'sdmi_k_knn_stream_read']


def test_entry_points_resolve_in_the_cross_compiled_library():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r' T (sdmi_[a-z0-9_]+)', nm))
    for name in KNN_SYMBOLS:
        assert name in _lib.exported_symbols() and name + '(' in hdr and name in exported and hasattr(lib, name), name
    assert f'#define SDMI_ABI_VERSION {lib.sdmi_abi_version()}' in hdr
    import stable_diffusion_amd
    assert 'SearcherHIP' in stable_diffusion_amd.__all__ and stable_diffusion_amd.SearcherHIP is retrieval.SearcherHIP


def _parts(rng, sizes, D):
    return [{'embedding': rng.standard_normal((n, D)).astype(np.float32), 'img_id': rng.integers(0, 1 << 40, n),
             'patch_coords': rng.integers(0, 256, (n, 4)).astype(np.int32)} for n in sizes]


def test_npz_single_file(tmp_path):
    (p,) = _parts(np.random.default_rng(0), [7], 8)
    np.savez_compressed(tmp_path / 'db.npz', **p)
    (got,) = retrieval.load_database(str(tmp_path))
    for k in retrieval.KEYS:
        assert got[k].dtype == p[k].dtype and np.array_equal(got[k], p[k]), k


def test_npz_multi_file_matches_the_reference_expression(tmp_path):
    parts = _parts(np.random.default_rng(1), [5, 1, 9], 8)
    for i, p in enumerate(parts):
        np.savez_compressed(tmp_path / f'part_{i:02d}.npz', **p)
    got = retrieval.load_database(str(tmp_path))
    # scripts/knn2img.py: Searcher.load_multi_files per loader process (one file each: n_proc = len(data)), then load_database's
    # expression over the gathered dicts -- the list per process is what gives its arrays their leading axis of 1
    data = [np.load(tmp_path / f'part_{i:02d}.npz') for i in range(3)]
    prefetched_data = []
    for d in data:
        out_data = {key: [] for key in retrieval.KEYS}
        for key in d.files:
            out_data[key].append(d[key])
        prefetched_data.append(out_data)
    ref = {key: np.concatenate([od[key] for od in prefetched_data], axis=1)[0] for key in retrieval.KEYS}
    for k in retrieval.KEYS:
        cat = np.concatenate([g[k] for g in got], axis=0)
        assert cat.dtype == ref[k].dtype and np.array_equal(cat, ref[k]), k


def test_npz_refusals(tmp_path):
    with pytest.raises(ValueError, match='No npz-files in specified path'):
        retrieval.load_database(str(tmp_path))
    np.savez(tmp_path / 'a.npz', embedding=np.zeros((3, 8), np.float32), img_id=np.zeros(3, np.int64))
    with pytest.raises(ValueError, match=r"lacks the key\(s\) \['patch_coords'\]"):
        retrieval.load_database(str(tmp_path))


def test_python_refusals_name_what_they_refuse():
    with pytest.raises(MemoryError, match=r'1000 rows x 768 needs 3076000 bytes of device memory, 4096 bytes are free'):
        retrieval.check_fits(1000, 768, 4096)
    retrieval.check_fits(1000, 768, 3076000)
    s = retrieval.SearcherHIP.__new__(retrieval.SearcherHIP)        # the argument checks need no device
    s.N, s.D = 12, 768
    with pytest.raises(ValueError, match='k = 13 exceeds the 12 rows of the database'):
        s._check(2, 768, 13)
    with pytest.raises(ValueError, match='query width D = 512 does not match the database width D = 768'):
        s._check(2, 512, 4)
    with pytest.raises(ValueError, match=r'k = 0 neighbours; 1 \.\. 64'):
        s._check(2, 768, 0)
    with pytest.raises(ValueError, match=r'B = 65 queries; 1 \.\. 64'):
        s._check(65, 768, 4)
    s._check(64, 768, 12)
    with pytest.raises(ValueError, match='multiple of 4'):
        retrieval.SearcherHIP({'embedding': np.ones((3, 6), np.float32), 'img_id': np.arange(3), 'patch_coords': np.zeros((3, 4))})
    with pytest.raises(ValueError, match="lacks the key"):
        retrieval.SearcherHIP({'embedding': np.ones((3, 8), np.float32)})


@pytest.mark.parametrize('N,D,B,k,msg', [
    (100, 64, 1, 0, 'k = 0 neighbours; 1 .. 64 are supported'),
    (100, 64, 1, 65, 'k = 65 neighbours; 1 .. 64 are supported'),
    (10, 64, 1, 11, 'k = 11 exceeds the 10 rows of the database'),
    (100, 64, 65, 4, 'B = 65 queries; 1 .. 64 are supported'),
    (100, 770, 1, 4, 'D = 770 must be a multiple of 4, at most 1024'),
    (100, 1028, 1, 4, 'D = 1028 must be a multiple of 4, at most 1024'),
])
def test_c_refusals_come_before_any_device_call(N, D, B, k, msg):
    lib = _lib.load()
    buf = (C.c_float * 64)()            # never dereferenced: the argument check returns first
    p = C.addressof(buf)
    assert lib.sdmi_k_knn_scan(p, p, N, D, p, B, k, 32, p, p, None) != 0
    assert msg in lib.sdmi_last_error().decode()
    assert lib.sdmi_k_knn_gather(p, p, N, D, p, B, k, None, p, D, None) != 0
    assert msg in lib.sdmi_last_error().decode()


def test_openai_text_state_dict_round_trips_bit_exact():
    """OpenAI-clip names <-> transformers' CLIPTextModelWithProjection names: in_proj split into q | k | v and joined again, text_projection
    ([W, E]) transposed both ways, nothing but the text half taken"""
    import torch
    from stable_diffusion_amd import vision
    W, E, I, V, L, layers = 16, 8, 32, 50, 12, 2
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
    oa = {'token_embedding.weight': r(V, W), 'positional_embedding': r(L, W), 'ln_final.weight': r(W), 'ln_final.bias': r(W),
          'text_projection': r(W, E), 'logit_scale': r(()), 'visual.proj': r(4, 4), 'visual.conv1.weight': r(4, 3, 2, 2)}
    for n in range(layers):
        p = f'transformer.resblocks.{n}.'
        oa.update({p + 'attn.in_proj_weight': r(3 * W, W), p + 'attn.in_proj_bias': r(3 * W), p + 'attn.out_proj.weight': r(W, W),
                   p + 'attn.out_proj.bias': r(W), p + 'ln_1.weight': r(W), p + 'ln_1.bias': r(W), p + 'ln_2.weight': r(W), p + 'ln_2.bias': r(W),
                   p + 'mlp.c_fc.weight': r(I, W), p + 'mlp.c_fc.bias': r(I), p + 'mlp.c_proj.weight': r(W, I), p + 'mlp.c_proj.bias': r(W)})
    tf = vision.openai_clip_text_to_transformers(oa)
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    want = CLIPTextModelWithProjection(CLIPTextConfig(vocab_size=V, hidden_size=W, intermediate_size=I, num_hidden_layers=layers,
                                                      num_attention_heads=2, max_position_embeddings=L, projection_dim=E)).state_dict()
    want = {k: v.shape for k, v in want.items() if not k.endswith('position_ids')}
    assert {k: v.shape for k, v in tf.items()} == want
    assert torch.equal(tf['text_projection.weight'], oa['text_projection'].t())
    assert torch.equal(tf['text_model.encoder.layers.1.self_attn.k_proj.weight'], oa['transformer.resblocks.1.attn.in_proj_weight'][W:2 * W])
    back = vision.transformers_to_openai_clip_text(tf)
    text_half = {k: v for k, v in oa.items() if not k.startswith('visual.') and k != 'logit_scale'}
    assert set(back) == set(text_half) and all(torch.equal(back[k], text_half[k]) for k in text_half)
    again = vision.openai_clip_text_to_transformers(back)
    assert set(again) == set(tf) and all(torch.equal(again[k], tf[k]) for k in tf)
    with pytest.raises(KeyError, match='unexpected OpenAI-clip key'):
        vision.openai_clip_text_to_transformers({'transformer.resblocks.0.attn.bogus': r(2)})


def test_text_embeds_entry_points_are_declared():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'sdmi.h')).read()
    for name in ('sdmi_clip_create_projection', 'sdmi_clip_projection_dim', 'sdmi_clip_text_embeds_workspace_bytes', 'sdmi_clip_text_embeds'):
        assert name in _lib.exported_symbols() and name + '(' in hdr and hasattr(lib, name), name
