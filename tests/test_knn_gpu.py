"""The exact k-NN search (csrc/knn.hip) on the MI355X, against fp64 numpy / torch, every kernel operand and output in guarded buffers.

Database rows are unit directions scaled by random factors in [0.5, 20], so a missing inverse norm shows.  The index tests first assert, in
fp64 and on the CPU, that every adjacent gap among the scores they compare exceeds 4 D 2^-24 -- twice the bound the scores are then held to,
|score - fp64| <= 2 D 2^-24 (the worst-case fp32 dot product of unit vectors, doubled for the two normalisations) -- so the fp32 order is
determined and `idx` must EQUAL the stable fp64 argsort.  Slab sizes are forced through the kernel-level entry points: one slab, two slabs
and ten slabs, the last one ragged.  Shapes cover every scan variant: 1, 4, 8 and 16 queries per workgroup (B = 1, 3, 5 / 8, 17 / 64, the
last two in two and four chunks) and 1 to 4 column groups of 256 floats (D = 64 and 260 with clamped columns, 512, 768, 1024).

Measured on an MI355X: max |score - fp64| 3.6e-8 ... 2.2e-7 over the planted cases (bars 7.6e-6 at D = 64 ... 1.2e-4 at D = 1024); gathered rows
1.5e-7 ... 1.7e-7 relative (bars 2.1e-6 ... 2.3e-5)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
from stable_diffusion_amd import _lib, retrieval  # noqa: E402

DEV = 'cuda'
U = 2.0 ** -24


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def with_cosine(rng, q, c):
    """a unit vector at cosine c to the unit vector q (fp64)"""
    u = rng.standard_normal(q.shape)
    u = unit(u - (u @ q) * q)
    return c * q + np.sqrt(1.0 - c * c) * u


def ref_search(db, q, k):
    """fp64: scores [B, N], the stable argsort of -score, its first k columns"""
    s = unit(q.astype(np.float64)) @ unit(db.astype(np.float64)).T
    order = np.argsort(-s, axis=1, kind='stable')
    return s, order[:, :k]


def assert_gaps(s, order, upto, D, what):
    top = np.take_along_axis(s, order[:, :upto], axis=1)
    gaps = top[:, :-1] - top[:, 1:]
    if gaps.size:
        assert gaps.min() > 4 * D * U, f'{what}: the seed leaves a gap of {gaps.min():.3e} (<= {4 * D * U:.3e}) among the compared scores'


def run_search(db, q, k, slab_rows, case):
    """inv_norm, scan, merge through the kernel-level entry points in one guarded pool -> (idx, score, pool, device views)"""
    lib = _lib.load()
    N, D = db.shape
    B = q.shape[0]
    n_slabs = -(-N // slab_rows)
    P = guard.Pool(DEV)
    gdb, gq = P.put('db', torch.from_numpy(db)), P.put('queries', torch.from_numpy(q))
    inv = P.new('inv_norm', (N,), torch.float32)
    cs, ci = P.new('cand_score', (B, n_slabs, k), torch.float32), P.new('cand_idx', (B, n_slabs, k), torch.int32)
    idx, sc = P.new('idx', (B, k), torch.int32), P.new('score', (B, k), torch.float32)
    st = _lib.stream_ptr()
    _lib.check(lib.sdmi_k_knn_inv_norm(gdb.data_ptr(), N, D, inv.data_ptr(), st))
    _lib.check(lib.sdmi_k_knn_scan(gdb.data_ptr(), inv.data_ptr(), N, D, gq.data_ptr(), B, k, slab_rows, cs.data_ptr(), ci.data_ptr(), st))
    _lib.check(lib.sdmi_k_knn_merge(cs.data_ptr(), ci.data_ptr(), B, n_slabs, k, idx.data_ptr(), sc.data_ptr(), st))
    torch.cuda.synchronize()
    P.check(case)
    assert torch.equal(gdb.cpu(), torch.from_numpy(db)) and torch.equal(gq.cpu(), torch.from_numpy(q)), f'{case}: an input was written'
    return idx.cpu().numpy(), sc.cpu().numpy(), P, (gdb, inv, idx)


def planted_database(D, N, B, k, slab_rows, seed):
    """random background rows; per query min(k + 3, N) planted rows at cosines 0.90, 0.89, ..; the best-ranked planted rows sit at row 0, row
    N - 1, the last row of a slab, the first row of the next one and in the ragged tail; every row scaled by a factor in [0.5, 20]"""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, D)) * rng.uniform(0.1, 30.0, (B, 1))
    qn = unit(q)
    db = unit(rng.standard_normal((N, D)))
    n_pl = min(k + 3, N)
    assert B * n_pl <= N, 'the case must leave every query its own planted rows'
    last0 = (N - 1) // slab_rows * slab_rows                       # first row of the last (ragged) slab
    special = [0, N - 1, min(slab_rows, N) - 1, min(slab_rows, N - 1), last0, (last0 + N - 1) // 2, max(last0 - 1, 0)]
    special = list(dict.fromkeys(special))
    rest = [r for r in rng.permutation(N) if r not in set(special)]
    pool = (special + rest)[:B * n_pl]
    for j in range(n_pl):              # rank-major: the special rows become the best neighbours of the first queries
        for b in range(B):
            db[pool[j * B + b]] = with_cosine(rng, qn[b], 0.90 - 0.01 * j)
    db *= rng.uniform(0.5, 20.0, (N, 1))
    return db.astype(np.float32), q.astype(np.float32)


# D, N, B, k, slab_rows: 1 slab (slab_rows >= N), 2 slabs, 10 slabs (257 = 9 x 28 + 5, 4097 = 9 x 448 + 65)
PLANTED = [
    (64, 1, 1, 1, 32),
    (64, 10, 1, 10, 6),
    (64, 257, 17, 1, 160),
    (64, 4097, 64, 10, 448),
    (260, 257, 5, 10, 160),
    (512, 64, 1, 64, 64),
    (512, 257, 1, 10, 28),
    (512, 4097, 17, 64, 448),
    (768, 257, 3, 64, 300),
    (768, 4097, 3, 64, 448),
    (768, 4097, 64, 10, 2100),
    (768, 4097, 1, 1, 448),
    (1024, 257, 8, 10, 28),
]


@pytest.mark.parametrize('D,N,B,k,slab_rows', PLANTED)
def test_planted_neighbours_come_back_in_exact_order(D, N, B, k, slab_rows):
    db, q = planted_database(D, N, B, k, slab_rows, seed=1000 + D + N + 7 * B + k)
    s, order = ref_search(db, q, k)
    assert_gaps(s, np.argsort(-s, axis=1, kind='stable'), min(k + 1, N), D, 'planted')
    case = f'planted D={D} N={N} B={B} k={k} slab={slab_rows}'
    idx, sc, _, _ = run_search(db, q, k, slab_rows, case)
    assert np.array_equal(idx, order), f'{case}: first difference at {np.argwhere(idx != order)[:4].tolist()}'
    err = np.abs(sc.astype(np.float64) - np.take_along_axis(s, order, axis=1)).max()
    print(f'{case}: max |score - fp64| = {err:.3e} (bar {2 * D * U:.3e})')
    assert err <= 2 * D * U


@pytest.mark.parametrize('D,N,B,k,slab_rows', [(64, 64, 2, 64, 24), (64, 257, 2, 10, 28), (768, 40, 1, 40, 64)])
def test_all_scores_negative(D, N, B, k, slab_rows):
    """queries = -(the direction every row leans to): a top-k that starts from 0 instead of -inf returns nothing.  k = N: every row once."""
    rng = np.random.default_rng(50 + N + D)
    m = unit(rng.standard_normal(D))
    cos = 0.05 + (0.80 / N) * rng.permutation(N)                   # a ladder: adjacent gaps 0.8 / N >= 3e-3
    db = np.stack([with_cosine(rng, m, c) for c in cos]) * rng.uniform(0.5, 20.0, (N, 1))
    q = np.stack([-m * s for s in (1.0, 7.5)][:B])
    db, q = db.astype(np.float32), q.astype(np.float32)
    s, order = ref_search(db, q, k)
    assert s.max() < 0 and (0.8 / N) > 8 * D * U
    assert_gaps(s, np.argsort(-s, axis=1, kind='stable'), min(k + 1, N), D, 'negative')
    idx, sc, _, _ = run_search(db, q, k, slab_rows, f'negative N={N} k={k}')
    assert np.array_equal(idx, order)
    assert np.abs(sc.astype(np.float64) - np.take_along_axis(s, order, axis=1)).max() <= 2 * D * U
    if k == N:
        assert all(sorted(r) == list(range(N)) for r in idx.tolist())


def test_exact_duplicates_tie_bitwise_and_go_to_the_lower_index():
    """copies of one row, scaled by powers of two (exact in fp32, so the scores must be bit-equal), in different slabs and in the ragged tail"""
    D, N, B, k, slab_rows = 512, 257, 3, 10, 28
    db, q = planted_database(D, N, B, k, slab_rows, seed=77)
    rng = np.random.default_rng(78)
    dup = with_cosine(rng, unit(q[1].astype(np.float64)), 0.97).astype(np.float32)     # the best row of query 1, above its planted ladder
    rows = {253: 1.0, 5: 4.0, 55: 0.5, 56: 2.0, 130: 0.25, 255: 8.0}                # tail slab, slab 0, last row of 1, first row of 2, 4, tail
    planted = {int(r) for r in ref_search(db, q, k + 3)[1].ravel()}
    assert not planted & set(rows), 'the seed puts a planted row where a duplicate goes'
    for r, f in rows.items():
        db[r] = dup * np.float32(f)
    s, order = ref_search(db, q, k)
    idx, sc, _, _ = run_search(db, q, k, slab_rows, 'duplicates')
    assert idx[1, :6].tolist() == sorted(rows), idx[1]
    assert len(set(sc[1, :6].view(np.int32).tolist())) == 1, sc[1, :6]
    full = np.argsort(-s[1], kind='stable')
    assert np.array_equal(idx[1, 6:], full[~np.isin(full, list(rows))][:k - 6])
    assert np.array_equal(idx[[0, 2]], order[[0, 2]])


@pytest.mark.parametrize('k,pow2', [(10, False), (64, False), (64, True)])
def test_identical_rows_return_the_first_k(k, pow2):
    D, N, slab_rows = 64, 257, 28
    rng = np.random.default_rng(5)
    row = rng.standard_normal(D).astype(np.float32)
    db = np.tile(row, (N, 1))
    if pow2:
        db *= (2.0 ** rng.integers(-3, 4, (N, 1))).astype(np.float32)
    q = rng.standard_normal((2, D)).astype(np.float32)
    idx, sc, _, _ = run_search(db, q, k, slab_rows, f'identical k={k}')
    assert np.array_equal(idx, np.tile(np.arange(k), (2, 1)))
    assert (sc.view(np.int32) == sc.view(np.int32)[:, :1]).all()


@pytest.mark.parametrize('D,pad', [(64, 0), (260, 8), (768, 4)])
def test_gather_and_conditioning(D, pad):
    """nn rows vs fp64 within (D / 2 + 3) 2^-24 relative (an fp32 sum of D squares, a root, a division, a product); slot 0 of c bit-equal to
    the input; an output pitch > D leaves the gap untouched (the guard checks the gap bytes)"""
    lib = _lib.load()
    N, B, k = 300, 3, 10
    rng = np.random.default_rng(D)
    db = (unit(rng.standard_normal((N, D))) * rng.uniform(0.5, 20.0, (N, 1))).astype(np.float32)
    idx = np.stack([rng.permutation(N)[:k] for _ in range(B)]).astype(np.int32)
    idx[0, 0], idx[1, 1] = 0, N - 1
    c0 = rng.standard_normal((B, D)).astype(np.float32)
    ref = unit(db.astype(np.float64))[idx]
    st = _lib.stream_ptr()
    for with_c in (False, True):
        P = guard.Pool(DEV)
        gdb, gi = P.put('db', torch.from_numpy(db)), P.put('idx', torch.from_numpy(idx))
        inv = P.new('inv_norm', (N,), torch.float32)
        gc = P.put('c', torch.from_numpy(c0))
        out = P.new('out', (B, k + with_c, D), torch.float32, ld=D + pad)
        _lib.check(lib.sdmi_k_knn_inv_norm(gdb.data_ptr(), N, D, inv.data_ptr(), st))
        _lib.check(lib.sdmi_k_knn_gather(gdb.data_ptr(), inv.data_ptr(), N, D, gi.data_ptr(), B, k, gc.data_ptr() if with_c else None,
                                         out.data_ptr(), D + pad, st))
        torch.cuda.synchronize()
        P.check(f'gather D={D} c={with_c}')
        got = out.cpu().numpy()
        if with_c:
            assert np.array_equal(got[:, 0].view(np.int32), c0.view(np.int32))
        nn = got[:, int(with_c):].astype(np.float64)
        rel = (np.abs(nn - ref) / np.abs(ref)).max()
        print(f'gather D={D}: max relative error {rel:.3e} (bar {(D / 2 + 3) * U:.3e})')
        assert rel <= (D / 2 + 3) * U


def test_row_offsets_are_64_bit():
    """N D passes 2^31 floats: 1.4 M rows of 768 (4.3 GB, generated on the device); the neighbours are planted in the last 1000 rows"""
    lib = _lib.load()
    N, D, B, k = 1_400_000, 768, 3, 10
    free = torch.cuda.mem_get_info()[0]
    if free < 12 << 30:
        print(f'skipped: {free / 2 ** 30:.1f} GiB of device memory free, the case needs 12 GiB')
        pytest.skip(f'{free / 2 ** 30:.1f} GiB of device memory free, the case needs 12 GiB')
    g = torch.Generator(device=DEV).manual_seed(9)
    P = guard.Pool(DEV)
    db = P.new('db', (N, D), torch.float32)
    CH = 100_000
    for r0 in range(0, N, CH):
        n = min(CH, N - r0)
        db[r0:r0 + n] = torch.randn((n, D), generator=g, device=DEV) * (0.5 + 19.5 * torch.rand((n, 1), generator=g, device=DEV))
    rng = np.random.default_rng(10)
    q = rng.standard_normal((B, D))
    rows = rng.permutation(1000)[:B * (k + 3)] + (N - 1000)
    rows[0] = N - 1
    for j in range(k + 3):
        for b in range(B):
            v = with_cosine(rng, unit(q[b]), 0.90 - 0.01 * j) * rng.uniform(0.5, 20.0)
            db[int(rows[j * B + b])] = torch.from_numpy(v.astype(np.float32)).to(DEV)
    gq = P.put('queries', torch.from_numpy(q.astype(np.float32)))
    # fp64 on the device, chunked: per chunk the k best, then the k best of those (stable in the row index)
    qn = torch.nn.functional.normalize(gq.double(), dim=1)
    best_s, best_i = [], []
    for r0 in range(0, N, CH):
        x = db[r0:r0 + CH].double()
        s = qn @ (x / x.norm(dim=1, keepdim=True)).T
        ts, ti = torch.sort(s, dim=1, descending=True, stable=True)
        best_s.append(ts[:, :k + 1])
        best_i.append(ti[:, :k + 1] + r0)
    cat_s, cat_i = torch.cat(best_s, 1), torch.cat(best_i, 1)
    ts, tj = torch.sort(cat_s, dim=1, descending=True, stable=True)
    ref_s, ref_i = ts[:, :k + 1].cpu().numpy(), torch.gather(cat_i, 1, tj)[:, :k + 1].cpu().numpy()
    assert (ref_s[:, :-1] - ref_s[:, 1:]).min() > 4 * D * U and (ref_i[:, :k] >= N - 1000).all()
    slab_rows = 2752                                        # 509 slabs, the last one ragged
    n_slabs = -(-N // slab_rows)
    inv = P.new('inv_norm', (N,), torch.float32)
    cs, ci = P.new('cand_score', (B, n_slabs, k), torch.float32), P.new('cand_idx', (B, n_slabs, k), torch.int32)
    idx, sc = P.new('idx', (B, k), torch.int32), P.new('score', (B, k), torch.float32)
    st = _lib.stream_ptr()
    _lib.check(lib.sdmi_k_knn_inv_norm(db.data_ptr(), N, D, inv.data_ptr(), st))
    _lib.check(lib.sdmi_k_knn_scan(db.data_ptr(), inv.data_ptr(), N, D, gq.data_ptr(), B, k, slab_rows, cs.data_ptr(), ci.data_ptr(), st))
    _lib.check(lib.sdmi_k_knn_merge(cs.data_ptr(), ci.data_ptr(), B, n_slabs, k, idx.data_ptr(), sc.data_ptr(), st))
    nn = P.new('nn', (B, k, D), torch.float32)
    _lib.check(lib.sdmi_k_knn_gather(db.data_ptr(), inv.data_ptr(), N, D, idx.data_ptr(), B, k, None, nn.data_ptr(), D, st))
    torch.cuda.synchronize()
    P.check('64-bit offsets')
    assert np.array_equal(idx.cpu().numpy(), ref_i[:, :k])
    assert np.abs(sc.cpu().numpy().astype(np.float64) - ref_s[:, :k]).max() <= 2 * D * U
    x = db[torch.from_numpy(ref_i[:, :k].astype(np.int64)).to(DEV)].double()
    ref_nn = (x / x.norm(dim=-1, keepdim=True))
    assert ((nn.double() - ref_nn).abs() / ref_nn.abs()).max().item() <= (D / 2 + 3) * U


@pytest.mark.parametrize('form', ['tensor_b1d', 'array_bd'])
def test_searcher_matches_numpy_brute_force_key_by_key(form, tmp_path):
    D, B, k = 64, 3, 5
    rng = np.random.default_rng(3)
    sizes = [100, 1, 156]
    slab = 32
    db, q = planted_database(D, sum(sizes), B, k, slab, seed=4)
    img_id = rng.integers(0, 1 << 40, sum(sizes))
    pc = rng.integers(0, 256, (sum(sizes), 4)).astype(np.int32)
    r0 = 0
    for i, n in enumerate(sizes):           # a multi-file database directory, uploaded in chunks of 64 rows
        np.savez_compressed(tmp_path / f'part_{i}.npz', embedding=db[r0:r0 + n], img_id=img_id[r0:r0 + n], patch_coords=pc[r0:r0 + n])
        r0 += n
    s = retrieval.SearcherHIP(str(tmp_path), chunk_rows=64)
    x = torch.from_numpy(q)[:, None].to(DEV) if form == 'tensor_b1d' else q
    out = s(x, k)
    # the reference's search, restated on numpy with a brute-force argsort in place of scann
    qe = q / np.linalg.norm(q, axis=1)[:, np.newaxis]
    sc64, nns = ref_search(db, q, k)
    assert_gaps(sc64, np.argsort(-sc64, axis=1, kind='stable'), k + 1, D, 'searcher')
    emb = db[nns]
    ref = {'nn_embeddings': emb / np.linalg.norm(emb, axis=-1)[..., np.newaxis], 'img_ids': img_id[nns], 'patch_coords': pc[nns], 'queries': q,
           'nns': nns.astype(np.uint32), 'q_embeddings': qe}
    assert set(ref) | {'exec_time'} <= set(out)
    assert isinstance(out['exec_time'], float) and out['exec_time'] > 0
    for key, r in ref.items():
        assert out[key].shape == r.shape and out[key].dtype == r.dtype, (key, out[key].shape, out[key].dtype, r.shape, r.dtype)
    for key in ('img_ids', 'patch_coords', 'queries', 'nns', 'q_embeddings'):
        assert np.array_equal(out[key], ref[key]), key
    assert np.abs(out['nn_embeddings'] / ref['nn_embeddings'] - 1).max() <= (D / 2 + 3) * U
    # condition(): the sampler's context, slot 0 the query bit for bit, the rest the same neighbours
    c = torch.from_numpy(q)[:, None].to(DEV)
    ctx = s.condition(c, k)
    assert ctx.shape == (B, 1 + k, D) and ctx.dtype == torch.float32 and ctx.is_cuda
    assert torch.equal(ctx[:, :1], c)
    assert np.array_equal(ctx[:, 1:].cpu().numpy(), out['nn_embeddings'])
    with pytest.raises(ValueError, match='does not match the database width D = 64'):
        s(q[:, :32], k)
    small = retrieval.SearcherHIP({'embedding': db[:3], 'img_id': img_id[:3], 'patch_coords': pc[:3]})
    with pytest.raises(ValueError, match='k = 5 exceeds the 3 rows of the database'):
        small(q, k)
    assert small(q, 3)['nns'].shape == (B, 3)


@pytest.mark.parametrize('D,N,B,k', [(64, 4097, 17, 10), (768, 4097, 3, 64)])
def test_searcher_above_64_slabs_merges_in_two_stages(D, N, B, k):
    """the handle's own slab size (32 rows here: 129 slabs, ragged) and its two-stage merge, through SearcherHIP; chunked upload"""
    db, q = planted_database(D, N, B, k, 32, seed=500 + D)
    s64, order = ref_search(db, q, k)
    assert_gaps(s64, np.argsort(-s64, axis=1, kind='stable'), k + 1, D, 'two-stage')
    s = retrieval.SearcherHIP({'embedding': db, 'img_id': np.arange(N) * 3, 'patch_coords': np.zeros((N, 4), np.int32)}, chunk_rows=1000)
    out = s(q, k)
    assert np.array_equal(out['nns'], order.astype(np.uint32)) and np.array_equal(out['img_ids'], order * 3)
    assert np.abs(out['distances'].astype(np.float64) - np.take_along_axis(s64, order, axis=1)).max() <= 2 * D * U
    ctx, idx, score = s.condition(torch.from_numpy(q)[:, None].to(DEV), k, return_neighbours=True)
    assert np.array_equal(idx.cpu().numpy(), order) and np.array_equal(ctx[:, 1:].cpu().numpy(), out['nn_embeddings'])
    assert np.array_equal(score.cpu().numpy().view(np.int32), out['distances'].view(np.int32))


def test_finalize_names_the_first_bad_row():
    db = np.ones((50, 8), np.float32)
    db[31] = 0
    db[40, 3] = np.inf
    with pytest.raises(_lib.SdmiError, match='row 31 has a zero or non-finite norm'):
        retrieval.SearcherHIP({'embedding': db, 'img_id': np.arange(50), 'patch_coords': np.zeros((50, 4))})


@pytest.mark.parametrize('N,D,B,k,msg', [(100, 64, 1, 0, 'k = 0'), (100, 64, 1, 65, 'k = 65'), (10, 64, 1, 11, 'k = 11 exceeds the 10 rows'),
                                         (100, 64, 65, 4, 'B = 65'), (100, 770, 1, 4, 'D = 770')])
def test_argument_refusals_launch_nothing(N, D, B, k, msg):
    lib = _lib.load()
    kk, BB = max(1, min(k, 64)), min(B, 64)
    P = guard.Pool(DEV)
    db = P.new('db', (N, D), torch.float32, fill=1.0)
    q = P.new('q', (B, D), torch.float32, fill=1.0)
    inv = P.new('inv_norm', (N,), torch.float32, fill=1.0)
    outs = [P.new('cand_score', (B, 4, kk), torch.float32), P.new('cand_idx', (B, 4, kk), torch.int32), P.new('out', (B, kk, D), torch.float32)]
    st = _lib.stream_ptr()
    assert lib.sdmi_k_knn_scan(db.data_ptr(), inv.data_ptr(), N, D, q.data_ptr(), B, k, 32, outs[0].data_ptr(), outs[1].data_ptr(), st) != 0
    assert msg in lib.sdmi_last_error().decode()
    assert lib.sdmi_k_knn_gather(db.data_ptr(), inv.data_ptr(), N, D, outs[1].data_ptr(), B, k, None, outs[2].data_ptr(), D, st) != 0
    assert msg in lib.sdmi_last_error().decode()
    torch.cuda.synchronize()
    P.check('refusal')
    for o in outs:      # still the guard's 0xFF fill: nothing ran
        assert (o.contiguous().view(torch.uint8) == guard.FILL).all()
