"""Retrieval conditioning: the `Searcher` of the reference's scripts/knn2img.py on the device.

    SearcherHIP  <- scripts/knn2img.py: Searcher (load_database, search, __call__)

The reference sends the query GPU -> numpy -> scann (score_brute_force, dot_product between unit vectors) -> numpy -> GPU.  Here the
database of raw CLIP patch embeddings lives in device memory once, with one inverse norm per row, and the search is the exact brute-force
maximum-cosine search of csrc/knn.hip: a database scan, a merge and a gather.  Results are ordered by descending score, ties go to the
lower row index (scann leaves the tie order unspecified).  No retriever network is loaded: the reference's `search` never uses it.
"""
import ctypes as C
import glob
import os
import time

import numpy as np
import torch

from . import _lib

KEYS = ('embedding', 'img_id', 'patch_coords')
MAX_K, MAX_B, MAX_D = 64, 64, 1024


def load_database(path):
    """The reference's `.npz` layout (keys embedding [n, D], img_id [n], patch_coords [n, ...]) from a directory: one file, or several
    files concatenated along the rows as `Searcher.load_database` does (it wraps each file's arrays in a list per loader process, which
    gives them a leading axis of 1, and concatenates along axis 1).  Files are taken in sorted order: the reference's glob order is the
    file system's.  Returns a list of per-file dicts of numpy arrays, so that the embeddings can be uploaded file by file without a
    concatenated host copy."""
    files = sorted(glob.glob(os.path.join(path, '*.npz')))
    if not files:
        raise ValueError(f'No npz-files in specified path "{path}" is this directory existing?')
    parts = []
    for f in files:
        with np.load(f) as z:
            missing = [k for k in KEYS if k not in z.files]
            if missing:
                raise ValueError(f'{f}: the retrieval database lacks the key(s) {missing} (it has {sorted(z.files)})')
            d = {k: z[k] for k in KEYS}
        parts.append(d)
    return parts


def free_device_memory(device):
    return int(torch.cuda.mem_get_info(device)[0])


def check_fits(N, D, free_bytes):
    """the raw rows plus one inverse norm per row must fit in the free device memory: there is no sharded or host-resident search"""
    need = N * (D + 1) * 4
    if need > free_bytes:
        raise MemoryError(f'retrieval database of {N} rows x {D} needs {need} bytes of device memory, {free_bytes} bytes are free')


class SearcherHIP(object):
    """`Searcher(database)` of knn2img.py.  `database` is a directory of `.npz` files (see load_database) or an in-memory dict with the
    keys embedding [N, D], img_id [N], patch_coords [N, ...].  A scann searcher directory (data/rdm/searchers/...) is ignored: the search
    is always the exact one, which is what a `score_brute_force` searcher computes.  The embeddings are uploaded raw, in chunks of
    `chunk_rows`; `search` / `__call__` return the reference's dict of numpy arrays, `condition` the sampler's device tensor."""

    def __init__(self, database, device='cuda', chunk_rows=1 << 18):
        if isinstance(database, dict):
            missing = [k for k in KEYS if k not in database]
            if missing:
                raise ValueError(f'the retrieval database lacks the key(s) {missing}')
            parts = [{k: np.asarray(database[k]) for k in KEYS}]
        else:
            parts = load_database(database)
        for p in parts:
            e = p['embedding']
            if e.ndim != 2 or e.shape[0] != p['img_id'].shape[0] or e.shape[0] != p['patch_coords'].shape[0]:
                raise ValueError(f'retrieval database: embedding {e.shape}, img_id {p["img_id"].shape}, patch_coords '
                                 f'{p["patch_coords"].shape} do not describe the same rows')
        D = int(parts[0]['embedding'].shape[1])
        if any(int(p['embedding'].shape[1]) != D for p in parts):
            raise ValueError('retrieval database: the files disagree on the embedding width '
                             f'({sorted({int(p["embedding"].shape[1]) for p in parts})})')
        N = sum(int(p['embedding'].shape[0]) for p in parts)
        if N < 1:
            raise ValueError('retrieval database: no rows')
        if D % 4 or D > MAX_D:
            raise ValueError(f'retrieval database: embedding width D = {D} must be a multiple of 4, at most {MAX_D}')
        self.N, self.D = N, D
        self.device = torch.device(device)
        self.img_id = np.concatenate([p['img_id'] for p in parts], axis=0)
        self.patch_coords = np.concatenate([p['patch_coords'] for p in parts], axis=0)
        self._check_memory(N, D)
        self.lib = _lib.load()
        self.h = _lib.c_ptr()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sdmi_knn_create(D, N, C.byref(self.h)))
            first = 0
            for p in parts:
                e = p['embedding']
                for r0 in range(0, e.shape[0], chunk_rows):
                    chunk = np.ascontiguousarray(e[r0:r0 + chunk_rows], dtype=np.float32)
                    _lib.check(self.lib.sdmi_knn_set_rows(self.h, first, chunk.shape[0], chunk.ctypes.data, _lib.stream_ptr()))
                    torch.cuda.current_stream().synchronize()       # (the chunk is pageable host memory that dies with this iteration)
                    first += chunk.shape[0]
            _lib.check(self.lib.sdmi_knn_finalize(self.h, _lib.stream_ptr()))
        self._ws = None

    def _check_memory(self, N, D):
        check_fits(N, D, free_device_memory(self.device))

    def __del__(self):
        h = getattr(self, 'h', None)
        if h is not None and h.value:
            self.lib.sdmi_knn_destroy(h)
            self.h = None

    def _check(self, B, D, k):
        if D != self.D:
            raise ValueError(f'query width D = {D} does not match the database width D = {self.D}')
        if not 1 <= k <= MAX_K:
            raise ValueError(f'k = {k} neighbours; 1 .. {MAX_K} are supported')
        if k > self.N:
            raise ValueError(f'k = {k} exceeds the {self.N} rows of the database')
        if not 1 <= B <= MAX_B:
            raise ValueError(f'B = {B} queries; 1 .. {MAX_B} are supported')

    def _workspace(self, B, k):
        need = int(self.lib.sdmi_knn_workspace_bytes(self.h, B, k))
        if need <= 0:
            _lib.check(-1)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _run(self, q, k, c_out):
        """q fp32 [B, D] on the device -> (idx int32 [B, k], score [B, k], nn [B, k, D] or c_out filled)"""
        B = q.shape[0]
        idx = torch.empty((B, k), dtype=torch.int32, device=self.device)
        score = torch.empty((B, k), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ws = self._workspace(B, k)
            if c_out is None:
                nn = torch.empty((B, k, self.D), dtype=torch.float32, device=self.device)
                _lib.check(self.lib.sdmi_knn_search(self.h, q.data_ptr(), B, k, idx.data_ptr(), score.data_ptr(), nn.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), _lib.stream_ptr()))
            else:
                nn = c_out
                _lib.check(self.lib.sdmi_knn_condition(self.h, q.data_ptr(), B, k, c_out.data_ptr(), idx.data_ptr(), score.data_ptr(),
                                                       ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return idx, score, nn

    def search(self, x, k):
        """x: tensor or array [B, D] or [B, 1, D].  Returns the reference's dict: nn_embeddings [B, k, D] (normalised), img_ids, patch_coords,
        queries (x as given, [B, D]), exec_time, nns (uint32 [B, k], as scann returns them), q_embeddings [B, D]; plus `distances`, the
        cosines the reference's search_batched returns and drops."""
        if isinstance(x, torch.Tensor):
            xt = x.detach()
        else:
            xt = torch.from_numpy(np.asarray(x))
        if xt.dim() == 3:
            xt = xt[:, 0]
        if xt.dim() != 2:
            raise ValueError(f'queries must be [B, D] or [B, 1, D], got {tuple(x.shape)}')
        self._check(int(xt.shape[0]), int(xt.shape[1]), int(k))
        x_np = xt.cpu().numpy()
        q = xt.to(device=self.device, dtype=torch.float32).contiguous()
        start = time.time()
        idx, score, nn = self._run(q, int(k), None)
        nns = idx.cpu().numpy().astype(np.uint32)        # (the copy synchronises)
        end = time.time()
        return {'nn_embeddings': nn.cpu().numpy(),
                'img_ids': self.img_id[nns],
                'patch_coords': self.patch_coords[nns],
                'queries': x_np,
                'exec_time': end - start,
                'nns': nns,
                'q_embeddings': x_np / np.linalg.norm(x_np, axis=1)[:, np.newaxis],
                'distances': score.cpu().numpy()}

    def __call__(self, x, n):
        return self.search(x, n)

    def condition(self, c, k, return_neighbours=False):
        """c: device tensor [B, 1, D] (FrozenCLIPTextEmbedder.encode's output with n_repeat = 1) -> [B, 1 + k, D], slot 0 = c bit for bit,
        slots 1 .. k the normalised neighbours: knn2img.py's `torch.cat([c, nn_embeddings], dim=1)` with no host round trip."""
        if c.dim() != 3 or c.shape[1] != 1:
            raise ValueError(f'c must be [B, 1, D], got {tuple(c.shape)}')
        B, _, D = c.shape
        self._check(int(B), int(D), int(k))
        q = c.detach().to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty((B, 1 + int(k), D), dtype=torch.float32, device=self.device)
        idx, score, _ = self._run(q.view(B, D), int(k), out)
        return (out, idx, score) if return_neighbours else out
