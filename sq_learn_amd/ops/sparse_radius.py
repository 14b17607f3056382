"""Radius neighbours of CSR queries against a CSR fit set (SURVEY.md N24 /
K18, sparse half): for every query row the fit rows within ``thr``, as CSR
lists ascending by fit index - what DBSCAN's expansion consumes.

Device path: ``csrc/spradius.hip``.  The inner products are those of the
sparse k-NN kernel (``ops/sparse_knn.py``: cached transpose, tile pointer
table, one fixed-point exponent per query row, 64-bit integer LDS atomics),
so they are bit-identical from run to run and independent of the launch
geometry.  ``sp_radius_mark`` tests ``D <= thr`` in fp64 and writes one bit
per (query, fit row) pair plus one int32 count per (query, tile); one
``torch.cumsum`` over the counts gives every list's offset and the chunk's
total (the one host read of a chunk), the index buffer is allocated to that
total and ``sp_radius_fill`` expands the bits.  A GPU input always takes the
native path and raises when the extension is missing.  The torch twin (CPU)
works in fp64 over densified row chunks with the same epilogue
(``sparse_knn._distances``), the same inclusive test and the same self rule.
"""

import numpy as np
import torch

from . import _native as nat
from ._csr import TWIN_CHUNK, chunks, native_ok, sp_row_norms_torch
from .sparse_knn import TILE_MAX, _MAX_GRID, InvertedIndex, _distances, _metric_code
from ..utils.pairwise import get_chunk_n_rows

TILE_DEFAULT = 4096    # fit rows per workgroup; the fastest measured (profiles/sparse_dbscan.md)


def _tile(tile):
    tile = TILE_DEFAULT if tile is None else int(tile)
    if tile < 64 or tile > TILE_MAX or tile % 64:
        raise ValueError(f"tile must be a multiple of 64 between 64 and {TILE_MAX}, got {tile}")
    return tile


def _check(fit_sd, query_sd, thr, include_self):
    if fit_sd.shape[1] != query_sd.shape[1]:
        raise ValueError(f"the queries have {query_sd.shape[1]} columns, the fit set "
                         f"{fit_sd.shape[1]}")
    if fit_sd.device != query_sd.device:
        raise ValueError("the queries and the fit set must be on the same device")
    if include_self and query_sd is not fit_sd:
        raise ValueError("include_self=True is the self-join: the queries must be the fit set "
                         "itself")
    thr = float(thr)
    if thr != thr:
        raise ValueError("thr must not be NaN")
    return thr


def _result(ends, parts, m):
    indptr = np.zeros(m + 1, dtype=np.int64)
    if ends:
        indptr[1:] = np.concatenate(ends)
    indices = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return indptr, indices.astype(np.int64, copy=False)


class _Plan(InvertedIndex):
    """The inverted-index operands plus the mask geometry of the two kernels."""

    def __init__(self, fit_sd, query_sd, tile, xn=None, qn=None):
        super().__init__(fit_sd, query_sd, tile, xn, qn)
        self.words = -(-self.n // 64)

    def buffers(self, rows):
        dev = self.fit.device
        return (torch.empty((rows, self.words), dtype=torch.int64, device=dev),
                torch.empty((rows, self.ntiles), dtype=torch.int32, device=dev))

    def mark(self, a, b, thr, code, include_self, mask, cnt):
        """Query rows [a, b): one bit per pair into ``mask``, hits per
        (query, tile) into ``cnt``."""
        self.lib.sp_radius_mark(*self.args(a, b), code, thr, 1 if include_self else 0,
                                mask.data_ptr(), cnt.data_ptr(),
                                nat.stream_handle(self.fit.device))

    def fill(self, rows, mask, cs, total):
        """int32 [total]: the marked pairs of ``rows`` query rows as fit-row
        indices; ``cs`` is the cumulative sum of the flattened counts."""
        out = torch.empty(total, dtype=torch.int32, device=self.fit.device)
        self.lib.sp_radius_fill(mask.data_ptr(), cs.data_ptr(), rows, self.n, self.tile, total,
                                out.data_ptr(), nat.stream_handle(self.fit.device))
        return out


def sp_radius(fit_sd, query_sd, thr, metric="euclidean", include_self=False, tile=None, rows=None,
              xn=None, qn=None):
    """(indptr int64 [m + 1], indices int64 [total]) on the host: the fit
    rows ``j`` with ``D(q_i, x_j) <= thr`` of every query row ``i``, ascending.
    ``D`` is the squared distance for ``euclidean`` (``thr = eps ** 2``) and
    the distance itself for ``cosine``.  ``include_self``: the self-join
    (``query_sd is fit_sd``), in which row i lists itself whatever its
    computed distance.  ``tile``: fit rows per workgroup, a multiple of 64;
    ``rows``: query rows per launch (default: what keeps a chunk in which
    every pair is a neighbour within ``working_memory``); ``xn`` / ``qn``:
    precomputed squared row norms of the two sides."""
    code = _metric_code(metric)
    thr = _check(fit_sd, query_sd, thr, include_self)
    tile = _tile(tile)
    if not native_ok(fit_sd):
        return sp_radius_torch(fit_sd, query_sd, thr, metric, include_self, xn=xn, qn=qn)
    native_ok(query_sd)
    plan = _Plan(fit_sd, query_sd, tile, xn, qn)
    m = query_sd.shape[0]
    ntiles = plan.ntiles
    if rows is None:
        # worst case per query row: n int32 indices, the mask, the counts and
        # their int64 cumulative sum
        rows = get_chunk_n_rows(4 * plan.n + 8 * plan.words + 12 * ntiles)
    rows = max(1, min(int(rows), _MAX_GRID // ntiles))
    mask, cnt = plan.buffers(min(rows, m))
    ends, parts = [], []
    total = 0
    for a, b in chunks(m, rows):
        plan.mark(a, b, thr, code, include_self, mask, cnt)
        cs = torch.cumsum(cnt[:b - a].reshape(-1), 0, dtype=torch.int64)
        row_end = cs[ntiles - 1::ntiles].cpu().numpy()     # the host read of the chunk
        found = int(row_end[-1])
        ends.append(total + row_end)
        total += found
        if found:
            parts.append(plan.fill(b - a, mask, cs, found).cpu().numpy())
    return _result(ends, parts, m)


def sp_radius_torch(fit_sd, query_sd, thr, metric="euclidean", include_self=False, xn=None,
                    qn=None, chunk_rows=TWIN_CHUNK):
    """fp64 twin of :func:`sp_radius` over densified row chunks."""
    code = _metric_code(metric)
    thr = _check(fit_sd, query_sd, thr, include_self)
    n = fit_sd.shape[0]
    m = query_sd.shape[0]
    if xn is None:
        xn = sp_row_norms_torch(fit_sd)
    if qn is None:
        qn = xn if query_sd is fit_sd else sp_row_norms_torch(query_sd)
    xn, qn = xn.double(), qn.double()
    # one bool per pair of a query chunk
    q_rows = max(1, min(int(chunk_rows), get_chunk_n_rows(max(n, 1))))
    ends, parts = [], []
    total = 0
    for a, b in chunks(m, q_rows):
        Q = query_sd.dense_rows(a, b)
        hit = torch.empty((b - a, n), dtype=torch.bool, device=fit_sd.device)
        for s, e in chunks(n, chunk_rows):
            dot = Q @ fit_sd.dense_rows(s, e).T
            hit[:, s:e] = _distances(dot, qn[a:b], xn[s:e], code) <= thr
        if include_self:
            own = torch.arange(a, b, device=fit_sd.device)
            hit[own - a, own] = True
        r, c = torch.nonzero(hit, as_tuple=True)           # row-major: ascending per row
        counts = torch.bincount(r, minlength=b - a).cpu().numpy().astype(np.int64)
        ends.append(total + np.cumsum(counts))
        total += int(counts.sum())
        parts.append(c.cpu().numpy().astype(np.int64))
    return _result(ends, parts, m)
