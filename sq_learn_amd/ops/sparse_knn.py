"""Brute-force k-NN of CSR queries against a CSR fit set (SURVEY.md S11 /
K18, sparse half): squared euclidean or cosine distances and the ``kk``
nearest fit rows of every query, ordered by (distance, fit index).

Device path: ``csrc/spknn.hip`` - one workgroup per (query row, tile of
``tile`` fit rows).  The fit set is read through its cached transpose
(``_csr.csr_transpose``) and a tile pointer table built once per
fit set (:func:`tile_table`), so a query nonzero in column c touches only the
stored values of column c: the work is ``sum_c nnz_q(c) * nnz_x(c)``.  Inner
products are accumulated as 64-bit integer quanta of ``2^e_i`` (one exponent
per query row, :func:`query_exps`) with integer LDS atomics: no
floating-point atomics, results bit-identical from run to run and
independent of the launch geometry.  ``kk <= 32`` selects in the kernel;
larger ``kk`` writes a dense distance block and selects with ``torch.topk``.
A GPU input always takes the native path and raises when the extension is
missing.  The torch twin (CPU) works in fp64 over densified row chunks with
the same epilogue formulae and a stable sort on (distance, index).
"""

import torch

from . import _native as nat
from ._csr import (TWIN_CHUNK, chunks, csr_ptrs, csr_transpose, native_ok, sp_row_norms,
                   sp_row_norms_torch)
from ..utils.pairwise import get_chunk_n_rows

TILE_MAX = 8192        # 64 KiB of LDS accumulators: two workgroups per CU (csrc/spknn.hip)
TILE_DEFAULT = 8192    # fit rows per workgroup; the fastest measured (profiles/sparse_knn.md)
KMAX = 32              # in-kernel selection; above: dist mode + topk
METRICS = {"euclidean": 0, "cosine": 1}
_MAX_GRID = 2 ** 31 - 1


def _metric_code(metric):
    if metric not in METRICS:
        raise ValueError(f"sparse k-NN supports the metrics 'euclidean' and 'cosine', got "
                         f"{metric!r}")
    return METRICS[metric]


def _tile(tile):
    tile = TILE_DEFAULT if tile is None else int(tile)
    if tile < 1 or tile > TILE_MAX:
        raise ValueError(f"tile must be between 1 and {TILE_MAX}, got {tile}")
    return tile


# ------------------------------------------------------------- tile table
def tile_table_bytes(sd, tile=None):
    """Device bytes :func:`tile_table` needs beyond the matrix itself: the
    transpose (when not yet cached), the int64 key of every stored value and
    the table with the ``arange`` it is searched against."""
    tile = _tile(tile)
    n, d = sd.shape
    ntiles = -(-n // tile)
    entries = d * ntiles + 1
    t = 0 if sd._transpose is not None else sd.nnz * 8 + (d + 1) * 8 + 2 * sd.nnz * 8
    return t + sd.nnz * 8 + 2 * entries * 8


def tile_table(sd, tile=None):
    """``tab`` [d * ntiles + 1] int64 (cached on ``sd``): the stored values
    of column c of the fit set that fall into fit rows ``[t * tile, (t + 1) *
    tile)`` are ``tab[c * ntiles + t] .. tab[c * ntiles + t + 1]`` of the
    transposed matrix.  The key ``c * ntiles + row // tile`` is non-decreasing
    along the transpose (sorted rows inside every column), so one
    ``searchsorted`` builds the table."""
    tile = _tile(tile)
    if tile in sd._knn_tables:
        return sd._knn_tables[tile]
    n, d = sd.shape
    if n >= 2 ** 31:
        raise ValueError("sparse k-NN supports fewer than 2^31 fit rows (int32 indices)")
    ntiles = -(-n // tile)
    if sd.device.type == "cuda":
        need = tile_table_bytes(sd, tile)
        free = torch.cuda.mem_get_info(sd.device)[0]
        if need > free:
            raise ValueError(f"the tile table of sparse k-NN on a {n} x {d} fit set with "
                             f"{sd.nnz} stored values and tiles of {tile} rows needs {need} "
                             f"bytes of device memory (the transposed matrix, one int64 key per "
                             f"stored value, {d * ntiles + 1} table entries twice); {free} are "
                             f"free")
    t = csr_transpose(sd)
    key = t.row_ids() * ntiles + torch.div(t.indices.to(torch.int64), tile, rounding_mode="floor")
    edges = torch.arange(d * ntiles + 1, dtype=torch.int64, device=sd.device)
    tab = torch.searchsorted(key, edges).contiguous()
    sd._knn_tables[tile] = tab
    return tab


# -------------------------------------------------------------- exponents
def query_exps(q_sd, max_x):
    """int32 [m]: ``ops.kmeans.fixed_point_exp(max|q_i| * max|X|, nnz_i)`` of
    every query row, vectorised (``frexp`` gives the exact ceil(log2))."""
    m = q_sd.shape[0]
    dev = q_sd.device
    cnt = (q_sd.indptr[1:] - q_sd.indptr[:-1]).to(torch.float64)
    mx = torch.zeros(m, dtype=torch.float64, device=dev)
    if q_sd.nnz:
        mx.scatter_reduce_(0, q_sd.row_ids(), q_sd.data.abs().double(), "amax")
    bound = mx * float(max_x) * cnt.clamp(min=1.0)
    if not bool(torch.isfinite(bound).all()):
        raise ValueError("non-finite values in the data: cannot accumulate inner products")
    mant, ex = torch.frexp(bound)                  # bound = mant * 2^ex, mant in [0.5, 1)
    e = torch.where(mant == 0.5, ex - 1, ex).to(torch.int64) - 52
    e = torch.where(bound > 0, e, torch.full_like(e, -120)).clamp(-120, 120)
    return e.to(torch.int32).contiguous()


# ---------------------------------------------------------------- epilogue
def _distances(dot, qn, xn, metric):
    """The kernel's epilogue on an fp64 block of inner products."""
    if metric == 0:
        return ((qn[:, None] + xn[None, :]) - 2.0 * dot).clamp_(min=0.0)
    den = torch.sqrt(qn)[:, None] * torch.sqrt(xn)[None, :]
    D = (1.0 - dot / den).clamp_(0.0, 2.0)
    zero = (qn == 0)[:, None] | (xn == 0)[None, :]
    return torch.where(zero, torch.ones_like(D), D)


def _select_block(D, kk):
    """The ``kk`` smallest of every row of ``D`` by (value, column): topk for
    the threshold, then the ties at the threshold by ascending column."""
    v = torch.topk(D, kk, dim=1, largest=False, sorted=True).values
    tau = v[:, -1:]
    lt = D < tau
    eq = D == tau
    need = kk - lt.sum(1, keepdim=True)
    sel = lt | (eq & (torch.cumsum(eq, 1, dtype=torch.int32) <= need))
    idx = torch.nonzero(sel)[:, 1].reshape(D.shape[0], kk)
    order = torch.sort(D.gather(1, idx), dim=1, stable=True).indices
    idx = idx.gather(1, order)
    return D.gather(1, idx), idx


# ---------------------------------------------------------------- operands
class InvertedIndex:
    """Operands of the inverted-index kernels (``csrc/spknn_acc.h``) for one
    (fit set, queries, tile): the tile table, the cached transpose, the
    squared row norms of both sides (``qn`` is ``xn`` in a self-join) and one
    fixed-point exponent per query row."""

    def __init__(self, fit_sd, query_sd, tile, xn=None, qn=None):
        self.fit, self.qry, self.tile = fit_sd, query_sd, tile
        self.n, self.d = fit_sd.shape
        self.tab = tile_table(fit_sd, tile)
        self.t = csr_transpose(fit_sd)
        self.ntiles = -(-self.n // tile)
        self.xn = sp_row_norms(fit_sd) if xn is None else xn
        if qn is None:
            qn = self.xn if query_sd is fit_sd else sp_row_norms(query_sd)
        self.qn = qn
        max_x = float(fit_sd.data.abs().max()) if fit_sd.nnz else 0.0
        self.qexp = query_exps(query_sd, max_x)
        self.lib = nat.native()

    def args(self, a, b):
        """The leading arguments of a launch on the query rows [a, b), the
        same for ``sp_knn`` and ``sp_radius_mark``: nine pointers, then q0, m,
        n, d, T, nnz_x."""
        return (*csr_ptrs(self.qry), self.t.indices.data_ptr(), self.t.data.data_ptr(),
                self.tab.data_ptr(), self.qn.data_ptr(), self.xn.data_ptr(),
                self.qexp.data_ptr(), a, b - a, self.n, self.d, self.tile, self.t.nnz)


# --------------------------------------------------------------------- op
def _check(fit_sd, query_sd, kk):
    if fit_sd.shape[1] != query_sd.shape[1]:
        raise ValueError(f"the queries have {query_sd.shape[1]} columns, the fit set "
                         f"{fit_sd.shape[1]}")
    if fit_sd.device != query_sd.device:
        raise ValueError("the queries and the fit set must be on the same device")
    kk = int(kk)
    if kk < 1 or kk > fit_sd.shape[0]:
        raise ValueError(f"kk must be between 1 and the {fit_sd.shape[0]} fit rows, got {kk}")
    return kk


def sp_knn(fit_sd, query_sd, kk, metric="euclidean", tile=None, rows=None, xn=None, qn=None):
    """(D [m, kk] fp64, idx [m, kk] int64): the ``kk`` nearest fit rows of
    every query row, ascending by (distance, fit index).  ``D`` is the squared
    distance for ``euclidean`` and the distance itself for ``cosine``.
    ``tile``: fit rows per workgroup; ``rows``: query rows per launch (default:
    what keeps the scratch within ``working_memory``); ``xn`` / ``qn``:
    precomputed squared row norms of the two sides."""
    code = _metric_code(metric)
    kk = _check(fit_sd, query_sd, kk)
    if not native_ok(fit_sd):
        return sp_knn_torch(fit_sd, query_sd, kk, metric)
    native_ok(query_sd)
    tile = _tile(tile)
    op = InvertedIndex(fit_sd, query_sd, tile, xn, qn)
    n, ntiles = op.n, op.ntiles
    m = query_sd.shape[0]
    dev = fit_sd.device
    select = kk <= KMAX
    if rows is None:
        # partials: fp64 + int32 per (tile, slot); dist mode: the block, the
        # two masks and the int32 running count of the tie rule
        rows = get_chunk_n_rows(12 * kk * ntiles if select else 14 * n)
    rows = max(1, min(int(rows), _MAX_GRID // ntiles))
    D = torch.empty((m, kk), dtype=torch.float64, device=dev)
    idx = torch.empty((m, kk), dtype=torch.int64, device=dev)
    mc = min(rows, m)
    if select:
        pd = torch.empty((mc, ntiles, kk), dtype=torch.float64, device=dev)
        pi = torch.empty((mc, ntiles, kk), dtype=torch.int32, device=dev)
        block = None
    else:
        pd = pi = None
        block = torch.empty((mc, n), dtype=torch.float64, device=dev)
    st = nat.stream_handle(dev)
    for a, b in chunks(m, rows):
        op.lib.sp_knn(*op.args(a, b), kk if select else 0, code, 0 if select else 1, nat.ptr(pd),
                      nat.ptr(pi), nat.ptr(block), D[a:b].data_ptr() if select else 0,
                      idx[a:b].data_ptr() if select else 0, st)
        if not select:
            D[a:b], idx[a:b] = _select_block(block[:b - a], kk)
    return D, idx


def sp_knn_torch(fit_sd, query_sd, kk, metric="euclidean", xn=None, qn=None,
                 chunk_rows=TWIN_CHUNK):
    """fp64 twin of :func:`sp_knn` over densified row chunks: the running
    best ``kk`` of every query row is merged with each fit chunk by a stable
    sort on the distance (the columns are in ascending fit index, so ties go
    to the smaller index)."""
    code = _metric_code(metric)
    kk = _check(fit_sd, query_sd, kk)
    n = fit_sd.shape[0]
    m = query_sd.shape[0]
    dev = fit_sd.device
    if xn is None:
        xn = sp_row_norms_torch(fit_sd)
    if qn is None:
        qn = xn if query_sd is fit_sd else sp_row_norms_torch(query_sd)
    D = torch.empty((m, kk), dtype=torch.float64, device=dev)
    idx = torch.empty((m, kk), dtype=torch.int64, device=dev)
    for a, b in chunks(m, chunk_rows):
        Q = query_sd.dense_rows(a, b)
        bd = torch.empty((b - a, 0), dtype=torch.float64, device=dev)
        bi = torch.empty((b - a, 0), dtype=torch.int64, device=dev)
        for s, e in chunks(n, chunk_rows):
            dot = Q @ fit_sd.dense_rows(s, e).T
            cd = torch.cat([bd, _distances(dot, qn[a:b].double(), xn[s:e].double(), code)], 1)
            ci = torch.cat([bi, torch.arange(s, e, dtype=torch.int64,
                                             device=dev).expand(b - a, e - s)], 1)
            order = torch.sort(cd, dim=1, stable=True).indices[:, :kk]
            bd, bi = cd.gather(1, order), ci.gather(1, order)
        D[a:b], idx[a:b] = bd, bi
    return D, idx
