"""Kernel matrices of CSR queries against a CSR fit set (SURVEY.md E4/E5 /
K17, sparse half): the linear, polynomial, rbf and sigmoid kernels of
``utils/pairwise.py`` on sparse rows, written out (:func:`sp_kernel_matrix`)
or applied to at most four vectors without being formed
(:func:`sp_kernel_matvec`) - what the least-squares SVMs fit and predict with.

Device path: ``csrc/spgram.hip``.  The inner products are those of the
sparse k-NN kernel (``ops/sparse_knn.py``: cached transpose, tile pointer
table, one fixed-point exponent per query row, 64-bit integer LDS atomics),
so they are bit-identical from run to run and independent of the launch
geometry; the kernel function (``csrc/spgram.h``) runs on them in fp64.
Matrix mode stores with a caller-given row stride, so ``out`` may be a view
into a larger matrix; apply mode sums in a fixed order (thread, wave
butterfly, wave order, tile order: no floating-point atomics).  The linear
apply is ``Q (X^T V)`` through ``sparse_linalg.sp_xty`` / ``sp_xw``:
``O(nnz)``.  A GPU input always takes the native path and raises when the
extension is missing.  The torch twins (CPU) work in fp64 over densified row
chunks with the same formulae in the same operation order.
"""

import math

import torch

from . import _native as nat
from ._csr import TWIN_CHUNK, chunks, native_ok, sp_row_norms_torch
from .sparse_knn import _MAX_GRID, InvertedIndex, _tile
from .sparse_linalg import sp_xty, sp_xw
from ..utils.pairwise import get_chunk_n_rows

KINDS = {"linear": 0, "poly": 1, "rbf": 2, "sigmoid": 3}
RMAX = 4               # right-hand sides of one apply (csrc/spgram.h)


def _kind_code(kind):
    if kind not in KINDS:
        raise ValueError(f"sparse kernels are 'linear', 'poly', 'rbf' and 'sigmoid', got {kind!r}")
    return KINDS[kind]


def _params(fit_sd, query_sd, gamma, coef0, degree):
    if fit_sd.shape[1] != query_sd.shape[1]:
        raise ValueError(f"the queries have {query_sd.shape[1]} columns, the fit set "
                         f"{fit_sd.shape[1]}")
    if fit_sd.device != query_sd.device:
        raise ValueError("the queries and the fit set must be on the same device")
    gamma = 1.0 / fit_sd.shape[1] if gamma is None else float(gamma)
    return gamma, float(coef0), float(degree)


def kernel_values(dot, qn, xn, code, gamma, coef0, degree):
    """``kernel_value`` of ``csrc/spgram.h`` on an fp64 block of inner
    products: multiply by gamma, add coef0, then the function."""
    if code == 0:
        return dot
    if code == 2:
        D = ((qn[:, None] + xn[None, :]) - 2.0 * dot).clamp_(min=0.0)
        return torch.exp(-gamma * D)
    arg = gamma * dot + coef0
    return torch.pow(arg, degree) if code == 1 else torch.tanh(arg)


def _own_pairs(K, a, b, s, e, code, gamma, diag_add):
    """The pairs (i, i) of a self-join inside the block K = rows [a, b) x
    columns [s, e): distance exactly 0 for rbf, plus the addend."""
    lo, hi = max(a, s), min(b, e)
    if lo >= hi:
        return
    own = torch.arange(lo, hi, device=K.device)
    if code == 2:
        K[own - a, own - s] = math.exp(-gamma * 0.0)
    if diag_add:
        K[own - a, own - s] += diag_add


def _out(out, m, n, dev):
    if out is None:
        return torch.empty((m, n), dtype=torch.float64, device=dev)
    if out.dtype != torch.float64 or out.dim() != 2 or tuple(out.shape) != (m, n) \
            or (n > 1 and out.stride(1) != 1) or (m > 1 and out.stride(0) < n) \
            or out.device != dev:
        raise ValueError(f"out must be an fp64 matrix of shape ({m}, {n}) with a contiguous last "
                         "dimension on the device of the sparse matrices")
    return out


def _diag(diag_add, self_join):
    diag_add = float(diag_add)
    if diag_add != 0.0 and not self_join:
        raise ValueError("diag_add belongs to the self-join: the queries must be the fit set "
                         "itself")
    return diag_add


# ------------------------------------------------------------------ matrix
def sp_kernel_matrix(fit_sd, query_sd, kind, gamma=None, coef0=1.0, degree=3.0, out=None,
                     diag_add=0.0, tile=None, rows=None, op=None):
    """K [m, n] fp64: ``K[i, j] = kernel(query row i, fit row j)``.
    ``query_sd is fit_sd`` is the self-join: ``K[i, i]`` is taken at distance
    exactly 0 (rbf) and ``diag_add`` is added to it.  ``out``: an fp64 [m, n]
    tensor to fill, possibly a strided view with a contiguous last dimension
    (nothing outside the view is touched).  ``gamma=None``: 1 / n_features.
    ``tile``: fit rows per workgroup; ``rows``: query rows per launch (default:
    what the grid limit allows); ``op``: the :class:`InvertedIndex` of the
    pair, when the caller keeps one."""
    code = _kind_code(kind)
    gamma, coef0, degree = _params(fit_sd, query_sd, gamma, coef0, degree)
    self_join = query_sd is fit_sd
    diag_add = _diag(diag_add, self_join)
    if not native_ok(fit_sd):
        return sp_kernel_matrix_torch(fit_sd, query_sd, kind, gamma, coef0, degree, out, diag_add)
    native_ok(query_sd)
    if op is None:
        op = InvertedIndex(fit_sd, query_sd, _tile(tile))
    m, n = query_sd.shape[0], op.n
    out = _out(out, m, n, fit_sd.device)
    rows = _MAX_GRID // op.ntiles if rows is None else int(rows)
    rows = max(1, min(rows, _MAX_GRID // op.ntiles))
    ld = out.stride(0) if m > 1 else max(out.stride(0), n)
    st = nat.stream_handle(fit_sd.device)
    for a, b in chunks(m, rows):
        op.lib.gram.sp_gram(*op.args(a, b), code, gamma, coef0, degree, 1 if self_join else 0,
                            diag_add, out.data_ptr(), ld, st)
    return out


def sp_kernel_matrix_torch(fit_sd, query_sd, kind, gamma=None, coef0=1.0, degree=3.0, out=None,
                           diag_add=0.0, chunk_rows=TWIN_CHUNK):
    """fp64 twin of :func:`sp_kernel_matrix` over densified row chunks."""
    code = _kind_code(kind)
    gamma, coef0, degree = _params(fit_sd, query_sd, gamma, coef0, degree)
    self_join = query_sd is fit_sd
    diag_add = _diag(diag_add, self_join)
    m, n = query_sd.shape[0], fit_sd.shape[0]
    out = _out(out, m, n, fit_sd.device)
    xn = sp_row_norms_torch(fit_sd)
    qn = xn if self_join else sp_row_norms_torch(query_sd)
    for a, b in chunks(m, chunk_rows):
        Q = query_sd.dense_rows(a, b)
        for s, e in chunks(n, chunk_rows):
            K = kernel_values(Q @ fit_sd.dense_rows(s, e).T, qn[a:b], xn[s:e], code, gamma, coef0,
                              degree)
            if self_join:
                _own_pairs(K, a, b, s, e, code, gamma, diag_add)
            out[a:b, s:e] = K
    return out


# ------------------------------------------------------------------- apply
def _rhs(V, n, dev):
    V = torch.as_tensor(V)
    flat = V.dim() == 1
    if flat:
        V = V[:, None]
    if V.dim() != 2 or V.shape[0] != n:
        raise ValueError(f"operand of shape {tuple(V.shape)} does not match a fit set of {n} rows")
    if not 1 <= V.shape[1] <= RMAX:
        raise ValueError(f"a kernel matrix is applied to between 1 and {RMAX} vectors at a time, "
                         f"got {V.shape[1]}")
    return V.to(device=dev, dtype=torch.float64).contiguous(), flat


def sp_kernel_matvec(fit_sd, query_sd, V, kind, gamma=None, coef0=1.0, degree=3.0, tile=None,
                     rows=None, op=None):
    """K V [m, R] fp64 for V [n, R], ``1 <= R <= 4`` (a vector gives a
    vector), without forming K.  ``query_sd is fit_sd`` is the self-join of
    :func:`sp_kernel_matrix`.  'linear' is ``Q (X^T V)`` through the CSR
    products; the other kinds run the fused kernel, ``rows`` query rows per
    launch (default: what keeps the partials within ``working_memory``)."""
    code = _kind_code(kind)
    gamma, coef0, degree = _params(fit_sd, query_sd, gamma, coef0, degree)
    Vd, flat = _rhs(V, fit_sd.shape[0], fit_sd.device)
    if not native_ok(fit_sd):
        return sp_kernel_matvec_torch(fit_sd, query_sd, V, kind, gamma, coef0, degree)
    native_ok(query_sd)
    if code == 0:
        out = sp_xw(query_sd, sp_xty(fit_sd, Vd))
        return out[:, 0] if flat else out
    if op is None:
        op = InvertedIndex(fit_sd, query_sd, _tile(tile))
    m, R = query_sd.shape[0], Vd.shape[1]
    dev = fit_sd.device
    if rows is None:
        rows = get_chunk_n_rows(8 * op.ntiles * R)
    rows = max(1, min(int(rows), _MAX_GRID // op.ntiles))
    out = torch.empty((m, R), dtype=torch.float64, device=dev)
    part = torch.empty((min(rows, m), op.ntiles, R), dtype=torch.float64, device=dev)
    st = nat.stream_handle(dev)
    for a, b in chunks(m, rows):
        op.lib.gram.sp_gram_matvec(*op.args(a, b), code, gamma, coef0, degree,
                                   1 if query_sd is fit_sd else 0, Vd.data_ptr(), R,
                                   part.data_ptr(), out.data_ptr(), st)
    return out[:, 0] if flat else out


def sp_kernel_matvec_torch(fit_sd, query_sd, V, kind, gamma=None, coef0=1.0, degree=3.0,
                           chunk_rows=TWIN_CHUNK):
    """fp64 twin of :func:`sp_kernel_matvec` over densified row chunks; the
    linear apply is ``Q (X^T V)`` here too."""
    code = _kind_code(kind)
    gamma, coef0, degree = _params(fit_sd, query_sd, gamma, coef0, degree)
    m, n = query_sd.shape[0], fit_sd.shape[0]
    Vd, flat = _rhs(V, n, fit_sd.device)
    out = torch.zeros((m, Vd.shape[1]), dtype=torch.float64, device=fit_sd.device)
    if code == 0:
        Z = torch.zeros((fit_sd.shape[1], Vd.shape[1]), dtype=torch.float64, device=fit_sd.device)
        for s, e in chunks(n, chunk_rows):
            Z += fit_sd.dense_rows(s, e).T @ Vd[s:e]
        for a, b in chunks(m, chunk_rows):
            out[a:b] = query_sd.dense_rows(a, b) @ Z
        return out[:, 0] if flat else out
    self_join = query_sd is fit_sd
    xn = sp_row_norms_torch(fit_sd)
    qn = xn if self_join else sp_row_norms_torch(query_sd)
    for a, b in chunks(m, chunk_rows):
        Q = query_sd.dense_rows(a, b)
        for s, e in chunks(n, chunk_rows):
            K = kernel_values(Q @ fit_sd.dense_rows(s, e).T, qn[a:b], xn[s:e], code, gamma, coef0,
                              degree)
            if self_join:
                _own_pairs(K, a, b, s, e, code, gamma, 0.0)
            out[a:b] += K @ Vd[s:e]
    return out[:, 0] if flat else out
