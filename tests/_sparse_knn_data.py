"""Shared fixtures of the sparse k-NN tests (CPU and GPU files)."""

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53

# ---- the structured case of the GPU tests
N_FIT, D, M, TILE = 700, 500, 70, 256          # 3 tiles, the last holds 188 rows
Q_FORCED = [0, 1, 63, 64, 65, 300]             # nonzeros of query rows 0..5
Q_ZERO_ROW, Q_LAST_COL_ROW = 6, 7              # a stored zero first; the last column
Q_TWIN_ROW = 8                                 # equals the identical fit rows
FULL_COL, EMPTY_COL = 11, D - 2                # fit side: in every non-empty row; in none
EMPTY_FIT_ROWS = (40, 650)
TWIN_ROWS = (5, 6, 300)                        # identical fit rows: inside and across tiles


def _values(rng, kind, size):
    if kind == "exact":
        return rng.randint(1, 9, size=size) * rng.choice([-1.0, 1.0], size=size)
    return rng.standard_normal(size).astype(np.float32).astype(np.float64)


def structured(kind, seed=4242):
    """(fit CSR [700, 500], query CSR [70, 500]) with ``kind`` 'exact'
    (integers in [-8, 8]) or 'random' (fp32-rounded normals); the sparsity
    structure is the same for both.  Columns D - 2 (empty on the fit side)
    and D - 1 (query row 7 only) are outside the random draws."""
    rng = np.random.RandomState(seed)
    pool = np.setdiff1d(np.arange(D - 2), [FULL_COL])
    # fit side: FULL_COL plus 8..20 more columns in every non-empty row
    counts = rng.randint(9, 22, size=N_FIT)
    counts[list(EMPTY_FIT_ROWS)] = 0
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(np.append(rng.choice(pool, size=c - 1, replace=False),
                                                FULL_COL)) for c in counts if c]).astype(np.int32)
    X = sp.csr_matrix((_values(rng, kind, len(indices)), indices, indptr),
                      shape=(N_FIT, D)).tolil()
    for r in TWIN_ROWS[1:]:
        X[r] = X[TWIN_ROWS[0]]
    X = X.tocsr()
    X.sort_indices()
    # query side: rows 0..5 forced lengths; rows of two or more nonzeros from
    # row 2 on include FULL_COL
    # row Q_TWIN_ROW is a copy of the identical fit rows
    twin = X[TWIN_ROWS[0]]
    counts = rng.randint(5, 31, size=M)
    counts[:len(Q_FORCED)] = Q_FORCED
    counts[Q_TWIN_ROW] = twin.nnz
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows = []
    for i, c in enumerate(counts):
        if i == Q_TWIN_ROW:
            rows.append(twin.indices.copy())
        elif i >= 2 and c >= 2:
            rows.append(np.sort(np.append(rng.choice(pool, size=c - 1, replace=False), FULL_COL)))
        else:
            rows.append(np.sort(rng.choice(pool, size=c, replace=False)))
    indices = np.concatenate(rows).astype(np.int32)
    indices[indptr[Q_LAST_COL_ROW + 1] - 1] = D - 1
    qv = _values(rng, kind, len(indices))
    qv[indptr[Q_ZERO_ROW]] = 0.0
    qv[indptr[Q_TWIN_ROW]:indptr[Q_TWIN_ROW + 1]] = twin.data
    Q = sp.csr_matrix((qv, indices, indptr), shape=(M, D))
    return X, Q


# ---- continuous data for the comparisons with scikit-learn
def random_pair(n=150, m=40, d=60, nnz_row=(3, 12), seed=3):
    """(fit CSR, query CSR, class labels, float targets): fp32-rounded
    uniform values in [0.1, 1], 3 to 12 nonzeros per row."""
    rng = np.random.RandomState(seed)

    def one(rows):
        counts = rng.randint(nnz_row[0], nnz_row[1] + 1, size=rows)
        indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        indices = np.concatenate([np.sort(rng.choice(d, size=c, replace=False)) for c in counts])
        vals = rng.uniform(0.1, 1.0, size=len(indices)).astype(np.float32).astype(np.float64)
        return sp.csr_matrix((vals, indices.astype(np.int32), indptr), shape=(rows, d))
    X, Q = one(n), one(m)
    return X, Q, rng.randint(0, 3, size=n), rng.standard_normal(n)


def sq_norms(A):
    return np.asarray(A.multiply(A).sum(1)).ravel()


def dot_tolerance(X, Q, metric="euclidean"):
    """[m, n] bound on the fp64 rounding of one implementation's squared
    euclidean distance ``|q|^2 + |x|^2 - 2 q.x``: ``(nnz_row + 4) * 2^-53 *
    (|q|^2 + |x|^2)`` with ``nnz_row = nnz_q + nnz_x``, the number of terms of
    the two norms (the dot has at most min(nnz_q, nnz_x) terms of at most
    (|q|^2 + |x|^2) / 2 in total, doubled; four more roundings combine them).
    Cosine: the same with unit norms (the distance of the normalised rows)."""
    nnz = np.diff(Q.indptr)[:, None] + np.diff(X.indptr)[None, :]
    if metric == "cosine":
        return (nnz + 4) * U * 2.0
    return (nnz + 4) * U * (sq_norms(Q)[:, None] + sq_norms(X)[None, :])
