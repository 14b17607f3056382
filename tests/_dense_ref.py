"""Plain numpy / fp64 references for the dense service kernels (k-NN top-k,
column moments, row norms, mu(A) power sums, forest traversal) and the small
inputs the CPU and GPU tests share.  Nothing in here calls torch: the
references are written from the definitions, not from the code under test.
"""
import math

import numpy as np

U32 = 2.0 ** -24      # unit roundoff of fp32
U64 = 2.0 ** -53      # unit roundoff of fp64


def gamma(k, u=U32):
    """Higham's gamma_k = k u / (1 - k u)."""
    return k * u / (1.0 - k * u)


# ------------------------------------------------------------------- top-k
def topk_ref(D, kk, col_offset=0):
    """(dist fp32 [m, kk], idx int64 [m, kk]): per row the kk smallest
    entries in the stable order (value, column); NaN entries are no
    candidates; rows with fewer than kk candidates are padded with
    (inf, -1).  ``col_offset`` is added to real columns only."""
    D = np.asarray(D, dtype=np.float32)
    m, nref = D.shape
    od = np.full((m, kk), np.inf, dtype=np.float32)
    oi = np.full((m, kk), -1, dtype=np.int64)
    for r in range(m):
        cols = np.nonzero(~np.isnan(D[r]))[0]
        vals = D[r, cols]
        order = np.lexsort((cols, vals))[:kk]      # last key is the primary one
        od[r, :len(order)] = vals[order]
        oi[r, :len(order)] = cols[order].astype(np.int64) + col_offset
    return od, oi


TOPK_PATTERNS = ("random", "descending", "ascending", "ties", "constant", "lane7")


def topk_pattern(name, m, nref, seed=0):
    """fp32 [m, nref] distance tiles that stress the selection kernel."""
    rng = np.random.RandomState(seed)
    j = np.arange(nref, dtype=np.float32)[None, :]
    r = np.arange(m, dtype=np.float32)[:, None]
    if name == "random":
        D = rng.standard_normal((m, nref))
    elif name == "descending":       # every element inserts at the head of its lane's list
        D = (nref - j) + 0.25 * r
    elif name == "ascending":
        D = j + 0.25 * r
    elif name == "ties":             # the index decides nearly every comparison
        D = rng.randint(0, 4, size=(m, nref))
    elif name == "constant":
        D = np.full((m, nref), 1.5) + r
    elif name == "lane7":            # one lane's list supplies every round of the merge
        D = 1.0 + rng.random_sample((m, nref))
        cols = np.arange(7, nref, 64)
        D[:, cols] = -2.0 + rng.random_sample((m, len(cols)))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(D, dtype=np.float32)


# ------------------------------------------------------- k-NN estimator data
def knn_data(d, seed=3):
    """(X_fit [300, d], Q [40, d]) fp64 arrays of fp32-representable values
    (the device estimator stores fp32: no input rounding enters the bound);
    rows 5, 6 and 200 of X_fit are identical."""
    rng = np.random.RandomState(seed + d)
    X = rng.standard_normal((300, d)).astype(np.float32)
    X[6] = X[5]
    X[200] = X[5]
    Q = rng.standard_normal((40, d)).astype(np.float32)
    return X.astype(np.float64), Q.astype(np.float64)


def sqdist_ref(Q, X):
    """(D [mq, n] fp64 squared distances from the differences, bound [mq, n]):
    the device forms qn + xn - 2 q.x in fp32; for any summation order
    |D_gpu - D| <= 2 gamma_{d+3} (qn + xn)."""
    Q = np.asarray(Q, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[1]
    D = ((Q[:, None, :] - X[None, :, :]) ** 2).sum(2)
    bound = 2.0 * gamma(d + 3) * ((Q * Q).sum(1)[:, None] + (X * X).sum(1)[None, :])
    return D, bound


def knn_ref(D, bound, k, exclude_self=False):
    """Reference neighbours of every query from the fp64 distances ``D``:
    (dist2 [mq, k], idx [mq, k], safe [mq, k]).  ``safe`` marks the ranks
    whose gaps to both neighbours in the reference order exceed twice the
    row's largest bound: there any fp32 evaluation within the bound keeps
    the reference's index."""
    D = np.array(D, dtype=np.float64)
    mq, n = D.shape
    if exclude_self:
        D[np.arange(mq), np.arange(mq)] = np.inf
    cols = np.broadcast_to(np.arange(n), D.shape)
    order = np.stack([np.lexsort((cols[r], D[r])) for r in range(mq)])
    srt = np.take_along_axis(D, order, 1)[:, :k + 1]
    gap_next = srt[:, 1:] - srt[:, :-1]                       # rank r to r + 1
    gap_prev = np.concatenate([np.full((mq, 1), np.inf), gap_next[:, :-1]], 1)
    b2 = 2.0 * bound.max(1)[:, None]
    safe = (gap_next > b2) & (gap_prev > b2)
    return srt[:, :k], order[:, :k], safe


# --------------------------------------------------------- moments / norms
def col_moments_ref(X):
    """(sum, sum of squares) of every column, each correctly rounded fp64
    (``math.fsum`` of the exact fp64 terms; the square of an fp32 or bf16
    value is exact in fp64)."""
    X = np.asarray(X, dtype=np.float64)
    s = np.array([math.fsum(c) for c in X.T], dtype=np.float64)
    ss = np.array([math.fsum(c) for c in (X * X).T], dtype=np.float64)
    return s, ss


def row_norms_ref(X):
    """||x_i||^2 in fp64."""
    X = np.asarray(X, dtype=np.float64)
    return np.array([math.fsum(r) for r in X * X], dtype=np.float64)


# ---------------------------------------------------------------------- mu
def mu_rowsums_ref(X, exponents, mean=None):
    """(row sums [nq, n], column sums [nq, d]) of |x - mean|^q in fp64;
    q = 0 counts the nonzeros of x - mean."""
    A = np.asarray(X, dtype=np.float64)
    if mean is not None:
        A = A - np.asarray(mean, dtype=np.float64)[None, :]
    A = np.abs(A)
    nz = A != 0
    rows = np.zeros((len(exponents), A.shape[0]))
    cols = np.zeros((len(exponents), A.shape[1]))
    for i, q in enumerate(exponents):
        if q == 0:
            P = nz.astype(np.float64)
        else:
            P = np.zeros_like(A)
            P[nz] = A[nz] ** float(q)
        rows[i] = P.sum(1)
        cols[i] = P.sum(0)
    return rows, cols


def mu_ref(X, exponents, mean=None):
    """(row_max [nq], col_sums [nq, d]) as ``ops.linalg.mu_power_sums_local``
    defines them: row_max[i] = max_r sum_c |a_rc|^q_i, col_sums[i, c] =
    sum_r |a_rc|^q_i with a = x - mean."""
    rows, cols = mu_rowsums_ref(X, exponents, mean)
    rmax = rows.max(1) if rows.shape[1] else np.zeros(len(exponents))
    return rmax, cols


MU_EXP_SETS = {
    "arith11": [round(0.2 * i, 10) for i in range(11)],        # ops.linalg.MU_EXPONENTS_STEP01
    "mixed7": [0.0, 0.1, 0.2, 1.0, 1.8, 1.9, 2.0],
    "mixed12": [0.0, 0.1, 0.3, 0.5, 0.7, 1.0, 1.1, 1.3, 1.5, 1.7, 1.9, 2.0],
}


def mu_rpw(n):
    """Rows per workgroup of the mu_sums launcher (1024 partial slots)."""
    wgs = min(1024, max(1, -(-n // 256)))
    return -(-n // wgs)


def mu_rstars(n):
    """Rows where a dropped row slot, tail row or workgroup-first row would
    sit: 0, n - 1, rpw - 1, rpw."""
    rpw = mu_rpw(n)
    return sorted({r for r in (0, n - 1, rpw - 1, rpw) if 0 <= r < n})


def mu_data(n, d, rstar, with_mean, seed=0):
    """(X [n, d] fp64, mean [d] fp64 or None).  The centred matrix a =
    x - mean holds multiples of 1/16: rows other than ``rstar`` have
    0 < |a| < 2 and exactly one zero (at column r mod d, an entry equal to
    the mean); row ``rstar`` has no zero and 4 <= |a| < 8, so each of its
    entries exceeds every entry of every other row and its power sum is the
    row maximum for every exponent.  mean is a multiple of 1/16 with
    |mean| <= 3/16, so x = a + mean is a multiple of 1/16 in (-8, 8): exact
    in bf16, and x - mean is exact in fp32.  The rows are those of one base
    matrix (seeded by n, d only) with rows 0 and ``rstar`` exchanged."""
    rng = np.random.RandomState(seed + 7919 * n + d)
    k = rng.randint(1, 32, size=(n, d)) * rng.choice([-1, 1], size=(n, d))
    r = np.arange(n)
    k[r, r % d] = 0
    k[0] = 4 * rng.randint(16, 32, size=d) * rng.choice([-1, 1], size=d)
    mean_k = rng.randint(-3, 4, size=d)
    if rstar != 0:
        k[[0, rstar]] = k[[rstar, 0]]
    a = k.astype(np.float64) / 16.0
    if not with_mean:
        return a, None
    mean = mean_k.astype(np.float64) / 16.0
    return a + mean[None, :], mean


# ------------------------------------------------------------------ forest
def complete_tree(depth, d, S, rng, int_values=False):
    """Node arrays of a complete binary tree of ``depth`` in breadth-first
    order (children 2i + 1, 2i + 2: always larger than the parent; the last
    level are leaves, left = right = -1, feature = -2)."""
    m = 2 ** (depth + 1) - 1
    inner = 2 ** depth - 1
    left = np.full(m, -1, dtype=np.int64)
    right = np.full(m, -1, dtype=np.int64)
    feat = np.full(m, -2, dtype=np.int64)
    thr = np.full(m, -2.0, dtype=np.float64)
    i = np.arange(inner)
    left[:inner] = 2 * i + 1
    right[:inner] = 2 * i + 2
    feat[:inner] = rng.randint(0, d, size=inner)
    thr[:inner] = rng.standard_normal(inner)
    if int_values:
        val = rng.randint(-8, 9, size=(m, S)).astype(np.float64)
    else:
        val = rng.standard_normal((m, S)) * np.exp(rng.uniform(-3, 3, size=(m, 1)))
    return dict(left=left, right=right, feat=feat, thr=thr, values=val,
                missing=rng.randint(0, 2, size=m).astype(np.uint8))


def stack_tables(trees):
    """One forest table from per-tree node arrays (``complete_tree`` dicts)."""
    offs = np.cumsum([0] + [len(t["left"]) for t in trees])[:-1].astype(np.int64)
    cat = lambda key: np.concatenate([t[key] for t in trees])      # noqa: E731
    return dict(left=cat("left"), right=cat("right"), feat=cat("feat"), thr=cat("thr"),
                values=np.concatenate([t["values"] for t in trees], 0), missing=cat("missing"),
                offs=offs, sizes=np.array([len(t["left"]) for t in trees]))


def make_forest(depths, d, S, seed=0, int_values=False):
    rng = np.random.RandomState(seed)
    return stack_tables([complete_tree(dep, d, S, rng, int_values) for dep in depths])


def forest_depths(T):
    """Depths 0-4 over the trees of a forest; T = 3 puts a root leaf between
    two deep trees."""
    return {1: [3], 3: [4, 0, 4], 7: [2, 0, 4, 1, 3, 4, 0]}[T]


def forest_ref(tables, X, use_missing=False):
    """(leaves int64 [n, T], sums fp64 [n, S], abs_sums fp64 [n, S] = the
    per-row sum of |v| behind the error bound) by a Python walk of every
    (row, tree): go left when (double)x <= thr; a NaN feature goes by the
    node's ``missing`` flag when ``use_missing``, else right (the comparison
    is false).  The walk is capped at the tree's node count and raises when
    the cap is hit (a table with a cycle must never reach a device kernel,
    which loops until it meets a leaf).  sums = per-row sum of the leaf
    value vectors over the trees, correctly rounded (``math.fsum``)."""
    X = np.asarray(X, dtype=np.float32)
    left, right, feat, thr = tables["left"], tables["right"], tables["feat"], tables["thr"]
    offs, sizes, vals = tables["offs"], tables["sizes"], tables["values"]
    n, T = X.shape[0], len(offs)
    leaves = np.empty((n, T), dtype=np.int64)
    for i in range(n):
        xi = X[i]
        for t in range(T):
            base, node, cap = int(offs[t]), 0, int(sizes[t])
            steps = 0
            while left[base + node] != -1:
                if steps >= cap:
                    raise RuntimeError(f"forest_ref: tree {t} does not reach a leaf in {cap} steps")
                steps += 1
                q = base + node
                xv = float(xi[feat[q]])
                if use_missing and math.isnan(xv):
                    go_left = tables["missing"][q] != 0
                else:
                    go_left = xv <= float(thr[q])
                node = int(left[q] if go_left else right[q])
                if not 0 <= node < cap:
                    raise RuntimeError(f"forest_ref: tree {t} child {node} out of range")
            leaves[i, t] = node
    picked = vals[offs[None, :] + leaves]                  # [n, T, S]
    sums = np.array([[math.fsum(picked[i, :, s]) for s in range(vals.shape[1])]
                     for i in range(n)], dtype=np.float64).reshape(n, vals.shape[1])
    return leaves, sums, np.abs(picked).sum(1)


def forest_rows(n, d, seed=0, nan_frac=0.0):
    """fp32 rows; a ``nan_frac`` share of the entries is NaN."""
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    if nan_frac:
        X[rng.random_sample((n, d)) < nan_frac] = np.nan
    return X
