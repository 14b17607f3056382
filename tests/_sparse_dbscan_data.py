"""Shared fixtures of the sparse DBSCAN tests (CPU and GPU files)."""

import numpy as np
import scipy.sparse as sp

from _sparse_knn_data import dot_tolerance, sq_norms

N, D_COLS = 600, 400
TOPICS, TOPIC_COLS, LOOSE = 5, 12, 60


def clustered(seed=2024):
    """CSR [600, 400]: 5 "topics" of 12 columns with values U(0.5, 1); a topic
    row is its topic plus N(0, 0.05) on the topic's columns and 0 to 4 extra
    columns at U(0.05, 0.3); the last 60 rows are unstructured (3 to 12
    columns at U(0.1, 1)).  Values are fp32-rounded, the rows permuted."""
    rng = np.random.RandomState(seed)
    dense = np.zeros((N, D_COLS))
    cols = rng.permutation(D_COLS)[:TOPICS * TOPIC_COLS].reshape(TOPICS, TOPIC_COLS)
    centre = rng.uniform(0.5, 1.0, size=(TOPICS, TOPIC_COLS))
    per = (N - LOOSE) // TOPICS
    for i in range(N - LOOSE):
        t = i // per
        dense[i, cols[t]] = centre[t] + 0.05 * rng.standard_normal(TOPIC_COLS)
        extra = rng.choice(np.setdiff1d(np.arange(D_COLS), cols[t]), size=rng.randint(0, 5),
                           replace=False)
        dense[i, extra] = rng.uniform(0.05, 0.3, size=len(extra))
    for i in range(N - LOOSE, N):
        c = rng.choice(D_COLS, size=rng.randint(3, 13), replace=False)
        dense[i, c] = rng.uniform(0.1, 1.0, size=len(c))
    dense = dense.astype(np.float32).astype(np.float64)[rng.permutation(N)]
    X = sp.csr_matrix(dense)
    X.sort_indices()
    return X


def pair_distances(X, metric):
    """fp64 [n, n]: squared euclidean or cosine distances of the rows."""
    A = np.asarray(X.todense())
    xn = sq_norms(X)
    dot = A @ A.T
    if metric == "euclidean":
        return np.maximum(xn[:, None] + xn[None, :] - 2.0 * dot, 0.0)
    den = np.sqrt(xn)[:, None] * np.sqrt(xn)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, np.clip(1.0 - dot / den, 0.0, 2.0), 1.0)


def gap_threshold(dist, q=0.10, width=0.01):
    """The midpoint of the widest gap between consecutive sorted values of
    ``dist`` between its ``q`` and ``q + width`` quantiles."""
    v = np.sort(np.asarray(dist).ravel())
    lo, hi = int(q * len(v)), int((q + width) * len(v))
    w = v[lo:hi + 1]
    g = int(np.argmax(np.diff(w)))
    return 0.5 * (w[g] + w[g + 1])


def decided_threshold(X, metric, q=0.10):
    """(thr, pair distances): ``gap_threshold`` of the off-diagonal pairs, with
    the condition that no pair lies within ``4 * dot_tolerance`` of it - two
    fp64 implementations then find the same neighbourhoods."""
    dist = pair_distances(X, metric)
    off = ~np.eye(X.shape[0], dtype=bool)
    thr = gap_threshold(dist[off], q)
    tol = 4.0 * dot_tolerance(X, X, metric)
    assert (np.abs(dist - thr)[off] > tol[off]).all()
    return thr, dist
