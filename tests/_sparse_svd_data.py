"""Shared fixtures of the sparse SVD tests (CPU and GPU files)."""

import numpy as np
import scipy.sparse as sp

N_PLANTED, D_PLANTED, TOPICS = 2500, 2000, 6


def planted_topics(seed=0):
    """n = 2500, d = 2000, 6 topics (n * d > 4e6: the sparse branch runs).
    Row i belongs to topic i % 6: 9 to 25 nonzeros 1 + 0.25 u in its topic's
    block of 333 columns, 3 off-block nonzeros 0.05 N(0, 1); fp32-rounded
    values.  The last two columns are empty.  Singular values: six near 23,
    then about 10."""
    rng = np.random.RandomState(seed)
    block = D_PLANTED // TOPICS
    rows, cols, vals = [], [], []
    for i in range(N_PLANTED):
        t = i % TOPICS
        m = rng.randint(9, 26)
        c = t * block + rng.choice(block, size=m, replace=False)
        rows += [i] * m
        cols += list(c)
        vals += list(1.0 + 0.25 * rng.uniform(size=m))
        off = rng.choice(TOPICS * block - block, size=3, replace=False)
        off = np.where(off >= t * block, off + block, off)       # skip the own block
        rows += [i] * 3
        cols += list(off)
        vals += list(0.05 * rng.standard_normal(3))
    v = np.asarray(vals).astype(np.float32).astype(np.float64)
    X = sp.csr_matrix((v, (rows, cols)), shape=(N_PLANTED, D_PLANTED))
    X.sort_indices()
    return X


def two_vocab_docs(n_docs=40, seed=0):
    """Short documents drawn from two disjoint vocabularies; (docs, truth)."""
    rng = np.random.RandomState(seed)
    vocab = [["apple", "banana", "cherry", "grape", "lemon", "mango", "peach", "plum"],
             ["engine", "wheel", "brake", "clutch", "piston", "gear", "axle", "valve"]]
    docs, truth = [], []
    for i in range(n_docs):
        g = i % 2
        docs.append(" ".join(rng.choice(vocab[g], size=6)))
        truth.append(g)
    return docs, np.asarray(truth)
