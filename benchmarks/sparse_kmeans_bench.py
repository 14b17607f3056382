"""Sparse (CSR) k-means / q-means benchmark: E-step (band), M-step and
10-iteration ``KMeans`` / ``QMeans`` fits on a synthetic TF-IDF-like matrix
generated in place (Zipf column draws, ~100 stored values per row, rows L2
normalised), next to two baselines: the dense path on ``X.toarray()`` (second
shape only, where the dense matrix fits) and scikit-learn's CPU ``KMeans`` on
the same CSR.

    python benchmarks/sparse_kmeans_bench.py --shape small --baselines

Prints one JSON line per measurement; ``profiles/sparse_kmeans.md`` records a
run.  There is no pass/fail time.
"""

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from sq_learn_amd.models._data import as_sparse_data      # noqa: E402
from sq_learn_amd.models.cluster import KMeans, QMeans    # noqa: E402
from sq_learn_amd.ops import sparse_kmeans as S           # noqa: E402
from sq_learn_amd.runtime.rng import RngKey               # noqa: E402

SHAPES = {"big": (1_000_000, 100_000, 256), "small": (200_000, 4096, 1024)}


def make_csr(n, d, nnz_row=100, seed=0):
    """Zipf-like (log-uniform rank) column draws, duplicates merged, values
    uniform, rows L2-normalised; built in row blocks on the host."""
    rng = np.random.RandomState(seed)
    blocks = []
    step = 100_000
    for s in range(0, n, step):
        m = min(step, n - s)
        cols = np.minimum((d ** rng.random_sample((m, nnz_row))).astype(np.int64) - 1, d - 1)
        cols.sort(axis=1)
        keep = np.ones_like(cols, dtype=bool)
        keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
        counts = keep.sum(1)
        vals = rng.random_sample(int(counts.sum())) + 0.1
        indptr = np.concatenate([[0], np.cumsum(counts)])
        norm = np.sqrt(np.add.reduceat(vals * vals, indptr[:-1]))
        vals /= np.repeat(norm, counts)
        blocks.append(sp.csr_matrix((vals.astype(np.float32), cols[keep].astype(np.int32), indptr),
                                    shape=(m, d)))
    return sp.vstack(blocks, format="csr")


def timed(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def emit(**kw):
    print(json.dumps(kw), flush=True)


def fit_time(make, X, reps=1):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        make().fit(X)                      # warm-up (lazy kernel loading, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            est = make().fit(X)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, est


def run(name, baselines, fits):
    n, d, k = SHAPES[name]
    t0 = time.perf_counter()
    X = make_csr(n, d)
    emit(shape=name, n=n, d=d, k=k, nnz=int(X.nnz), gen_s=round(time.perf_counter() - t0, 2))
    sd = as_sparse_data(X, device="cuda")
    xn = S.sp_row_norms(sd)
    rows = np.random.RandomState(1).choice(n, size=k, replace=False)
    C = sd.gather_dense(rows)
    op = S.center_operand(C)
    key = RngKey(0, "band_select", 0)
    k_pad = op[0].shape[1]
    ms = timed(lambda: S.sp_estep(sd, C, 0.05, key, 0, xn=xn, operand=op))
    # every stored value gathers one CT row per centroid tile pass: 8 k_pad bytes
    gather = sd.nnz * 8.0 * k_pad
    emit(shape=name, what="estep_band", ms=round(ms, 3), ct_gather_TBps=round(gather / ms / 1e9, 3))
    labels, _, _ = S.sp_estep(sd, C, 0.0, key, 0, xn=xn, operand=op)
    ws = S.SparseReduce(sd, k)
    ms = timed(lambda: S.sp_centroid_sums(sd, labels, k, ws=ws))
    z = timed(lambda: ws.q.zero_())
    emit(shape=name, what="mstep", ms=round(ms, 3), zero_ms=round(z, 3),
         atomics_per_s=round(sd.nnz / ms * 1e3, 0),
         atomic_GBps=round(sd.nnz * 8.0 / ms / 1e6, 2),
         note="rate over the whole op (zeroing + atomics + k*d finish)")
    if fits:
        init = C.cpu().numpy()
        s, est = fit_time(lambda: KMeans(k, init=init, n_init=1, max_iter=10, tol=0.0,
                                         device="cuda"), X)
        emit(shape=name, what="kmeans_fit_10it", s=round(s, 3), n_iter=int(est.n_iter_),
             inertia=float(est.inertia_))
        s, est = fit_time(lambda: QMeans(k, init=init, n_init=1, max_iter=10, tol=0.0, delta=0.05,
                                         true_distance_estimate=False, compute_prelude=False,
                                         random_state=0, device="cuda"), X)
        emit(shape=name, what="qmeans_fit_10it", s=round(s, 3), n_iter=int(est.n_iter_),
             inertia=float(est.inertia_))
        if baselines:
            if n * d * 4 <= 4 << 30:
                Xd = torch.as_tensor(X.toarray(), device="cuda")
                s, est = fit_time(lambda: KMeans(k, init=init, n_init=1, max_iter=10, tol=0.0,
                                                 device="cuda"), Xd)
                emit(shape=name, what="dense_kmeans_fit_10it", s=round(s, 3),
                     n_iter=int(est.n_iter_), inertia=float(est.inertia_))
                del Xd
            from sklearn.cluster import KMeans as SkKMeans
            torch.set_num_threads(16)
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = SkKMeans(k, init=init, n_init=1, max_iter=10, tol=0.0,
                               algorithm="lloyd").fit(X)
            emit(shape=name, what="sklearn_cpu_kmeans_fit_10it",
                 s=round(time.perf_counter() - t0, 3), n_iter=int(ref.n_iter_),
                 inertia=float(ref.inertia_),
                 threads=os.environ.get("OMP_NUM_THREADS", "default"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["big", "small", "both"], default="small")
    ap.add_argument("--baselines", action="store_true")
    ap.add_argument("--no-fits", action="store_true")
    a = ap.parse_args()
    for name in (["big", "small"] if a.shape == "both" else [a.shape]):
        run(name, a.baselines, not a.no_fits)


if __name__ == "__main__":
    main()
