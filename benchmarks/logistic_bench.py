"""Sparse LogisticRegression benchmark: the loss kernels of
``ops.sparse_logistic`` (multinomial at K classes, binary at ``--classes 1``),
``sp_matvec`` on the cached transpose, one whole objective evaluation and
whole fits of ``LogisticRegression(device="cuda")`` on TF-IDF-like rows: the
synthetic bag-of-words corpus of ``lda_bench.py`` (about 100 stored words per
document) with every count scaled by its word's inverse document frequency.
Next to it, on the same machine,

(a) the route composed from pieces that existed before the kernels: ``sp_xw``,
    torch's logsumexp / softmax (sigmoid for the binary problem), ``sp_xty``;
(b) the host path (``device=None``, ``--host``), which densifies: only at a
    shape that fits as a dense fp64 array;
(c) scikit-learn's CPU ``LogisticRegression`` on the same CSR (``--sklearn``).

    python benchmarks/logistic_bench.py --shape large --classes 1 20 300 --kernels-only
    python benchmarks/logistic_bench.py --shape small --classes 1 20 --host --sklearn

Prints one JSON line per measurement (kernels: medians over ``--reps`` event
pairs after a warm-up; objective evaluations and device fits: medians of
warmed host-clock samples around a device synchronise; host-path and
scikit-learn fits: one sample); ``profiles/logistic_device.md`` records a run.
There is no pass/fail time.
"""

import argparse
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

from lda_bench import SHAPES, make_corpus, wall               # noqa: E402
from sparse_kmeans_bench import emit                         # noqa: E402
from sparse_knn_bench import median_ms                       # noqa: E402
from sq_learn_amd.linear_model import LogisticRegression     # noqa: E402
from sq_learn_amd.models._data import as_sparse_data         # noqa: E402
from sq_learn_amd.models.linear_model._logistic import _SparseObjective  # noqa: E402
from sq_learn_amd.ops import sparse_linalg as SL             # noqa: E402
from sq_learn_amd.ops import sparse_logistic as S            # noqa: E402
from sq_learn_amd.ops._csr import csr_transpose              # noqa: E402

HOST_DENSE_BYTES = 8 << 30     # the host path runs only where dense X stays below this


def tfidf(n, d):
    X = sp.csr_matrix(make_corpus(n, d), dtype=np.float64)
    df = np.bincount(X.indices, minlength=d)
    X.data *= (np.log((1.0 + n) / (1.0 + df)) + 1.0)[X.indices]
    return X


def composed_multi(sd, W, b, lab, sw):
    z = SL.sp_xw(sd, W.T) + b
    lse = torch.logsumexp(z, dim=1)
    ar = torch.arange(sd.shape[0], device=sd.device)
    loss = (sw * (lse - z[ar, lab])).sum()
    R = torch.exp(z - lse[:, None])
    R[ar, lab] -= 1.0
    R *= sw[:, None]
    return loss, R


def composed_bin(sd, w, b, t, sw):
    tz = t * (SL.sp_xw(sd, w[:, None])[:, 0] + b)
    loss = -(sw * torch.nn.functional.logsigmoid(tz)).sum()
    return loss, sw * (torch.sigmoid(tz) - 1) * t


def run(name, K, a):
    n, d = SHAPES[name]
    X = tfidf(n, d)
    base = dict(shape=name, n=n, d=d, K=K, nnz_row=round(X.nnz / n, 1))
    dev = torch.device("cuda")
    rng = np.random.RandomState(0)
    sd = as_sparse_data(X, dev)
    sdt = csr_transpose(sd)
    SL.segments(sd), SL.segments(sdt)
    sw = torch.ones(n, dtype=torch.float64, device=dev)
    if K == 1:
        y = rng.randint(0, 2, n)
        lab = torch.from_numpy(y.astype(np.int32)).to(dev)
        t = torch.where(lab != 0, 1.0, -1.0).double()
        w = torch.from_numpy(0.01 * rng.randn(d)).to(dev)
        emit(what="logit_bin", ms=median_ms(lambda: S.logit_bin(sd, w, 0.1, lab, sw), reps=a.reps),
             **base)
        emit(what="logit_bin_composed",
             ms=median_ms(lambda: composed_bin(sd, w, 0.1, t, sw), reps=a.reps), **base)
        r = S.logit_bin(sd, w, 0.1, lab, sw)[1]
        ref = composed_bin(sd, w, 0.1, t, sw)[1]
        emit(what="logit_bin_vs_composed", max_abs=float((r - ref).abs().max()), **base)
        emit(what="matvec_xt", ms=median_ms(lambda: S.sp_matvec(sdt, r), reps=a.reps), **base)
        emit(what="matvec_xt_composed",
             ms=median_ms(lambda: SL.sp_xty(sd, r[:, None]), reps=a.reps), **base)
        emit(what="matvec_x", ms=median_ms(lambda: S.sp_matvec(sd, w), reps=a.reps), **base)
        obj = _SparseObjective(sd, y, 2, np.ones(n), 1.0, True, False)
        w0 = 0.01 * rng.randn(d + 1)
    else:
        y = rng.randint(0, K, n)
        lab = torch.from_numpy(y.astype(np.int64)).to(dev)
        W = torch.from_numpy(0.01 * rng.randn(K, d)).to(dev)
        b = torch.from_numpy(0.01 * rng.randn(K)).to(dev)
        Wt = S.transposed_weights(W, dev)
        emit(what="logit_multi", ms=median_ms(lambda: S.logit_multi(sd, Wt, b, lab, sw),
                                              reps=a.reps), **base)
        emit(what="logit_multi_composed",
             ms=median_ms(lambda: composed_multi(sd, W, b, lab, sw), reps=a.reps), **base)
        R = S.logit_multi(sd, Wt, b, lab, sw)[1]
        emit(what="logit_multi_vs_composed",
             max_abs=float((R - composed_multi(sd, W, b, lab, sw)[1]).abs().max()), **base)
        emit(what="gradient_sp_xty", ms=median_ms(lambda: SL.sp_xty(sd, R), reps=a.reps), **base)
        obj = _SparseObjective(sd, y, K, np.ones(n), 1.0, True, True)
        w0 = 0.01 * rng.randn(K * (d + 1))
    obj.smooth(w0)
    emit(what="objective_evaluation",
         seconds=float(np.median([wall(lambda: obj.smooth(w0))[0] for _ in range(a.reps)])), **base)
    if a.kernels_only:
        return
    kw = dict(max_iter=a.iters, tol=1e-4)
    yy = y
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        LogisticRegression(device="cuda", **dict(kw, max_iter=1)).fit(X, yy)
        runs = [wall(lambda: LogisticRegression(device="cuda", **kw).fit(X, yy)) for _ in range(3)]
        t_fit, est = sorted(runs, key=lambda r: r[0])[1]
        emit(what="fit", path="cuda", iters=int(est.n_iter_.max()), seconds=t_fit, **base)
        if a.host and n * d * 8 <= HOST_DENSE_BYTES:
            t_h, est = wall(lambda: LogisticRegression(device=None, **kw).fit(X, yy))
            emit(what="fit", path="host (densifies)", iters=int(est.n_iter_.max()), seconds=t_h,
                 **base)
            t_h, est = wall(lambda: LogisticRegression(device="cuda", **kw).fit(X.toarray(), yy))
            emit(what="fit", path="cuda on dense rows", iters=int(est.n_iter_.max()), seconds=t_h,
                 **base)
        if a.sklearn:
            import sklearn.linear_model as SK
            t_s, est = wall(lambda: SK.LogisticRegression(**kw).fit(X, yy))
            emit(what="fit", path="sklearn", iters=int(est.n_iter_.max()), seconds=t_s, **base)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", default="small", choices=sorted(SHAPES))
    p.add_argument("--classes", type=int, nargs="+", default=[1, 20],
                   help="1: the binary problem; more: the multinomial problem")
    p.add_argument("--iters", type=int, default=30, help="max_iter of the fits")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--host", action="store_true")
    p.add_argument("--sklearn", action="store_true")
    a = p.parse_args()
    for K in a.classes:
        run(a.shape, K, a)


if __name__ == "__main__":
    main()
