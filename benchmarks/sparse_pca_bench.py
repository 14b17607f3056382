"""Sparse (CSR) PCA / qPCA benchmark on the synthetic TF-IDF-like matrix of
``sparse_kmeans_bench.make_csr`` (the shapes of ``sparse_svd_bench.py``):

* the mu(A) power sums of the centred matrix (``sp_mu_power_sums``,
  csrc/spmu.hip: row pass and column pass; ``--mu-only`` under
  ``rocprofv3 --kernel-trace --stats`` gives the two passes' own times) next
  to the torch route composed from one ``index_add_`` per exponent and side;
* the centred randomized fit (``PCA``) next to the uncentred ``TruncatedSVD``
  fit of the same matrix with the same iteration count, so the cost of
  centring is visible;
* the whole ``qPCA(quantum_truncated=True)`` fit by phase;
* scikit-learn's CPU ``PCA(svd_solver='arpack')`` on the same CSR.

    python benchmarks/sparse_pca_bench.py --shape small --torch-route --sklearn

``--cpu-only`` runs just the scikit-learn baseline (no GPU needed).  Prints
one JSON line per measurement; ``profiles/sparse_pca.md`` records a run.
There is no pass/fail time.
"""

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

from sparse_kmeans_bench import make_csr, timed                        # noqa: E402
from sparse_svd_bench import SHAPES, N_ITER                             # noqa: E402
from sq_learn_amd.models._data import (_mu_grid, as_sparse_data,        # noqa: E402
                                       sparse_mean_var)
from sq_learn_amd.models.decomposition import PCA, TruncatedSVD, qPCA   # noqa: E402
from sq_learn_amd.ops import sparse_linalg as SL                        # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def torch_mu_route(sd, exps, mean):
    """The power sums from torch ops alone: one ``index_add_`` per exponent
    and side (a floating-point atomic), an nnz-sized temporary each."""
    n, d = sd.shape
    cols, rows = sd.indices.to(torch.int64), sd.row_ids()
    a = (sd.data.double() - mean[cols]).abs()
    am = mean.abs()
    la = torch.log(torch.where(a > 0, a, torch.ones_like(a)))
    lm = torch.log(torch.where(am > 0, am, torch.ones_like(am)))
    cnt = torch.bincount(cols, minlength=d)
    rowmax, colsum = [], []
    for q in exps:
        pa = torch.where(a > 0, torch.exp(q * la), torch.zeros_like(a))
        pm = torch.where(am > 0, torch.exp(q * lm), torch.zeros_like(am))
        rs = torch.full((n,), float(pm.sum()), dtype=torch.float64, device=a.device)
        rs.index_add_(0, rows, pa - pm[cols])
        cs = (n - cnt) * pm
        cs.index_add_(0, cols, pa)
        rowmax.append(rs.max())
        colsum.append(cs)
    return torch.stack(rowmax), torch.stack(colsum)


def wall(make, X):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        make().fit(X)                                  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        est = make().fit(X)
        torch.cuda.synchronize()
    return time.perf_counter() - t0, est


def sklearn_fit(X, k, name):
    from sklearn.decomposition import PCA as SkPCA
    t0 = time.perf_counter()
    ref = SkPCA(k, svd_solver="arpack").fit(X)
    emit(shape=name, what="sklearn_cpu_pca_arpack_fit", s=round(time.perf_counter() - t0, 3),
         sv_first=float(ref.singular_values_[0]), sv_last=float(ref.singular_values_[-1]),
         threads=os.environ.get("OMP_NUM_THREADS", "default"))


def run(name, a):
    n, d, k = SHAPES[name]
    l = k + 10
    t0 = time.perf_counter()
    X = make_csr(n, d)
    emit(shape=name, n=n, d=d, components=k, l=l, n_iter=N_ITER, nnz=int(X.nnz),
         longest_column=int(np.bincount(X.indices, minlength=d).max()),
         gen_s=round(time.perf_counter() - t0, 2))
    if a.cpu_only:
        sklearn_fit(X, k, name)
        return
    sd = as_sparse_data(X, device="cuda")
    SL.csr_transpose(sd)
    mean = sparse_mean_var(sd)[0]
    _, exps = _mu_grid(0, 1.0, 0.1)
    nq = len(exps)
    rm, cs = SL.sp_mu_power_sums(sd, exps, mean=mean)
    ms = timed(lambda: SL.sp_mu_power_sums(sd, exps, mean=mean))
    # per stored value and side: 8 bytes of (index, value) read, one log and one exp
    emit(shape=name, what="sp_mu_power_sums_centred", nq=nq, ms=round(ms, 3),
         stored_values_per_us=round(2 * sd.nnz / ms / 1e3, 1))
    ms = timed(lambda: SL.sp_mu_power_sums(sd, exps))
    emit(shape=name, what="sp_mu_power_sums_uncentred", nq=nq, ms=round(ms, 3))
    if a.mu_only:
        return
    if a.torch_route:
        # one timed call after the one that gives the values: the atomics of the long columns
        # make a call take seconds
        tr, tc = torch_mu_route(sd, exps, mean)
        ms = timed(lambda: torch_mu_route(sd, exps, mean), warmup=0, reps=1)
        emit(shape=name, what="torch_index_add_route", nq=nq, ms=round(ms, 3),
             rowmax_max_rel_gap=float(((tr - rm).abs() / rm).max()),
             colsum_max_rel_gap=float(((tc - cs).abs() / cs.clamp(min=1e-300)).max()))
        del tr, tc
    del rm, cs
    mk = dict(n_components=k, random_state=0, device="cuda")
    s_u, _ = wall(lambda: TruncatedSVD(n_iter=N_ITER, **mk), X)
    emit(shape=name, what="truncated_svd_fit_uncentred", s=round(s_u, 3))
    s_c, est = wall(lambda: PCA(svd_solver="randomized", iterated_power=N_ITER, **mk), X)
    emit(shape=name, what="pca_fit_centred", s=round(s_c, 3), over_uncentred_s=round(s_c - s_u, 3),
         sv_first=float(est.singular_values_[0]), sv_last=float(est.singular_values_[-1]))
    os.environ["SQ_QPCA_PHASES"] = "1"
    s_q, q = wall(lambda: qPCA(svd_solver="randomized", iterated_power=N_ITER,
                               quantum_truncated=True, **mk), X)
    os.environ.pop("SQ_QPCA_PHASES")
    emit(shape=name, what="qpca_fit_quantum_truncated", s=round(s_q, 3), norm_muA=q.norm_muA,
         muA=float(q.muA), phases={p: round(v, 4) for p, v in q.fit_phases_.items()})
    if a.sklearn:
        sklearn_fit(X, k, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["big", "small", "both", "tiny"], default="small")
    ap.add_argument("--mu-only", action="store_true")
    ap.add_argument("--torch-route", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--cpu-only", action="store_true")
    a = ap.parse_args()
    for name in (["big", "small"] if a.shape == "both" else [a.shape]):
        run(name, a)


if __name__ == "__main__":
    main()
