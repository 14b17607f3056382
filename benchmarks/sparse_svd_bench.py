"""Sparse (CSR) TruncatedSVD benchmark: one ``sp_xw``, one ``sp_xty``, the
transpose build and whole ``TruncatedSVD`` fits (with the host QR share) on
the synthetic TF-IDF-like matrix of ``sparse_kmeans_bench.make_csr`` (Zipf
column draws, so long columns exist), next to ``torch.sparse.mm`` on the same
CSR in fp64, the dense path on ``X.toarray()`` (second shape only) and
scikit-learn's CPU ``TruncatedSVD``.

    python benchmarks/sparse_svd_bench.py --shape small --torch-sparse --dense --sklearn

``--cpu-only`` runs just the scikit-learn baseline (no GPU needed).  Prints
one JSON line per measurement; ``profiles/sparse_svd.md`` records a run.
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

from sparse_kmeans_bench import make_csr, timed            # noqa: E402
from sq_learn_amd.models._data import as_sparse_data        # noqa: E402
from sq_learn_amd.models.decomposition import TruncatedSVD  # noqa: E402
from sq_learn_amd.ops import sparse_linalg as SL            # noqa: E402

# (n, d, components); l = components + 10 range vectors
SHAPES = {"big": (1_000_000, 100_000, 100), "small": (200_000, 4096, 100),
          "tiny": (3000, 2000, 10)}
N_ITER = 5


def emit(**kw):
    print(json.dumps(kw), flush=True)


class HostQR:
    """Wall clock spent inside ``torch.linalg.qr`` (the per-iteration d x l
    factorisation on the host; its input is already on the host, so no device
    wait is counted)."""

    def __enter__(self):
        self.seconds, self.calls = 0.0, 0
        self._qr = torch.linalg.qr

        def qr(*a, **kw):
            t0 = time.perf_counter()
            out = self._qr(*a, **kw)
            self.seconds += time.perf_counter() - t0
            self.calls += 1
            return out
        torch.linalg.qr = qr
        return self

    def __exit__(self, *exc):
        torch.linalg.qr = self._qr


def fit_time(X, k, device="cuda"):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        TruncatedSVD(k, n_iter=N_ITER, random_state=0, device=device).fit(X)     # warm-up
        torch.cuda.synchronize()
        with HostQR() as qr:
            t0 = time.perf_counter()
            est = TruncatedSVD(k, n_iter=N_ITER, random_state=0, device=device).fit(X)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
    return s, qr, est


def sklearn_fit(X, k, name):
    from sklearn.decomposition import TruncatedSVD as SkSVD
    t0 = time.perf_counter()
    ref = SkSVD(k, n_iter=N_ITER, random_state=0).fit(X)
    emit(shape=name, what="sklearn_cpu_truncated_svd_fit", s=round(time.perf_counter() - t0, 3),
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
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t = SL.csr_transpose(sd)
    torch.cuda.synchronize()
    emit(shape=name, what="transpose_build_first", s=round(time.perf_counter() - t0, 4))

    def rebuild():
        sd._transpose = None
        SL.csr_transpose(sd)
    emit(shape=name, what="transpose_build", ms=round(timed(rebuild, warmup=1, reps=3), 3))
    t0 = time.perf_counter()
    tabs = SL.segments(sd), SL.segments(t)
    torch.cuda.synchronize()
    emit(shape=name, what="segment_tables", s=round(time.perf_counter() - t0, 4),
         seg=SL.SEG_DEFAULT, x_segments=tabs[0].nseg, x_long_rows=tabs[0].nlong,
         xt_segments=tabs[1].nseg, xt_long_rows=tabs[1].nlong, xt_partials=tabs[1].slots)
    g = torch.Generator(device="cuda").manual_seed(0)
    W = torch.randn((d, l), dtype=torch.float64, device="cuda", generator=g)
    Y = torch.empty((n, l), dtype=torch.float64, device="cuda")
    ms = timed(lambda: SL.sp_xw(sd, W, out=Y))
    # every stored value gathers one row of the dense operand: 8 l bytes requested
    emit(shape=name, what="sp_xw", ms=round(ms, 3),
         gather_TBps=round(sd.nnz * 8.0 * l / ms / 1e9, 3),
         gflops=round(2.0 * sd.nnz * l / ms / 1e6, 1))
    ms = timed(lambda: SL.sp_xty(sd, Y))
    emit(shape=name, what="sp_xty", ms=round(ms, 3),
         gather_TBps=round(sd.nnz * 8.0 * l / ms / 1e9, 3),
         gflops=round(2.0 * sd.nnz * l / ms / 1e6, 1))
    s1, s2 = SL.sp_col_moments(sd)
    emit(shape=name, what="sp_col_moments", ms=round(timed(lambda: SL.sp_col_moments(sd)), 3))
    if a.torch_sparse:
        try:
            A = torch.sparse_csr_tensor(sd.indptr, sd.indices.to(torch.int64), sd.data.double(),
                                        size=(n, d))
            ref = torch.sparse.mm(A, W)
            gap = float((ref - SL.sp_xw(sd, W)).abs().max())
            ms = timed(lambda: torch.sparse.mm(A, W))
            emit(shape=name, what="torch_sparse_mm_xw_fp64", ms=round(ms, 3), max_abs_gap=gap)
            At = torch.sparse_csr_tensor(t.indptr, t.indices.to(torch.int64), t.data.double(),
                                         size=(d, n))
            ms = timed(lambda: torch.sparse.mm(At, Y))
            emit(shape=name, what="torch_sparse_mm_xty_fp64", ms=round(ms, 3))
            del A, At, ref
        except Exception as e:       # this torch build may lack the fp64 CSR product
            emit(shape=name, what="torch_sparse_mm_fp64", error=f"{type(e).__name__}: {e}"[:200])
    del W, Y
    s, qr, est = fit_time(X, k)
    emit(shape=name, what="truncated_svd_fit_sparse", s=round(s, 3),
         host_qr_s=round(qr.seconds, 3), host_qr_calls=qr.calls,
         host_qr_share=round(qr.seconds / s, 3), sv_first=float(est.singular_values_[0]),
         sv_last=float(est.singular_values_[-1]),
         evr_sum=float(est.explained_variance_ratio_.sum()))
    if a.dense and n * d * 4 <= 4 << 30:
        Xd = X.toarray()
        s, qr, estd = fit_time(Xd, k)
        emit(shape=name, what="truncated_svd_fit_dense_array", s=round(s, 3),
             host_qr_s=round(qr.seconds, 3), host_qr_calls=qr.calls,
             sv_first=float(estd.singular_values_[0]), sv_last=float(estd.singular_values_[-1]),
             sv_max_rel_gap=float(np.abs(estd.singular_values_ / est.singular_values_ - 1).max()))
        del Xd
    if a.sklearn:
        sklearn_fit(X, k, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["big", "small", "both", "tiny"], default="small")
    ap.add_argument("--torch-sparse", action="store_true")
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--cpu-only", action="store_true")
    a = ap.parse_args()
    for name in (["big", "small"] if a.shape == "both" else [a.shape]):
        run(name, a)


if __name__ == "__main__":
    main()
