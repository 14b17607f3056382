"""Sparse (CSR) LS-SVM benchmark: the kernel-matrix kernels of
``ops.sparse_kernel`` (``csrc/spgram.hip``) and whole ``LSSVC`` fits on the
synthetic TF-IDF-like matrix of ``sparse_kmeans_bench.make_csr`` (Zipf column
draws, so long columns exist; L2-normalised rows), next to the routes that
existed before:

* ``sp_kernel_matrix`` (rbf) next to (a) ``sp_knn`` dist mode (the same
  accumulate phase, squared distances to memory) plus the ``exp`` epilogue in
  torch and (b) densified rows plus the fp64 GEMM of ``utils.pairwise``;
* the fused build of the LS-SVM matrix F (K, I / penalty and the placement in
  one pass) next to K, ``eye`` and the copy;
* ``sp_kernel_matvec`` next to forming the block and ``matmul``;
* whole ``classic`` / ``cg`` / matrix-free ``cg`` fits and
  ``decision_function`` next to the same estimator on ``X.toarray()``.

    python benchmarks/lssvc_sparse_bench.py --shape small

Prints one JSON line per measurement (medians over ``--reps`` runs after a
warm-up); ``profiles/lssvc_sparse.md`` records a run.  There is no pass/fail
time.
"""

import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

from sparse_kmeans_bench import emit, make_csr               # noqa: E402
from sparse_knn_bench import inverted_work, median_ms, median_wall   # noqa: E402
from sq_learn_amd.models._data import as_sparse_data         # noqa: E402
from sq_learn_amd.models.svm.lssvm import LSSVC              # noqa: E402
from sq_learn_amd.ops import _native as nat                  # noqa: E402
from sq_learn_amd.ops import sparse_kernel as SPK            # noqa: E402
from sq_learn_amd.ops import sparse_knn as SK                # noqa: E402
from sq_learn_amd.utils import pairwise as PW                # noqa: E402

# (fit rows, columns, queries)
SHAPES = {"text": (16384, 100_000, 2048), "small": (4096, 20_000, 2048),
          "tiny": (1024, 2000, 256)}
GAMMA, PENALTY = 0.5, 1.0


def knn_dist_epilogue(op, block, m, gamma):
    """Route (a): squared distances by ``sp_knn`` dist mode, ``exp`` in torch."""
    op.lib.sp_knn(*op.args(0, m), 0, 0, 1, 0, 0, block.data_ptr(), 0, 0,
                  nat.stream_handle(block.device))
    return torch.exp(-gamma * block)


def dense_gemm(fit_sd, qry_sd, gamma):
    """Route (b): both sides densified (fp64), the GEMM path of ``utils.pairwise``."""
    Xd = fit_sd.dense_rows(0, fit_sd.shape[0])
    Qd = qry_sd.dense_rows(0, qry_sd.shape[0])
    return PW.rbf_kernel(Qd, Xd, gamma=gamma)


def composed_F(fit_sd, op, penalty, kind, kw):
    """The LS-SVM matrix as the dense path builds it: K, then eye and the copy."""
    N = fit_sd.shape[0]
    K = SPK.sp_kernel_matrix(fit_sd, fit_sd, kind, op=op, **kw)
    F = torch.zeros((N + 1, N + 1), dtype=torch.float64, device=K.device)
    F[0, 1:] = 1.0
    F[1:, 0] = 1.0
    F[1:, 1:] = K + (1.0 / penalty) * torch.eye(N, dtype=torch.float64, device=K.device)
    return F


def fused_F(fit_sd, op, penalty, kind, kw):
    N = fit_sd.shape[0]
    F = torch.empty((N + 1, N + 1), dtype=torch.float64, device=fit_sd.device)
    F[0, 0] = 0.0
    F[0, 1:] = 1.0
    F[1:, 0] = 1.0
    SPK.sp_kernel_matrix(fit_sd, fit_sd, kind, out=F[1:, 1:], diag_add=1.0 / penalty, op=op, **kw)
    return F


def run(name, a):
    n, d, m = SHAPES[name]
    t0 = time.perf_counter()
    X = make_csr(n + m, d)
    fit, qry = X[:n], X[n:]
    w = np.random.RandomState(1).standard_normal(d)
    y = np.where(fit @ w >= np.median(fit @ w), 1.0, -1.0)
    emit(shape=name, n=n, d=d, queries=m, nnz_fit=int(fit.nnz), nnz_query=int(qry.nnz),
         inverted_madds_queries=inverted_work(fit, qry), inverted_madds_self=inverted_work(fit, fit),
         dense_madds_queries=float(n) * m * d, gen_s=round(time.perf_counter() - t0, 2))
    fit_sd = as_sparse_data(fit, device="cuda")
    qry_sd = as_sparse_data(qry, device="cuda")
    kw = dict(gamma=GAMMA, coef0=1.0, degree=3.0)
    op_q = SK.InvertedIndex(fit_sd, qry_sd, SK.TILE_DEFAULT)
    op_s = SK.InvertedIndex(fit_sd, fit_sd, SK.TILE_DEFAULT)
    torch.cuda.synchronize()

    # ---- matrix mode, queries against the fit set
    for kind in ("linear", "poly", "rbf", "sigmoid"):
        ms = median_ms(lambda: SPK.sp_kernel_matrix(fit_sd, qry_sd, kind, op=op_q, **kw),
                       reps=a.reps)
        emit(shape=name, what="sp_kernel_matrix", kind=kind, rows=m, ms=round(ms, 3),
             GBps_written=round(8.0 * m * n / ms / 1e6, 1))
    for tile in (1024, 2048, 4096):
        if tile >= SK.TILE_DEFAULT:
            continue
        ms = median_ms(lambda: SPK.sp_kernel_matrix(fit_sd, qry_sd, "rbf", tile=tile, **kw),
                       reps=a.reps)
        emit(shape=name, what="sp_kernel_matrix_with_operands", kind="rbf", tile=tile,
             ms=round(ms, 3))
    ms_op = median_ms(lambda: SPK.sp_kernel_matrix(fit_sd, qry_sd, "rbf", **kw), reps=a.reps)
    emit(shape=name, what="sp_kernel_matrix_with_operands", kind="rbf", tile=SK.TILE_DEFAULT,
         ms=round(ms_op, 3))
    block = torch.empty((m, n), dtype=torch.float64, device="cuda")
    K = SPK.sp_kernel_matrix(fit_sd, qry_sd, "rbf", op=op_q, **kw)
    Ka = knn_dist_epilogue(op_q, block, m, GAMMA)
    ms = median_ms(lambda: knn_dist_epilogue(op_q, block, m, GAMMA), reps=a.reps)
    emit(shape=name, what="sp_knn_dist_plus_torch_exp", kind="rbf", ms=round(ms, 3),
         max_abs_diff=float((Ka - K).abs().max()))
    if (n + m) * d * 8 <= a.dense_bytes:
        Kb = dense_gemm(fit_sd, qry_sd, GAMMA)
        ms = median_ms(lambda: dense_gemm(fit_sd, qry_sd, GAMMA), reps=a.reps)
        emit(shape=name, what="densify_plus_gemm", kind="rbf", ms=round(ms, 3),
             max_abs_diff=float((Kb - K).abs().max()))
        del Kb
    del Ka, block

    # ---- the LS-SVM matrix
    for kind in ("linear", "rbf"):
        Ff = fused_F(fit_sd, op_s, PENALTY, kind, kw)
        Fc = composed_F(fit_sd, op_s, PENALTY, kind, kw)
        same = bool(torch.equal(Ff, Fc))
        del Ff, Fc
        ms_f = median_ms(lambda: fused_F(fit_sd, op_s, PENALTY, kind, kw), reps=a.reps)
        ms_c = median_ms(lambda: composed_F(fit_sd, op_s, PENALTY, kind, kw), reps=a.reps)
        emit(shape=name, what="F_build", kind=kind, fused_ms=round(ms_f, 3),
             k_eye_copy_ms=round(ms_c, 3), equal=same)

    # ---- apply mode
    for kind in ("linear", "rbf"):
        for R in (1, 2, 4):
            V = torch.randn((n, R), dtype=torch.float64, device="cuda")
            for label, sd, op in (("queries", qry_sd, op_q), ("self", fit_sd, op_s)):
                ms_a = median_ms(lambda: SPK.sp_kernel_matvec(fit_sd, sd, V, kind, op=op, **kw),
                                 reps=a.reps)
                ms_b = median_ms(lambda: SPK.sp_kernel_matrix(fit_sd, sd, kind, op=op, **kw) @ V,
                                 reps=a.reps)
                emit(shape=name, what="sp_kernel_matvec", kind=kind, R=R, side=label,
                     apply_ms=round(ms_a, 3), form_block_matmul_ms=round(ms_b, 3))

    # ---- whole estimators
    est_kw = dict(kernel="rbf", penalty=PENALTY, gamma=GAMMA, device="cuda")
    dense_ok = (n + m) * d * 8 <= a.dense_bytes
    Xd, Qd = (fit.toarray(), qry.toarray()) if dense_ok else (None, None)
    for algo, env in (("classic", None), ("cg", None), ("cg", "0")):
        if algo == "classic" and n > a.classic_rows:
            continue
        if env is None:
            os.environ.pop("SQ_SVM_DENSE_BYTES", None)
        else:
            os.environ["SQ_SVM_DENSE_BYTES"] = env
        s_sp = median_wall(lambda: LSSVC(algorithm=algo, **est_kw).fit(fit, y), reps=a.fit_reps)
        est = LSSVC(algorithm=algo, **est_kw).fit(fit, y)
        line = dict(shape=name, what="LSSVC_fit", algorithm=algo,
                    matrix_free=env == "0", csr_s=round(s_sp, 4),
                    train_accuracy=float(np.mean(est.predict(fit) == y)))
        os.environ.pop("SQ_SVM_DENSE_BYTES", None)
        if dense_ok and env is None:
            s_d = median_wall(lambda: LSSVC(algorithm=algo, **est_kw).fit(Xd, y), reps=a.fit_reps)
            ref = LSSVC(algorithm=algo, **est_kw).fit(Xd, y)
            line.update(densified_s=round(s_d, 4),
                        max_alpha_diff=float(np.abs(ref.alpha_ - est.alpha_).max()))
        emit(**line)
    est = LSSVC(algorithm="cg", **est_kw).fit(fit, y)
    s_sp = median_wall(lambda: est.decision_function(qry), reps=a.fit_reps)
    line = dict(shape=name, what="decision_function", queries=m, csr_s=round(s_sp, 4))
    if dense_ok:
        ref = LSSVC(algorithm="cg", **est_kw).fit(Xd, y)
        s_d = median_wall(lambda: ref.decision_function(Qd), reps=a.fit_reps)
        line.update(densified_s=round(s_d, 4), max_diff=float(np.abs(
            ref.decision_function(Qd) - est.decision_function(qry)).max()))
    emit(**line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small",
                    help="comma-separated names of " + ", ".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--classic-rows", type=int, default=8192,
                    help="largest fit set the O(N^3) classic fit is timed on")
    ap.add_argument("--dense-bytes", type=int, default=8 << 30,
                    help="largest fp64 densified input the dense routes are timed on")
    a = ap.parse_args()
    for name in a.shape.split(","):
        run(name, a)


if __name__ == "__main__":
    main()
