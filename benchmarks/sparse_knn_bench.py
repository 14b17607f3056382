"""Sparse (CSR) brute-force k-NN benchmark: the tile table build, the
inverted-index kernel per query chunk (``ops.sparse_knn.sp_knn``) over a list
of tile sizes and whole ``NearestNeighbors.kneighbors`` calls on the synthetic
TF-IDF-like matrix of ``sparse_kmeans_bench.make_csr`` (Zipf column draws, so
long columns exist; L2-normalised rows), next to

(a) the composed route on existing kernels: a query chunk densified into
    ``W = Q^T`` [d, m_chunk], ``sp_xw(fit, W)`` (work nnz(X) * m_chunk, an
    n x m_chunk fp64 block), the distance epilogue in torch and ``knn_topk``;
(b) the dense estimator on ``X.toarray()`` where that fits;
(c) scikit-learn's CPU ``NearestNeighbors(algorithm='brute')`` on the same CSR.

    python benchmarks/sparse_knn_bench.py --shape small --composed --dense --sklearn

``--cpu-only`` runs just the scikit-learn baseline (no GPU needed).  Prints
one JSON line per measurement (medians over ``--reps`` runs after warm-up);
``profiles/sparse_knn.md`` records a run.  There is no pass/fail time.
"""

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

from sparse_kmeans_bench import emit, make_csr               # noqa: E402
from sq_learn_amd.models._data import as_sparse_data         # noqa: E402
from sq_learn_amd.models.neighbors import NearestNeighbors   # noqa: E402
from sq_learn_amd.models.neighbors.knn import _topk_rows     # noqa: E402
from sq_learn_amd.ops import sparse_knn as SK                # noqa: E402
from sq_learn_amd.ops import sparse_linalg as SL             # noqa: E402
from sq_learn_amd.ops.sparse_kmeans import sp_row_norms      # noqa: E402

# (fit rows, columns, queries)
SHAPES = {"big": (1_000_000, 100_000, 1024), "text": (200_000, 100_000, 2048),
          "small": (200_000, 4096, 2048), "tiny": (3000, 2000, 64)}
K = 10


def median_ms(fn, warmup=1, reps=5):
    """Median device time of ``fn`` in ms (one event pair per run)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def median_wall(fn, warmup=1, reps=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def inverted_work(fit, qry):
    """sum_c nnz_q(c) * nnz_x(c): the multiply-adds of the inverted index."""
    cx = np.bincount(fit.indices, minlength=fit.shape[1]).astype(np.float64)
    cq = np.bincount(qry.indices, minlength=fit.shape[1]).astype(np.float64)
    return float(cx @ cq)


def composed(fit_sd, qry_sd, xn, qn, k, chunk):
    """Route (a) over all the queries, ``chunk`` at a time: (D fp32 squared,
    idx int64)."""
    n = fit_sd.shape[0]
    m = qry_sd.shape[0]
    ds, ix = [], []
    G = torch.empty((n, chunk), dtype=torch.float64, device=fit_sd.device)
    for a in range(0, m, chunk):
        b = min(m, a + chunk)
        W = qry_sd.dense_rows(a, b).T                      # [d, mc] fp64
        g = SL.sp_xw(fit_sd, W, out=G)                     # [n, mc]
        D = ((xn[:, None] + qn[None, a:b]) - 2.0 * g).clamp_(min=0).T.float().contiguous()
        v, i = _topk_rows(D, k)
        ds.append(v)
        ix.append(i)
    return torch.cat(ds), torch.cat(ix)


def sklearn_knn(fit, qry, name, metric, mq):
    from sklearn.neighbors import NearestNeighbors as SkNN
    ref = SkNN(n_neighbors=K, algorithm="brute", metric=metric).fit(fit)
    q = qry[:mq]
    s = median_wall(lambda: ref.kneighbors(q), warmup=0, reps=3)
    emit(shape=name, what="sklearn_cpu_brute_kneighbors", metric=metric, queries=int(q.shape[0]),
         s=round(s, 3), ms_per_query=round(1e3 * s / q.shape[0], 3),
         threads=os.environ.get("OMP_NUM_THREADS", "default"), cpus=os.cpu_count())
    return ref.kneighbors(q)


def run(name, a):
    n, d, m = SHAPES[name]
    t0 = time.perf_counter()
    X = make_csr(n + m, d)
    fit, qry = X[:n], X[n:]
    emit(shape=name, n=n, d=d, queries=m, k=K, nnz_fit=int(fit.nnz), nnz_query=int(qry.nnz),
         longest_column=int(np.bincount(fit.indices, minlength=d).max()),
         inverted_madds=inverted_work(fit, qry), gather_madds=float(fit.nnz) * m,
         gen_s=round(time.perf_counter() - t0, 2))
    if a.cpu_only:
        for metric in ("euclidean", "cosine"):
            sklearn_knn(fit, qry, name, metric, a.sklearn_queries)
        return
    fit_sd = as_sparse_data(fit, device="cuda")
    qry_sd = as_sparse_data(qry, device="cuda")
    xn, qn = sp_row_norms(fit_sd), sp_row_norms(qry_sd)
    SL.csr_transpose(fit_sd)
    torch.cuda.synchronize()
    tiles = [int(t) for t in a.tiles.split(",")]
    if SK.TILE_DEFAULT not in tiles:
        tiles.append(SK.TILE_DEFAULT)
    base = None
    for tile in tiles:
        def rebuild():
            fit_sd._knn_tables.pop(tile, None)
            SK.tile_table(fit_sd, tile)
        ms_tab = median_ms(rebuild, warmup=1, reps=3)
        tab = SK.tile_table(fit_sd, tile)
        ms = median_ms(lambda: SK.sp_knn(fit_sd, qry_sd, K, tile=tile, xn=xn, qn=qn),
                       reps=a.reps)
        emit(shape=name, what="sp_knn", metric="euclidean", tile=tile,
             table_build_ms=round(ms_tab, 3), table_MB=round(tab.numel() * 8 / 2 ** 20, 1),
             ms=round(ms, 3),
             ms_per_query=round(ms / m, 4), default=tile == SK.TILE_DEFAULT)
        if tile == SK.TILE_DEFAULT:
            base = ms
    Dn, In = SK.sp_knn(fit_sd, qry_sd, K, xn=xn, qn=qn)
    ms = median_ms(lambda: SK.sp_knn(fit_sd, qry_sd, K, metric="cosine", xn=xn, qn=qn),
                   reps=a.reps)
    emit(shape=name, what="sp_knn", metric="cosine", tile=SK.TILE_DEFAULT, ms=round(ms, 3),
         ms_per_query=round(ms / m, 4))
    mq = min(m, 256)
    q_small = as_sparse_data(qry[:mq], device="cuda")
    ms = median_ms(lambda: SK.sp_knn(fit_sd, q_small, 64, xn=xn, qn=qn[:mq]), reps=3)
    emit(shape=name, what="sp_knn_dist_mode_topk", kk=64, queries=mq, ms=round(ms, 3),
         ms_per_query=round(ms / mq, 4))
    # whole estimator calls (host conversion of the queries, norms, exponents,
    # kernel, the copy back)
    t0 = time.perf_counter()
    nn = NearestNeighbors(n_neighbors=K, device="cuda").fit(fit)
    nn.kneighbors(qry[:8])                                  # builds transpose and table
    torch.cuda.synchronize()
    emit(shape=name, what="fit_and_first_query", s=round(time.perf_counter() - t0, 3))
    s = median_wall(lambda: nn.kneighbors(qry))
    emit(shape=name, what="kneighbors_sparse", queries=m, s=round(s, 4),
         ms_per_query=round(1e3 * s / m, 4), kernel_share=round(base / (1e3 * s), 3))
    if a.composed:
        mc = min(m, a.composed_queries)
        q_c = as_sparse_data(qry[:mc], device="cuda")
        chunk = min(mc, a.composed_chunk)
        fn = lambda: composed(fit_sd, q_c, xn, qn[:mc], K, chunk)           # noqa: E731
        Dc, Ic = fn()
        same = float((Ic == In[:mc]).double().mean())
        ms = median_ms(fn, warmup=1, reps=3)
        emit(shape=name, what="composed_spxw_topk", queries=mc, chunk=chunk, ms=round(ms, 3),
             ms_per_query=round(ms / mc, 4), index_agreement=round(same, 5),
             sp_knn_speedup=round((ms / mc) / (base / m), 2))
        del Dc, Ic
    if a.dense and n * d * 4 <= 4 << 30:
        Xd, Qd = fit.toarray(), qry.toarray()
        dn = NearestNeighbors(n_neighbors=K, device="cuda").fit(Xd)
        s = median_wall(lambda: dn.kneighbors(Qd))
        same = float((dn.kneighbors(Qd)[1] == In.cpu().numpy()).mean())
        emit(shape=name, what="kneighbors_dense_array", queries=m, s=round(s, 4),
             ms_per_query=round(1e3 * s / m, 4), index_agreement=round(same, 5))
        del Xd, Qd, dn
    if a.sklearn:
        _, ind = sklearn_knn(fit, qry, name, "euclidean", a.sklearn_queries)
        same = float((ind == In[:ind.shape[0]].cpu().numpy()).mean())
        emit(shape=name, what="sklearn_index_agreement", value=round(same, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small",
                    help="comma-separated names of " + ", ".join(SHAPES))
    ap.add_argument("--tiles", default="1024,2048,4096,8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed", action="store_true")
    ap.add_argument("--composed-queries", type=int, default=256)
    ap.add_argument("--composed-chunk", type=int, default=128)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-queries", type=int, default=256)
    ap.add_argument("--cpu-only", action="store_true")
    a = ap.parse_args()
    for name in a.shape.split(","):
        run(name, a)


if __name__ == "__main__":
    main()
