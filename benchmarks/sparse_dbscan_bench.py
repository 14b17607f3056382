"""Sparse (CSR) radius neighbours and DBSCAN benchmark: the mark kernel of
``ops.sparse_radius`` over a list of tile sizes, the fill kernel, whole
``sp_radius`` calls and a whole ``DBSCAN.fit`` on the synthetic TF-IDF-like
matrix of ``sparse_kmeans_bench.make_csr`` (the shapes of
``sparse_knn_bench.py``).  The join is a self-join: the queries are the first
``--queries`` fit rows, and the squared-euclidean threshold is the median
distance of a query to its ``--neighbours``-th nearest fit row, so a row has
on the order of that many neighbours.  Next to it

(a) the route composed from what existed before: the sparse k-NN kernel in
    dist mode (an fp64 [rows, n] block), ``<= thr`` and ``nonzero`` in torch,
    the lists copied to the host as ``sp_radius`` does;
(b) ``DBSCAN.fit`` on ``X.toarray()`` (the densifying path) where that fits;
(c) scikit-learn's brute-force ``radius_neighbors`` on the same CSR (CPU).

    python benchmarks/sparse_dbscan_bench.py --shape small --composed --dense --sklearn

Prints one JSON line per measurement (medians over ``--reps`` event pairs
after a warm-up; fits and scikit-learn by the host clock);
``profiles/sparse_dbscan.md`` records a run.  There is no pass/fail time.
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
from sparse_knn_bench import SHAPES, median_ms, median_wall  # noqa: E402
from sq_learn_amd.cluster import DBSCAN                      # noqa: E402
from sq_learn_amd.models._data import as_sparse_data         # noqa: E402
from sq_learn_amd.ops import _native as nat                  # noqa: E402
from sq_learn_amd.ops import sparse_knn as SK                # noqa: E402
from sq_learn_amd.ops import sparse_radius as SR             # noqa: E402
from sq_learn_amd.ops.sparse_kmeans import sp_row_norms      # noqa: E402


def composed(fit_sd, q_sd, thr, xn, qn, chunk):
    """Route (a): (indptr, indices) on the host through dist-mode blocks."""
    n, d = fit_sd.shape
    m = q_sd.shape[0]
    tile = SK.TILE_DEFAULT
    tab = SK.tile_table(fit_sd, tile)
    t = SK.csr_transpose(fit_sd)
    qexp = SK.query_exps(q_sd, float(fit_sd.data.abs().max()))
    block = torch.empty((min(chunk, m), n), dtype=torch.float64, device=fit_sd.device)
    fn = nat.native().sp_knn
    st = nat.stream_handle(fit_sd.device)
    ends, parts, total = [], [], 0
    for a in range(0, m, chunk):
        b = min(m, a + chunk)
        fn(q_sd.indptr.data_ptr(), q_sd.indices.data_ptr(), q_sd.data.data_ptr(),
           t.indices.data_ptr(), t.data.data_ptr(), tab.data_ptr(), qn.data_ptr(), xn.data_ptr(),
           qexp.data_ptr(), a, b - a, n, d, tile, t.nnz, 0, 0, 1, 0, 0, block.data_ptr(), 0, 0, st)
        r, c = torch.nonzero(block[:b - a] <= thr, as_tuple=True)
        counts = torch.bincount(r, minlength=b - a).cpu().numpy().astype(np.int64)
        ends.append(total + np.cumsum(counts))
        total += int(counts.sum())
        parts.append(c.cpu().numpy())
    return np.concatenate([[0]] + ends), np.concatenate(parts)


def run(name, a):
    n, d, _ = SHAPES[name]
    mq = min(a.queries, n)
    t0 = time.perf_counter()
    X = make_csr(n, d)
    emit(shape=name, n=n, d=d, queries=mq, nnz=int(X.nnz), gen_s=round(time.perf_counter() - t0, 2))
    fit_sd = as_sparse_data(X, device="cuda")
    q_sd = as_sparse_data(X[:mq], device="cuda")
    xn = sp_row_norms(fit_sd)
    qn = xn[:mq].contiguous()
    # the threshold: the median distance to the --neighbours-th nearest row
    Dk, _ = SK.sp_knn(fit_sd, q_sd, a.neighbours, xn=xn, qn=qn)
    thr = float(Dk[:, -1].median())
    torch.cuda.synchronize()
    tiles = [int(t) for t in a.tiles.split(",")]
    if SR.TILE_DEFAULT not in tiles:
        tiles.append(SR.TILE_DEFAULT)
    ref = None
    per_query = {}
    for tile in tiles:
        plan = SR._Plan(fit_sd, q_sd, tile, xn, qn)
        rows = min(mq, a.launch_rows)
        mask, cnt = plan.buffers(rows)
        ms_mark = median_ms(lambda: plan.mark(0, rows, thr, 0, False, mask, cnt), reps=a.reps)
        cs = torch.cumsum(cnt.reshape(-1), 0, dtype=torch.int64)
        total = int(cs[-1])
        ms_fill = median_ms(lambda: plan.fill(rows, mask, cs, total), reps=a.reps)
        res = [None]

        def whole():
            res[0] = SR.sp_radius(fit_sd, q_sd, thr, tile=tile, xn=xn, qn=qn)
        ms = median_ms(whole, reps=a.reps)
        per_query[tile] = ms / mq
        emit(shape=name, what="sp_radius", tile=tile, launch_rows=rows,
             mark_ms=round(ms_mark, 3), mark_us_per_query=round(1e3 * ms_mark / rows, 3),
             fill_ms=round(ms_fill, 4), pairs_in_launch=total,
             sp_radius_ms=round(ms, 3), us_per_query=round(1e3 * ms / mq, 3),
             neighbours_per_row=round(len(res[0][1]) / mq, 1), default=tile == SR.TILE_DEFAULT)
        if ref is None:
            ref = res[0]
        else:
            assert np.array_equal(ref[0], res[0][0]) and np.array_equal(ref[1], res[0][1])
    # unit rows: the cosine distance is half the squared euclidean one
    ms = median_ms(lambda: SR.sp_radius(fit_sd, q_sd, 0.5 * thr, "cosine", xn=xn, qn=qn),
                   reps=a.reps)
    emit(shape=name, what="sp_radius", metric="cosine", tile=SR.TILE_DEFAULT,
         sp_radius_ms=round(ms, 3), us_per_query=round(1e3 * ms / mq, 3))
    base = per_query[SR.TILE_DEFAULT]
    if a.composed:
        mc = min(mq, a.composed_queries)
        qc = as_sparse_data(X[:mc], device="cuda")
        got = [None]

        def fn():
            got[0] = composed(fit_sd, qc, thr, xn, qn[:mc].contiguous(), a.composed_chunk)
        ms = median_ms(fn, warmup=1, reps=3)
        same = bool(np.array_equal(got[0][0], ref[0][:mc + 1]) and
                    np.array_equal(got[0][1], ref[1][:ref[0][mc]]))
        emit(shape=name, what="composed_dist_mode_nonzero", queries=mc, chunk=a.composed_chunk,
             ms=round(ms, 3), us_per_query=round(1e3 * ms / mc, 3), same_lists=same,
             sp_radius_speedup=round((ms / mc) / base, 2))
    if a.sklearn:
        from sklearn.neighbors import NearestNeighbors as SkNN
        ms_q = min(mq, a.sklearn_queries)
        sk = SkNN(radius=float(np.sqrt(thr)), algorithm="brute", metric="euclidean").fit(X)
        s = median_wall(lambda: sk.radius_neighbors(X[:ms_q], return_distance=False), warmup=0,
                        reps=3)
        ind = sk.radius_neighbors(X[:ms_q], return_distance=False)
        agree = float(np.mean([np.array_equal(np.sort(ind[i]), ref[1][ref[0][i]:ref[0][i + 1]])
                               for i in range(ms_q)]))
        emit(shape=name, what="sklearn_cpu_brute_radius_neighbors", queries=ms_q, s=round(s, 3),
             ms_per_query=round(1e3 * s / ms_q, 3), rows_with_equal_lists=round(agree, 4),
             sp_radius_speedup=round((1e3 * s / ms_q) / base, 1),
             threads=os.environ.get("OMP_NUM_THREADS", "default"))
    if a.fit_rows:
        nf = min(n, a.fit_rows)
        Xf = X[:nf]
        eps = float(np.sqrt(thr))
        kw = dict(eps=eps, min_samples=a.min_samples, device="cuda")
        est = [None]

        def fit_sparse():
            est[0] = DBSCAN(**kw).fit(Xf)
        s = median_wall(fit_sparse, warmup=1, reps=3)
        lab = est[0].labels_
        emit(shape=name, what="dbscan_fit_csr", rows=nf, eps=round(eps, 4), s=round(s, 3),
             clusters=int(lab.max() + 1), noise=int((lab == -1).sum()),
             core=int(len(est[0].core_sample_indices_)))
        s_cos = median_wall(lambda: DBSCAN(eps=0.5 * thr, min_samples=a.min_samples,
                                           metric="cosine", device="cuda").fit(Xf), warmup=0,
                            reps=1)
        emit(shape=name, what="dbscan_fit_csr", metric="cosine", rows=nf, s=round(s_cos, 3))
        if a.dense and nf * d * 4 <= 4 << 30:
            Xd = Xf.toarray()
            dn = [None]

            def fit_dense():
                dn[0] = DBSCAN(**kw).fit(Xd)
            sd = median_wall(fit_dense, warmup=1, reps=3)
            emit(shape=name, what="dbscan_fit_dense_array", rows=nf, s=round(sd, 3),
                 label_agreement=round(float(np.mean(dn[0].labels_ == lab)), 5),
                 csr_speedup=round(sd / s, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small",
                    help="comma-separated names of " + ", ".join(SHAPES))
    ap.add_argument("--tiles", default="2048,4096,8192")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--launch-rows", type=int, default=256,
                    help="query rows of the timed single mark / fill launches")
    ap.add_argument("--neighbours", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed", action="store_true")
    ap.add_argument("--composed-queries", type=int, default=256)
    ap.add_argument("--composed-chunk", type=int, default=128)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-queries", type=int, default=256)
    ap.add_argument("--fit-rows", type=int, default=0,
                    help="rows of the shape that whole DBSCAN fits run on (0: none)")
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--dense", action="store_true")
    a = ap.parse_args()
    for name in a.shape.split(","):
        run(name, a)


if __name__ == "__main__":
    main()
