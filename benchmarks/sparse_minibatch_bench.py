"""Sparse (CSR) mini-batch k-means benchmark on a synthetic TF-IDF-like matrix
(the generator of ``sparse_kmeans_bench.py``): for k in {100, 1000} and batch
sizes {1024, 8192, 65536}

* the fused row-list step (``ops.sparse_kmeans.MiniBatchState``): E-step,
  scatter and fused centre update timed on their own, and the whole step with
  its one record read (steps per second);
* the same step composed from the full-batch sparse ops: a sub-CSR of the
  batch, ``sp_estep``, ``sp_centroid_sums``, the torch update and
  ``center_operand``, with one packed read as well - the baseline;
* a whole ``MiniBatchKMeans`` fit next to the full sparse ``KMeans`` fit.

    python benchmarks/sparse_minibatch_bench.py [--n 200000 --d 20000]

Prints one JSON line per measurement; ``profiles/sparse_minibatch.md`` records
a run.  There is no pass/fail time.
"""

import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

from sparse_kmeans_bench import emit, make_csr, timed          # noqa: E402
from sq_learn_amd.cluster import KMeans, MiniBatchKMeans      # noqa: E402
from sq_learn_amd.models._data import as_sparse_data          # noqa: E402
from sq_learn_amd.models.cluster._sparse import take_rows     # noqa: E402
from sq_learn_amd.ops import sparse_kmeans as S               # noqa: E402
from sq_learn_amd.runtime.rng import RngKey                   # noqa: E402


def wall(fn, warmup=3, reps=100):
    """Host wall-clock per call (the steps end in a host read)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def med3(measure):
    """(median, relative spread) of three repeats of one measurement."""
    v = sorted(measure() for _ in range(3))
    return v[1], (v[2] - v[0]) / v[1]


class Composed:
    """The mini-batch step built from the full-batch sparse ops."""

    def __init__(self, sd, xn, C, counts):
        self.sd, self.xn, self.C, self.counts = sd, xn, C.clone(), counts.clone()
        self.k = C.shape[0]
        self.op = S.center_operand(self.C)
        self.key = RngKey(0, "band_select", 0)

    def step(self, rows):
        sub = take_rows(self.sd, rows)
        labels, _, inertia = S.sp_estep(sub, self.C, 0.0, self.key, 0, xn=self.xn[rows],
                                        operand=self.op)
        sums, wsum = S.sp_centroid_sums(sub, labels, self.k)
        Cn, counts, shift = S.minibatch_update_torch(self.C, self.counts, sums, wsum)
        self.C, self.counts = Cn, counts
        self.op = S.center_operand(Cn)
        return torch.stack([inertia[0], shift, counts.min()]).tolist()


def run(n, d, ks, batches, fits):
    t0 = time.perf_counter()
    X = make_csr(n, d)
    emit(n=n, d=d, nnz=int(X.nnz), gen_s=round(time.perf_counter() - t0, 2))
    sd = as_sparse_data(X, device="cuda")
    xn = S.sp_row_norms(sd)
    mx = float(sd.data.abs().max())
    rng = np.random.RandomState(1)
    for k in ks:
        C0 = S.sp_rows_dense(sd, rng.choice(n, size=k, replace=False))
        counts0 = torch.zeros(k, dtype=torch.float64, device="cuda")
        for m in batches:
            rows = torch.as_tensor(rng.randint(0, n, m), dtype=torch.int64).cuda()
            st = S.MiniBatchState("cuda", C0, counts0, mx)
            labels, _, _ = st.estep(sd, xn, rows, None)
            e_ms, _ = med3(lambda: timed(lambda: st.estep(sd, xn, rows, None), 3, 100))

            def scatter_update():
                st.scatter(sd, rows, labels, None)
                st.update()
            su_ms, _ = med3(lambda: timed(scatter_update, 3, 100))
            # the update consumes what the scatter left, so the scatter alone is timed
            # into a spare state and the update is the difference
            spare = S.MiniBatchState("cuda", C0, counts0, mx)

            def scatter_only():
                spare.scatter(sd, rows, labels, None)
            s_ms, _ = med3(lambda: timed(scatter_only, 3, 100))
            base = Composed(sd, xn, C0, counts0)
            # the two whole steps alternate, three windows of 100 steps each
            pairs = [(wall(lambda: st.step(sd, xn, rows, None)), wall(lambda: base.step(rows)))
                     for _ in range(3)]
            step_ms, step_spread = med3(iter([p[0] for p in pairs]).__next__)
            base_ms, base_spread = med3(iter([p[1] for p in pairs]).__next__)
            u_ms = max(su_ms - s_ms, 0.0)
            emit(k=k, batch=m, estep_ms=round(e_ms, 4), scatter_ms=round(s_ms, 4),
                 update_ms=round(u_ms, 4), step_ms=round(step_ms, 4),
                 steps_per_s=round(1e3 / step_ms, 1), rows_per_s=round(m * 1e3 / step_ms, 0),
                 step_spread=round(step_spread, 3), composed_step_ms=round(base_ms, 4),
                 composed_spread=round(base_spread, 3), speedup=round(base_ms / step_ms, 2),
                 dense_pass_share=round(u_ms / (e_ms + s_ms + u_ms), 3))
            del st, spare, base
        if fits:
            init = C0.cpu().numpy()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for est, what in ((lambda: MiniBatchKMeans(k, init=init.copy(), batch_size=8192,
                                                           max_iter=2, max_no_improvement=None,
                                                           random_state=0, device="cuda"),
                                   "minibatch_fit_2epochs_b8192"),
                                  (lambda: KMeans(k, init=init, n_init=1, max_iter=10, tol=0.0,
                                                  device="cuda"), "kmeans_fit_10it")):
                    est().fit(X)                      # warm-up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m_ = est().fit(X)
                    torch.cuda.synchronize()
                    emit(k=k, what=what, s=round(time.perf_counter() - t0, 3),
                         n_iter=int(m_.n_iter_), inertia=float(m_.inertia_))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--d", type=int, default=20_000)
    ap.add_argument("--k", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 8192, 65536])
    ap.add_argument("--no-fits", action="store_true")
    a = ap.parse_args()
    run(a.n, a.d, a.k, a.batch, not a.no_fits)


if __name__ == "__main__":
    main()
