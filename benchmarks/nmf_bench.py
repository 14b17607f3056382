"""Device NMF benchmark: the Kullback-Leibler ratio kernel of
``ops.sparse_nmf`` in both orientations, the coordinate-descent sweep, one
multiplicative (KL) and one coordinate-descent iteration end to end and whole
fits of ``NMF(device="cuda")`` on the synthetic bag-of-words corpus of
``lda_bench.py`` (about 100 stored words per document).  Next to it, on the
same machine,

(a) the route composed from pieces that existed before the kernels: the torch
    gather-multiply-sum of ``W[ii] * Ht[jj]`` over the stored entries followed
    by ``sp_xw`` on the ratio matrix, and ``sqh_cdnmf_update`` on the host with
    the device-to-host and host-to-device copies it forces;
(b) the host path (``device=None``, ``--host``), which densifies: only at a
    shape that fits as a dense fp64 array;
(c) scikit-learn's CPU ``NMF`` on the same CSR matrix (``--sklearn``).

    python benchmarks/nmf_bench.py --shape small --components 64 128 --host --sklearn

``--tokens 12 --kernels-only`` times the kernels alone on rows short enough for
the ratio kernel to stage their gathered operand rows in LDS (every row of
the default corpus is too long for that).  With ``SQ_NATIVE_VARIANT`` naming
an extension built from a copy of ``csrc`` (``SQ_CSRC_DIR``) whose ratio kernel
never stages, the same command times the other branch.

Prints one JSON line per measurement (kernels: medians over ``--reps`` event
pairs after a warm-up; the host sweep, single iterations and device fits:
medians of warmed host-clock samples around a device synchronise; host-path
and scikit-learn fits: one sample); ``profiles/nmf_device.md`` records a run.
There is no pass/fail time.
"""

import argparse
import ctypes
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

from lda_bench import SHAPES, make_corpus, wall               # noqa: E402
from sparse_kmeans_bench import emit                         # noqa: E402
from sparse_knn_bench import median_ms                       # noqa: E402
from sq_learn_amd.decomposition import NMF                   # noqa: E402
from sq_learn_amd.models._data import SparseData, as_sparse_data  # noqa: E402
from sq_learn_amd.models.decomposition._nmf_device import DeviceNMF  # noqa: E402
from sq_learn_amd.ops import _host                           # noqa: E402
from sq_learn_amd.ops import sparse_linalg as SL             # noqa: E402
from sq_learn_amd.ops import sparse_nmf as S                 # noqa: E402
from sq_learn_amd.ops._csr import chunks, csr_transpose      # noqa: E402

HOST_DENSE_BYTES = 8 << 30     # the host path runs only where dense X stays below this


def composed_kl_num(sd, W, Ht, chunk=1 << 24):
    """num of the W update from existing pieces: gather-multiply-sum in torch,
    then the CSR product of the ratio matrix (fp32 values, as every CSR op)."""
    ii, jj = sd.row_ids(), sd.indices.to(torch.int64)
    k = W.shape[1]
    wh = torch.empty(sd.nnz, dtype=torch.float64, device=sd.device)
    for s, e in chunks(sd.nnz, max(1, chunk // k)):
        wh[s:e] = (W[ii[s:e]] * Ht[jj[s:e]]).sum(1)
    wh = torch.where(wh == 0, S.EPSILON, wh)
    ratio = SparseData(sd.indptr, sd.indices, (sd.data.double() / wh).float(), sd.shape)
    return SL.sp_xw(ratio, Ht)


def composed_cd_sweep(W, HHt, XHt, perm):
    """The host sweep on device operands: three copies down, one up."""
    Wh, Gh, Xh = (np.ascontiguousarray(t.cpu().numpy()) for t in (W, HHt, XHt))
    p = np.ascontiguousarray(perm, dtype=np.int64)
    c = lambda a: ctypes.c_void_p(a.ctypes.data)                     # noqa: E731
    v = _host.lib().sqh_cdnmf_update(c(Wh), c(Gh), c(Xh), c(p), Wh.shape[0], Wh.shape[1])
    W.copy_(torch.from_numpy(Wh))
    return v


def run(name, k, a):
    n, d = SHAPES[name]
    X = make_corpus(n, d, tokens=a.tokens)
    base = dict(shape=name, n=n, d=d, k=k, nnz_row=round(X.nnz / n, 1))
    dev = torch.device("cuda")
    rng = np.random.RandomState(0)
    avg = np.sqrt(X.mean() / k)
    W = torch.from_numpy(np.abs(avg * rng.randn(n, k))).to(dev)
    Ht = torch.from_numpy(np.abs(avg * rng.randn(d, k))).to(dev)
    sd = as_sparse_data(X, dev)
    sdt = csr_transpose(sd)
    lens = np.diff(X.indptr)
    base["staged_rows"] = float((lens <= S.stage_entries(k)).mean())
    # ---- ratio kernel, both orientations, against the composed route
    emit(what="kl_ratio", on="X", ms=median_ms(lambda: S.nmf_kl_ratio(sd, W, Ht), reps=a.reps),
         **base)
    emit(what="kl_ratio", on="X^T", ms=median_ms(lambda: S.nmf_kl_ratio(sdt, Ht, W), reps=a.reps),
         **base)
    emit(what="kl_ratio_div_only", on="X",
         ms=median_ms(lambda: S.nmf_kl_ratio(sd, W, Ht, want_num=False, want_div=True),
                      reps=a.reps), **base)
    emit(what="kl_ratio_composed", on="X",
         ms=median_ms(lambda: composed_kl_num(sd, W, Ht), reps=a.reps), **base)
    got, ref = S.nmf_kl_ratio(sd, W, Ht)[0], composed_kl_num(sd, W, Ht)
    emit(what="kl_ratio_vs_composed", max_rel=float(((got - ref).abs() / ref.abs().clamp(min=1e-300))
                                                    .max()), **base)
    # ---- sweep (one lane per row: the only mapping written), against the host with copies
    HHt = Ht.T @ Ht
    XHt = SL.sp_xw(sd, Ht)
    perm = torch.arange(k, device=dev)
    W1 = W.clone()
    emit(what="cd_sweep", rows=n, ms=median_ms(lambda: S.nmf_cd_sweep(W1, HHt, XHt, perm),
                                               reps=a.reps), **base)
    W2 = W.clone()
    composed_cd_sweep(W2, HHt, XHt, np.arange(k))        # warm-up: loads the host library
    t_h = np.median([wall(lambda: composed_cd_sweep(W2, HHt, XHt, np.arange(k)))[0]
                     for _ in range(a.reps)])
    emit(what="cd_sweep_host_with_copies", rows=n, ms=1e3 * t_h, **base)
    emit(what="cd_products", ms=median_ms(lambda: (SL.sp_xw(sd, Ht), SL.sp_xty(sd, W), Ht.T @ Ht),
                                          reps=a.reps), **base)
    if a.kernels_only:
        return
    # ---- one iteration end to end, whole fits
    W0, H0 = W.cpu().numpy(), np.ascontiguousarray(Ht.T.cpu().numpy())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for solver, loss in (("cd", "frobenius"), ("mu", "kullback-leibler"), ("mu", "frobenius")):
            kw = dict(init="custom", solver=solver, beta_loss=loss, tol=0.0)
            # warm-up at the timed shape: the first GEMMs of a shape pick their algorithm
            NMF(k, max_iter=1, device="cuda", **kw).fit(X, W=W0, H=H0)
            state = DeviceNMF(NMF(k, max_iter=1, device="cuda", **kw), X)
            beta = 2 if loss == "frobenius" else 1
            # upload of the factors, one iteration, download; for 'mu' also the initial divergence
            t_it = np.median([wall(lambda: state.fit(W0, H0, beta, True))[0]
                              for _ in range(a.reps)])
            emit(what="one_iteration", solver=solver, loss=loss, seconds=t_it, **base)
            runs = [wall(lambda: NMF(k, max_iter=a.iters, device="cuda", **kw).fit(X, W=W0, H=H0))
                    for _ in range(3)]
            t_fit, est = sorted(runs, key=lambda r: r[0])[1]
            emit(what="fit", path="cuda", solver=solver, loss=loss, iters=a.iters, seconds=t_fit,
                 err=est.reconstruction_err_, **base)
            if a.host and n * d * 8 <= HOST_DENSE_BYTES:
                t_hf, est = wall(lambda: NMF(k, max_iter=a.iters, **kw).fit(X, W=W0, H=H0))
                emit(what="fit", path="host", solver=solver, loss=loss, iters=a.iters,
                     seconds=t_hf, err=est.reconstruction_err_,
                     threads=int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)), **base)
            if a.sklearn:
                import sklearn.decomposition as SK
                t_s, est = wall(lambda: SK.NMF(n_components=k, max_iter=a.iters, **kw)
                                .fit(X, W=W0.copy(), H=H0.copy()))
                emit(what="fit", path="sklearn", solver=solver, loss=loss, iters=a.iters,
                     seconds=t_s, err=est.reconstruction_err_, **base)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", default="small", choices=sorted(SHAPES))
    p.add_argument("--components", type=int, nargs="+", default=[64, 128])
    p.add_argument("--iters", type=int, default=10, help="iterations of the fits")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--tokens", type=int, default=130,
                   help="draws per document: 130 give about 100 stored words, 12 give "
                        "rows short enough for the ratio kernel to stage at k = 64")
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--host", action="store_true")
    p.add_argument("--sklearn", action="store_true")
    a = p.parse_args()
    for k in a.components:
        run(a.shape, k, a)


if __name__ == "__main__":
    main()
