"""CSR sparse Lloyd / q-means engine and the sparse estimator paths.

Reference: the sparse branches of ``cluster/_kmeans.py`` (``KMeans`` accepts
``accept_sparse='csr'``, ``lloyd_iter_chunked_sparse``) and of
``cluster/_dmeans.py``, whose sparse q-means is a stub that warns and falls
back to the classical iteration (``_dmeans.py:631-635, 713-716, 811``).  Here
the quantum model runs on CSR rows as well: the delta-band rule, the IPE
distance estimates, the centre noise and the tomography are the dense
engine's, keyed the same way.

:class:`SparseLloydEngine` follows the step contract ``KMeans`` and
``QMeans._run_lloyd`` drive (``restart``, ``it``, ``xn``, ``set_centers``,
``centers``, ``estep``, ``step``, ``mstep``).  The data are not centred
(sparse stays sparse, like sklearn), so the centres live in data coordinates
and are kept in fp64; the kernels are ``csrc/spkmeans.hip`` through
``ops/sparse_kmeans.py`` (torch twins on CPU).  Sparse input is single
process.
"""

import math
import warnings

import numpy as np
import torch

from ...exceptions import ConvergenceWarning
from ...ops import kmeans as K
from ...ops import sparse_kmeans as S
from ...ops.random import trunc_normal_add_
from ...parallel.comm import Comm
from ...quantum.fejer import median_repetitions
from ...runtime.device import to_numpy
from ...runtime.rng import RngKey
from ...utils.validation import check_is_fitted, check_random_state, seed_from_random_state
from .._data import SparseData, as_sparse_data
from ._init import permutation_head


class SparseLloydEngine:
    def __init__(self, sd, k, *, delta=0.0, true_distance_estimate=False,
                 intermediate_error=False, true_tomography=False, tomography_kw=None,
                 sample_weight=None, seed=0, ipe_Q=13, empty_policy=0, relocate_empty=False,
                 xn=None, ipe_chunk=None):
        self.sd = sd
        self.device = sd.device
        self.n, self.d = sd.shape
        self.k = int(k)
        self.delta = float(delta or 0.0)
        self.ipe = bool(true_distance_estimate) and self.delta > 0
        self.intermediate_error = bool(intermediate_error)
        self.true_tomography = bool(true_tomography)
        self.tomography_kw = dict(tomography_kw or {})
        self.sample_weight = (None if sample_weight is None
                              else sample_weight.to(torch.float64).to(self.device).contiguous())
        self.seed = seed
        self.comm = sd.comm if getattr(sd, "comm", None) is not None else Comm(None)
        self.row_offset = int(sd.row_offset)
        self.ipe_Q = int(ipe_Q)
        self.empty_policy = int(empty_policy)
        self.relocate_empty = bool(relocate_empty)
        self.n_relocated = 0
        self.k_pad = K.pad_clusters(self.k)
        self.restart = 0
        self.it = 0
        self.pipeline = False
        self.ipe_chunk = ipe_chunk
        # [estimations made, corrupted rows]: failure injection is refused on CSR
        self.failure_counters = torch.zeros(2, dtype=torch.int64, device=self.device)
        if self.device.type == "cuda":
            S.check_k(self.k)
        self.xn = xn if xn is not None else S.sp_row_norms(sd)
        self.C = torch.zeros((self.k, self.d), dtype=torch.float64, device=self.device)
        self._operand = None
        self._reduce = S.SparseReduce(sd, self.k, self.sample_weight)

    # ---------------------------------------------------------- keys
    def _key(self, purpose, it=None):
        it = self.it if it is None else it
        return RngKey(self.seed, purpose, (self.restart << 24) | (it & 0xFFFFFF))

    # ---------------------------------------------------------- state
    def drop_pending(self):
        pass

    def set_centers(self, C):
        self.C = C.to(self.device).to(torch.float64).clone()
        self._operand = None

    def centers(self):
        return self.C

    def _op(self):
        """Transposed centre operand of the kernels, built once per centre update."""
        if self.device.type != "cuda":
            return None
        if self._operand is None:
            self._operand = S.center_operand(self.C)
        return self._operand

    # ---------------------------------------------------------- E-step
    def estep(self, C=None):
        if C is not None:
            self.set_centers(C)
        return self._estep(self._key("band_select"))

    def _estep(self, key):
        if self.ipe:
            lab, mind = self._estep_ipe()
            inertia = None
        else:
            lab, mind, inertia = S.sp_estep(self.sd, self.C, self.delta, key, self.row_offset,
                                            xn=self.xn, operand=self._op())
        if self.sample_weight is not None or inertia is None:
            m = mind.double()
            inertia = (m if self.sample_weight is None else m * self.sample_weight).sum().reshape(1)
        return lab, mind, inertia

    def _ipe_chunk_rows(self):
        if self.ipe_chunk is not None:
            return max(1, int(self.ipe_chunk))
        budget = 1 << 28
        if self.device.type == "cuda":
            budget = max(1 << 24, min(1 << 30, torch.cuda.mem_get_info(self.device)[0] // 8))
        return max(256, min(1 << 16, budget // (4 * max(self.k, 1))))

    def _estep_ipe(self):
        """IPE distance estimates (``_dmeans.py:753-772``): inner products
        of a row chunk, then the dense engine's per-pair estimator."""
        eps = self.delta / 2.0
        key = self._key("ipe")
        n, k = self.n, self.k
        step = self._ipe_chunk_rows()
        if self.device.type == "cuda":
            labels = torch.empty(n, dtype=torch.int32, device=self.device)
            mind = torch.empty(n, dtype=torch.float32, device=self.device)
            op = self._op()
            xn32 = self.xn.float().contiguous()
            cn32 = op[1].float().contiguous()
            G = torch.empty((min(step, n), k), dtype=torch.float32, device=self.device)
            for s in range(0, n, step):
                e = min(n, s + step)
                g = S.sp_gram(self.sd, self.C, rows=slice(s, e), out=G, operand=op)
                K.ipe_estep_native(g, xn32[s:e], cn32, eps, self.ipe_Q, key, self.row_offset + s,
                                   labels[s:e], mind[s:e])
            return labels, mind
        labels = torch.empty(n, dtype=torch.int64)
        mind = torch.empty(n, dtype=torch.float64)
        step = min(step, S.TWIN_CHUNK)
        for s in range(0, n, step):
            e = min(n, s + step)
            labels[s:e], mind[s:e] = K.ipe_estep_torch(self.sd.dense_rows(s, e), self.C, eps, key,
                                                       self.row_offset + s, self.k_pad,
                                                       Q=self.ipe_Q)
        return labels, mind

    # ---------------------------------------------------------- M-step
    def _noise_bound(self):
        if not self.intermediate_error or self.delta <= 0 or self.true_tomography:
            return 0.0
        return (self.delta / 2.0) / math.sqrt(self.k * self.d)

    def mstep(self, labels, inertia):
        """Centre update from labels; returns [inertia, shift^2, 0] (device)."""
        sums, counts = S.sp_centroid_sums(self.sd, labels, self.k, self.sample_weight,
                                          ws=self._reduce)
        self._last_counts = counts
        old = self.C
        self._C_prev = old
        new = torch.where(counts[:, None] > 0, sums / counts[:, None],
                          old if self.empty_policy == 0 else torch.zeros_like(sums)).contiguous()
        b = self._noise_bound()
        if b > 0:
            trunc_normal_add_(new.view(-1), b, self._key("trunc_normal"), offset=0)
        self.C = new
        self._operand = None
        if self.intermediate_error and self.true_tomography and self.delta > 0:
            from ...quantum.device import tomography_rows_torch
            est = tomography_rows_torch(self.C, self.delta / 2.0, self._key("tomography"),
                                        **self.tomography_kw)
            self.C = est.to(torch.float64).contiguous()
        dd = self.C - old
        return torch.stack([inertia.double().reshape(()), (dd * dd).sum(),
                            torch.zeros((), dtype=torch.float64, device=self.device)])

    def _relocate(self, labels, mind, counts):
        """sklearn's empty-cluster relocation: each empty cluster takes one of
        the rows farthest from their centre (descending ``mind``)."""
        empty = torch.nonzero(counts == 0)[:, 0]
        e = min(int(empty.numel()), self.n)
        if e == 0:
            return labels
        far = torch.topk(mind.double(), e).indices
        labels = labels.clone()
        labels[far] = empty[:e].to(labels.dtype)
        self.n_relocated += e
        return labels

    def step(self):
        labels, mind, inertia = self._estep(self._key("band_select"))
        sc = self.mstep(labels, inertia)
        if self.relocate_empty and bool((self._last_counts == 0).any()):
            self.C = self._C_prev
            labels = self._relocate(labels, mind, self._last_counts)
            sc = self.mstep(labels, inertia)
        self.it += 1
        return labels, sc


# ------------------------------------------------------------------ init
def sparse_kmeans_plusplus(sd, n_clusters, random_state, xn=None, n_local_trials=None,
                           gather=None):
    """Sequential k-means++ on CSR rows: the torch path of
    ``_init.kmeans_plusplus`` draw for draw (``randint(n)``, then
    ``random_sample((k - 1, t))``), distances by ``sp_sqdist`` against the
    densified candidate rows (``gather(ids)``, default ``sd.gather_dense``).
    Returns (centres [k, d] fp64, row ids)."""
    gather = sd.gather_dense if gather is None else gather
    n = sd.shape[0]
    k = int(n_clusters)
    dev = sd.device
    t = 2 + int(np.log(k)) if n_local_trials is None else int(n_local_trials)
    rs = random_state
    if xn is None:
        xn = S.sp_row_norms(sd)
    center_id = int(rs.randint(n))
    draws = torch.as_tensor(rs.random_sample((max(k - 1, 0), t)), dtype=torch.float64, device=dev)
    ids = torch.empty(k, dtype=torch.int64, device=dev)
    ids[0] = center_id
    centers = torch.empty((k, sd.d), dtype=torch.float64, device=dev)
    centers[0] = gather([center_id])[0]
    closest = S.sp_sqdist(sd, centers[:1], xn=xn)[:, 0].contiguous()
    current_pot = closest.sum()
    for c in range(1, k):
        vals = draws[c - 1] * current_pot
        cs = torch.cumsum(closest, 0)
        pos = torch.searchsorted(cs, vals.contiguous()).clamp(0, max(n - 1, 0))
        cands = gather(pos.cpu().numpy())
        newd = torch.minimum(closest[:, None], S.sp_sqdist(sd, cands, xn=xn))
        pots = newd.sum(0)
        best = torch.argmin(pots)
        current_pot = pots.index_select(0, best.reshape(1))[0]
        closest = newd.index_select(1, best.reshape(1))[:, 0].contiguous()
        centers[c] = cands.index_select(0, best.reshape(1))[0]
        ids[c] = pos.index_select(0, best.reshape(1))[0]
    return centers, ids.cpu().numpy()


def _init_centers(est, X, sd, rs, xn):
    init = est.init
    k = est.n_clusters
    if isinstance(init, str) and init == "k-means++":
        C, _ = sparse_kmeans_plusplus(sd, k, rs, xn=xn)
    elif isinstance(init, str) and init == "k-means||":
        raise ValueError("init='k-means||' is not supported for sparse input")
    elif isinstance(init, str) and init == "random":
        C = sd.gather_dense(permutation_head(rs, sd.shape[0], k))
    elif hasattr(init, "__array__") or isinstance(init, torch.Tensor):
        C = torch.as_tensor(np.asarray(to_numpy(init), dtype=np.float64)).to(sd.device)
    elif callable(init):
        C = torch.as_tensor(np.asarray(init(X, k, random_state=rs), dtype=np.float64)).to(sd.device)
    else:
        raise ValueError("init should be either 'k-means++', 'random', a ndarray or a callable, "
                         f"got '{init}' instead.")
    if tuple(C.shape) != (k, sd.d):
        raise ValueError(f"The shape of the initial centers {tuple(C.shape)} does not match the "
                         f"number of clusters {k} / features {sd.d}.")
    return C.double()


# ------------------------------------------------------------- estimators
def _weights(sample_weight, sd):
    if sample_weight is None:
        return None
    sw = torch.as_tensor(np.asarray(to_numpy(sample_weight), dtype=np.float64)).to(sd.device)
    if sw.ndim != 1 or sw.numel() != sd.shape[0]:
        raise ValueError("sample_weight must have one weight per sample")
    return sw


def _tolerance(X, tol):
    from ...utils.sparsefuncs import mean_variance_axis
    _, var = mean_variance_axis(X if X.format in ("csr", "csc") else X.tocsr(), axis=0)
    return float(np.mean(var)) * tol


def _refuse(est):
    """Combinations that are not handled on CSR: a clear error instead of
    mis-handling them."""
    name = type(est).__name__
    if float(getattr(est, "failure_prob", 0.0) or 0.0) > 0:
        raise ValueError(f"{name}: failure_prob > 0 is not supported for sparse input")
    if getattr(est, "checkpoint_dir", None) is not None:
        raise ValueError(f"{name}: checkpoint_dir is not supported for sparse input")
    if getattr(est, "gemm_precision", None) == "bf16":
        raise ValueError(f"{name}: gemm_precision='bf16' is not supported for sparse input "
                         "(the sparse kernels are fp64)")
    if isinstance(est.init, str) and est.init == "k-means||":
        raise ValueError(f"{name}: init='k-means||' is not supported for sparse input")


def _warn_distinct(labels_np, k):
    distinct = len(np.unique(labels_np))
    if distinct < k:
        warnings.warn(f"Number of distinct clusters ({distinct}) found smaller than n_clusters "
                      f"({k}). Possibly due to duplicate points in X.", ConvergenceWarning,
                      stacklevel=3)


def _label_inertia(eng, C, labels, sw):
    """sum_i w_i |x_i - c_label(i)|^2 in fp64."""
    n = eng.n
    total = torch.zeros((), dtype=torch.float64, device=eng.device)
    op = S.center_operand(C) if eng.device.type == "cuda" else None
    step = max(256, min(n, (1 << 25) // max(eng.k, 1)))
    lab = labels.to(torch.int64)
    for s in range(0, n, step):
        e = min(n, s + step)
        D = S.sp_sqdist(eng.sd, C, rows=slice(s, e), xn=eng.xn, operand=op)
        v = D.gather(1, lab[s:e, None])[:, 0]
        total += (v if sw is None else v * sw[s:e]).sum()
    return float(total)


def kmeans_fit(est, X, sample_weight=None):
    """``KMeans.fit`` on a scipy sparse matrix (Lloyd; 'elkan' runs 'full')."""
    _refuse(est)
    sd = as_sparse_data(X, device=est.device)
    if est.n_init <= 0:
        raise ValueError(f"n_init should be > 0, got {est.n_init} instead.")
    if est.max_iter <= 0:
        raise ValueError(f"max_iter should be > 0, got {est.max_iter} instead.")
    if sd.shape[0] < est.n_clusters:
        raise ValueError(f"n_samples={sd.shape[0]} should be >= n_clusters={est.n_clusters}.")
    if est.algorithm not in ("auto", "full", "elkan", "lloyd"):
        raise ValueError(f"Algorithm must be 'auto', 'full' or 'elkan', got {est.algorithm} instead.")
    est.n_features_in_ = sd.d
    n_init = est.n_init
    if hasattr(est.init, "__array__") and n_init != 1:
        warnings.warn("Explicit initial center position passed: performing only one init in "
                      f"KMeans instead of n_init={n_init}.", RuntimeWarning, stacklevel=3)
        n_init = 1
    rs = check_random_state(est.random_state)
    seed = (int(rs.get_state()[1][0]) if isinstance(est.random_state, np.random.RandomState)
            else seed_from_random_state(est.random_state))
    tol = _tolerance(X, est.tol)
    sw = _weights(sample_weight, sd)
    eng = SparseLloydEngine(sd, est.n_clusters, delta=0.0, sample_weight=sw, seed=seed,
                            relocate_empty=True)
    best = None
    for r in range(n_init):
        eng.restart, eng.it = r, 0
        C0 = _init_centers(est, X, sd, rs, eng.xn)
        eng.set_centers(C0)
        labels_old, strict, it = None, False, 0
        for it in range(est.max_iter):
            labels, sc = eng.step()
            shift = float(sc[1].item())
            if labels_old is not None and torch.equal(labels, labels_old):
                strict = True
                break
            if shift <= tol:
                break
            labels_old = labels.clone()
        C = eng.centers().clone()
        if not strict:
            labels, _, _ = eng.estep()
        labels = labels.clone()
        inertia = _label_inertia(eng, C, labels, sw)
        if best is None or inertia < best[1]:
            best = (labels, inertia, C, it + 1)
    labels, inertia, C, n_iter = best
    est.cluster_centers_ = to_numpy(C.double())
    est.labels_ = to_numpy(labels).astype(np.int32)
    est.inertia_ = inertia
    est.n_iter_ = n_iter
    _warn_distinct(est.labels_, est.n_clusters)
    return est


def _fitted(est, X):
    check_is_fitted(est)
    sd = as_sparse_data(X, device=est.device)
    if sd.d != est.n_features_in_:
        raise ValueError(f"X has {sd.d} features, but {type(est).__name__} is expecting "
                         f"{est.n_features_in_} features as input.")
    return sd, torch.as_tensor(np.asarray(est.cluster_centers_, dtype=np.float64)).to(sd.device)


def assign(est, X, delta=0.0):
    """Sparse E-step on the fitted centres: (labels, mind, inertia, sd)."""
    sd, C = _fitted(est, X)
    delta = float(delta or 0.0)
    eng = SparseLloydEngine(sd, est.n_clusters, delta=delta,
                            true_distance_estimate=bool(getattr(est, "true_distance_estimate",
                                                                False)) and delta > 0,
                            seed=seed_from_random_state(est.random_state),
                            ipe_Q=_ipe_q(est))
    eng.restart = 0xFF
    labels, mind, inertia = eng.estep(C)
    return labels, mind, inertia, sd


def _ipe_q(est):
    q = getattr(est, "ipe_Q", None)
    return q if q is not None else median_repetitions(0.1)


def predict(est, X, delta=0.0):
    labels, _, _, _ = assign(est, X, delta)
    return to_numpy(labels).astype(np.int32)


def score(est, X, sample_weight=None):
    _, mind, inertia, sd = assign(est, X, 0.0)
    if sample_weight is not None:
        return -float((mind.double() * _weights(sample_weight, sd)).sum())
    return -float(inertia.double().sum())


def transform(est, X):
    """Dense (n, k) Euclidean distances to the fitted centres."""
    sd, C = _fitted(est, X)
    n, k = sd.shape[0], C.shape[0]
    out = np.empty((n, k), dtype=np.float64)
    xn = S.sp_row_norms(sd)
    op = S.center_operand(C) if sd.device.type == "cuda" else None
    step = max(256, (1 << 25) // max(k, 1))
    for s in range(0, n, step):
        e = min(n, s + step)
        out[s:e] = to_numpy(torch.sqrt(S.sp_sqdist(sd, C, rows=slice(s, e), xn=xn, operand=op)))
    return out


def sparse_mu(sd, xn, start=0.0, end=0.1, step=0.05):
    """mu(A) over the p-grid of ``best_mu_distributed`` from the stored
    values; for exponent 0 a zero entry counts as 1 (numpy's ``0 ** 0`` in the
    reference): d per row, n per column."""
    n, d = sd.shape
    domain = [i for i in np.arange(start, end, step)] + [end]
    a = sd.data.double().abs()
    rows, cols = sd.row_ids(), sd.indices.to(torch.int64)

    def sums(e):
        if e == 0.0:
            return float(d), float(n)
        p = a ** e
        r = torch.zeros(n, dtype=torch.float64, device=sd.device).index_add_(0, rows, p)
        c = torch.zeros(d, dtype=torch.float64, device=sd.device).index_add_(0, cols, p)
        return float(r.max()), float(c.max())

    cache = {}
    vals = []
    for p in domain:
        e1, e2 = round(float(2 * p), 12), round(float(2 * (1 - p)), 12)
        for e in (e1, e2):
            if e not in cache:
                cache[e] = sums(e)
        vals.append(float(np.sqrt(cache[e1][0] * cache[e2][1])))
    best = int(np.argmin(vals))
    fro = float(np.sqrt(float(xn.sum())))
    if vals[best] <= fro:
        return f"p={domain[best]}", vals[best]
    return "Frobenius", fro


def qmeans_fit(est, X, sample_weight=None):
    """``QMeans.fit`` on a scipy sparse matrix: the quantum Lloyd loop
    (``QMeans._run_lloyd``) on the sparse engine."""
    import time as _time
    _refuse(est)
    sd = as_sparse_data(X, device=est.device)
    est._check_params(sd)
    est.n_features_in_ = sd.d
    delta = est._delta()
    if est.delta == 0:
        warnings.warn("Attention! You are running classic version of kmeans!")
        if est.intermediate_error:
            raise ValueError("intermediate_error value cannot be True if delta is zero.")
    t0 = _time.perf_counter()
    xn = S.sp_row_norms(sd)
    if est.compute_prelude:
        est.eta = float(xn.max()) if xn.numel() else 0.0
        est.muA_norm, est.muA = sparse_mu(sd, xn)
        # a d x d Gram is not formed for sparse data
        est.condition_number = None
    rs = check_random_state(est.random_state)
    seed = seed_from_random_state(est.random_state)
    est._tol = _tolerance(X, est.tol)
    sw = _weights(sample_weight, sd)
    tomo_kw = dict(stop_when_reached_accuracy=est.stop_when_reached_accuracy,
                   preserve_norm=est.preserve_norm_tomography)
    engine = SparseLloydEngine(sd, est.n_clusters, delta=delta,
                               true_distance_estimate=est.true_distance_estimate,
                               intermediate_error=est.intermediate_error,
                               true_tomography=est.true_tomography, tomography_kw=tomo_kw,
                               sample_weight=sw, seed=seed, ipe_Q=_ipe_q(est),
                               empty_policy=1 if est.empty_cluster == "zero" else 0,
                               relocate_empty=est.empty_cluster == "relocate", xn=xn)
    best = None
    restart_inertias = []
    for restart in range(est._n_init):
        engine.restart, engine.it = restart, 0
        C0 = _init_centers(est, X, sd, rs, xn)
        labels, inertia, centers, n_iter = est._run_lloyd(engine, C0)
        restart_inertias.append(float(inertia))
        if best is None or inertia < best[1]:
            best = (labels, inertia, centers, n_iter)
    labels, inertia, centers, n_iter = best
    est.n_estimations_ = 0
    est.n_failed_rows_ = 0
    est.cluster_centers_ = to_numpy(centers.double())
    est._labels_t = labels
    est.labels_ = to_numpy(labels).astype(np.int32)
    est.inertia_ = float(inertia)
    est.n_iter_ = int(n_iter)
    est.fit_phase_s_ = {"fit_s": _time.perf_counter() - t0}
    est.fit_restart_inertias_ = restart_inertias
    est._mean = np.zeros(sd.d)
    est._engine_comm = engine.comm
    _warn_distinct(est.labels_, est.n_clusters)
    return est


# ------------------------------------------------------ mini-batch k-means
# Reference: ``cluster/_kmeans.py`` MiniBatchKMeans on CSR (``fit`` :1470,
# ``partial_fit`` :1638, ``_mini_batch_step`` :1133-1150).  The loop is the
# dense path's (``minibatch.py``), draw for draw; a step never copies or
# densifies the batch: ``ops.sparse_kmeans.MiniBatchState`` walks the id list.
def take_rows(sd, ids):
    """The rows ``ids`` (any order, repeats allowed) as a new CSR container,
    built with torch ops on the device."""
    ids = torch.as_tensor(ids, dtype=torch.int64).to(sd.device)
    lo = sd.indptr[ids]
    cnt = sd.indptr[ids + 1] - lo
    indptr = torch.zeros(ids.numel() + 1, dtype=torch.int64, device=sd.device)
    indptr[1:] = torch.cumsum(cnt, 0)
    total = int(indptr[-1])
    src = torch.arange(total, dtype=torch.int64, device=sd.device) \
        + torch.repeat_interleave(lo - indptr[:-1], cnt, output_size=total)
    return SparseData(indptr, sd.indices[src].contiguous(), sd.data[src].contiguous(),
                      (ids.numel(), sd.d))


def _mb_init_centers(est, X, sd, rs, xn):
    """``MiniBatchKMeans._init_centers`` on CSR: the same host draws."""
    n, k = sd.shape[0], est.n_clusters
    init = est.init
    if hasattr(init, "__array__"):
        C = torch.as_tensor(np.asarray(init, dtype=np.float64)).to(sd.device)
    else:
        idx = rs.randint(0, n, est._init_size)
        if isinstance(init, str) and init == "k-means++":
            sub = take_rows(sd, idx)
            sub_xn = xn[torch.as_tensor(idx, dtype=torch.int64).to(sd.device)].contiguous()
            C, _ = sparse_kmeans_plusplus(sub, k, rs, xn=sub_xn,
                                          gather=lambda r: S.sp_rows_dense(sub, np.asarray(r)))
        elif isinstance(init, str) and init == "random":
            sel = rs.permutation(len(idx))[:k]
            C = S.sp_rows_dense(sd, idx[sel])
        elif callable(init):
            C = torch.as_tensor(np.asarray(init(X.tocsr()[idx], k, rs),
                                           dtype=np.float64)).to(sd.device)
        else:
            raise ValueError("init should be 'k-means++', 'random' or an ndarray, "
                             f"got {init!r}")
    if tuple(C.shape) != (k, sd.d):
        raise ValueError(f"The shape of the initial centers {tuple(C.shape)} does not match the "
                         f"number of clusters {k} / features {sd.d}.")
    return C.double()


def _mb_reassign(est, st, sd, rows, rs):
    """Random reassignment of starved centres (``_mini_batch_step``
    :1093-1117) from the batch's CSR rows; True when centres were replaced."""
    counts = st.counts
    m = sd.shape[0] if rows is None else rows.numel()
    to_reassign = counts < est.reassignment_ratio * counts.max()
    nre = int(to_reassign.sum())                      # the step's one extra read
    if nre > 0.5 * m:
        keep = torch.argsort(counts)[int(0.5 * m):]
        to_reassign[keep] = False
        nre = int(to_reassign.sum())
    if not nre:
        return False
    new = torch.as_tensor(rs.choice(m, replace=False, size=nre), dtype=torch.int64).to(sd.device)
    dst = torch.nonzero(to_reassign)[:, 0]
    S.sp_rows_dense(sd, new if rows is None else rows[new], out=st.C, dst=dst)
    counts[to_reassign] = counts[~to_reassign].min()
    return True


def _mb_state(est, sd, sw, C, counts):
    if sd.device.type == "cuda":
        S.check_k(est.n_clusters)
    mx = float(sd.data.abs().max()) if sd.nnz else 0.0
    mw = None if sw is None else (float(sw.abs().max()) if sw.numel() else 0.0)
    return S.MiniBatchState(sd.device, C, counts, mx, mw)


def _mb_publish(est, st):
    est._C, est._counts = st.C, st.counts
    est.cluster_centers_ = to_numpy(st.C.double())
    est.counts_ = to_numpy(st.counts)


def _mb_labels(est, sd, st, sw, xn):
    labels, _, inertia = S.sp_list_estep(sd, st.C, None, sw, xn=xn, operand=st.operand())
    est.labels_ = to_numpy(labels).astype(np.int32)
    est.inertia_ = float(inertia)


def minibatch_fit(est, X, sample_weight=None):
    """``MiniBatchKMeans.fit`` on a scipy sparse matrix."""
    sd = as_sparse_data(X, device=est.device)
    n, d = sd.shape
    est._check_params(n)
    est.n_features_in_ = d
    rs = check_random_state(est.random_state)
    sw = _weights(sample_weight, sd)
    tol = _tolerance(X, est.tol) if est.tol > 0.0 else 0.0
    n_batches = int(np.ceil(n / est.batch_size))
    n_iter = int(est.max_iter * n_batches)
    k = est.n_clusters
    xn = S.sp_row_norms(sd)
    zeros = torch.zeros(k, dtype=torch.float64)
    vidx = torch.as_tensor(rs.randint(0, n, est._init_size), dtype=torch.int64).to(sd.device)
    wv = None if sw is None else sw[vidx]
    best = None
    for _ in range(est._n_init):
        st = _mb_state(est, sd, sw, _mb_init_centers(est, X, sd, rs, xn), zeros)
        st.advance(sd, xn, vidx, wv)
        inertia = float(st.estep(sd, xn, vidx, wv)[2])
        if best is None or inertia < best[0]:
            best = (inertia, st)
    st = best[1]
    min_count = float(st.counts.min())
    ctx = {}
    it = 0
    for it in range(n_iter):
        rows = torch.as_tensor(rs.randint(0, n, est.batch_size), dtype=torch.int64).to(sd.device)
        reassign = None
        if (it + 1) % (10 + int(min_count)) == 0 and est.reassignment_ratio > 0:
            def reassign(s, rows=rows):
                return _mb_reassign(est, s, sd, rows, rs)
        inertia, diff, min_count = st.step(sd, xn, rows, None if sw is None else sw[rows],
                                           reassign)
        if est._converged(it, n_iter, tol, n, diff if tol > 0.0 else 0.0, inertia, ctx):
            break
    est.n_iter_ = it + 1
    est.n_steps_ = it + 1
    _mb_publish(est, st)
    if est.compute_labels:
        _mb_labels(est, sd, st, sw, xn)
    return est


def minibatch_partial_fit(est, X, sample_weight=None):
    """``MiniBatchKMeans.partial_fit`` on a scipy sparse matrix: one step over
    all rows of ``X``."""
    sd = as_sparse_data(X, device=est.device)
    n, d = sd.shape
    sw = _weights(sample_weight, sd)
    if not hasattr(est, "_rs"):
        est._rs = check_random_state(est.random_state)
    xn = S.sp_row_norms(sd)
    reassign = None
    if not hasattr(est, "_C"):
        est._check_params(n)
        est.n_features_in_ = d
        counts = torch.zeros(est.n_clusters, dtype=torch.float64)
        C = _mb_init_centers(est, X, sd, est._rs, xn)
        est.n_steps_ = 0
    else:
        if d != est.n_features_in_:
            raise ValueError(f"X has {d} features, but MiniBatchKMeans is expecting "
                             f"{est.n_features_in_} features as input.")
        C, counts = est._C, est._counts
        # (a restored estimator holds its state as arrays)
        counts = torch.as_tensor(counts)
        if est._rs.randint(10 * (1 + int(counts.min()))) == 0 and est.reassignment_ratio > 0:
            def reassign(s):
                return _mb_reassign(est, s, sd, None, est._rs)
    st = _mb_state(est, sd, sw, C, counts)
    st.advance(sd, xn, None, sw, reassign)
    est.n_steps_ += 1
    _mb_publish(est, st)
    if est.compute_labels:
        _mb_labels(est, sd, st, sw, xn)
    return est


def minibatch_predict(est, X):
    sd, C = _fitted(est, X)
    return to_numpy(S.sp_list_estep(sd, C)[0]).astype(np.int32)


def minibatch_score(est, X, sample_weight=None):
    sd, C = _fitted(est, X)
    return -float(S.sp_list_estep(sd, C, None, _weights(sample_weight, sd))[2])
