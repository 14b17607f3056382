"""Brute-force k-nearest neighbours on MI355X.

Reference: ``sklearn/neighbors/_classification.py`` (``KNeighborsClassifier``)
and ``_base.py`` (``kneighbors``).  The reference chooses KD/Ball trees or
brute force on the CPU; on the GPU brute force wins for the dimensions of
the reference pipelines (MNIST-shape, d = 61-784): query tiles x reference
set distances by one library GEMM, then the per-row top-k selection kernel
(``csrc/knn.hip``).  Tiles are sized by ``working_memory``.
"""

import numpy as np
import torch

from ...base import BaseEstimator, ClassifierMixin, RegressorMixin
from ...utils.validation import check_is_fitted, check_array
from ...utils.pairwise import get_chunk_n_rows
from ...runtime.device import resolve_device, to_numpy
from ...ops import _native as nat


def _topk_rows(D, k, col_offset=0):
    """(dist, idx) of the k smallest entries per row of D."""
    if nat.use_native(D) and k <= 32:
        m, nref = D.shape
        D = D.contiguous()
        od = torch.empty((m, k), dtype=torch.float32, device=D.device)
        oi = torch.empty((m, k), dtype=torch.int64, device=D.device)
        nat.native().knn_topk(D.data_ptr(), od.data_ptr(), oi.data_ptr(), m, nref, D.stride(0), k,
                              int(col_offset), nat.stream_handle(D.device))
        return od, oi
    v, i = torch.topk(D, k, dim=1, largest=False, sorted=True)
    return v, i + col_offset


# Query rows per library GEMM call on the device.  The BLAS picks its kernel,
# and with it the summation order, by the shape of the product: an 8-row
# tile of q @ X.T differs from the same rows of a 40-row tile in most entries
# at d = 61 (one fp32 ulp).  So the products are always formed in slabs of
# _gemm_rows(n_fit) query rows at row offsets that are multiples of it (only
# the query's last slab is shorter), and a distance tile is a whole number
# of slabs: every GEMM call is then the same call whatever
# ``working_memory`` is, and ``kneighbors`` returns the same bits for every
# tile size.  A query of at most one slab is the one GEMM it was before.
# The slab height depends on the fitted set alone: 1024 rows while such a
# slab of products stays within 256 MiB, down to 128 for larger sets.
# Measured against one GEMM per tile (queries x fit x d): 7000 x 63000 x 61
# 5.98 -> 6.08 ms, 10000 x 60000 x 784 14.77 -> 14.95 ms, 2000 x 1M x 64
# 82.3 -> 82.2 ms, 5000 x 5000 x 32 (launch-bound) 0.38 -> 0.43 ms; slabs of
# 128 rows there cost 1.09 ms, hence the larger slab for small fitted sets.
_SLAB_BYTES = 256 << 20


def _gemm_rows(n_fit):
    fit = _SLAB_BYTES // (4 * max(int(n_fit), 1))
    return 1 << max(7, min(10, fit.bit_length() - 1))


def _slab_products(Q, X, s, e, B):
    """Rows s:e of Q @ X.T (s a multiple of the slab height B), slab by slab."""
    G = torch.empty((e - s, X.shape[0]), dtype=Q.dtype, device=Q.device)
    XT = X.T
    for b in range(s, e, B):
        torch.mm(Q[b:min(b + B, e)], XT, out=G[b - s:min(b + B, e) - s])
    return G


def _drop_self(dist, ind, k):
    """Drop each sample itself (first occurrence of its own index) from the
    k + 1 neighbours of a self-query."""
    kk = ind.shape[1]
    keep = np.ones_like(ind, dtype=bool)
    self_pos = (ind == np.arange(ind.shape[0])[:, None])
    first = np.where(self_pos.any(1), self_pos.argmax(1), kk - 1)
    keep[np.arange(ind.shape[0]), first] = False
    return dist[keep].reshape(dist.shape[0], k), ind[keep].reshape(ind.shape[0], k)


class _NeighborsBase(BaseEstimator):
    def _fit_sparse(self, X):
        """Sparse rows stay CSR: euclidean / cosine brute force through
        ``ops.sparse_knn`` (the reference resolves ``algorithm='auto'`` to
        brute force on sparse input)."""
        from ...models._data import as_sparse_data
        from ...ops._csr import sp_row_norms
        from ._extra import _is_euclidean
        algo = getattr(self, "algorithm", "auto")
        if algo in ("kd_tree", "ball_tree"):
            raise ValueError(f"{algo} does not work with sparse matrices. Densify the data, or "
                             "set algorithm='brute'")
        if algo not in ("auto", "brute"):
            raise ValueError(f"unrecognized algorithm: '{algo}'")
        euclid = _is_euclidean(self.metric, getattr(self, "p", 2), self.metric_params)
        if not euclid and self.metric != "cosine":
            raise ValueError(f"Metric '{self.metric}' is not supported on sparse input: the "
                             "sparse brute-force path computes 'euclidean' (or 'minkowski' with "
                             "p=2) and 'cosine'; densify the data for any other metric")
        self._sp = as_sparse_data(X, resolve_device(self.device))
        self._sp_xn = sp_row_norms(self._sp)
        self._X = None
        self._host = None
        self.n_samples_fit_, self.n_features_in_ = self._sp.shape
        self._fit_method = "brute"
        self.effective_metric_ = "euclidean" if euclid else self.metric
        return self

    def __getstate__(self):
        state = super().__getstate__()
        sd = state.get("_sp")
        if sd is not None:
            # host CSR arrays; caches (transpose, tile tables) are rebuilt on use
            state["_sp"] = (sd.indptr.cpu().numpy(), sd.indices.cpu().numpy(),
                            sd.data.cpu().numpy().astype(np.float64), sd.shape)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        sd = self.__dict__.get("_sp")
        if isinstance(sd, tuple):
            from ...models._data import SparseData
            self._sp = SparseData(torch.as_tensor(sd[0]), torch.as_tensor(sd[1]),
                                  torch.as_tensor(sd[2]), sd[3])
            self._sp_xn = torch.as_tensor(self._sp_xn)

    def _kneighbors_sparse(self, X, k, return_distance):
        from ...models._data import as_sparse_data
        from ...ops._csr import sp_row_norms
        from ...ops.sparse_knn import sp_knn
        import scipy.sparse as sp
        fit = self._sp
        query_is_train = X is None
        kk = k + 1 if query_is_train else k
        if kk > self.n_samples_fit_:
            raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = "
                             f"{self.n_samples_fit_}, n_neighbors = {kk}")
        if query_is_train:
            Q, qn = fit, self._sp_xn
        else:
            if not sp.issparse(X):
                # a dense query against a sparse fit: CSR of its nonzeros
                X = sp.csr_matrix(np.asarray(check_array(to_numpy(X)), dtype=np.float64))
            Q = as_sparse_data(X, fit.device)
            qn = sp_row_norms(Q)
        D, idx = sp_knn(fit, Q, kk, metric=self.effective_metric_, xn=self._sp_xn, qn=qn)
        if self.effective_metric_ == "euclidean":
            D = torch.sqrt(D)
        dist, ind = D.cpu().numpy(), idx.cpu().numpy()
        if query_is_train:
            dist, ind = _drop_self(dist, ind, k)
        return (dist, ind) if return_distance else ind

    def _fit(self, X, y=None):
        import scipy.sparse as sp
        if sp.issparse(X):
            return self._fit_sparse(X)
        self._sp = None
        dev = resolve_device(self.device)
        if isinstance(X, torch.Tensor):
            Xt = X.to(dev)
        else:
            Xt = torch.as_tensor(np.asarray(check_array(X), dtype=np.float64)).to(dev)
        self._dt = torch.float64 if dev.type == "cpu" else torch.float32
        self._X = Xt.to(self._dt).contiguous()
        self._xn = (self._X * self._X).sum(1)
        self.n_features_in_ = self._X.shape[1]
        self.n_samples_fit_ = self._X.shape[0]
        # euclidean + auto/brute -> device GEMM + top-k; anything else (other
        # metrics, explicit kd_tree / ball_tree) -> host trees / pairwise
        from ._extra import _HostEngine, _is_euclidean
        euclid = _is_euclidean(self.metric, getattr(self, "p", 2), self.metric_params)
        algo = getattr(self, "algorithm", "auto")
        self._host = None
        if not euclid or algo in ("kd_tree", "ball_tree"):
            self._host = _HostEngine(to_numpy(Xt).astype(np.float64), algo, self.metric,
                                     getattr(self, "p", 2), self.metric_params,
                                     getattr(self, "leaf_size", 30))
        self._fit_method = self._host.method if self._host is not None else "brute"
        self.effective_metric_ = "euclidean" if euclid else self.metric
        return self

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
        check_is_fitted(self, "_X")
        if X is not None and np.shape(X)[-1] != self.n_features_in_:
            raise ValueError(f"X has {np.shape(X)[-1]} features, but {type(self).__name__} is "
                             f"expecting {self.n_features_in_} features as input.")
        k = self.n_neighbors if n_neighbors is None else n_neighbors
        if getattr(self, "_sp", None) is not None:
            return self._kneighbors_sparse(X, k, return_distance)
        import scipy.sparse as sp
        if sp.issparse(X):
            X = X.toarray()      # a sparse query against a dense fit is small: densify
        if getattr(self, "_host", None) is not None:
            return self._host.kneighbors(X, k, return_distance)
        dev = self._X.device
        query_is_train = X is None
        Q = self._X if query_is_train else torch.as_tensor(
            np.asarray(to_numpy(X), dtype=np.float64)).to(dev).to(self._dt)
        kk = k + 1 if query_is_train else k
        if kk > self.n_samples_fit_:
            raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = "
                             f"{self.n_samples_fit_}, n_neighbors = {kk}")
        rows = get_chunk_n_rows(4 * self.n_samples_fit_)
        slabs = nat.use_native(Q)
        if slabs:
            # whole slabs per tile (at least one: working_memory is honoured
            # in units of one slab of query rows); the norms once for all rows
            B = _gemm_rows(self.n_samples_fit_)
            rows = max(B, rows // B * B)
            qn = (Q * Q).sum(1)
        dists, idxs = [], []
        for s in range(0, Q.shape[0], rows):
            q = Q[s:s + rows]
            if slabs:
                D = (qn[s:s + rows, None] + self._xn[None, :]
                     - 2.0 * _slab_products(Q, self._X, s, s + q.shape[0], B)).clamp_(min=0)
            else:
                D = ((q * q).sum(1)[:, None] + self._xn[None, :]
                     - 2.0 * (q @ self._X.T)).clamp_(min=0)
            if D.dtype != torch.float32 and nat.use_native(D):
                D = D.float()
            v, i = _topk_rows(D, kk)
            dists.append(v.to(torch.float64))
            idxs.append(i)
        dist = torch.sqrt(torch.cat(dists)).cpu().numpy()
        ind = torch.cat(idxs).cpu().numpy()
        if query_is_train:
            dist, ind = _drop_self(dist, ind, k)
        return (dist, ind) if return_distance else ind


class KNeighborsClassifier(ClassifierMixin, _NeighborsBase):
    def __init__(self, n_neighbors=5, *, weights="uniform", algorithm="auto", leaf_size=30, p=2,
                 metric="minkowski", metric_params=None, n_jobs=None, device=None):
        self.n_neighbors = n_neighbors
        self.weights = weights
        self.algorithm = algorithm
        self.leaf_size = leaf_size
        self.p = p
        self.metric = metric
        self.metric_params = metric_params
        self.n_jobs = n_jobs
        self.device = device

    def fit(self, X, y):
        X, y = self._validate_data(X, y, accept_sparse=True) \
            if not isinstance(X, torch.Tensor) else (X, y)
        self._fit(X)
        y = np.asarray(to_numpy(y))
        self.classes_, self._y = np.unique(y, return_inverse=True)
        self.outputs_2d_ = False
        return self

    def _weights(self, dist):
        if self.weights == "uniform":
            return np.ones_like(dist)
        if self.weights == "distance":
            with np.errstate(divide="ignore"):
                w = 1.0 / dist
            inf = np.isinf(w)
            w[inf.any(1)] = inf[inf.any(1)].astype(float)
            return w
        if callable(self.weights):
            return self.weights(dist)
        raise ValueError("weights not recognized")

    def predict_proba(self, X):
        dist, ind = self.kneighbors(X)
        w = self._weights(dist)
        lab = self._y[ind]
        P = np.zeros((ind.shape[0], len(self.classes_)))
        for c in range(len(self.classes_)):
            P[:, c] = (w * (lab == c)).sum(1)
        P /= P.sum(1, keepdims=True)
        return P

    def predict(self, X):
        return self.classes_[np.argmax(self.predict_proba(X), axis=1)]


class KNeighborsRegressor(RegressorMixin, _NeighborsBase):
    def __init__(self, n_neighbors=5, *, weights="uniform", algorithm="auto", leaf_size=30, p=2,
                 metric="minkowski", metric_params=None, n_jobs=None, device=None):
        self.n_neighbors = n_neighbors
        self.weights = weights
        self.algorithm = algorithm
        self.leaf_size = leaf_size
        self.p = p
        self.metric = metric
        self.metric_params = metric_params
        self.n_jobs = n_jobs
        self.device = device

    def fit(self, X, y):
        self._fit(X)
        self._yv = np.asarray(to_numpy(y), dtype=np.float64)
        return self

    def predict(self, X):
        dist, ind = self.kneighbors(X)
        if self.weights == "distance":
            with np.errstate(divide="ignore"):
                w = 1.0 / dist
            w[np.isinf(w).any(1)] = np.isinf(w[np.isinf(w).any(1)]).astype(float)
        else:
            w = np.ones_like(dist)
        return (w * self._yv[ind]).sum(1) / w.sum(1)


class NearestNeighbors(_NeighborsBase):
    def __init__(self, n_neighbors=5, *, radius=1.0, algorithm="auto", leaf_size=30,
                 metric="minkowski", p=2, metric_params=None, n_jobs=None, device=None):
        self.n_neighbors = n_neighbors
        self.radius = radius
        self.algorithm = algorithm
        self.leaf_size = leaf_size
        self.metric = metric
        self.p = p
        self.metric_params = metric_params
        self.n_jobs = n_jobs
        self.device = device

    def fit(self, X, y=None):
        return self._fit(X)
