"""Shared input handling for the estimators: numpy / tensor / ShardedArray
-> (local device tensor, global geometry, communicator), plus the global
(cross-rank) statistics every estimator needs."""

import numpy as np
import torch

from ..parallel.comm import Comm
from ..parallel.sharding import ShardedArray
from ..runtime.device import resolve_device
from ..utils.validation import check_array
from ..ops import linalg as L


class Data:
    """Local rows of a (possibly sharded) dataset on the compute device."""

    def __init__(self, local, n_global, row_offset, comm, source_kind):
        self.X = local
        self.n_global = int(n_global)
        self.row_offset = int(row_offset)
        self.comm = comm
        self.source_kind = source_kind   # 'numpy' | 'tensor' | 'sharded'

    @property
    def n_local(self):
        return self.X.shape[0]

    @property
    def d(self):
        return self.X.shape[1]

    @property
    def device(self):
        return self.X.device


def as_data(X, device=None, dtype=None, copy=False, comm=None):
    """Validate and place X.  ``dtype=None``: float64 on CPU, float32 on GPU
    (bf16 tensors are kept as given - they are the data)."""
    dev = resolve_device(device)
    if isinstance(X, ShardedArray):
        loc = X.local
        if loc.device != dev:
            loc = loc.to(dev)
        loc = _cast(loc, dev, dtype)
        check_array(loc, dtype=None, ensure_min_samples=0)
        return Data(loc.contiguous(), X.n_global, X.row_offset, X.comm, "sharded")
    comm = comm if comm is not None else Comm(None)
    if isinstance(X, torch.Tensor):
        t = check_array(X, dtype=None)
        if not t.is_floating_point():
            t = t.double()
        t = t.to(dev) if t.device != dev else (t.clone() if copy else t)
        t = _cast(t, dev, dtype)
        return Data(t.contiguous(), t.shape[0], 0, comm, "tensor")
    arr = check_array(X, dtype=[np.float64, np.float32])
    t = torch.as_tensor(np.ascontiguousarray(arr))
    t = _cast(t, dev, dtype)
    t = t.to(dev)
    return Data(t.contiguous(), t.shape[0], 0, comm, "numpy")


def _cast(t, dev, dtype):
    if dtype is not None:
        return t.to(dtype)
    if t.dtype == torch.bfloat16:
        return t
    if dev.type == "cuda" and t.dtype == torch.float64:
        return t.to(torch.float32)
    if not t.is_floating_point():
        return t.to(torch.float64 if dev.type == "cpu" else torch.float32)
    return t


def global_sum(data: Data, t):
    data.comm.all_reduce_(t)
    return t


def global_mean_var(data: Data):
    """Column mean and (population) variance over all ranks in one collective."""
    X = data.X
    s, ss = L.col_moments_local(X)
    buf = torch.cat([s, ss])
    data.comm.all_reduce_(buf)
    d = X.shape[1]
    mean = buf[:d] / data.n_global
    var = (buf[d:] / data.n_global - mean ** 2).clamp(min=0.0)
    return mean, var


def gather_rows(data: Data, global_idx):
    """Rows with the given global indices, replicated on every rank (one
    all-reduce: owners contribute their rows, others zeros)."""
    idx = torch.as_tensor(np.asarray(global_idx, dtype=np.int64), device=data.device)
    out = torch.zeros((idx.numel(), data.d), dtype=torch.float64 if data.device.type == "cpu"
                      else torch.float32, device=data.device)
    lo, hi = data.row_offset, data.row_offset + data.n_local
    mine = (idx >= lo) & (idx < hi)
    if bool(mine.any()):
        out[mine] = data.X[idx[mine] - lo].to(out.dtype)
    data.comm.all_reduce_(out)
    return out


def prelude_stats(data: Data, mu_start=0.0, mu_end=1.0, mu_step=0.1, condition=True):
    """eta = max ||x||^2, mu(A) p-grid search and 1/sigma_min on the raw data
    (reference ``_dmeans.py:1242-1245``, ``_qPCA.py:634-636``), all ranks."""
    X = data.X
    rn = L.row_norms_sq(X).double()
    eta = torch.tensor([float(rn.max()) if rn.numel() else 0.0], dtype=torch.float64, device=X.device)
    data.comm.all_reduce_(eta, op="max")
    eta = float(eta.item())
    label, mu = best_mu_distributed(data, mu_start, mu_end, mu_step, fro_sq=float(rn.sum()))
    cond = None
    if condition:
        smin = sigma_min(data)
        cond = float("inf") if smin == 0 else 1.0 / smin
    return eta, label, mu, cond


def _mu_grid(start, end, step):
    """The p-grid of ``best_mu`` and the exponents 2p, 2(1 - p) its power sums need."""
    domain = [i for i in np.arange(start, end, step)] + [end]
    exps = sorted(set([round(float(2 * p), 12) for p in domain] +
                      [round(float(2 * (1 - p)), 12) for p in domain]))
    return domain, exps


def _mu_search(domain, exps, rowmax, colsum):
    """sqrt(s_2p(A) s_2(1-p)(A^T)) for every p of the grid and the position of
    the smallest, from the (global) row maxima [nq] and column sums [nq, d]."""
    colmax = colsum.max(dim=1).values
    pos = {e: i for i, e in enumerate(exps)}
    vals = []
    for p in domain:
        s1 = float(rowmax[pos[round(float(2 * p), 12)]])
        s2 = float(colmax[pos[round(float(2 * (1 - p)), 12)]])
        vals.append(float(np.sqrt(s1 * s2)))
    return vals, int(np.argmin(vals))


def best_mu_distributed(data: Data, start=0.0, end=1.0, step=0.05, fro_sq=None, fro_sq_global=None,
                        mean=None):
    """``best_mu`` (``Utility.py:196-231``) over a row-sharded matrix: one
    fused power-sum pass (row-max and column sums for every exponent of the
    p-grid), then MAX / SUM all-reduces.  ``mean``: mu of the centred matrix
    X - mean, subtracted inside the pass."""
    domain, exps = _mu_grid(start, end, step)
    rowmax, colsum = L.mu_power_sums_local(data.X, exps, mean=mean)
    data.comm.all_reduce_(rowmax, op="max")
    data.comm.all_reduce_(colsum, op="sum")
    vals, best = _mu_search(domain, exps, rowmax, colsum)
    if fro_sq_global is not None:
        fro = float(np.sqrt(fro_sq_global))
    else:
        if fro_sq is None:
            Xd = data.X.double() if mean is None else data.X.double() - mean.double().to(data.device)
            fro_sq = float((Xd ** 2).sum())
        t = torch.tensor([fro_sq], dtype=torch.float64, device=data.device)
        data.comm.all_reduce_(t)
        fro = float(np.sqrt(t.item()))
    if vals[best] <= fro:
        return f"p={domain[best]}", vals[best]
    return "Frobenius", fro


def sigma_min(data: Data, mean=None):
    """Smallest singular value of the (optionally centred) global matrix.

    The reference takes it from an fp64 LAPACK SVD of X
    (``_dmeans.py:1244-1245``).  Here: sharded CholeskyQR2 in fp64
    (:func:`ops.linalg.cholqr2_r`, two passes over X, two d x d
    all-reduces) and the singular values of the d x d R - accurate to
    ~eps64 * cond(X) relative.  Rank-deficient / cond >~ 1e8 matrices fall
    back to the square roots of the fp64 Gram eigenvalues."""
    n, d = data.n_global, data.d
    if n < d:
        full = gather_full(data).double()
        if mean is not None:
            full = full - mean.double().to(full.device)
        s = torch.linalg.svdvals(full)
        return float(s.min()) if s.numel() else 0.0
    R = L.cholqr2_r(data.X, data.comm, mean)
    if R is not None:
        return float(torch.linalg.svdvals(R.cpu()).min())      # d x d, host LAPACK
    G = data.comm.all_reduce_(L.gram64_local(data.X, mean)).cpu()
    ev = torch.linalg.eigvalsh(0.5 * (G + G.T))
    return float(torch.sqrt(ev.clamp(min=0.0)).min())


def gather_full(data: Data):
    if data.comm.world_size == 1:
        return data.X
    return torch.cat(data.comm.all_gather_varlen(data.X), 0)


def check_n_features(est, data):
    """Raise like the reference's ``_check_n_features(reset=False)``."""
    n_in = getattr(est, "n_features_in_", None)
    if n_in is not None and data.d != n_in:
        raise ValueError(f"X has {data.d} features, but {type(est).__name__} is expecting "
                         f"{n_in} features as input.")
    return data


class SparseData:
    """A CSR matrix on the compute device (single process): ``indptr``
    (int64), ``indices`` (int32) and ``data`` (fp32 on GPU, fp64 on CPU - the
    dense dtype policy), canonical (sorted column indices, no duplicates;
    explicitly stored zeros are kept)."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr = indptr
        self.indices = indices
        self.data = data
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(data.numel())
        self.n_global = self.shape[0]
        self.row_offset = 0
        self.comm = Comm(None)
        self.source_kind = "sparse"
        self._rows = None
        # caches of ops/sparse_linalg.py (the sparsity structure never changes)
        self._transpose = None
        self._segments = {}
        # tile pointer tables of ops/sparse_knn.py, by tile size
        self._knn_tables = {}
        # (max |value|, largest column count) of ops/sparse_lda.py: the fixed-point bound
        self._lda_bound = None

    @property
    def n_local(self):
        return self.shape[0]

    @property
    def d(self):
        return self.shape[1]

    @property
    def device(self):
        return self.data.device

    def row_ids(self):
        """Row index of every stored value (int64, cached)."""
        if self._rows is None:
            cnt = self.indptr[1:] - self.indptr[:-1]
            self._rows = torch.repeat_interleave(
                torch.arange(self.shape[0], dtype=torch.int64, device=self.device), cnt,
                output_size=self.nnz)
        return self._rows

    def dense_rows(self, s, e, dtype=torch.float64):
        """Rows [s, e) as a dense (e - s, d) tensor of ``dtype``."""
        lo, hi = int(self.indptr[s]), int(self.indptr[e])
        out = torch.zeros((e - s) * self.d, dtype=dtype, device=self.device)
        if hi > lo:
            flat = (self.row_ids()[lo:hi] - s) * self.d + self.indices[lo:hi].to(torch.int64)
            out.index_add_(0, flat, self.data[lo:hi].to(dtype))
        return out.view(e - s, self.d)

    def gather_dense(self, rows, dtype=torch.float64):
        """The given rows (any order, repeats allowed) as a dense tensor."""
        rows = [int(r) for r in np.asarray(rows).reshape(-1)]
        out = torch.zeros((len(rows), self.d), dtype=dtype, device=self.device)
        for t, r in enumerate(rows):
            lo, hi = int(self.indptr[r]), int(self.indptr[r + 1])
            if hi > lo:
                out[t].index_add_(0, self.indices[lo:hi].to(torch.int64),
                                  self.data[lo:hi].to(dtype))
        return out


def as_sparse_data(X, device=None):
    """Validate a ``scipy.sparse`` matrix and place it on the device as CSR.
    The caller's matrix is never mutated (sorting / duplicate summing run on a
    copy)."""
    import scipy.sparse as sp
    if not sp.issparse(X):
        raise TypeError("as_sparse_data expects a scipy.sparse matrix")
    dev = resolve_device(device)
    A = X.tocsr()                      # CSR input: no copy yet
    if not A.has_canonical_format:
        if A is X:
            A = A.copy()
        A.sum_duplicates()
        A.sort_indices()
    n, d = A.shape
    if n < 1:
        raise ValueError(f"Found array with {n} sample(s) (shape={A.shape}) while a minimum of 1 "
                         "is required.")
    if d < 1:
        raise ValueError(f"Found array with {d} feature(s) (shape={A.shape}) while a minimum of 1 "
                         "is required.")
    if d >= 2 ** 31:
        raise ValueError("sparse input supports fewer than 2^31 features")
    if not np.isfinite(A.data).all():
        raise ValueError("Input contains NaN, infinity or a value too large for dtype('float64').")
    if A.nnz and (A.indices.min() < 0 or A.indices.max() >= d):
        raise ValueError("CSR column index out of range")
    # a fresh array in the compute dtype: the container never aliases the caller's values
    vals = torch.from_numpy(np.array(A.data, dtype=np.float32 if dev.type == "cuda"
                                     else np.float64))
    return SparseData(torch.as_tensor(A.indptr.astype(np.int64)).to(dev),
                      torch.as_tensor(A.indices.astype(np.int32)).to(dev),
                      vals.to(dev).contiguous(), (n, d))


def sparse_mean_var(sd):
    """Column mean and (population) variance of a CSR matrix, fp64 [d] each,
    from its column moments (``ops.sparse_linalg.sp_col_moments``)."""
    from ..ops import sparse_linalg
    s, ss = sparse_linalg.sp_col_moments(sd)
    n = sd.shape[0]
    mean = s / n
    return mean, (ss / n - mean ** 2).clamp(min=0.0)


def best_mu_sparse(sd, mean, start, end, step, fro_sq_global):
    """:func:`best_mu_distributed` for the centred CSR matrix X - mean, which
    is never formed (``ops.sparse_linalg.sp_mu_power_sums``)."""
    from ..ops import sparse_linalg
    domain, exps = _mu_grid(start, end, step)
    rowmax, colsum = sparse_linalg.sp_mu_power_sums(sd, exps, mean=mean)
    vals, best = _mu_search(domain, exps, rowmax, colsum)
    fro = float(np.sqrt(fro_sq_global))
    if vals[best] <= fro:
        return f"p={domain[best]}", vals[best]
    return "Frobenius", fro
