"""PCA base class (reference ``sklearn/decomposition/_base.py`` incl. the
fork's ``use_classical_components`` switch at :97-164).

``transform`` / ``inverse_transform`` project on ``components_`` (classical)
or on ``estimate_right_sv`` (the tomography estimates of the right singular
vectors produced by ``QPCA(estimate_all=True)``).  Inputs may be numpy,
tensors (any device) or row-sharded arrays; outputs follow the input kind
(numpy in -> numpy out).
"""

import numbers

import numpy as np
import scipy.sparse as sp
import torch
from scipy import linalg

from ...base import BaseEstimator, TransformerMixin
from ...ops import sparse_linalg
from ...utils.extmath import randomized_svd_sparse
from ...utils.validation import check_is_fitted, seed_from_random_state
from ...runtime.device import to_numpy, resolve_device
from .._data import as_data, as_sparse_data, sparse_mean_var

# sparse input of at most this many elements is densified (the exact branch)
_SPARSE_DENSIFY_MAX = 4e6


def _as_out(t, kind):
    return to_numpy(t) if kind == "numpy" else t


def _stays_sparse(X):
    """``scipy.sparse`` rows above the densify limit: they stay CSR."""
    return sp.issparse(X) and X.shape[0] * X.shape[1] > _SPARSE_DENSIFY_MAX


def _sparse_solver(name, svd_solver, n_components, n_samples, n_features):
    """(n_components, solver) of a fit on CSR rows above the densify limit:
    the dense selection rule, with everything that needs the full spectrum
    refused (``'full'``, also as the choice of ``'auto'``; ``n_components``
    None, ``'mle'`` or a fraction)."""
    if svd_solver not in ("auto", "full", "arpack", "randomized"):
        raise ValueError(f"Unrecognized svd_solver='{svd_solver}'")
    k = n_components
    integral = isinstance(k, numbers.Integral) and not isinstance(k, bool)
    solver = svd_solver
    if solver == "auto":    # max(n, d) > 500 holds above the limit
        solver = "randomized" if integral and 1 <= k < 0.8 * min(n_samples, n_features) \
            else "full"
    if solver == "full" or not integral:
        raise ValueError(f"{name} keeps sparse input of more than {int(_SPARSE_DENSIFY_MAX)} "
                         "elements sparse and runs the centred randomized SVD on it: use "
                         "svd_solver='randomized' with an integer n_components (got "
                         f"svd_solver={svd_solver!r}, n_components={n_components!r}); the "
                         "full spectrum needs a dense matrix")
    if not 1 <= k <= min(n_samples, n_features):
        raise ValueError(f"n_components={k!r} must be between 1 and "
                         f"min(n_samples, n_features)={min(n_samples, n_features)!r} with "
                         f"svd_solver='{solver}'")
    if solver == "arpack" and k == min(n_samples, n_features):
        raise ValueError(f"n_components={k!r} must be strictly less than "
                         f"min(n_samples, n_features)={min(n_samples, n_features)!r} with "
                         f"svd_solver='{solver}'")
    return int(k), solver


class _BasePCA(TransformerMixin, BaseEstimator):

    def _fit_sparse(self, X, arpack_min_iter=None):
        """Fit on ``scipy.sparse`` rows above the densify limit: the column
        moments give ``mean_`` and the total variance, the centred randomized
        SVD (``utils.extmath.randomized_svd_sparse`` with the mean as a
        rank-one term) the factors; the attributes follow the dense truncated
        fit.  Neither an n x d nor a d x d dense array is formed.  Returns
        (sd, mean, var, U [n, k] fp64 on the device, S)."""
        sd = as_sparse_data(X, device=getattr(self, "device", None))
        n_samples, n_features = sd.shape
        k, solver = _sparse_solver(type(self).__name__, self.svd_solver, self.n_components,
                                   n_samples, n_features)
        self.n_features_in_ = n_features
        self._fit_svd_solver = solver
        mean, var = sparse_mean_var(sd)
        self.mean_ = to_numpy(mean)
        n_iter = self.iterated_power
        if solver == "arpack" and arpack_min_iter is not None:
            n_iter = max(arpack_min_iter, n_iter if isinstance(n_iter, int) else arpack_min_iter)
        U, S, Vt = randomized_svd_sparse(sd, k, n_iter=n_iter, mean=mean,
                                         seed=seed_from_random_state(self.random_state))
        S = S.cpu().numpy()
        self.n_samples_, self.n_features_ = n_samples, n_features
        self.components_ = Vt.cpu().numpy()
        self.n_components_ = k
        self.explained_variance_ = (S ** 2) / (n_samples - 1)
        total_var = to_numpy(var) * n_samples / (n_samples - 1)
        self.explained_variance_ratio_ = self.explained_variance_ / total_var.sum()
        self.singular_values_ = S.copy()
        if k < min(n_features, n_samples):
            self.noise_variance_ = (total_var.sum() - self.explained_variance_.sum()) / (
                min(n_features, n_samples) - k)
        else:
            self.noise_variance_ = 0.0
        return sd, mean, total_var, U, S

    def _transform_sparse(self, X, use_classical_components):
        """(X - mean_) basis^T on sparse rows: X basis^T by the sparse product
        (fp64), the mean as a row of the k-wide result.  numpy out."""
        sd = as_sparse_data(X, device=getattr(self, "device", None))
        if sd.d != self.n_features_in_:
            raise ValueError(f"X has {sd.d} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input.")
        basis = np.asarray(self._projection_basis(use_classical_components), dtype=np.float64)
        W = torch.as_tensor(np.ascontiguousarray(basis.T), device=sd.device)
        out = sparse_linalg.sp_xw(sd, W)
        if self.mean_ is not None:
            out -= torch.as_tensor(self.mean_, dtype=torch.float64, device=sd.device) @ W
        if self.whiten and use_classical_components:
            out /= torch.sqrt(torch.as_tensor(self.explained_variance_, dtype=torch.float64,
                                              device=sd.device))
        return to_numpy(out)

    def get_covariance(self):
        components_ = self.components_
        exp_var = self.explained_variance_
        if self.whiten:
            components_ = components_ * np.sqrt(exp_var[:, np.newaxis])
        exp_var_diff = np.maximum(exp_var - self.noise_variance_, 0.0)
        cov = np.dot(components_.T * exp_var_diff, components_)
        cov.flat[:: len(cov) + 1] += self.noise_variance_
        return cov

    def get_precision(self):
        n_features = self.components_.shape[1]
        if self.n_components_ == 0:
            return np.eye(n_features) / self.noise_variance_
        if self.n_components_ == n_features:
            return linalg.inv(self.get_covariance())
        components_ = self.components_
        exp_var = self.explained_variance_
        if self.whiten:
            components_ = components_ * np.sqrt(exp_var[:, np.newaxis])
        exp_var_diff = np.maximum(exp_var - self.noise_variance_, 0.0)
        precision = np.dot(components_, components_.T) / self.noise_variance_
        precision.flat[:: len(precision) + 1] += 1.0 / exp_var_diff
        precision = np.dot(components_.T, np.dot(linalg.inv(precision), components_))
        precision /= -(self.noise_variance_ ** 2)
        precision.flat[:: len(precision) + 1] += 1.0 / self.noise_variance_
        return precision

    def _projection_basis(self, use_classical_components):
        if use_classical_components:
            return self.components_
        if not hasattr(self, "estimate_right_sv"):
            raise AttributeError("estimate_right_sv is not available: fit with estimate_all=True")
        return to_numpy(self.estimate_right_sv)

    def transform(self, X, use_classical_components=True):
        """(X - mean_) @ basis^T (``_base.py:97-128``).  ``scipy.sparse`` rows
        stay sparse, whatever input the estimator was fitted on."""
        check_is_fitted(self)
        if sp.issparse(X):
            return self._transform_sparse(X, use_classical_components)
        data = as_data(X, device=getattr(self, "device", None))
        if data.d != self.n_features_in_:
            raise ValueError(f"X has {data.d} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input.")
        dt = torch.float64 if data.device.type == "cpu" else torch.float32
        basis = torch.as_tensor(np.asarray(self._projection_basis(use_classical_components)),
                                dtype=dt, device=data.device)
        Xt = data.X.to(dt)
        if self.mean_ is not None:
            Xt = Xt - torch.as_tensor(self.mean_, dtype=dt, device=data.device)
        out = Xt @ basis.T
        if self.whiten and use_classical_components:
            out = out / torch.sqrt(torch.as_tensor(self.explained_variance_, dtype=dt,
                                                   device=data.device))
        return _as_out(out, data.source_kind)

    def inverse_transform(self, X, use_classical_components=True):
        """X @ basis + mean_ (``_base.py:130-164``)."""
        check_is_fitted(self)
        basis = np.asarray(self._projection_basis(use_classical_components))
        if isinstance(X, torch.Tensor):
            dt = X.dtype if X.dtype in (torch.float32, torch.float64) else torch.float32
            B = torch.as_tensor(basis, dtype=dt, device=X.device)
            if self.whiten and use_classical_components:
                B = B * torch.sqrt(torch.as_tensor(self.explained_variance_, dtype=dt,
                                                   device=X.device))[:, None]
            return X.to(dt) @ B + torch.as_tensor(self.mean_, dtype=dt, device=X.device)
        X = np.asarray(X)
        if self.whiten and use_classical_components:
            return np.dot(X, np.sqrt(self.explained_variance_[:, np.newaxis]) * basis) + self.mean_
        return np.dot(X, basis) + self.mean_
