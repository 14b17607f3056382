"""Least-squares SVM classifiers: classical ``LSSVC`` and quantum-simulated
``QLSSVC``.

References: ``sklearn/svm/_classes.py:1465-1697`` (LSSVC) and
``sklearn/svm/_qSVM.py:10-404`` (QLSSVC).

The (N+1) x (N+1) system F = [[0, 1^T], [1, K + I/penalty]] is built on the
device (kernel matrix = one library GEMM + elementwise epilogue) and solved
by a symmetric eigendecomposition (QLSSVC: the reference's hermitian SVD with
optional low-rank truncation) or, for LSSVC 'cg', by batched conjugate
gradients on H = K + I/penalty.  Prediction is vectorised over test samples
(the reference loops per sample in Python).

Fixed reference defects (§2.8): ``LSSVC._cg_fit`` used the (x, info) tuple
from scipy's cg as an array and had the b / alpha formulas swapped - here
b = 1^T eta / 1^T nu, alpha = eta - nu b with H eta = y, H nu = 1, which
equals the direct solve; ``LSSVC.get_P`` used ||x_i|| in place of ||x_j||^2 -
here it uses QLSSVC's beta = sqrt((N ||x||^2 + 1) Nu).

Sparse input: scipy sparse ``X`` stays CSR (``self.X`` is the scipy matrix;
the device copy and its caches are private runtime state, dropped on
pickling).  The K block of F is written in place by
``ops.sparse_kernel.sp_kernel_matrix`` (``csrc/spgram.hip``), decision values
are ``sp_kernel_matvec(train, queries, alpha) + b`` without the M x N block,
and LSSVC 'cg' runs matrix-free once the N x N matrix would exceed
``SQ_SVM_DENSE_BYTES`` (there a kernel that is not positive semidefinite is
refused: no ``lstsq`` fallback exists without the matrix).  On a GPU the stored values are fp32.
"""

import math

import numpy as np
import scipy.sparse as sp
import torch

from ...base import BaseEstimator, ClassifierMixin
from ...utils.validation import check_is_fitted, check_array, seed_from_random_state
from ...utils import pairwise as PW
from ...utils.metrics import accuracy_score
from ...runtime.device import resolve_device, to_numpy
from ...runtime.rng import RngKey
from ...ops.random import trunc_normal_add_
from ...ops._csr import sp_row_norms
from ...ops.sparse_knn import TILE_DEFAULT, InvertedIndex
from ...ops.sparse_kernel import sp_kernel_matrix, sp_kernel_matvec
from ...ops.sparse_linalg import sp_xty
from .._data import SparseData, as_sparse_data
from ._libsvm import _dense_limit_bytes


# a smallest Ritz value this far (relative to the largest) below 1 / penalty is a
# negative eigenvalue of K, not the rounding of the Lanczos recurrence
_RITZ_TOL = 2.0 ** -26


def _ritz_range(coeffs, tol):
    """(smallest, largest) eigenvalue over the Lanczos tridiagonals that the CG
    coefficients of ``conjugate_gradient`` define, one per right-hand side:
    diagonal ``1 / alpha_k + beta_{k-1} / alpha_{k-1}``, off-diagonal
    ``sqrt(beta_k) / alpha_k``.  A column counts up to the iteration at which
    it met ``tol``: the steps it takes while another column still runs are
    rounding."""
    al, be, rel = (torch.stack([c[i] for c in coeffs]).cpu().numpy() for i in range(3))
    lo, hi = np.inf, -np.inf
    for c in range(al.shape[1]):
        done = np.nonzero(rel[:, c] <= tol ** 2)[0]
        k = int(done[0]) + 1 if done.size else al.shape[0]
        a, b = al[:k, c], be[:k, c]
        d = 1.0 / a
        d[1:] += b[:-1] / a[:-1]
        e = np.sqrt(b[:-1]) / a[:-1]
        ev = np.linalg.eigvalsh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
        lo, hi = min(lo, ev[0]), max(hi, ev[-1])
    return float(lo), float(hi)


class _KernelMixin:
    def _get_gamma(self, X):
        if self.gamma == "scale":
            if sp.issparse(X):
                # the variance over all n * d entries from the stored values
                size = X.shape[0] * X.shape[1]
                mean = X.data.sum() / size
                return 1.0 / (X.shape[1] * (np.square(X.data).sum() / size - mean * mean))
            Xn = to_numpy(X) if isinstance(X, torch.Tensor) else np.asarray(X)
            return 1.0 / (Xn.shape[1] * Xn.var())
        if self.gamma == "auto":
            return 1.0 / self.n_features_in_
        return float(self.gamma)

    def get_kernel(self, X, Y=None):
        """Kernel matrix K(X, Y) on the estimator device (tensor)."""
        dev = self._device()
        Xt = torch.as_tensor(np.asarray(to_numpy(X), dtype=np.float64), device=dev)
        Yt = None if Y is None else torch.as_tensor(np.asarray(to_numpy(Y), dtype=np.float64), device=dev)
        if self.kernel == "linear":
            return PW.linear_kernel(Xt, Yt)
        gamma = self._get_gamma(self._gamma_ref if hasattr(self, "_gamma_ref") else X)
        if self.kernel == "poly":
            return PW.polynomial_kernel(Xt, Yt, degree=self.degree, gamma=gamma, coef0=self.coef0)
        if self.kernel == "rbf":
            return PW.rbf_kernel(Xt, Yt, gamma=gamma)
        if self.kernel == "sigmoid":
            return PW.sigmoid_kernel(Xt, Yt, gamma=gamma, coef0=self.coef0)
        raise ValueError(f"unknown kernel {self.kernel!r}")

    def _device(self):
        dev = resolve_device(getattr(self, "device", None))
        return dev

    # ------------------------------------------------------- sparse rows
    def _fit_input(self, X, y):
        """Validated (X, y): scipy sparse ``X`` of any format as canonical
        fp64 CSR, anything else as a dense fp64 array."""
        X, y = self._validate_data(X, y, accept_sparse=True)
        self._engine_sparse = None
        if sp.issparse(X):
            X = X.tocsr().astype(np.float64)         # a copy: the caller's matrix stays as it is
            if not X.has_canonical_format:
                X.sum_duplicates()
                X.sort_indices()
        else:
            X = np.asarray(to_numpy(X), dtype=np.float64)
        return X, np.asarray(to_numpy(y), dtype=np.float64)

    def _sparse_fit(self):
        """True for an estimator fitted on scipy sparse rows."""
        return sp.issparse(getattr(self, "X", None))

    def _train(self):
        """(SparseData, InvertedIndex of the self-join) of the training rows
        on the estimator device: uploaded once, runtime state only."""
        eng = getattr(self, "_engine_sparse", None)
        if eng is None:
            sd = as_sparse_data(self.X, self._device())
            op = InvertedIndex(sd, sd, TILE_DEFAULT) if sd.device.type == "cuda" else None
            eng = self._engine_sparse = (sd, op)
        return eng

    def _queries(self, X):
        """Query rows of an estimator fitted on CSR as a ``SparseData`` on its
        device; dense rows are converted to CSR."""
        if isinstance(X, SparseData):
            return X
        if not sp.issparse(X):
            X = sp.csr_matrix(np.asarray(to_numpy(check_array(X)), dtype=np.float64))
        self._check_n_features(X, reset=False)
        return as_sparse_data(X, self._device())

    def _check_queries(self, X):
        """``check_array`` of the predict methods: sparse queries only for an
        estimator fitted on sparse rows."""
        check_is_fitted(self, "alpha_")
        if self._sparse_fit():
            return self._queries(X)
        return check_array(X)

    def _kernel_params(self):
        if self.kernel not in ("linear", "poly", "rbf", "sigmoid"):
            raise ValueError(f"unknown kernel {self.kernel!r}")
        gamma = 1.0 if self.kernel == "linear" else self._get_gamma(self._gamma_ref)
        return dict(kind=self.kernel, gamma=gamma, coef0=self.coef0, degree=self.degree)

    def _sparse_H(self, out=None):
        """K + I / penalty of the training rows in one pass, into ``out``."""
        sd, op = self._train()
        return sp_kernel_matrix(sd, sd, out=out, diag_add=1.0 / self.penalty, op=op,
                                **self._kernel_params())

    def _row_sq(self, X):
        """Squared row norms (numpy) of dense rows or a ``SparseData``."""
        if isinstance(X, SparseData):
            return sp_row_norms(X).cpu().numpy()
        return np.sum(np.asarray(to_numpy(X), dtype=np.float64) ** 2, 1)

    def _train_row_sq(self):
        return self._row_sq(self._train()[0] if self._sparse_fit() else self.X)

    def _xt(self, v):
        """X^T v over the training rows (numpy)."""
        if not self._sparse_fit():
            return v @ self.X
        sd = self._train()[0]
        return sp_xty(sd, torch.as_tensor(np.asarray(v, dtype=np.float64))[:, None])[:, 0] \
            .cpu().numpy()

    def _F(self, X):
        N = X.shape[0]
        if sp.issparse(X):
            F = torch.empty((N + 1, N + 1), dtype=torch.float64, device=self._train()[0].device)
            F[0, 0] = 0.0
            F[0, 1:] = 1.0
            F[1:, 0] = 1.0
            self._sparse_H(out=F[1:, 1:])
            return F
        K = self.get_kernel(X)
        dev = K.device
        F = torch.zeros((N + 1, N + 1), dtype=torch.float64, device=dev)
        F[0, 1:] = 1.0
        F[1:, 0] = 1.0
        F[1:, 1:] = K.double() + (1.0 / self.penalty) * torch.eye(N, dtype=torch.float64, device=dev)
        return F

    def get_h(self, X):
        check_is_fitted(self, "alpha_")
        if self._sparse_fit():
            # K(queries, train) alpha + b without the M x N block
            h = sp_kernel_matvec(self._train()[0], self._queries(X),
                                 torch.as_tensor(self.alpha_, dtype=torch.float64),
                                 **self._kernel_params())
            return (h + self.b_).cpu().numpy()
        if sp.issparse(X) or isinstance(X, SparseData):
            raise TypeError("A sparse matrix was passed, but dense data is required: the "
                            "estimator was fitted on dense rows. Use X.toarray() to convert to "
                            "a dense numpy array.")
        Kx = self.get_kernel(self.X, X)
        return (torch.as_tensor(self.alpha_, device=Kx.device).double() @ Kx.double()
                + self.b_).cpu().numpy()

    def _gram_for_gamma(self, X):
        self._gamma_ref = X if sp.issparse(X) else np.asarray(to_numpy(X), dtype=np.float64)


class LSSVC(_KernelMixin, ClassifierMixin, BaseEstimator):
    """Classical least-squares SVM classifier (labels in {-1, +1})."""

    def _more_tags(self):
        return {"binary_only": True}


    def __init__(self, kernel="linear", penalty=0.1, degree=3, gamma="scale", coef0=0.0,
                 verbose=False, algorithm="classic", device=None, cg_tol=1e-10, cg_maxiter=1000):
        self.kernel = kernel
        self.penalty = penalty
        self.degree = degree
        self.gamma = gamma
        self.coef0 = coef0
        self.verbose = verbose
        self.algorithm = algorithm
        self.device = device
        self.cg_tol = cg_tol
        self.cg_maxiter = cg_maxiter

    def _classical_fit(self, X, y):
        F = self._F(X)
        rhs = torch.cat([torch.zeros(1, dtype=torch.float64, device=F.device),
                         torch.as_tensor(y, dtype=torch.float64, device=F.device)])
        sol = torch.linalg.pinv(F, hermitian=True) @ rhs
        return float(sol[0]), sol[1:].cpu().numpy()

    def _cg_fit(self, X, y):
        N = X.shape[0]
        if sp.issparse(X):
            if 8 * N * N > _dense_limit_bytes():
                return self._cg_fit_matrix_free(y)
            H = self._sparse_H()
        else:
            H = self.get_kernel(X).double()
            H = H + (1.0 / self.penalty) * torch.eye(N, dtype=torch.float64, device=H.device)
        B = torch.stack([torch.as_tensor(y, dtype=torch.float64, device=H.device),
                         torch.ones(N, dtype=torch.float64, device=H.device)], 1)
        Z = conjugate_gradient(H, B, tol=self.cg_tol, maxiter=self.cg_maxiter)
        res = (H @ Z - B).norm() / B.norm()
        if not bool(torch.isfinite(Z).all()) or float(res) > 1e-6:
            # H is not SPD (e.g. sigmoid kernel): CG does not apply, solve directly
            Z = torch.linalg.lstsq(H, B).solution
        return self._cg_solution(Z)

    def _cg_fit_matrix_free(self, y):
        """CG on H = K + I / penalty of CSR rows whose N x N matrix exceeds
        ``SQ_SVM_DENSE_BYTES``: H is applied to the two right-hand sides at a
        time by the fused kernel and never formed.  Without the matrix there
        is no ``lstsq`` fallback, so the run is accepted only when it ends
        with the residual test passed and the kernel seen as positive
        semidefinite: the CG coefficients are the Lanczos tridiagonal of H,
        whose eigenvalues (Ritz values) lie inside the spectrum of H, so a
        smallest Ritz value below ``1 / penalty`` (beyond rounding) certifies
        a negative eigenvalue of K.  Anything else raises."""
        sd, op = self._train()
        params = self._kernel_params()
        ridge = 1.0 / self.penalty

        def matvec(P):
            return sp_kernel_matvec(sd, sd, P, op=op, **params) + P * ridge
        B = torch.stack([torch.as_tensor(y, dtype=torch.float64, device=sd.device),
                         torch.ones(sd.shape[0], dtype=torch.float64, device=sd.device)], 1)
        coeffs = []
        Z = conjugate_gradient(None, B, tol=self.cg_tol, maxiter=self.cg_maxiter, matvec=matvec,
                               coeffs=coeffs)
        ok = bool(torch.isfinite(Z).all())
        if ok:
            ok = float((matvec(Z) - B).norm() / B.norm()) <= 1e-6
        lo, hi = _ritz_range(coeffs, self.cg_tol) if ok else (ridge, ridge)
        indefinite = lo - ridge < -_RITZ_TOL * hi
        if indefinite or not ok:
            what = (f"the kernel matrix is not positive semidefinite (the run saw an eigenvalue of "
                    f"about {lo - ridge:.3g})" if indefinite else
                    "K + I / penalty is not symmetric positive definite (or cg_maxiter is too "
                    "small)")
            raise ValueError(
                f"matrix-free conjugate gradients refuse the {self.kernel!r} LS-SVM system: "
                f"{what}, and its N x N matrix exceeds SQ_SVM_DENSE_BYTES, so there is no dense "
                "fallback. Raise SQ_SVM_DENSE_BYTES or use algorithm='classic'.")
        return self._cg_solution(Z)

    @staticmethod
    def _cg_solution(Z):
        eta, nu = Z[:, 0], Z[:, 1]
        b = float(eta.sum() / nu.sum())
        alpha = (eta - nu * b).cpu().numpy()
        return b, alpha

    def fit(self, X, y):
        X, y = self._fit_input(X, y)
        self._gram_for_gamma(X)
        self.X = X
        if self.algorithm == "classic":
            self.b_, self.alpha_ = self._classical_fit(X, y)
        elif self.algorithm == "cg":
            self.b_, self.alpha_ = self._cg_fit(X, y)
        else:
            raise ValueError("Algorithm not implemented")
        self.b, self.alpha = self.b_, self.alpha_
        if self.kernel == "linear":
            self.coef_ = self._xt(self.alpha_)
        self.classes_ = np.array([-1.0, 1.0])
        self.is_fitted_ = True
        return self

    def decision_function(self, X):
        X = self._check_queries(X)
        return self.get_h(X)

    def predict(self, X):
        return np.sign(self.decision_function(X))

    def get_P(self, X):
        X = self._check_queries(X)
        if not self._sparse_fit():
            X = np.asarray(X, dtype=np.float64)
        N = self.X.shape[0]
        h = self.get_h(X)
        Nu = self.b_ ** 2 + float(np.sum(self.alpha_ ** 2 * self._train_row_sq()))
        betas = np.sqrt((N * self._row_sq(X) + 1) * Nu)
        return 0.5 * (1 - h / betas), betas


def conjugate_gradient(A, B, tol=1e-10, maxiter=1000, matvec=None, coeffs=None):
    """Batched CG for SPD A with several right-hand sides (columns of B).
    ``matvec``: a callable ``P -> A P`` used in place of the tensor ``A``;
    ``coeffs``: a list that receives ``(alpha_k, beta_k, |r_k|^2 / |b|^2)`` of
    every iteration: the step and direction coefficients and the relative
    squared residual, one entry per column each."""
    if matvec is None:
        def matvec(P):
            return A @ P
    X = torch.zeros_like(B)
    R = B - matvec(X)
    P = R.clone()
    rs = (R * R).sum(0)
    b2 = (B * B).sum(0).clamp(min=1e-300)
    for _ in range(maxiter):
        AP = matvec(P)
        alpha = rs / (P * AP).sum(0).clamp(min=1e-300)
        X = X + P * alpha
        R = R - AP * alpha
        rs_new = (R * R).sum(0)
        if coeffs is not None:
            coeffs.append((alpha, rs_new / rs.clamp(min=1e-300), rs_new / b2))
        if bool((rs_new <= (tol ** 2) * b2).all()):
            break
        P = R + P * (rs_new / rs.clamp(min=1e-300))
        rs = rs_new
    return X


class QLSSVC(_KernelMixin, ClassifierMixin, BaseEstimator):
    """Quantum least-squares SVM (``_qSVM.py:10-404``)."""

    def _more_tags(self):
        return {"binary_only": True}


    def __init__(self, kernel="linear", penalty=0.1, degree=3, gamma="scale", coef0=0.0,
                 verbose=False, algorithm="classic", low_rank=False, var=0.9,
                 error_type="absolute", relative_error=0.5, absolute_error=0.01, train_error=0.01,
                 random_state=None, device=None):
        if error_type not in ("absolute", "relative"):
            raise Exception(r"The error should be either 'absolute' or 'relative'")
        self.kernel = kernel
        self.penalty = penalty
        self.degree = degree
        self.gamma = gamma
        self.coef0 = coef0
        self.verbose = verbose
        self.algorithm = algorithm
        self.low_rank = low_rank
        self.var = var
        self.error_type = error_type
        self.relative_error = relative_error
        self.absolute_error = absolute_error
        self.train_error = train_error
        self.random_state = random_state
        self.device = device

    # -------------------------------------------------------------- fit
    def _classical_fit(self, y):
        """(b, alpha) = F^+ [0; y] with the optional low-rank truncation of
        the hermitian spectrum (``_qSVM.py:84-130``)."""
        F = self._F(self.X)
        lam, Qm = torch.linalg.eigh(F)
        order = torch.argsort(lam.abs(), descending=True)
        lam, Qm = lam[order], Qm[:, order]
        s = lam.abs()
        s_new = torch.zeros_like(s)
        if self.low_rank:
            if 0 <= self.var < 1.0:
                sums = float((s ** 2).sum())
                cum = torch.cumsum(s ** 2, 0) / sums
                idx = int(torch.nonzero(cum >= self.var - 1e-15)[0][0]) if bool((cum >= self.var - 1e-15).any()) else len(s) - 1
            elif self.var >= 1.0:
                idx = int(self.var) - 1
            else:
                raise Exception("QLSSVC.var shoud be greater than 0")
            s_new[:idx + 1] = s[:idx + 1]
            self.cond = float(s_new[0] / s_new[idx])
            self.normF = float(s_new[0])
        else:
            s_new = s.clone()
            self.cond = float(s[0] / s[-1])
            self.normF = float(s[0])
        self.singular_values_F_ = s_new.cpu().numpy()
        inv = torch.where(s_new > 0, 1.0 / s_new.clamp(min=1e-300), torch.zeros_like(s_new))
        sign = torch.sign(lam)
        Finv = (Qm * (inv * sign)) @ Qm.T
        rhs = torch.cat([torch.zeros(1, dtype=torch.float64, device=F.device),
                         torch.as_tensor(y, dtype=torch.float64, device=F.device)])
        sol = Finv @ rhs
        return float(sol[0]), sol[1:].cpu().numpy()

    def fit(self, X, y):
        X, y = self._fit_input(X, y)
        self._gram_for_gamma(X)
        self.X = X
        N = X.shape[0]
        if self.algorithm == "classic":
            self.b_, self.alpha_ = self._classical_fit(y)
        else:
            raise ValueError("Algorithm not implemented")
        self.b, self.alpha = self.b_, self.alpha_
        if sp.issparse(X):
            xn = self._train_row_sq()
            self.alpha_F = math.sqrt(N) + self.penalty ** -1 + float(xn.sum())
            self.Nu = self.b_ ** 2 + float(np.sum(self.alpha_ ** 2 * xn))
        else:
            self.alpha_F = math.sqrt(N) + self.penalty ** -1 + float(np.linalg.norm(X, ord="fro") ** 2)
            self.Nu = self.b_ ** 2 + float(np.sum(self.alpha_ ** 2 * np.sum(X ** 2, 1)))
        if self.kernel == "linear":
            self.coef_ = self._xt(self.alpha_)
        self.classes_ = np.array([-1.0, 1.0])
        self.is_fitted_ = True
        self._calls = 0
        return self

    # ------------------------------------------------------------ noise
    def _noise(self, bounds):
        """One TN(-b_i, b_i) draw per element (Philox, fresh stream per call)."""
        self._calls = getattr(self, "_calls", 0) + 1
        key = RngKey(seed_from_random_state(self.random_state), "trunc_normal", self._calls)
        bounds = np.asarray(bounds, dtype=np.float64).reshape(-1)
        out = np.empty_like(bounds)
        # one stream, per-element bound: draw uniforms and map with each bound
        from ...runtime.rng import Philox
        from scipy.special import erf, erfinv
        u = Philox(key).uniform_flat(bounds.size, dtype=torch.float64).numpy()
        e = erf(bounds / np.sqrt(2.0))
        out = np.sqrt(2.0) * erfinv((2 * u - 1) * e)
        return np.clip(out, -bounds, bounds)

    def relative_error_routine(self, delta, Xmax, Xreal):
        """Iterative halving (``_qSVM.py:245-261``), vectorised over samples:
        returns (Xhat, delta_r, epsilon_abs) arrays."""
        Xmax = np.atleast_1d(np.asarray(Xmax, dtype=np.float64))
        Xreal = np.broadcast_to(np.asarray(Xreal, dtype=np.float64), Xmax.shape).copy()
        r = np.zeros_like(Xmax)
        Xr = Xmax.copy()
        Xhat = np.zeros_like(Xmax)
        eps_abs = np.zeros_like(Xmax)
        delta_r = np.zeros_like(Xmax)
        active = Xr > Xhat
        for _ in range(200):
            if not active.any():
                break
            r = np.where(active, r + 1.0, r)
            Xr = np.where(active, Xmax / 2 ** r, Xr)
            eps_abs = np.where(active, self.relative_error * Xr / 2, eps_abs)
            delta_r = np.where(active, 6 * delta / (np.pi ** 2 * r ** 2), delta_r)
            draw = Xreal + self._noise(np.where(active, eps_abs, 0.0))
            Xhat = np.where(active, draw, Xhat)
            active = Xr > Xhat
        return Xhat, delta_r, eps_abs

    # ---------------------------------------------------------- predict
    def get_betas(self, X):
        check_is_fitted(self, "alpha_")
        if self._sparse_fit():
            X = self._check_queries(X)
        N = self.X.shape[0]
        return np.sqrt((N * self._row_sq(X) + 1) * self.Nu)

    def get_h(self, X, approx=False):
        if self._sparse_fit():
            X = self._check_queries(X)      # uploaded once for h and the betas
            hs = super().get_h(X)
        else:
            hs = super().get_h(np.asarray(to_numpy(X), dtype=np.float64))
        if approx:
            betas = self.get_betas(X)
            if self.error_type == "absolute":
                hs = hs + self._noise(np.full(hs.shape, self.absolute_error))
            else:
                _, _, ea = self.relative_error_routine(0.1, betas, np.abs(hs))
                hs = hs + self._noise(ea)
        return hs

    def get_P(self, X, approx=False):
        if self._sparse_fit():
            X = self._check_queries(X)
        hs = self.get_h(X)
        beta = self.get_betas(X)
        P = 0.5 * (1 - hs / beta)
        if approx:
            if self.error_type == "absolute":
                P = P + self._noise(self.absolute_error / (2 * beta))
            else:
                _, _, ea = self.relative_error_routine(0.1, beta, np.abs(hs))
                P = P + self._noise(ea / (2 * beta))
        return P

    def predict(self, X):
        """+1 if the noisy P(x) <= 1/2 else -1 (``_qSVM.py:178-215``)."""
        if self._sparse_fit():
            X = self._check_queries(X)
        else:
            check_array(X)
        check_is_fitted(self, "alpha_")
        P = self.get_P(X)
        betas = self.get_betas(X)
        if self.error_type == "absolute":
            P = P + self._noise(self.absolute_error / (2 * betas))
        else:
            h = self.get_h(X)
            _, _, ea = self.relative_error_routine(0.1, betas, np.abs(h))
            P = P + self._noise(ea / (2 * betas))
        return np.where(P <= 0.5, 1.0, -1.0)

    def classical_predict(self, X):
        if self._sparse_fit():
            X = self._check_queries(X)
        else:
            check_array(X)
        return np.sign(self.get_h(X))

    def get_training_complexity(self):
        return self.cond * self.alpha_F

    def get_classification_complexity(self, X, relative_error=False):
        betas = self.get_betas(X)
        nrm = np.linalg.norm(np.append(self.b_, self.alpha_), ord=2)
        if relative_error:
            hs = np.abs(self.get_h(X))
            return (self.cond * betas * self.alpha_F) / (self.relative_error * hs * self.normF ** 2 * nrm)
        return (self.cond * betas * self.alpha_F) / (self.absolute_error * self.normF ** 2 * nrm)

    def get_approximated_hyperplane(self, x):
        beta = self.get_betas(x)
        ba = np.append(self.b_, self.alpha_)
        if self.error_type == "absolute":
            bound = self.relative_error / beta
        else:
            bound = self.relative_error * np.abs(self.get_h(x)) / beta
        bound = float(np.asarray(bound).reshape(-1)[0])
        approx = ba + self._noise(np.full(ba.shape, bound / np.sqrt(ba.size)))
        return approx[0], self._xt(approx[1:])

    def get_all_attributes(self, X):
        betas = self.get_betas(X)
        hs = self.get_h(X)
        Ps = self.get_P(X)
        rel = (self.cond * (betas - np.abs(hs)) * self.alpha_F) / (np.abs(hs) * np.sqrt(Ps))
        ab = self.cond * betas * self.alpha_F
        return betas, hs, Ps, self.cond, rel, ab

    def score(self, X, y, sample_weight=None):
        check_is_fitted(self, "alpha_")
        return accuracy_score(y, self.predict(X), sample_weight=sample_weight)
