"""Shared fixtures of the sparse LS-SVM / sparse kernel-matrix tests (CPU and
GPU files): the structured CSR case of ``_sparse_knn_data`` with labels, the
kernel parameters and the per-element error bounds."""

import numpy as np

from _sparse_knn_data import D, U, sq_norms, structured

PENALTY = 1.0
KINDS = ("exact", "random")
KERNELS = ("linear", "poly", "rbf", "sigmoid")
DEGREE = 3


def gamma_of(kind):
    return 2.0 ** -9 if kind == "exact" else 2.0 ** -5


def kernel_kw(kernel, kind):
    """The keyword arguments of ``ops.sparse_kernel`` for one kernel."""
    coef0 = {"poly": 1.0, "sigmoid": 0.5}.get(kernel, 0.0)
    return dict(gamma=gamma_of(kind), coef0=coef0, degree=DEGREE)


def estimator_kw(kernel, kind):
    return dict(kernel=kernel, penalty=PENALTY, **kernel_kw(kernel, kind))


_CACHE = {}


def case(kind):
    """(fit CSR [700, 500], query CSR [70, 500], labels [700]) - computed once."""
    if kind not in _CACHE:
        X, Q = structured(kind)
        w = np.random.RandomState(1).standard_normal(D)
        _CACHE[kind] = (X, Q, np.where(X @ w >= 0, 1.0, -1.0))
    return _CACHE[kind]


def kernel_args(kernel, kind, X, Q):
    """The exact argument of pow / exp / tanh for every pair, [m, n] fp64, in
    the operation order of the kernels (meaningful for 'exact' data, where
    every step is exact)."""
    kw = kernel_kw(kernel, kind)
    dot = (Q @ X.T).toarray()
    if kernel == "rbf":
        dist = np.maximum((sq_norms(Q)[:, None] + sq_norms(X)[None, :]) - 2.0 * dot, 0.0)
        return -kw["gamma"] * dist
    return kw["gamma"] * dot + kw["coef0"]


def propagate(kernel, kind, e_dot, e_dist, K, arg=None):
    """A bound on the inner product (``e_dot``) or on the squared distance
    (``e_dist``) through the derivative of the kernel function, [m, n]:
    linear 1; poly degree * gamma * max|arg|^(degree - 1); rbf gamma * K on
    the distance bound; sigmoid gamma."""
    g = gamma_of(kind)
    if kernel == "linear":
        return e_dot
    if kernel == "poly":
        return DEGREE * g * np.abs(arg).max() ** (DEGREE - 1) * e_dot
    if kernel == "rbf":
        return g * np.abs(K) * e_dist
    return g * e_dot
