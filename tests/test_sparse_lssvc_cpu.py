"""LS-SVM classifiers and the pairwise kernels on scipy sparse input, CPU
path: the fp64 torch twins of ``ops/sparse_kernel.py``.

Data: ``_sparse_knn_data.structured`` - 700 x 500 fit rows, 70 queries, empty
rows on both sides, identical rows, a stored zero, a column present in every
row; labels ``where(X @ w >= 0, 1, -1)``; ``penalty = 1``, ``gamma = 2^-9``
('exact') or ``2^-5`` ('random'), ``coef0 = 1, degree = 3`` (poly), ``coef0 =
0.5`` (sigmoid).  With these ``cond(F) <= 1.8e4`` and every decision value has
``|h| >= 1.4e-4``; the tests assert the margin ``min |h| > 1e-5`` before they
compare signs.
"""

import pickle

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from _sparse_knn_data import D, M, N_FIT, U, dot_tolerance
from _sparse_lssvc_data import DEGREE, KERNELS, KINDS, case, estimator_kw, kernel_kw, propagate
from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.models.svm.lssvm import LSSVC, QLSSVC
from sq_learn_amd.ops import sparse_kernel as SPK
from sq_learn_amd.utils import pairwise as PW

LS = dict(rtol=1e-6, atol=1e-8)         # the LS-SVM tolerance of test_svm_knn_cpu.py
CG = dict(rtol=1e-5, atol=1e-7)         # its cg tolerance


# ----------------------------------------------------------------- pairwise
def _ours(kernel, A, B, kind):
    kw = kernel_kw(kernel, kind)
    if kernel == "linear":
        return PW.linear_kernel(A, B)
    if kernel == "poly":
        return PW.polynomial_kernel(A, B, degree=DEGREE, gamma=kw["gamma"], coef0=kw["coef0"])
    if kernel == "rbf":
        return PW.rbf_kernel(A, B, gamma=kw["gamma"])
    return PW.sigmoid_kernel(A, B, gamma=kw["gamma"], coef0=kw["coef0"])


def _sklearn(kernel, A, B, kind):
    skp = pytest.importorskip("sklearn.metrics.pairwise")
    kw = kernel_kw(kernel, kind)
    if kernel == "linear":
        return skp.linear_kernel(A, B)
    if kernel == "poly":
        return skp.polynomial_kernel(A, B, degree=DEGREE, gamma=kw["gamma"], coef0=kw["coef0"])
    if kernel == "rbf":
        return skp.rbf_kernel(A, B, gamma=kw["gamma"])
    return skp.sigmoid_kernel(A, B, gamma=kw["gamma"], coef0=kw["coef0"])


def _pairwise_bound(kernel, kind, A, B, K):
    """Two fp64 implementations of K(A, B): the rounding of the squared
    distance (``dot_tolerance``; half of it for the inner product alone, as
    sum |a||b| <= (|a|^2 + |b|^2) / 2) through the derivative of the kernel
    function, plus 4 * 2^-53 |K| for the two math libraries."""
    e_dist = dot_tolerance(B, A)                 # [rows of A, rows of B]
    kw = kernel_kw(kernel, kind)
    arg = kw["gamma"] * (A @ B.T).toarray() + kw["coef0"]
    return propagate(kernel, kind, e_dist / 2.0, e_dist, K, arg) + 4 * U * np.abs(K)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_pairwise_kernels_on_csr_match_sklearn(kernel, kind):
    X, Q, _ = case(kind)
    for A, B in ((Q, X), (X, None)):
        want = _sklearn(kernel, A, B, kind)
        got = _ours(kernel, A, B, kind)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        assert got.shape == want.shape
        err = np.abs(got - want)
        bound = _pairwise_bound(kernel, kind, A, A if B is None else B, want)
        assert (err <= bound).all(), (err - bound).max()
    # mixed input: the dense partner is converted to CSR - the same numbers
    want = _ours(kernel, Q, X, kind)
    np.testing.assert_array_equal(_ours(kernel, Q.toarray(), X, kind), want)
    np.testing.assert_array_equal(_ours(kernel, Q, X.toarray(), kind), want)
    np.testing.assert_array_equal(_ours(kernel, Q.tocoo(), X.tocsc(), kind), want)
    if kernel == "rbf":                          # the self-join has an exact diagonal
        np.testing.assert_array_equal(np.diag(_ours(kernel, X, None, kind)), np.ones(N_FIT))


def test_pairwise_defaults_and_dispatch():
    skp = pytest.importorskip("sklearn.metrics.pairwise")
    X, Q, _ = case("random")
    # gamma=None stays 1 / n_features
    for name in ("rbf", "poly", "sigmoid"):
        got = PW.pairwise_kernels(Q, X, metric=name)
        np.testing.assert_array_equal(got, PW.pairwise_kernels(Q, X, metric=name, gamma=1.0 / D))
        np.testing.assert_allclose(got, skp.pairwise_kernels(Q, X, metric=name), rtol=1e-12,
                                   atol=1e-14)
    np.testing.assert_allclose(PW.pairwise_kernels(Q, X, metric="linear"),
                               (Q @ X.T).toarray(), rtol=1e-13, atol=1e-13)
    # dense behaviour is unchanged: arrays in, the GEMM path's array out
    Qd, Xd = Q.toarray(), X.toarray()
    np.testing.assert_allclose(PW.linear_kernel(Qd, Xd), Qd @ Xd.T, rtol=1e-12, atol=1e-12)
    assert isinstance(PW.rbf_kernel(torch.as_tensor(Qd), torch.as_tensor(Xd)), torch.Tensor)


# --------------------------------------------------------------------- ops
def _sd(kind):
    X, Q, _ = case(kind)
    return as_sparse_data(X, "cpu"), as_sparse_data(Q, "cpu")


@pytest.mark.parametrize("kernel", KERNELS)
def test_matvec_equals_matrix_times_vectors(kernel):
    fit, qry = _sd("random")
    kw = kernel_kw(kernel, "random")
    rng = np.random.RandomState(5)
    for q in (qry, fit):
        K = SPK.sp_kernel_matrix(fit, q, kernel, **kw)
        assert K.shape == (q.shape[0], N_FIT) and K.dtype == torch.float64
        for R in (1, 2, 4):
            V = torch.as_tensor(rng.standard_normal((N_FIT, R)))
            got = SPK.sp_kernel_matvec(fit, q, V, kernel, **kw)
            assert got.shape == (q.shape[0], R)
            # summation rounding of n terms on both sides
            tol = 2 * N_FIT * U * (K.abs() @ V.abs())
            if kernel == "linear":
                # Q (X^T V): the bound of the two-stage sum, over |Q| |X|^T |V|
                Qa, Xa = q.dense_rows(0, q.shape[0]).abs(), fit.dense_rows(0, N_FIT).abs()
                tol = 2 * (N_FIT + D) * U * (Qa @ (Xa.T @ V.abs()))
            assert ((got - K @ V).abs() <= tol).all()
        v = torch.as_tensor(rng.standard_normal(N_FIT))
        got = SPK.sp_kernel_matvec(fit, q, v, kernel, **kw)
        assert got.shape == (q.shape[0],)
        np.testing.assert_array_equal(got, SPK.sp_kernel_matvec(fit, q, v[:, None], kernel,
                                                                **kw)[:, 0])


def test_op_refusals():
    fit, qry = _sd("exact")
    with pytest.raises(ValueError, match="between 1 and 4 vectors"):
        SPK.sp_kernel_matvec(fit, qry, torch.zeros((N_FIT, 5), dtype=torch.float64), "rbf")
    with pytest.raises(ValueError, match="between 1 and 4 vectors"):
        SPK.sp_kernel_matvec(fit, qry, torch.zeros((N_FIT, 5), dtype=torch.float64), "linear")
    with pytest.raises(ValueError, match="does not match a fit set"):
        SPK.sp_kernel_matvec(fit, qry, torch.zeros((M, 2), dtype=torch.float64), "rbf")
    with pytest.raises(ValueError, match="sparse kernels are"):
        SPK.sp_kernel_matrix(fit, qry, "cosine")
    with pytest.raises(ValueError, match="diag_add belongs to the self-join"):
        SPK.sp_kernel_matrix(fit, qry, "rbf", diag_add=1.0)
    with pytest.raises(ValueError, match="out must be an fp64 matrix"):
        SPK.sp_kernel_matrix(fit, qry, "rbf", out=torch.zeros((M, N_FIT), dtype=torch.float32))
    with pytest.raises(ValueError, match="out must be an fp64 matrix"):
        SPK.sp_kernel_matrix(fit, qry, "rbf", out=torch.zeros((N_FIT, M), dtype=torch.float64).T)


def test_matrix_into_a_strided_view():
    fit, _ = _sd("exact")
    kw = kernel_kw("rbf", "exact")
    F = torch.full((N_FIT + 1, N_FIT + 1), -7.0, dtype=torch.float64)
    got = SPK.sp_kernel_matrix(fit, fit, "rbf", out=F[1:, 1:], diag_add=0.25, **kw)
    assert got.data_ptr() == F[1:, 1:].data_ptr()
    assert (F[0] == -7.0).all() and (F[:, 0] == -7.0).all()
    K = SPK.sp_kernel_matrix(fit, fit, "rbf", **kw)
    np.testing.assert_array_equal(torch.diagonal(K), np.ones(N_FIT))
    np.testing.assert_array_equal(F[1:, 1:], K + 0.25 * torch.eye(N_FIT, dtype=torch.float64))


# --------------------------------------------------------------- estimators
FITTED = ("alpha_", "b_")
QUANTUM = ("cond", "normF", "alpha_F", "Nu", "singular_values_F_")


def _margin(h):
    assert np.abs(h).min() > 1e-5
    return np.sign(h)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_lssvc_on_csr_matches_dense(kernel, kind):
    X, Q, y = case(kind)
    s = LSSVC(device="cpu", **estimator_kw(kernel, kind)).fit(X, y)
    d = LSSVC(device="cpu", **estimator_kw(kernel, kind)).fit(X.toarray(), y)
    assert sp.issparse(s.X) and s.X.format == "csr"
    for name in FITTED + (("coef_",) if kernel == "linear" else ()):
        np.testing.assert_allclose(getattr(s, name), getattr(d, name), err_msg=name, **LS)
    assert hasattr(s, "coef_") == (kernel == "linear")
    for A in (X, Q):
        want = _margin(d.decision_function(A.toarray()))
        np.testing.assert_array_equal(_margin(s.decision_function(A)), want)
        np.testing.assert_array_equal(s.predict(A), want)
    Ps, bs = s.get_P(Q)
    Pd, bd = d.get_P(Q.toarray())
    np.testing.assert_allclose(bs, bd, **LS)
    np.testing.assert_allclose(Ps, Pd, **LS)


PREDICT_SEED = 233
_QPAIRS = {}


def _qlssvc_pair(kernel, kind):
    """(fitted on CSR, fitted on the dense rows), fitted once."""
    if (kernel, kind) not in _QPAIRS:
        X, _, y = case(kind)
        kw = dict(device="cpu", random_state=PREDICT_SEED, **estimator_kw(kernel, kind))
        _QPAIRS[kernel, kind] = (QLSSVC(**kw).fit(X, y), QLSSVC(**kw).fit(X.toarray(), y))
    return _QPAIRS[kernel, kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_qlssvc_on_csr_matches_dense(kernel, kind):
    X, Q, y = case(kind)
    s, d = _qlssvc_pair(kernel, kind)
    assert sp.issparse(s.X) and s.X.format == "csr"
    assert d.cond <= 1.8e4
    for name in FITTED + QUANTUM + (("coef_",) if kernel == "linear" else ()):
        np.testing.assert_allclose(getattr(s, name), getattr(d, name), err_msg=name, **LS)
    np.testing.assert_allclose(s.get_betas(Q), d.get_betas(Q.toarray()), **LS)
    for A in (X, Q):
        want = _margin(d.get_h(A.toarray()))
        np.testing.assert_array_equal(s.classical_predict(A), want)
    # the hyperplane of the linear kernel from the sparse rows
    if kernel == "linear":
        s._calls = d._calls = 0
        bs, ws = s.get_approximated_hyperplane(Q[1:2])
        bd, wd = d.get_approximated_hyperplane(Q[1:2].toarray())
        np.testing.assert_allclose(bs, bd, **LS)
        np.testing.assert_allclose(ws, wd, **LS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_qlssvc_predict_on_csr_matches_dense(kernel):
    """``predict`` adds TN noise of scale ``absolute_error / (2 beta)`` to P
    and thresholds at 1/2.  With the same ``random_state`` the CSR and the
    dense estimator draw the same noise, so they agree wherever the dense
    noisy P is not within 1e-6 of 1/2 (their P differ by ~1e-15), which is
    asserted.  On the 'random' values ``random_state = 233`` leaves a margin of
    7.6e-6 / 3.2e-6 / 1.01e-6 / 2.3e-6 (linear / poly / rbf / sigmoid; the
    widest smallest margin of the seeds 0..299).  The 'exact' values cannot
    serve here: their noiseless P already comes within 5.2e-7 (linear), 1.8e-7
    (poly), 3.5e-8 (rbf) and 1.8e-8 (sigmoid) of 1/2, with noise of scale
    2.6e-8 .. 9.0e-8, so no seed gives the margin."""
    _, Q, _ = case("random")
    s, d = _qlssvc_pair(kernel, "random")
    Qd = Q.toarray()
    d._calls = 0
    noisy = d.get_P(Qd) + d._noise(d.absolute_error / (2 * d.get_betas(Qd)))
    assert np.abs(noisy - 0.5).min() > 1e-6
    s._calls = d._calls = 0
    want = d.predict(Qd)
    np.testing.assert_array_equal(want, np.where(noisy <= 0.5, 1.0, -1.0))
    np.testing.assert_array_equal(s.predict(Q), want)
    s._calls = 0
    np.testing.assert_array_equal(s.predict(Qd), want)      # dense queries, sparse fit


@pytest.mark.parametrize("matrix_free", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_cg_matches_classic_on_csr(kernel, kind, matrix_free, monkeypatch):
    X, Q, y = case(kind)
    kw = dict(device="cpu", **estimator_kw(kernel, kind))
    c = LSSVC(**kw).fit(X, y)
    if matrix_free:
        monkeypatch.setenv("SQ_SVM_DENSE_BYTES", "0")
        formed = []
        monkeypatch.setattr(LSSVC, "_sparse_H", lambda self, out=None: formed.append(1))
    g = LSSVC(algorithm="cg", **kw).fit(X, y)
    if matrix_free:
        assert not formed                        # H was never formed
    np.testing.assert_allclose(g.alpha_, c.alpha_, **CG)
    np.testing.assert_allclose(g.b_, c.b_, **CG)
    np.testing.assert_array_equal(_margin(g.decision_function(Q)),
                                  _margin(c.decision_function(Q)))


@pytest.mark.parametrize("kind", KINDS)
def test_matrix_free_sigmoid_raises(kind, monkeypatch):
    """The sigmoid kernel matrix of this data is indefinite (smallest
    eigenvalue -0.430 on 'exact', -0.339 on 'random').  At penalty 1 the
    system H = K + I is still positive definite (0.570 / 0.661) and CG itself
    converges, so the refusal cannot come from the residual: it comes from the
    Lanczos tridiagonal of the CG coefficients, whose smallest Ritz value
    (0.5706 / 0.6614 after 35 / 26 iterations) lies below 1 / penalty and so
    certifies a negative eigenvalue of K.  With the dense toggle the same fit
    is solved as before."""
    X, _, y = case(kind)
    kw = dict(device="cpu", **estimator_kw("sigmoid", kind))
    c = LSSVC(**kw).fit(X, y)
    g = LSSVC(algorithm="cg", **kw).fit(X, y)
    np.testing.assert_allclose(g.alpha_, c.alpha_, **CG)
    monkeypatch.setenv("SQ_SVM_DENSE_BYTES", "0")
    with pytest.raises(ValueError, match="not positive semidefinite.*SQ_SVM_DENSE_BYTES"):
        LSSVC(algorithm="cg", **kw).fit(X, y)


def test_matrix_free_refuses_an_indefinite_system(monkeypatch):
    """penalty = 8: I / penalty = 0.125 does not lift the sigmoid kernel's
    smallest eigenvalue (-0.430), H itself is indefinite and the matrix-free
    run is refused whether or not CG stumbles to a small residual; with the
    dense toggle the same fit falls back to ``lstsq`` as before."""
    X, _, y = case("exact")
    kw = dict(estimator_kw("sigmoid", "exact"), penalty=8.0)
    LSSVC(algorithm="cg", device="cpu", **kw).fit(X, y)
    monkeypatch.setenv("SQ_SVM_DENSE_BYTES", "0")
    with pytest.raises(ValueError, match="refuse the 'sigmoid' LS-SVM system.*SQ_SVM_DENSE_BYTES"):
        LSSVC(algorithm="cg", device="cpu", **kw).fit(X, y)


@pytest.mark.parametrize("kind", KINDS)
def test_gamma_scale_from_the_stored_values(kind):
    X, _, y = case(kind)
    dense = X.toarray()
    want = 1.0 / (D * dense.var())
    est = LSSVC(kernel="rbf", penalty=1.0, gamma="scale", device="cpu").fit(X, y)
    got = est._get_gamma(est._gamma_ref)
    rel = (X.nnz + 4) * U * np.mean(dense ** 2) / dense.var()
    assert abs(got - want) <= rel * want
    ref = LSSVC(kernel="rbf", penalty=1.0, gamma=want, device="cpu").fit(X, y)
    np.testing.assert_allclose(est.alpha_, ref.alpha_, **LS)


def test_query_kinds_and_refusals():
    X, Q, y = case("random")
    kw = dict(device="cpu", **estimator_kw("rbf", "random"))
    s = LSSVC(**kw).fit(X, y)
    h = s.decision_function(Q)
    # dense queries against a sparse fit are converted to CSR: the same numbers
    np.testing.assert_array_equal(s.decision_function(Q.toarray()), h)
    np.testing.assert_array_equal(s.decision_function(Q.tocsc()), h)
    with pytest.raises(ValueError, match="features"):
        s.decision_function(Q[:, :D - 1])
    # any sparse format fits
    np.testing.assert_array_equal(LSSVC(**kw).fit(X.tocoo(), y).alpha_, s.alpha_)
    # an estimator fitted on dense rows keeps refusing sparse queries
    d = LSSVC(**kw).fit(X.toarray(), y)
    q = QLSSVC(**kw).fit(X.toarray(), y)
    for call in (d.decision_function, d.predict, d.get_P, d.get_h, q.predict, q.classical_predict):
        with pytest.raises(TypeError, match="dense data is required"):
            call(Q)


@pytest.mark.parametrize("Est", [LSSVC, QLSSVC])
def test_pickle_round_trip(Est):
    X, Q, y = case("exact")
    est = Est(device="cpu", random_state=1, **estimator_kw("poly", "exact")) if Est is QLSSVC \
        else Est(device="cpu", **estimator_kw("poly", "exact"))
    est.fit(X, y)
    before = est.predict(Q) if Est is LSSVC else est.classical_predict(Q)
    assert est._engine_sparse is not None         # the uploaded rows are kept for prediction
    state = est.__getstate__()
    assert state["_engine_sparse"] is None
    assert not any(isinstance(v, torch.Tensor) for v in state.values())
    back = pickle.loads(pickle.dumps(est))
    assert sp.issparse(back.X) and back.X.format == "csr" and (back.X != X).nnz == 0
    after = back.predict(Q) if Est is LSSVC else back.classical_predict(Q)
    np.testing.assert_array_equal(after, before)
    np.testing.assert_array_equal(back.get_h(Q), est.get_h(Q))
