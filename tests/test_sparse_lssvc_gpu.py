"""The sparse kernel-matrix kernels (``csrc/spgram.hip``) against the fp64
torch twin, and ``LSSVC`` / ``QLSSVC`` on CSR input on the GPU.

Shapes: ``_sparse_knn_data.structured`` - 700 fit rows, 500 columns, 70
queries; with ``tile = 256`` three tiles, the last holding 188 rows, with
``tile = 64`` eleven, with the default one.  Fit rows 40 and 650 and query row
0 are empty, rows 5, 6 and 300 identical, a column is present in every row
(the shared-slice pass).  The values are fp32-representable, so the GPU (fp32
storage) and the twin (fp64) see the same numbers.

* exact (integers in [-8, 8]), linear: the fixed-point sums are exact - equal.
* exact, other kinds: the arguments of pow / exp / tanh are exact on both
  sides (gamma = 2^-9, coef0 in {1, 0.5}), so only the math libraries differ:
  ``|K_gpu - K_twin| <= L_kind * 2^-53 * |K_twin|``.  ``L_kind`` comes from the
  gap between ``torch.pow / exp / tanh`` on the GPU and on the CPU in fp64
  over exactly these arguments (queries and self-join together), in units of
  ``2^-53 |value|`` - measured on an MI355X over the 539000 arguments of each
  kind (684 distinct for pow and tanh, 2547 for exp): pow 0.0 (both sides
  cube by two multiplications), exp 1.94, tanh 1.62 - doubled (a few
  thousand arguments sample the functions thinly), rounded up to a power of
  two, at least 4: ``L_KIND = 4`` for the three kinds.  (The kernel itself,
  which calls the device ``pow``, is 1.81 / 1.94 / 1.62 from the twin.)
* random (fp32-rounded normals): the inner product differs by at most
  ``nnz_i 2^(e_i - 1)`` (fixed-point rounding) plus ``(nnz_i + 2) 2^-53 sum
  |q||x|`` (the twin's dot), as in ``test_sparse_dbscan_gpu.bounds``; rbf adds
  the norm terms of that bound.  It goes through the derivative bound of the
  kind (linear 1; poly ``degree gamma max|arg|^(degree - 1)``; rbf ``gamma K``
  on the distance bound; sigmoid ``gamma``), plus the same ``L_kind`` term.
* apply mode: the matrix bound times ``sum_j |V_j|`` plus ``n 2^-53 sum_j
  |K_j V_j|``; the linear route (``Q (X^T V)`` through the CSR products) within
  the bound of the spmm tests, ``(nnz + 2) 2^-53 |A| |W|`` per product.
* estimators: the CPU CSR fit within the LS-SVM tolerances of
  ``test_svm_knn_cpu.py`` (1e-6 / 1e-8; cg 1e-5 / 1e-7), decision signs equal
  on all 700 + 70 rows (``min |h| > 1e-5`` asserted).
"""

import json
import os

import numpy as np
import pytest
import torch

from _sparse_knn_data import D, M, N_FIT, TILE, U, sq_norms
from _sparse_lssvc_data import (KERNELS, KINDS, case, estimator_kw, kernel_args, kernel_kw,
                                propagate)
from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.models.svm.lssvm import LSSVC, QLSSVC
from sq_learn_amd.ops import _native as nat
from sq_learn_amd.ops import kmeans as KM
from sq_learn_amd.ops import sparse_kernel as SPK
from sq_learn_amd.ops import sparse_knn as SK

pytestmark = pytest.mark.gpu

TILES = [64, TILE, None]
L_KIND = {"linear": 0, "poly": 4, "rbf": 4, "sigmoid": 4}
LS = dict(rtol=1e-6, atol=1e-8)
CG = dict(rtol=1e-5, atol=1e-7)


def dot_bound(X, Q):
    """[m, n] bound on |dot_gpu - dot_twin|: the inner-product part of
    ``test_sparse_dbscan_gpu.bounds``."""
    nq = np.diff(Q.indptr)
    mx = float(abs(X).max())
    e = np.array([KM.fixed_point_exp(float(abs(Q[i]).max()) * mx if nq[i] else 0.0, nq[i])
                  for i in range(Q.shape[0])], dtype=np.float64)
    absdot = (abs(Q) @ abs(X).T).toarray()
    return nq[:, None] * 2.0 ** (e[:, None] - 1) + (nq[:, None] + 2) * U * absdot


def dist_bound(X, Q, e_dot):
    """The euclidean branch of ``test_sparse_dbscan_gpu.bounds``."""
    nnz = np.maximum(np.diff(Q.indptr)[:, None], np.diff(X.indptr)[None, :])
    return 2.0 * e_dot + (2 * nnz + 6) * U * (sq_norms(Q)[:, None] + sq_norms(X)[None, :])


class Case:
    """One value set on both devices; twins and bounds computed once."""

    def __init__(self, kind, dev):
        self.kind = kind
        self.X, self.Q, self.y = case(kind)
        self.cpu = {False: as_sparse_data(self.Q, "cpu"), True: None}
        self.fit_cpu = self.cpu[True] = as_sparse_data(self.X, "cpu")
        self.fit = as_sparse_data(self.X, dev)
        self.qry = as_sparse_data(self.Q, dev)
        self._store = {}

    def sides(self, self_join):
        """(fit, queries) on the GPU."""
        return self.fit, (self.fit if self_join else self.qry)

    def twin(self, kernel, self_join):
        key = ("K", kernel, self_join)
        if key not in self._store:
            self._store[key] = SPK.sp_kernel_matrix_torch(
                self.fit_cpu, self.cpu[self_join], kernel, **kernel_kw(kernel, self.kind)).numpy()
        return self._store[key]

    def bound(self, kernel, self_join):
        """[m, n] bound on |K_gpu - K_twin| (module docstring)."""
        key = ("B", kernel, self_join)
        if key not in self._store:
            K = self.twin(kernel, self_join)
            lib = L_KIND[kernel] * U * np.abs(K)
            if self.kind == "exact":
                self._store[key] = lib
            else:
                Qs = self.X if self_join else self.Q
                e_dot = dot_bound(self.X, Qs)
                arg = kernel_args(kernel, self.kind, self.X, Qs)
                self._store[key] = propagate(kernel, self.kind, e_dot,
                                             dist_bound(self.X, Qs, e_dot), K, arg) + lib
        return self._store[key]


@pytest.fixture(scope="module")
def cases(cuda):
    store = {}

    def get(kind):
        if kind not in store:
            store[kind] = Case(kind, cuda)
        return store[kind]
    return get


# ------------------------------------------------------------------ bindings
def test_bindings_match_their_table():
    """The bindings of ``_C.gram`` against ``golden/native_formats_gram.json``,
    as ``test_native_api_gpu.py`` checks those of ``_C`` against its table."""
    path = os.path.join(os.path.dirname(__file__), "golden", "native_formats_gram.json")
    with open(path) as f:
        formats = json.load(f)
    m = nat.native().gram
    names = {n for n in dir(m) if not n.startswith("_") and callable(getattr(m, n))}
    assert names == set(formats)
    for name, fmt in formats.items():
        head, sep, got = getattr(m, name).__doc__.rpartition("\n\nargs: ")
        assert sep and head and got == fmt, (name, got)
    with pytest.raises(TypeError):
        m.sp_gram(0)


def test_launchers_refuse_bad_arguments(cuda):
    """Every refusal returns before a launch: the pointers are those of one
    small zero buffer, which no kernel could run on."""
    g = nat.native().gram
    z = torch.zeros(8, dtype=torch.int64, device=cuda)
    p = z.data_ptr()
    ptrs = (p,) * 9

    def gram(m=1, n=700, T=256, kind=0, self_join=0, diag=0.0, ld=700):
        g.sp_gram(*ptrs, 0, m, n, 4, T, 0, kind, 1.0, 0.0, 3.0, self_join, diag, p, ld, 0)

    def matvec(m=1, n=700, T=256, kind=0, R=1):
        g.sp_gram_matvec(*ptrs, 0, m, n, 4, T, 0, kind, 1.0, 0.0, 3.0, 0, p, R, p, p, 0)
    bad = [dict(kind=9), dict(kind=-1), dict(ld=699), dict(T=0), dict(T=SK.TILE_MAX + 1),
           dict(m=2 ** 20, n=2 ** 30, T=64, ld=2 ** 30), dict(diag=0.5), dict(n=2 ** 31, ld=2 ** 31)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="invalid"):
            gram(**kw)
    for kw in (dict(kind=9), dict(R=5), dict(R=0), dict(T=SK.TILE_MAX + 1),
               dict(m=2 ** 20, n=2 ** 30, T=64)):
        with pytest.raises(RuntimeError, match="invalid"):
            matvec(**kw)
    assert nat.native().sp_knn_tile_max() == SK.TILE_MAX
    torch.cuda.synchronize()
    assert int(z.abs().sum()) == 0


# --------------------------------------------------------------- matrix mode
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("self_join", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_matrix_against_twin(cases, kernel, kind, self_join, tile):
    c = cases(kind)
    fit, qry = c.sides(self_join)
    got = SPK.sp_kernel_matrix(fit, qry, kernel, tile=tile, **kernel_kw(kernel, kind))
    assert got.dtype == torch.float64 and got.shape == (qry.shape[0], N_FIT)
    got = got.cpu().numpy()
    want = c.twin(kernel, self_join)
    if kind == "exact" and kernel == "linear":
        np.testing.assert_array_equal(got, want)
    else:
        err, bound = np.abs(got - want), c.bound(kernel, self_join)
        print(kernel, kind, self_join, tile, "max err / (2^-53 |K|):",
              float((err[want != 0] / (U * np.abs(want[want != 0]))).max()), "max err - bound:",
              float((err - bound).max()))
        assert (err <= bound).all(), float((err - bound).max())
    if self_join and kernel == "rbf":
        np.testing.assert_array_equal(np.diag(got), np.ones(N_FIT))


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_matrix_into_the_view_of_a_larger_buffer(cases, kernel, tile):
    c = cases("exact")
    kw = kernel_kw(kernel, "exact")
    for self_join, diag in ((True, 0.25), (False, 0.0)):
        fit, qry = c.sides(self_join)
        m = qry.shape[0]
        buf = torch.full((m + 1, N_FIT + 1), -7.0, dtype=torch.float64, device=fit.device)
        out = SPK.sp_kernel_matrix(fit, qry, kernel, out=buf[1:, 1:], diag_add=diag, tile=tile,
                                   **kw)
        assert out.data_ptr() == buf[1:, 1:].data_ptr()
        assert bool((buf[0] == -7.0).all()) and bool((buf[:, 0] == -7.0).all())
        plain = SPK.sp_kernel_matrix(fit, qry, kernel, tile=tile, **kw)
        if self_join:
            plain = plain + diag * torch.eye(N_FIT, dtype=torch.float64, device=fit.device)
        assert torch.equal(buf[1:, 1:], plain)
        if self_join and kernel == "rbf":
            assert bool((torch.diagonal(buf[1:, 1:]) == 1.25).all())


@pytest.mark.parametrize("rows", [1, 32])
def test_matrix_does_not_depend_on_the_query_chunks(cases, rows):
    c = cases("random")
    for kernel in KERNELS:
        kw = kernel_kw(kernel, "random")
        for self_join in (False, True):
            fit, qry = c.sides(self_join)
            whole = SPK.sp_kernel_matrix(fit, qry, kernel, tile=TILE, **kw)
            assert torch.equal(SPK.sp_kernel_matrix(fit, qry, kernel, tile=TILE, rows=rows, **kw),
                               whole)


# ---------------------------------------------------------------- apply mode
def _rhs(R):
    return torch.as_tensor(np.random.RandomState(11 + R).standard_normal((N_FIT, R)))


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("self_join", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", ["poly", "rbf", "sigmoid"])
def test_matvec_against_twin(cases, kernel, kind, self_join, R):
    c = cases(kind)
    fit, qry = c.sides(self_join)
    kw = kernel_kw(kernel, kind)
    V = _rhs(R)
    want = SPK.sp_kernel_matvec_torch(c.fit_cpu, c.cpu[self_join], V, kernel, **kw).numpy()
    K, Va = c.twin(kernel, self_join), V.abs().numpy()
    tol = c.bound(kernel, self_join) @ Va + N_FIT * U * (np.abs(K) @ Va)
    for tile in TILES:
        got = SPK.sp_kernel_matvec(fit, qry, V, kernel, tile=tile, **kw)
        assert got.shape == (qry.shape[0], R) and got.dtype == torch.float64
        err = np.abs(got.cpu().numpy() - want)
        assert (err <= tol).all(), float((err - tol).max())
        # bit-equal from run to run and for every cut of the queries
        assert torch.equal(SPK.sp_kernel_matvec(fit, qry, V, kernel, tile=tile, **kw), got)
        assert torch.equal(SPK.sp_kernel_matvec(fit, qry, V, kernel, tile=tile, rows=9, **kw), got)


@pytest.mark.parametrize("kind", KINDS)
def test_linear_matvec_through_the_csr_products(cases, kind):
    c = cases(kind)
    nx_col = np.diff(c.X.tocsc().indptr)
    for self_join in (False, True):
        fit, qry = c.sides(self_join)
        Qs = c.X if self_join else c.Q
        nq = np.diff(Qs.indptr)
        for R in (1, 2, 4):
            V = _rhs(R)
            want = SPK.sp_kernel_matvec_torch(c.fit_cpu, c.cpu[self_join], V, "linear").numpy()
            got = SPK.sp_kernel_matvec(fit, qry, V, "linear")
            assert got.shape == (qry.shape[0], R)
            # Z = X^T V within (nnz_col + 2) u |X|^T |V|, then Q Z within
            # (nnz_q + 2) u |Q| |Z| plus |Q| times the error of Z
            B = abs(c.X).T @ V.abs().numpy()
            tol = (nq[:, None] + 2) * U * (abs(Qs) @ B) + abs(Qs) @ ((nx_col[:, None] + 2) * U * B)
            err = np.abs(got.cpu().numpy() - want)
            assert (err <= tol).all(), float((err - tol).max())
            assert torch.equal(SPK.sp_kernel_matvec(fit, qry, V, "linear"), got)


# ---------------------------------------------------------------- estimators
_CPU_FITS = {}


def _cpu_fit(Est, kernel, kind):
    key = (Est, kernel, kind)
    if key not in _CPU_FITS:
        X, _, y = case(kind)
        extra = dict(random_state=0) if Est is QLSSVC else {}
        _CPU_FITS[key] = Est(device="cpu", **extra, **estimator_kw(kernel, kind)).fit(X, y)
    return _CPU_FITS[key]


def _signs(h):
    assert np.abs(h).min() > 1e-5
    return np.sign(h)


LSSVC_RUNS = [(k, "classic", False) for k in KERNELS] + \
    [("linear", "cg", False), ("rbf", "cg", False), ("rbf", "cg", True)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel,algorithm,matrix_free", LSSVC_RUNS)
def test_lssvc_gpu_matches_cpu(cuda, monkeypatch, kernel, algorithm, matrix_free, kind):
    X, Q, y = case(kind)
    cpu = _cpu_fit(LSSVC, kernel, kind)
    if matrix_free:
        monkeypatch.setenv("SQ_SVM_DENSE_BYTES", "0")
    gpu = LSSVC(device="cuda", algorithm=algorithm, **estimator_kw(kernel, kind)).fit(X, y)
    tol = LS if algorithm == "classic" else CG
    np.testing.assert_allclose(gpu.alpha_, cpu.alpha_, **tol)
    np.testing.assert_allclose(gpu.b_, cpu.b_, **tol)
    if kernel == "linear":
        np.testing.assert_allclose(gpu.coef_, cpu.coef_, **tol)
    for A in (X, Q):
        np.testing.assert_array_equal(_signs(gpu.decision_function(A)),
                                      _signs(cpu.decision_function(A)))
    np.testing.assert_array_equal(gpu.predict(Q.toarray()), np.sign(cpu.decision_function(Q)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_qlssvc_gpu_matches_cpu(cuda, kernel, kind):
    X, Q, y = case(kind)
    cpu = _cpu_fit(QLSSVC, kernel, kind)
    gpu = QLSSVC(device="cuda", random_state=0, **estimator_kw(kernel, kind)).fit(X, y)
    for name in ("alpha_", "b_", "cond", "normF", "alpha_F", "Nu", "singular_values_F_") + \
            (("coef_",) if kernel == "linear" else ()):
        np.testing.assert_allclose(getattr(gpu, name), getattr(cpu, name), err_msg=name, **LS)
    np.testing.assert_allclose(gpu.get_betas(Q), cpu.get_betas(Q), **LS)
    for A in (X, Q):
        np.testing.assert_array_equal(gpu.classical_predict(A), _signs(cpu.get_h(A)))
