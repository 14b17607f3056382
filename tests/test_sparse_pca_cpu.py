"""PCA and qPCA on ``scipy.sparse`` rows: the torch twin of the mu(A) power
sums, the centred sparse randomized SVD and the estimators' sparse branch, on
the CPU."""

import pickle
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _sparse_pca_data as PD
from _sparse_svd_data import TOPICS, planted_topics
from sq_learn_amd.exceptions import ClassicalPathWarning
from sq_learn_amd.models._data import as_sparse_data, sparse_mean_var
from sq_learn_amd.models.decomposition import PCA, qPCA
from sq_learn_amd.ops import linalg as L
from sq_learn_amd.ops import sparse_linalg as SL
from sq_learn_amd.parallel.comm import Comm
from sq_learn_amd.utils.extmath import randomized_svd_distributed, randomized_svd_sparse

K = TOPICS - 1           # centring removes one topic direction: five values near 23, then 9.8
QKW = dict(svd_solver="randomized", quantum_truncated=True, estimate_all=True, eps=0.05,
           delta=0.05, theta_major=1.0, true_tomography=False, random_state=0, device="cpu")


@pytest.fixture(scope="module")
def planted():
    return planted_topics()


@pytest.fixture(scope="module")
def planted_dense(planted):
    return planted.toarray()


# ------------------------------------------------------------- mu(A) sums
@pytest.fixture(scope="module", params=[False, True], ids=["plain", "densecol"])
def mu_case(request):
    A = PD.matrix(request.param)
    sd = as_sparse_data(A, device="cpu")
    return A, sd, sparse_mean_var(sd)[0]


def test_fixture_structure():
    A, B = PD.matrix(True), PD.matrix(False)
    assert np.diff(B.indptr)[:len(PD.FORCED)].tolist() == PD.FORCED
    assert B.data[B.indptr[9]] == 0.0 and B.indices[B.indptr[11] - 1] == PD.LAST_COL
    col = np.diff(B.tocsc().indptr)
    assert col[PD.EMPTY_COL] == 0 and col[PD.SINGLE_COL] == 1 and col[PD.EQ_COL] == 3
    assert np.diff(A.tocsc().indptr)[PD.DENSE_COL] == PD.N
    mean = sparse_mean_var(as_sparse_data(B, device="cpu"))[0].numpy()
    assert mean[PD.EQ_COL] == 1.0 == B[PD.EQ_ROWS[0], PD.EQ_COL]
    assert mean[PD.ZERO_MEAN_COL] == 0.0 and col[PD.ZERO_MEAN_COL] == 2


@pytest.mark.parametrize("with_mean", [False, True])
def test_mu_twin_equals_dense_law(mu_case, with_mean):
    A, sd, mean = mu_case
    m = mean if with_mean else None
    rm, cs = SL.sp_mu_power_sums(sd, PD.GRID, mean=m)
    rd, cd = L.mu_power_sums_local(torch.as_tensor(A.toarray()), PD.GRID, mean=m)
    assert rm.dtype == torch.float64 and cs.shape == (len(PD.GRID), PD.D)
    assert torch.equal(rm, rd) and torch.equal(cs, cd)          # n <= TWIN_CHUNK: one chunk
    if with_mean:
        # the stored value equal to its mean is a zero of the centred matrix; the zero-mean
        # column keeps its unstored zeros
        assert cs[0, PD.EQ_COL] == PD.N - 1 and cs[0, PD.ZERO_MEAN_COL] == 2
        assert cs[0, PD.EMPTY_COL] == 0 and cs[0, PD.SINGLE_COL] == PD.N
    else:
        assert cs[0, PD.EQ_COL] == 3 and cs[0, PD.SINGLE_COL] == 1


@pytest.mark.parametrize("exps", [PD.GRID, PD.LIST, PD.ONE], ids=["grid", "list", "one"])
@pytest.mark.parametrize("with_mean", [False, True])
def test_mu_identity_within_derived_bound(mu_case, with_mean, exps):
    A, sd, mean = mu_case
    m = mean if with_mean else None
    rm, cs = SL.sp_mu_power_sums_torch(sd, exps, m)
    ri, ci = PD.identity_sums(A, None if m is None else m.numpy(), exps)
    rb, cb = PD.mu_tolerance(A, None if m is None else m.numpy(), exps, law="list")
    er, ec = np.abs(ri - rm.numpy()), np.abs(ci - cs.numpy())
    print("row err / bound", (er / np.maximum(rb, 1e-300)).max(),
          "col err / bound", (ec / np.maximum(cb, 1e-300)).max())
    assert (er <= rb).all() and (ec <= cb).all()
    for i, q in enumerate(exps):
        if q == 0:
            assert ri[i] == rm[i] and (ci[i] == cs[i].numpy()).all()


def test_mu_chunks_and_validation(planted):
    sd = as_sparse_data(planted, device="cpu")           # 2500 rows: two chunks
    mean = sparse_mean_var(sd)[0]
    rm, cs = SL.sp_mu_power_sums(sd, PD.GRID, mean=mean)
    rd, cd = L.mu_power_sums_local(torch.as_tensor(planted.toarray()), PD.GRID, mean=mean)
    assert torch.equal(rm, rd)
    np.testing.assert_allclose(cs.numpy(), cd.numpy(), rtol=1e-13)
    with pytest.raises(ValueError, match="exponent"):
        SL.sp_mu_power_sums(sd, [])
    with pytest.raises(ValueError, match="exponent"):
        SL.sp_mu_power_sums(sd, [-1.0])
    with pytest.raises(ValueError, match="columns"):
        SL.sp_mu_power_sums(sd, [1.0], mean=mean[:-1])
    assert SL.arithmetic_grid_step(PD.GRID) == 0.2 and SL.arithmetic_grid_step(PD.LIST) == 0.0
    assert SL.arithmetic_grid_step(PD.ONE) == 0.0
    n, d = sd.shape
    assert SL.svd_bytes(sd, 16, centred=True) == SL.svd_bytes(sd, 16) + n * 16 * 8
    assert SL.svd_bytes(sd, 16, centred=True, nq=11) >= SL.svd_bytes(sd, 16, centred=True) \
        + 11 * d * 8


# --------------------------------------------------- centred randomized SVD
@pytest.mark.parametrize("seed", [0, 7])
def test_centred_randomized_svd_matches_dense_stream(planted, planted_dense, seed):
    sd = as_sparse_data(planted, device="cpu")
    mean = sparse_mean_var(sd)[0]
    Xd = torch.as_tensor(planted_dense)
    Ud, s_d, Vd = randomized_svd_distributed(Xd, mean, K, Comm(None), method="stream", seed=seed,
                                             n_iter=5)
    U, s, Vt = randomized_svd_sparse(sd, K, seed=seed, n_iter=5, mean=mean)
    np.testing.assert_allclose(s.numpy(), s_d.numpy(), rtol=1e-9, atol=0)
    np.testing.assert_allclose(Vt.numpy(), Vd.numpy(), rtol=0, atol=1e-9)
    np.testing.assert_allclose(U.numpy(), Ud.numpy(), rtol=0, atol=1e-9)


def test_uncentred_randomized_svd_unchanged(planted):
    """``mean=None`` is the path of before, operation for operation."""
    from sq_learn_amd.ops.random import philox_normal
    from sq_learn_amd.runtime.rng import RngKey
    from sq_learn_amd.utils.extmath import _cholqr2_rows, _rsvd_finish
    sd = as_sparse_data(planted, device="cpu")
    Z = philox_normal((sd.d, TOPICS + 10), RngKey(0, "gaussian", 0), dtype=torch.float64,
                      device="cpu")
    for _ in range(5):
        Z, _ = torch.linalg.qr(SL.sp_power_iter(sd, Z))
    Y = _cholqr2_rows(SL.sp_xw(sd, Z), sd.comm)
    want = _rsvd_finish(Y, SL.sp_xty(sd, Y).T, TOPICS, sd.comm, True)
    got = randomized_svd_sparse(sd, TOPICS, seed=0, n_iter=5)
    again = randomized_svd_sparse(sd, TOPICS, seed=0, n_iter=5, mean=None)
    for w, g, a in zip(want, got, again):
        assert torch.equal(w, g) and torch.equal(w, a)


# --------------------------------------------------------------- estimators
@pytest.fixture(scope="module")
def pca_fits(planted, planted_dense):
    kw = dict(n_components=K, svd_solver="randomized", random_state=0, device="cpu")
    sparse, dense = PCA(**kw), PCA(**kw)
    return sparse, sparse.fit_transform(planted), dense, dense.fit_transform(planted_dense)


@pytest.fixture(scope="module")
def qpca_fits(planted, planted_dense):
    sparse, dense = qPCA(K, **QKW), qPCA(K, **QKW)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ClassicalPathWarning)
        sparse.fit(planted)
        dense.fit(planted_dense)
    return sparse, dense


def _same_fit(sparse, dense):
    np.testing.assert_allclose(sparse.singular_values_, dense.singular_values_, rtol=1e-6)
    np.testing.assert_allclose(sparse.explained_variance_, dense.explained_variance_, rtol=1e-6)
    np.testing.assert_allclose(sparse.explained_variance_ratio_, dense.explained_variance_ratio_,
                               rtol=1e-6)
    np.testing.assert_allclose(sparse.noise_variance_, dense.noise_variance_, rtol=1e-6)
    np.testing.assert_allclose(sparse.mean_, dense.mean_, rtol=0, atol=1e-15)
    np.testing.assert_allclose(sparse.components_, dense.components_, rtol=0, atol=1e-9)
    assert sparse.n_components_ == K and sparse.n_features_in_ == dense.n_features_in_
    assert sparse._fit_svd_solver == dense._fit_svd_solver == "randomized"


def test_pca_sparse_against_dense(pca_fits, planted, planted_dense):
    sparse, Ts, dense, Td = pca_fits
    _same_fit(sparse, dense)
    assert isinstance(Ts, np.ndarray) and Ts.shape == (planted.shape[0], K)
    np.testing.assert_allclose(Ts, Td, rtol=0, atol=1e-9)                # fit_transform: U S
    T = sparse.transform(planted)
    assert isinstance(T, np.ndarray)
    np.testing.assert_allclose(T, dense.transform(planted_dense), rtol=0, atol=1e-9)
    w = PCA(K, svd_solver="randomized", whiten=True, random_state=0, device="cpu")
    wd = PCA(K, svd_solver="randomized", whiten=True, random_state=0, device="cpu")
    np.testing.assert_allclose(w.fit_transform(planted), wd.fit_transform(planted_dense), rtol=0,
                               atol=1e-9)
    np.testing.assert_allclose(w.transform(planted), wd.transform(planted_dense), rtol=0,
                               atol=1e-9)


def test_qpca_sparse_against_dense(qpca_fits, planted, planted_dense):
    sparse, dense = qpca_fits
    _same_fit(sparse, dense)
    assert isinstance(sparse.left_sv, np.ndarray) and sparse.left_sv.shape == (K, planted.shape[0])
    np.testing.assert_allclose(sparse.left_sv, dense.left_sv, rtol=0, atol=1e-9)
    np.testing.assert_allclose(sparse.transform(planted), dense.transform(planted_dense), rtol=0,
                               atol=1e-9)
    np.testing.assert_allclose(qPCA(K, **QKW).fit_transform(planted),
                               qPCA(K, **QKW).fit_transform(planted_dense), rtol=0, atol=1e-9)
    # mu(A) of the centred matrix: the twin applies the dense law chunk by chunk
    assert sparse.norm_muA == dense.norm_muA
    np.testing.assert_allclose(sparse.muA, dense.muA, rtol=1e-12)
    np.testing.assert_allclose(sparse.frob_norm, dense.frob_norm, rtol=1e-12)
    # the quantum extras run on the dense factors
    for name in ("estimate_right_sv", "estimate_left_sv", "estimate_s_values", "estimate_fs_ratio"):
        got, want = np.asarray(getattr(sparse, name)), np.asarray(getattr(dense, name))
        assert got.shape == want.shape and np.isfinite(got).all()
    assert sparse.topk == dense.topk == K
    np.testing.assert_allclose(sparse.estimate_s_values, dense.estimate_s_values, rtol=1e-6)
    np.testing.assert_allclose(sparse.transform(planted, use_classical_components=False,
                                                classic_transform=False),
                               dense.transform(planted_dense, use_classical_components=False,
                                               classic_transform=False), rtol=0, atol=1e-6)


def test_qpca_classical_path_warning(planted):
    with pytest.warns(ClassicalPathWarning):
        q = qPCA(K, svd_solver="arpack", random_state=0, device="cpu").fit(planted)
    assert q._fit_svd_solver == "arpack" and not hasattr(q, "muA")


def test_singular_values_against_scikit_learn(pca_fits, planted):
    from sklearn.decomposition import PCA as SkPCA
    ref = SkPCA(K, svd_solver="arpack").fit(planted)
    np.testing.assert_allclose(pca_fits[0].singular_values_, ref.singular_values_, rtol=1e-6)


def test_auto_selects_randomized(pca_fits, planted):
    est = PCA(K, random_state=0, device="cpu").fit(planted)
    assert est._fit_svd_solver == "randomized"
    np.testing.assert_array_equal(est.singular_values_, pca_fits[0].singular_values_)


# ---------------------------------------------------------- other behaviour
@pytest.mark.parametrize("cls", [PCA, qPCA])
def test_small_input_equals_array_to_the_bit(cls):
    A = sp.random(300, 500, density=0.05, random_state=np.random.RandomState(1), format="csr")
    a = cls(4, svd_solver="full", random_state=0, device="cpu").fit(A)
    b = cls(4, svd_solver="full", random_state=0, device="cpu").fit(A.toarray())
    for name in ("components_", "singular_values_", "explained_variance_",
                 "explained_variance_ratio_", "mean_"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    np.testing.assert_array_equal(
        cls(4, random_state=0, device="cpu").fit_transform(A),
        cls(4, random_state=0, device="cpu").fit_transform(A.toarray()))


@pytest.mark.parametrize("fmt", ["csc", "coo"])
def test_other_sparse_formats(pca_fits, planted, fmt):
    est = PCA(K, svd_solver="randomized", random_state=0, device="cpu").fit(planted.asformat(fmt))
    np.testing.assert_array_equal(est.singular_values_, pca_fits[0].singular_values_)
    np.testing.assert_array_equal(est.components_, pca_fits[0].components_)


def test_unsorted_duplicates_and_caller_unchanged(pca_fits, planted):
    coo = planted.tocoo()
    perm = np.random.RandomState(0).permutation(coo.nnz)
    rows = np.concatenate([coo.row[perm], coo.row])
    cols = np.concatenate([coo.col[perm], coo.col])
    vals = np.concatenate([0.5 * coo.data[perm], 0.5 * coo.data])
    order = np.argsort(rows, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=planted.shape[0]))])
    A = sp.csr_matrix((vals[order], cols[order].astype(np.int32), indptr.astype(np.int32)),
                      shape=planted.shape)
    A.has_sorted_indices = False
    A.has_canonical_format = False
    assert not A.has_canonical_format and A.nnz == 2 * planted.nnz
    keep = (A.indptr.copy(), A.indices.copy(), A.data.copy())
    est = PCA(K, svd_solver="randomized", random_state=0, device="cpu").fit(A)
    for got, want in zip((A.indptr, A.indices, A.data), keep):
        np.testing.assert_array_equal(got, want)
    np.testing.assert_allclose(est.singular_values_, pca_fits[0].singular_values_, rtol=1e-12)


def test_integer_dtype():
    rng = np.random.RandomState(2)
    A = sp.random(2200, 2000, density=0.01, random_state=rng, format="csr")
    A.data = rng.randint(1, 6, size=A.nnz).astype(np.int64)
    assert A.dtype.kind == "i"
    a = PCA(3, svd_solver="randomized", random_state=0, device="cpu").fit(A)
    b = PCA(3, svd_solver="randomized", random_state=0, device="cpu").fit(A.astype(np.float64))
    np.testing.assert_array_equal(a.singular_values_, b.singular_values_)
    assert A.dtype.kind == "i"


@pytest.mark.parametrize("which", [0, 1])
def test_feature_count_error(pca_fits, qpca_fits, planted, which):
    est = (pca_fits[0], qpca_fits[0])[which]
    with pytest.raises(ValueError, match=f"X has 1999 features, but {type(est).__name__} is "
                                         "expecting 2000 features as input."):
        est.transform(planted[:, :1999])


@pytest.mark.parametrize("cls", [PCA, qPCA])
@pytest.mark.parametrize("kw", [dict(n_components=K, svd_solver="full"),
                                dict(n_components=None), dict(n_components="mle"),
                                dict(n_components=0.9),
                                dict(n_components=0.9, svd_solver="randomized"),
                                dict(n_components=1900),               # 'auto' resolves to 'full'
                                dict(n_components=None, svd_solver="arpack")])
def test_full_spectrum_refused_above_limit(planted, cls, kw):
    with pytest.raises(ValueError, match="'randomized'.*integer n_components"):
        cls(device="cpu", **kw).fit(planted)


def test_score_samples_refuses_sparse(pca_fits, qpca_fits, planted):
    for est in (pca_fits[0], qpca_fits[0]):
        with pytest.raises(TypeError, match="sparse"):
            est.score_samples(planted[:10])
        with pytest.raises(TypeError, match="sparse"):
            est.score(planted[:10])


def test_pickle_round_trip(pca_fits, qpca_fits, planted):
    for est in (pca_fits[0], qpca_fits[0]):
        again = pickle.loads(pickle.dumps(est))
        np.testing.assert_array_equal(again.components_, est.components_)
        np.testing.assert_array_equal(again.transform(planted[:50]), est.transform(planted[:50]))


def test_transform_across_input_kinds(pca_fits, planted, planted_dense):
    sparse, _, dense, _ = pca_fits
    # sparse rows through a dense-fitted estimator, dense rows through a sparse-fitted one
    np.testing.assert_allclose(dense.transform(planted[:200]), dense.transform(planted_dense[:200]),
                               rtol=0, atol=1e-9)
    np.testing.assert_allclose(sparse.transform(planted_dense[:200]),
                               sparse.transform(planted[:200]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(sparse.inverse_transform(sparse.transform(planted[:5])),
                               dense.inverse_transform(dense.transform(planted_dense[:5])),
                               rtol=0, atol=1e-9)
