"""``MiniBatchKMeans`` on scipy sparse input against the dense path (CPU).

``fit(csr)`` and ``fit(csr.toarray())`` consume the host ``RandomState`` in
the same order and work in fp64, so they walk the same trajectory; the only
difference is the rounding of the distance formula (the sparse twin clamps
the distances at 0 before the minimum and sums the dot products over the
stored values only).  The data are planted, well separated clusters, and
every comparison first checks on the dense path that no argmin of the run
sits within 1e-6 of the distance scale of the runner-up, so a rounding
difference cannot move a label.
"""

import pickle

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sq_learn_amd.cluster import MiniBatchKMeans
from sq_learn_amd.models.cluster import _sparse
from sq_learn_amd.models.cluster import minibatch as mb_mod

N, D, K_TRUE = 1500, 200, 5
SUPPORT = 24          # features of a planted cluster
RTOL = 1e-10


def _planted(seed=7, n=N):
    """(csr, dense, cluster centres): cluster c lives on its own block of
    SUPPORT features (value 4 plus noise on about 60 % of them), plus about
    eight noise entries anywhere; about 22 stored values per row."""
    rng = np.random.RandomState(seed)
    lab = rng.randint(K_TRUE, size=n)
    X = np.zeros((n, D))
    cent = np.zeros((K_TRUE, D))
    for c in range(K_TRUE):
        cent[c, c * SUPPORT:(c + 1) * SUPPORT] = 4.0 * 0.6
    for i in range(n):
        blk = np.arange(lab[i] * SUPPORT, (lab[i] + 1) * SUPPORT)
        on = blk[rng.rand(SUPPORT) < 0.6]
        X[i, on] = 4.0 + 0.3 * rng.standard_normal(len(on))
        noise = rng.choice(D, size=8, replace=False)
        X[i, noise] += 0.3 * rng.standard_normal(8)
    A = sp.csr_matrix(X)
    return A, A.toarray(), cent


@pytest.fixture(scope="module")
def data():
    return _planted()


@pytest.fixture
def gaps(monkeypatch):
    """Records, for every E-step of the dense path, the smallest
    best-to-second distance gap relative to the distance scale."""
    seen = []
    real = mb_mod._labels_inertia

    def spy(X, w, C, xn=None):
        if C.shape[0] > 1:
            x2 = (X * X).sum(1)
            c2 = (C * C).sum(1)
            Dm = x2[:, None] - 2.0 * (X @ C.T) + c2[None, :]
            two = Dm.topk(2, dim=1, largest=False).values
            seen.append(float((two[:, 1] - two[:, 0]).min() / (x2.max() + c2.max())))
        return real(X, w, C, xn)

    monkeypatch.setattr(mb_mod, "_labels_inertia", spy)
    return seen


def _pair(A, Xd, gaps, fit_kw=None, k=K_TRUE, **kw):
    """(sparse fit, dense fit) with the same parameters; the no-near-tie
    precondition is checked on the dense run."""
    kw.setdefault("batch_size", 100)
    kw.setdefault("max_iter", 3)
    kw.setdefault("random_state", 3)
    kw.setdefault("device", "cpu")
    fit_kw = fit_kw or {}
    init = kw.pop("init")
    own = (lambda: init.copy()) if isinstance(init, np.ndarray) else (lambda: init)
    # (the dense path updates an array init in place: each fit gets its own)
    dense = MiniBatchKMeans(k, init=own(), **kw).fit(Xd, **fit_kw)
    assert gaps and min(gaps) > 1e-6, min(gaps)
    given = own()
    sparse = MiniBatchKMeans(k, init=given, **kw).fit(A, **fit_kw)
    if isinstance(init, np.ndarray):
        assert np.array_equal(given, init)               # the sparse path leaves it alone
    return sparse, dense


def _assert_same(s, d):
    assert s.n_iter_ == d.n_iter_ and s.n_steps_ == d.n_steps_
    assert s.labels_.dtype == np.int32 and np.array_equal(s.labels_, d.labels_)
    assert s.cluster_centers_.dtype == np.float64
    np.testing.assert_allclose(s.cluster_centers_, d.cluster_centers_, rtol=RTOL, atol=0)
    np.testing.assert_allclose(s.counts_, d.counts_, rtol=RTOL, atol=0)
    np.testing.assert_allclose(s.inertia_, d.inertia_, rtol=RTOL)


def _array_init(cent):
    return cent + 0.05


@pytest.mark.parametrize("init", ["array", "random", "k-means++"])
def test_fit_matches_dense(data, gaps, init):
    A, Xd, cent = data
    s, d = _pair(A, Xd, gaps, init=_array_init(cent) if init == "array" else init)
    _assert_same(s, d)
    assert s.n_features_in_ == D


def test_fit_sample_weight(data, gaps):
    A, Xd, cent = data
    w = np.random.RandomState(1).choice([0.5, 1.0, 2.0, 3.5], size=N)
    s, d = _pair(A, Xd, gaps, fit_kw={"sample_weight": w}, init="k-means++")
    _assert_same(s, d)
    u, _ = _pair(A, Xd, gaps, init="k-means++")
    assert not np.array_equal(u.counts_, s.counts_)      # the weights reach the sums


def test_fit_tol_stops_at_the_same_step(data, gaps):
    A, Xd, cent = data
    s, d = _pair(A, Xd, gaps, init=_array_init(cent), tol=1e-2, max_iter=20,
                 max_no_improvement=None)
    _assert_same(s, d)
    assert 1 < d.n_iter_ < 20 * 15                       # stopped early, by the shift


def test_fit_max_no_improvement_stops_at_the_same_step(data, gaps):
    A, Xd, cent = data
    s, d = _pair(A, Xd, gaps, init=_array_init(cent), max_no_improvement=3, max_iter=20)
    _assert_same(s, d)
    assert 3 < d.n_iter_ < 20 * 15


def test_fit_reassignment(data, gaps, monkeypatch):
    """Seven centres: one per planted cluster plus a far-away point and its
    duplicate, which no row ever prefers (so the duplicate ties with nothing
    that matters); with a large ``reassignment_ratio`` the two starved
    centres are replaced by batch rows on the tenth step."""
    A, Xd, cent = data
    far = np.full((1, D), 50.0)
    init = np.vstack([_array_init(cent), far, far])
    done = []
    real = _sparse._mb_reassign

    def spy(*a):
        done.append(real(*a))
        return done[-1]

    monkeypatch.setattr(_sparse, "_mb_reassign", spy)
    s, d = _pair(A, Xd, gaps, k=K_TRUE + 2, init=init, reassignment_ratio=0.3, max_iter=2,
                 max_no_improvement=None)
    assert any(done)
    assert np.abs(s.cluster_centers_).max() < 10.0       # both starved centres were replaced
    _assert_same(s, d)


def test_partial_fit_matches_dense(data, gaps):
    A, Xd, cent = data
    s = MiniBatchKMeans(K_TRUE, init="k-means++", random_state=5, device="cpu")
    d = MiniBatchKMeans(K_TRUE, init="k-means++", random_state=5, device="cpu")
    for a, b in [(0, 500), (500, 1000), (1000, 1500)]:
        d.partial_fit(Xd[a:b])
        s.partial_fit(A[a:b])
        assert min(gaps) > 1e-6
        assert s.n_steps_ == d.n_steps_
        assert np.array_equal(s.labels_, d.labels_)
        np.testing.assert_allclose(s.cluster_centers_, d.cluster_centers_, rtol=RTOL, atol=0)
        np.testing.assert_allclose(s.counts_, d.counts_, rtol=RTOL, atol=0)
        np.testing.assert_allclose(s.inertia_, d.inertia_, rtol=RTOL)
    assert s.n_steps_ == 3
    assert s._rs.get_state()[1].tolist() == d._rs.get_state()[1].tolist()


@pytest.fixture(scope="module")
def fitted(data):
    A, Xd, cent = data
    kw = dict(batch_size=100, max_iter=2, random_state=0, device="cpu")
    return (MiniBatchKMeans(K_TRUE, init=_array_init(cent), **kw).fit(A),
            MiniBatchKMeans(K_TRUE, init=_array_init(cent), **kw).fit(Xd))


def test_predict_transform_score(data, fitted):
    A, Xd, _ = data
    s, d = fitted
    B, Bd = A[:700], Xd[:700]
    w = np.random.RandomState(2).rand(700) + 0.5
    assert np.array_equal(s.predict(B), d.predict(Bd))
    assert s.predict(B).dtype == np.int32
    T = s.transform(B)
    assert T.shape == (700, K_TRUE)
    np.testing.assert_allclose(T, d.transform(Bd), rtol=1e-9)
    np.testing.assert_allclose(s.score(B), d.score(Bd), rtol=RTOL)
    np.testing.assert_allclose(s.score(B, sample_weight=w), d.score(Bd, sample_weight=w),
                               rtol=RTOL)
    assert np.array_equal(MiniBatchKMeans(K_TRUE, init="random", batch_size=100, max_iter=1,
                                          random_state=1, device="cpu").fit_predict(B),
                          MiniBatchKMeans(K_TRUE, init="random", batch_size=100, max_iter=1,
                                          random_state=1, device="cpu").fit_predict(Bd))


@pytest.mark.parametrize("fmt", ["csc", "coo"])
def test_other_formats(data, fitted, fmt):
    A, _, cent = data
    B = A.asformat(fmt)
    m = MiniBatchKMeans(K_TRUE, init=_array_init(cent), batch_size=100, max_iter=2,
                        random_state=0, device="cpu").fit(B)
    assert np.array_equal(m.cluster_centers_, fitted[0].cluster_centers_)
    assert np.array_equal(m.predict(B), fitted[0].labels_)


def test_feature_mismatch_raises(data, fitted):
    A, _, _ = data
    s = fitted[0]
    bad = A[:50, :D - 1]
    for call in (s.predict, s.transform, s.score):
        with pytest.raises(ValueError, match="features"):
            call(bad)
    p = MiniBatchKMeans(K_TRUE, random_state=0, device="cpu").partial_fit(A[:300])
    with pytest.raises(ValueError, match="features"):
        p.partial_fit(bad)


def test_input_unchanged(data):
    A, _, _ = data
    # a duplicate entry in the last row: canonicalisation must run on a copy
    B = sp.csr_matrix((np.r_[A.data, 1.0], np.r_[A.indices, A.indices[-1]],
                       np.r_[A.indptr[:-1], A.indptr[-1] + 1]), shape=A.shape)
    snap = (B.data.copy(), B.indices.copy(), B.indptr.copy())
    m = MiniBatchKMeans(K_TRUE, batch_size=100, max_iter=1, random_state=0, device="cpu")
    m.fit(B, sample_weight=np.ones(N))
    m.partial_fit(B)
    m.predict(B), m.transform(B), m.score(B)
    for got, want in zip((B.data, B.indices, B.indptr), snap):
        assert np.array_equal(got, want)


def test_pickle_round_trip(data, fitted):
    A, _, _ = data
    s = fitted[0]
    r = pickle.loads(pickle.dumps(s))
    assert np.array_equal(r.cluster_centers_, s.cluster_centers_)
    assert np.array_equal(r.counts_, s.counts_)
    assert np.array_equal(r.predict(A[:300]), s.predict(A[:300]))
    # a restored estimator keeps learning from sparse batches
    r.partial_fit(A[:300])
    assert r.cluster_centers_.shape == (K_TRUE, D)


def test_random_state_left_as_by_dense_fit(data):
    A, Xd, _ = data
    for init in ("k-means++", "random"):
        ra, rb = np.random.RandomState(11), np.random.RandomState(11)
        kw = dict(init=init, batch_size=100, max_iter=2, reassignment_ratio=0.3, device="cpu")
        MiniBatchKMeans(K_TRUE, random_state=ra, **kw).fit(A)
        MiniBatchKMeans(K_TRUE, random_state=rb, **kw).fit(Xd)
        sa, sb = ra.get_state(), rb.get_state()
        assert sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


def test_sub_container_matches_scipy(data):
    A, _, _ = data
    sd = _sparse.as_sparse_data(A, device="cpu")
    ids = np.array([5, 0, 5, 1499, 7])
    sub = _sparse.take_rows(sd, ids)
    want = A[ids]
    assert np.array_equal(sub.indptr.numpy(), want.indptr)
    assert np.array_equal(sub.indices.numpy(), want.indices)
    assert np.array_equal(sub.data.numpy(), want.data)
    assert torch.equal(sub.dense_rows(0, 5), torch.as_tensor(want.toarray()))
