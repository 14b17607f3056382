"""CSR sparse input for KMeans / QMeans / k_means on the CPU (torch twins of
``csrc/spkmeans.hip``).  Every test here fails without the sparse path: the
estimators used to refuse a scipy sparse matrix with a TypeError."""

import pickle
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.spatial.distance import cdist

from sq_learn_amd.models._data import Data, as_sparse_data
from sq_learn_amd.models.cluster import KMeans, QMeans
from sq_learn_amd.models.cluster import _sparse
from sq_learn_amd.models.cluster._init import kmeans_plusplus
from sq_learn_amd.models.cluster.kmeans import k_means
from sq_learn_amd.ops import kmeans as K
from sq_learn_amd.ops import sparse_kmeans as S
from sq_learn_amd.pipeline import Pipeline
from sq_learn_amd.runtime.rng import RngKey
from sq_learn_amd.utils.validation import seed_from_random_state

K_PLANTED = 6


def _planted(n=600, d=200, seed=0):
    """sp.random(n, d, 0.05) plus three planted sparse centres."""
    base = sp.random(n, d, density=0.05, random_state=seed).toarray()
    for c in range(3):
        centre = sp.random(1, d, density=0.1, random_state=100 + c).toarray()[0] * 5.0
        base[c::3] += centre
    return sp.csr_matrix(base)


@pytest.fixture(scope="module")
def planted():
    X = _planted()
    return X, X.toarray()[:K_PLANTED].copy()


def _quiet(f):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f()


@pytest.mark.parametrize("weighted", [False, True])
def test_sklearn_parity(planted, weighted):
    from sklearn.cluster import KMeans as SkKMeans
    X, init = planted
    sw = np.random.RandomState(3).uniform(0.5, 2.0, X.shape[0]) if weighted else None
    ours = KMeans(K_PLANTED, device="cpu", n_init=1, init=init).fit(X, sample_weight=sw)
    ref = SkKMeans(K_PLANTED, n_init=1, init=init, algorithm="lloyd").fit(X, sample_weight=sw)
    assert np.array_equal(ours.labels_, ref.labels_)
    assert np.allclose(ours.cluster_centers_, ref.cluster_centers_, rtol=1e-9, atol=0)
    assert np.isclose(ours.inertia_, ref.inertia_, rtol=1e-9, atol=0)
    assert ours.n_iter_ == ref.n_iter_


def test_qmeans_delta0_equals_kmeans(planted):
    X, init = planted
    km = KMeans(K_PLANTED, device="cpu", n_init=1, init=init).fit(X)
    qm = _quiet(lambda: QMeans(K_PLANTED, device="cpu", n_init=1, init=init, delta=0).fit(X))
    assert np.array_equal(qm.labels_, km.labels_)
    assert np.allclose(qm.cluster_centers_, km.cluster_centers_, rtol=1e-12, atol=0)
    assert np.isclose(qm.inertia_, km.inertia_, rtol=1e-12)


def test_delta_band(planted):
    X, init = planted
    delta = 0.5
    qm = QMeans(K_PLANTED, device="cpu", n_init=1, init=init, delta=delta, true_distance_estimate=False,
                intermediate_error=False, random_state=0, max_iter=7).fit(X)
    C = qm.cluster_centers_
    D = torch.as_tensor(cdist(X.toarray(), C, "sqeuclidean"))
    lab = qm.labels_.astype(np.int64)
    mn = D.min(1).values.numpy()
    picked = D.numpy()[np.arange(len(lab)), lab]
    assert (picked <= mn + delta).all()
    # the labels are those of the last E-step: the band rule on the exact
    # distances with the engine's key (restart 0, iteration n_iter_)
    key = RngKey(seed_from_random_state(0), "band_select", qm.n_iter_)
    sd = as_sparse_data(X, device="cpu")
    Dt = S.sp_sqdist(sd, torch.as_tensor(C))
    want, _ = K.band_select_torch(Dt, torch.arange(X.shape[0]), delta, key, K.pad_clusters(K_PLANTED))
    assert np.array_equal(lab, want.numpy())
    assert (torch.as_tensor(lab) != Dt.argmin(1)).any()   # the band did pick non-minimal members


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ipe_twin(planted, seed):
    X, init = planted
    sd = as_sparse_data(X, device="cpu")
    C = torch.as_tensor(init)
    eng = _sparse.SparseLloydEngine(sd, K_PLANTED, delta=0.5, true_distance_estimate=True,
                                    seed=seed, ipe_Q=5, ipe_chunk=250)
    eng.restart, eng.it = 1, 3
    lab, mind, _ = eng.estep(C)
    want, wmin = K.ipe_estep_torch(torch.as_tensor(X.toarray()), C, 0.25, eng._key("ipe"), 0,
                                   K.pad_clusters(K_PLANTED), Q=5)
    assert np.array_equal(lab.numpy(), want.numpy())
    assert np.allclose(mind.numpy(), wmin.numpy(), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("rs", range(5))
def test_kmeans_plusplus_ids(rs):
    X = _planted(n=500, d=60, seed=7)
    sd = as_sparse_data(X, device="cpu")
    _, ids = _sparse.sparse_kmeans_plusplus(sd, 8, np.random.RandomState(rs))
    dense = torch.as_tensor(X.toarray())
    data = Data(dense, 500, 0, sd.comm, "numpy")
    _, want = kmeans_plusplus(data, 8, np.random.RandomState(rs))
    assert np.array_equal(ids, want)


def test_tfidf_pipeline():
    from sq_learn_amd.feature_extraction.text import TfidfVectorizer
    vocab = [["apple", "pear", "plum", "fig", "lime"], ["car", "bus", "tram", "bike", "boat"],
             ["red", "blue", "green", "pink", "grey"]]
    rng = np.random.RandomState(0)
    docs, truth = [], []
    for i in range(30):
        g = i % 3
        docs.append(" ".join(rng.choice(vocab[g], size=6)))
        truth.append(g)
    pipe = Pipeline([("tfidf", TfidfVectorizer()), ("km", KMeans(3, random_state=0, device="cpu"))])
    labels = pipe.fit(docs).named_steps["km"].labels_
    truth = np.array(truth)
    purity = sum(np.bincount(truth[labels == c]).max() for c in np.unique(labels)) / len(truth)
    assert purity == 1.0


@pytest.mark.parametrize("cls", [KMeans, QMeans])
def test_predict_transform_score(planted, cls):
    X, init = planted
    kw = dict(delta=0) if cls is QMeans else {}
    est = _quiet(lambda: cls(K_PLANTED, device="cpu", n_init=1, init=init, **kw).fit(X))
    assert np.array_equal(est.predict(X), est.labels_)
    T = est.transform(X)
    assert T.shape == (X.shape[0], K_PLANTED)
    assert np.allclose(T, cdist(X.toarray(), est.cluster_centers_), rtol=1e-7, atol=1e-7)
    assert np.isclose(est.score(X), -est.inertia_, rtol=1e-9)
    assert np.array_equal(_quiet(lambda: cls(K_PLANTED, device="cpu", n_init=1, init=init, **kw).fit_predict(X)),
                          est.labels_)
    assert np.allclose(_quiet(lambda: cls(K_PLANTED, device="cpu", n_init=1, init=init, **kw).fit_transform(X)),
                       T)


def test_k_means_function(planted):
    X, init = planted
    C, labels, inertia = k_means(X, K_PLANTED, init=init, n_init=1)
    km = KMeans(K_PLANTED, n_init=1, init=init).fit(X)     # same (default) device
    assert np.array_equal(labels, km.labels_) and inertia == km.inertia_


def test_input_handling(planted):
    X, init = planted
    # rows reversed (unsorted indices) and every first entry split in two
    # halves (duplicates that sum back exactly)
    data, indices, indptr = [], [], [0]
    for i in range(X.shape[0]):
        lo, hi = X.indptr[i], X.indptr[i + 1]
        c, v = X.indices[lo:hi][::-1], X.data[lo:hi][::-1].copy()
        if len(c):
            v[0] *= 0.5
            c, v = np.append(c, c[0]), np.append(v, v[0])
        data.append(v)
        indices.append(c)
        indptr.append(indptr[-1] + len(c))
    messy = sp.csr_matrix((np.concatenate(data), np.concatenate(indices), np.array(indptr)),
                          shape=X.shape)
    assert messy.nnz > X.nnz and not messy.has_canonical_format
    snap = (messy.data.copy(), messy.indices.copy(), messy.indptr.copy())
    km = KMeans(K_PLANTED, device="cpu", n_init=1, init=init).fit(messy)
    assert np.array_equal(messy.data, snap[0]) and np.array_equal(messy.indices, snap[1]) \
        and np.array_equal(messy.indptr, snap[2])
    ref = KMeans(K_PLANTED, device="cpu", n_init=1, init=init).fit(X)
    assert np.array_equal(km.labels_, ref.labels_)
    for conv in (sp.csc_matrix, sp.coo_matrix):
        assert np.array_equal(KMeans(K_PLANTED, device="cpu", n_init=1, init=init).fit(conv(X)).labels_,
                              ref.labels_)
    bad = X.copy()
    bad.data[3] = np.nan
    with pytest.raises(ValueError):
        KMeans(K_PLANTED, device="cpu", n_init=1, init=init).fit(bad)
    # explicitly stored zeros are kept and harmless
    z = X.copy()
    z.data[:10] = 0.0
    sd = as_sparse_data(z, device="cpu")
    assert sd.nnz == z.nnz


@pytest.mark.parametrize("cls,kw", [
    (QMeans, dict(failure_prob=0.1)),
    (QMeans, dict(checkpoint_dir="unused_dir")),
    (QMeans, dict(gemm_precision="bf16")),
    (KMeans, dict(gemm_precision="bf16")),
    (QMeans, dict(init="k-means||")),
    (KMeans, dict(init="k-means||")),
])
def test_refusals(planted, cls, kw):
    X, _ = planted
    with pytest.raises(ValueError):
        cls(3, device="cpu", **kw).fit(X)


def test_runtime_comparison_refused(planted):
    X, init = planted
    qm = QMeans(K_PLANTED, device="cpu", n_init=1, init=init, delta=0.5, true_distance_estimate=False, max_iter=2).fit(X)
    assert qm.condition_number is None and qm.eta > 0 and qm.muA > 0
    with pytest.raises(ValueError, match="condition_number"):
        qm.runtime_comparison(100, 10)


def test_elkan_runs_full_without_warning(planted):
    X, init = planted
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        el = KMeans(K_PLANTED, device="cpu", n_init=1, init=init, algorithm="elkan").fit(X)
    assert np.array_equal(el.labels_, KMeans(K_PLANTED, device="cpu", n_init=1, init=init).fit(X).labels_)


def test_random_and_callable_init(planted):
    X, init = planted
    a = KMeans(K_PLANTED, device="cpu", n_init=2, init="random", random_state=0).fit(X)
    rows = np.random.RandomState(0).permutation(X.shape[0])[:K_PLANTED]
    b = KMeans(K_PLANTED, device="cpu", n_init=1, init=X.toarray()[rows]).fit(X)
    assert a.inertia_ <= b.inertia_
    c = KMeans(K_PLANTED, device="cpu", n_init=1, init=lambda X_, k, random_state: init).fit(X)
    assert np.array_equal(c.labels_, KMeans(K_PLANTED, device="cpu", n_init=1, init=init).fit(X).labels_)


@pytest.mark.parametrize("cls", [KMeans, QMeans])
def test_pickle_round_trip(planted, cls):
    X, init = planted
    kw = dict(delta=0.5, true_distance_estimate=False, max_iter=3, random_state=0) if cls is QMeans else {}
    est = cls(K_PLANTED, device="cpu", n_init=1, init=init, **kw).fit(X)
    back = pickle.loads(pickle.dumps(est))
    assert np.array_equal(back.cluster_centers_, est.cluster_centers_)
    assert np.array_equal(back.predict(X), est.predict(X))
