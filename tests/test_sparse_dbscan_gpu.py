"""The radius-neighbour kernels (``csrc/spradius.hip``) against the fp64
torch twin, and ``DBSCAN`` on CSR input on the GPU.

Shapes: ``_sparse_knn_data.structured`` - 700 fit rows, 500 columns, 70
queries; with ``tile = 256`` three tiles, the last holding 188 rows (its last
mask word holds 60 rows), with ``tile = 64`` eleven.  Fit rows 40 and 650 are
empty, rows 5, 6 and 300 identical and equal to query row 8, query row 0 is
empty.

* exact (integers in [-8, 8]): fixed-point sums, norms and squared distances
  are exact, so the lists equal the twin's at every threshold, an attained
  distance included (the inclusive test).  Cosine distances differ from the
  twin's by at most ``8 * 2^-53`` (four correctly rounded operations on
  values in [0, 2]) and are exactly 1 on both sides where the inner product
  is zero or a row is empty; no other pair is within that of the thresholds
  used (1e-9, the fp64 number below 1, and 1), which is asserted, so the lists
  are equal there too.
* random (fp32-rounded normals): per pair ``|D_gpu - D_twin|`` is bounded as
  in ``test_sparse_knn_gpu.py`` (fixed-point rounding ``2 nnz_i 2^(e_i - 1)``,
  the twin's dot ``2 (nnz_i + 2) 2^-53 sum |q||x|``, the norms and three fp64
  operations of both implementations ``(2 nnz + 6) 2^-53 (qn + xn)``; cosine:
  over the denominator, plus its relative error and the final operations).
  The threshold sits in the widest gap of the twin's sorted distances between
  their 5% and 6% quantiles; no pair is within its bound of it (asserted), so
  the lists must be equal.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from _sparse_dbscan_data import clustered, decided_threshold, gap_threshold
from _sparse_knn_data import (EMPTY_FIT_ROWS, M, N_FIT, Q_TWIN_ROW, TILE, TWIN_ROWS, U, sq_norms,
                              structured)
from sq_learn_amd.cluster import DBSCAN
from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.ops import kmeans as K
from sq_learn_amd.ops import sparse_knn as SK
from sq_learn_amd.ops import sparse_radius as SR

pytestmark = pytest.mark.gpu

TILES = [64, TILE, None]
ALL = list(range(N_FIT))


def bounds(X, Q, metric):
    """[m, n] bound on |D_gpu - D_twin| (module docstring)."""
    nq, nx = np.diff(Q.indptr), np.diff(X.indptr)
    mx = float(abs(X).max())
    e = np.array([K.fixed_point_exp(float(abs(Q[i]).max()) * mx if nq[i] else 0.0, nq[i])
                  for i in range(Q.shape[0])], dtype=np.float64)
    absdot = (abs(Q) @ abs(X).T).toarray()
    qn, xn = sq_norms(Q), sq_norms(X)
    e_dot = nq[:, None] * 2.0 ** (e[:, None] - 1) + (nq[:, None] + 2) * U * absdot
    if metric == "euclidean":
        nnz = np.maximum(nq[:, None], nx[None, :])
        return 2.0 * e_dot + (2 * nnz + 6) * U * (qn[:, None] + xn[None, :])
    den = np.sqrt(qn)[:, None] * np.sqrt(xn)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        b = e_dot / den + (nq[:, None] + nx[None, :] + 6) * U + 8 * U
    return np.where(den > 0, b, 0.0)


class Case:
    """One value set on both devices; twin distances and lists computed once."""

    def __init__(self, kind, dev):
        self.X, self.Q = structured(kind)
        self.fit_cpu, self.qry_cpu = as_sparse_data(self.X, "cpu"), as_sparse_data(self.Q, "cpu")
        self.fit, self.qry = as_sparse_data(self.X, dev), as_sparse_data(self.Q, dev)
        self._store = {}

    def distances(self, metric):
        """The twin's [m, n] distance block."""
        if metric not in self._store:
            f, q = self.fit_cpu, self.qry_cpu
            dot = q.dense_rows(0, M) @ f.dense_rows(0, N_FIT).T
            D = SK._distances(dot, SR.sp_row_norms_torch(q), SR.sp_row_norms_torch(f),
                              SK.METRICS[metric])
            self._store[metric] = D.numpy()
        return self._store[metric]

    def twin(self, thr, metric, self_join=False):
        key = (thr, metric, self_join)
        if key not in self._store:
            q = self.fit_cpu if self_join else self.qry_cpu
            self._store[key] = SR.sp_radius_torch(self.fit_cpu, q, thr, metric,
                                                  include_self=self_join)
        return self._store[key]


@pytest.fixture(scope="module")
def cases(cuda):
    store = {}

    def get(kind):
        if kind not in store:
            store[kind] = Case(kind, cuda)
        return store[kind]
    return get


def _lists(res):
    indptr, indices = res
    return [indices[indptr[i]:indptr[i + 1]].tolist() for i in range(len(indptr) - 1)]


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def _median_attained(c):
    D = c.distances("euclidean")
    thr = float(np.sort(D.ravel())[D.size // 2])
    assert (D == thr).sum() >= 50                           # the inclusive test is pinned
    return thr


@pytest.mark.parametrize("tile", TILES)
def test_exact_euclidean(cases, tile):
    c = cases("exact")
    assert SR.TILE_DEFAULT > N_FIT
    mid = _median_attained(c)
    got = SR.sp_radius(c.fit, c.qry, mid, tile=tile)
    _same(got, c.twin(mid, "euclidean"))
    D = c.distances("euclidean")
    assert np.diff(got[0]).tolist() == (D <= mid).sum(1).tolist()
    # thr = 0: the identical rows, in one tile and across tiles; the empty
    # query finds the empty fit rows
    got = SR.sp_radius(c.fit, c.qry, 0.0, tile=tile)
    _same(got, c.twin(0.0, "euclidean"))
    lists = _lists(got)
    assert lists[Q_TWIN_ROW] == list(TWIN_ROWS) and lists[0] == list(EMPTY_FIT_ROWS)
    # every pair: prefixes across all the words and tiles
    got = SR.sp_radius(c.fit, c.qry, 1e30, tile=tile)
    assert got[0].tolist() == [N_FIT * i for i in range(M + 1)]
    assert (got[1].reshape(M, N_FIT) == np.arange(N_FIT)).all()
    got = SR.sp_radius(c.fit, c.qry, float("inf"), tile=tile)
    assert (got[1].reshape(M, N_FIT) == np.arange(N_FIT)).all()
    # nothing: the fill launch is skipped
    got = SR.sp_radius(c.fit, c.qry, -1.0, tile=tile)
    assert got[0].tolist() == [0] * (M + 1) and got[1].shape == (0,)


@pytest.mark.parametrize("rows", [1, 32, None])
def test_exact_query_chunks(cases, rows):
    c = cases("exact")
    mid = _median_attained(c)
    for thr in (mid, 0.0, 1e30):
        _same(SR.sp_radius(c.fit, c.qry, thr, tile=TILE, rows=rows), c.twin(thr, "euclidean"))
    _same(SR.sp_radius(c.fit, c.fit, mid, include_self=True, tile=TILE, rows=rows),
          c.twin(mid, "euclidean", True))


@pytest.mark.parametrize("tile", TILES)
def test_exact_self_join(cases, tile):
    c = cases("exact")
    for metric, thr in (("euclidean", 0.0), ("cosine", 1e-9)):
        got = SR.sp_radius(c.fit, c.fit, thr, metric, include_self=True, tile=tile)
        _same(got, c.twin(thr, metric, True))
        lists = _lists(got)
        for i, row in enumerate(lists):
            assert i in row
        for r in TWIN_ROWS:
            assert lists[r] == list(TWIN_ROWS)
        # an empty row: at distance 0 from the other empty row, at cosine
        # distance 1 from everything - there only the forced self hit
        for r in EMPTY_FIT_ROWS:
            assert lists[r] == (list(EMPTY_FIT_ROWS) if metric == "euclidean" else [r])
    # without the flag the empty rows have no cosine neighbour at all
    lists = _lists(SR.sp_radius(c.fit, c.fit, 1e-9, "cosine", tile=tile))
    assert [lists[r] for r in EMPTY_FIT_ROWS] == [[], []]
    assert lists[TWIN_ROWS[0]] == list(TWIN_ROWS)


@pytest.mark.parametrize("tile", TILES)
def test_exact_cosine(cases, tile):
    c = cases("exact")
    D = c.distances("cosine")
    one = D == 1.0          # a zero inner product or an empty row: exactly 1 on both sides
    below = float(np.nextafter(1.0, 0.0))
    for thr in (1e-9, below, 1.0):
        assert (np.abs(D - thr)[~one] > 8 * U).all()        # a condition on the data
        _same(SR.sp_radius(c.fit, c.qry, thr, "cosine", tile=tile), c.twin(thr, "cosine"))
    # the empty query row is at distance exactly 1 from every fit row
    assert _lists(SR.sp_radius(c.fit, c.qry, 1.0, "cosine", tile=tile))[0] == ALL
    assert _lists(SR.sp_radius(c.fit, c.qry, 1.5, "cosine", tile=tile))[0] == ALL
    assert _lists(SR.sp_radius(c.fit, c.qry, below, "cosine", tile=tile))[0] == []
    assert _lists(SR.sp_radius(c.fit, c.qry, 1e-9, "cosine", tile=tile))[Q_TWIN_ROW] == \
        list(TWIN_ROWS)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_random_decided_pairs(cases, metric, tile):
    c = cases("random")
    D = c.distances(metric)
    bound = bounds(c.X, c.Q, metric)
    thr = gap_threshold(D, q=0.05)
    assert (np.abs(D - thr) > bound).all()                  # a condition on the data
    want = c.twin(thr, metric)
    assert 0.04 * D.size < len(want[1]) < 0.07 * D.size
    got = SR.sp_radius(c.fit, c.qry, thr, metric, tile=tile)
    _same(got, want)
    # another launch geometry: the same lists
    _same(SR.sp_radius(c.fit, c.qry, thr, metric, tile=128, rows=9), want)


def test_refusals(cases):
    c = cases("exact")
    with pytest.raises(ValueError, match="include_self=True is the self-join"):
        SR.sp_radius(c.fit, c.qry, 1.0, include_self=True)
    for tile in (100, 32, SK.TILE_MAX + 64):
        with pytest.raises(ValueError, match="tile must be a multiple of 64"):
            SR.sp_radius(c.fit, c.qry, 1.0, tile=tile)
    from sq_learn_amd.ops import _native as nat
    lib = nat.native()
    z = torch.zeros(8, dtype=torch.int64, device=c.fit.device)
    p = z.data_ptr()
    for n, T, metric in ((2 ** 31, 8192, 0), (700, 96, 0), (700, 16384, 0), (700, 256, 2)):
        with pytest.raises(RuntimeError, match="invalid"):
            lib.sp_radius_mark(p, p, p, p, p, p, p, p, p, 0, 1, n, 4, T, 0, metric, 1.0, 0, p, p, 0)
    with pytest.raises(RuntimeError, match="invalid"):
        lib.sp_radius_mark(p, p, p, p, p, p, p, p, p, 0, 2 ** 20, 2 ** 30, 4, 64, 0, 0, 1.0, 0, p,
                           p, 0)                            # m * ntiles >= 2^31
    with pytest.raises(RuntimeError, match="invalid"):
        lib.sp_radius_fill(p, p, 1, 700, 96, 5, p, 0)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_dbscan_gpu_matches_cpu(cuda, metric):
    X = clustered()
    thr, dist = decided_threshold(X, metric)
    # the GPU's neighbourhoods are decided too
    assert (np.abs(dist - thr) > bounds(X, X, metric)).all()
    eps = float(np.sqrt(thr)) if metric == "euclidean" else float(thr)
    w = np.random.RandomState(7).randint(0, 5, size=X.shape[0]) / 2.0
    for min_samples, sw in ((5, None), (10, None), (5, w)):
        gpu = DBSCAN(eps=eps, min_samples=min_samples, metric=metric, device="cuda")
        cpu = DBSCAN(eps=eps, min_samples=min_samples, metric=metric, device="cpu")
        gpu.fit(X, sample_weight=sw)
        cpu.fit(X, sample_weight=sw)
        np.testing.assert_array_equal(gpu.labels_, cpu.labels_)
        np.testing.assert_array_equal(gpu.core_sample_indices_, cpu.core_sample_indices_)
        assert sp.issparse(gpu.components_) and gpu.components_.format == "csr"
        assert gpu.components_.shape == cpu.components_.shape
        assert (gpu.components_ != cpu.components_).nnz == 0
    assert cpu.labels_.max() + 1 == 5 and (cpu.labels_ == -1).any()
    np.testing.assert_array_equal(
        DBSCAN(eps=eps, metric=metric, device="cuda").fit_predict(X.tocoo()),
        DBSCAN(eps=eps, metric=metric, device="cpu").fit_predict(X))
