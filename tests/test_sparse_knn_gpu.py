"""The inverted-index k-NN kernels (``csrc/spknn.hip``) against the fp64
torch twin, and the neighbour estimators on CSR input on the GPU.

One structure (``_sparse_knn_data.structured``): 700 fit rows, 500 columns,
70 queries, ``tile = 256`` - three tiles, the last holding 188 rows.  Query
rows 0..5 hold 0, 1, 63, 64, 65 and 300 nonzeros (both sides of the 64-wide
load), row 6 starts with an explicitly stored zero, row 7 uses the last
column, row 8 is a copy of fit row 5.  On the fit side column 11 has an entry in every non-empty row,
column 498 is empty, rows 40 and 650 are empty, rows 5, 6 and 300 are
identical (a tie inside a tile and one across tiles).  Two value sets:

* exact: integers in [-8, 8].  Every product is an integer and every
  exponent is negative, so the fixed-point sums, the norms and the squared
  distances are exact: the GPU matches the twin bit for bit, every tie
  included.  Cosine: same indices, distances within ``8 * 2^-53`` (four
  correctly rounded operations on values in [0, 2]).
* random: fp32-rounded normals.  Per pair ``|D_gpu - D_twin|`` is bounded by
  ``2 nnz_i 2^(e_i - 1)`` (fixed-point rounding) ``+ 2 (nnz_i + 2) 2^-53
  sum |q||x|`` (the twin's dot) ``+ (2 nnz + 6) 2^-53 (qn + xn)`` (the norms
  of both implementations, nnz the longer of the two rows, and three fp64
  operations each).  Indices must agree wherever the twin's gaps to both
  neighbours in the order exceed twice the bound; the gap between neighbour
  kk and kk + 1 does so for every query row.
"""

import numpy as np
import pytest
import torch

from _sparse_knn_data import (D, EMPTY_COL, EMPTY_FIT_ROWS, FULL_COL, M, N_FIT, Q_FORCED,
                              Q_LAST_COL_ROW, Q_TWIN_ROW, Q_ZERO_ROW, TILE, TWIN_ROWS, U, sq_norms,
                              structured)
from sq_learn_amd.models._data import as_sparse_data
from sq_learn_amd.models.neighbors import KNeighborsClassifier, NearestNeighbors
from sq_learn_amd.ops import _native as nat
from sq_learn_amd.ops import kmeans as K
from sq_learn_amd.ops import sparse_knn as SK

pytestmark = pytest.mark.gpu

KKS = [1, 5, 32]
TILES = [TILE, None]


class Case:
    """One value set on both devices; twin results computed once per (kk, metric)."""

    def __init__(self, kind, dev):
        self.X, self.Q = structured(kind)
        self.fit_cpu, self.qry_cpu = as_sparse_data(self.X, "cpu"), as_sparse_data(self.Q, "cpu")
        self.fit, self.qry = as_sparse_data(self.X, dev), as_sparse_data(self.Q, dev)
        self._twin = {}

    def twin(self, kk, metric):
        if (kk, metric) not in self._twin:
            self._twin[(kk, metric)] = SK.sp_knn_torch(self.fit_cpu, self.qry_cpu, kk, metric)
        return self._twin[(kk, metric)]

    def bounds(self, metric):
        """[m, n] bound on |D_gpu - D_twin| (module docstring)."""
        X, Q = self.X, self.Q
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
        # cosine, 1 - dot / (sqrt(qn) sqrt(xn)): the dot error over the
        # denominator, the relative error of the denominator (each norm
        # nnz * 2^-53 per implementation, halved by the root, plus two roots
        # and a product: 3 roundings each) times |dot| / den <= 1, and the
        # division and subtraction of both implementations (values <= 2)
        den = np.sqrt(qn)[:, None] * np.sqrt(xn)[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            b = e_dot / den + (nq[:, None] + nx[None, :] + 6) * U + 8 * U
        return np.where(den > 0, b, 0.0)


@pytest.fixture(scope="module")
def cases(cuda):
    store = {}

    def get(kind):
        if kind not in store:
            store[kind] = Case(kind, cuda)
        return store[kind]
    return get


def test_fixture_structure(cases):
    c = cases("exact")
    X, Q = c.X, c.Q
    assert X.shape == (N_FIT, D) and Q.shape == (M, D) and -(-N_FIT // TILE) == 3
    assert N_FIT - 2 * TILE == 188
    nq, nx = np.diff(Q.indptr), np.diff(X.indptr)
    assert nq[:len(Q_FORCED)].tolist() == Q_FORCED
    assert Q.data[Q.indptr[Q_ZERO_ROW]] == 0.0
    assert Q.indices[Q.indptr[Q_LAST_COL_ROW + 1] - 1] == D - 1
    assert [i for i in range(N_FIT) if nx[i] == 0] == list(EMPTY_FIT_ROWS)
    colcnt = np.diff(X.tocsc().indptr)
    assert colcnt[FULL_COL] == N_FIT - 2 and colcnt[EMPTY_COL] == 0
    assert (Q[2:, FULL_COL].toarray() != 0).sum() >= M - 3
    for r in TWIN_ROWS[1:]:
        assert (X[r] != X[TWIN_ROWS[0]]).nnz == 0
    assert np.abs(X.data).max() <= 8 and (X.data == np.round(X.data)).all()
    assert (Q.data == np.round(Q.data)).all()
    assert c.fit.data.dtype == torch.float32 and c.fit_cpu.data.dtype == torch.float64
    assert SK.TILE_DEFAULT > N_FIT and nat.native().sp_knn_tile_max() == SK.TILE_MAX
    tab = SK.tile_table(c.fit, TILE)
    assert tab.numel() == D * 3 + 1 and int(tab[-1]) == X.nnz
    # the full column per tile: every row but the empty ones (40 and 650)
    cnt = (tab[FULL_COL * 3 + 1:FULL_COL * 3 + 4] - tab[FULL_COL * 3:FULL_COL * 3 + 3]).tolist()
    assert cnt == [TILE - 1, TILE, 188 - 1]
    # query row 8 equals the identical fit rows: a three-way tie at distance 0
    assert (Q[Q_TWIN_ROW] != X[TWIN_ROWS[0]]).nnz == 0
    Dt, it = c.twin(5, "euclidean")
    assert it[Q_TWIN_ROW, :3].tolist() == list(TWIN_ROWS) and (Dt[Q_TWIN_ROW, :3] == 0).all()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kk", KKS + [33])
def test_exact_euclidean(cases, kk, tile):
    c = cases("exact")
    Dt, it = c.twin(kk, "euclidean")
    Dg, ig = SK.sp_knn(c.fit, c.qry, kk, tile=tile)
    assert Dg.dtype == torch.float64 and ig.dtype == torch.int64 and Dg.shape == (M, kk)
    assert torch.equal(ig.cpu(), it)
    assert torch.equal(Dg.cpu(), Dt)
    # the three-way tie of query row 8 goes by fit index, in and across tiles
    assert ig[Q_TWIN_ROW, :min(kk, 3)].tolist() == list(TWIN_ROWS)[:kk]


@pytest.mark.parametrize("kk", [5, 33])
def test_exact_query_chunks(cases, kk):
    c = cases("exact")
    Dt, it = c.twin(kk, "euclidean")
    Dg, ig = SK.sp_knn(c.fit, c.qry, kk, tile=TILE, rows=32)      # 3 launches
    assert torch.equal(ig.cpu(), it) and torch.equal(Dg.cpu(), Dt)
    Dg, ig = SK.sp_knn(c.fit, c.qry, kk, tile=TILE, rows=1)
    assert torch.equal(ig.cpu(), it) and torch.equal(Dg.cpu(), Dt)
    # tiles of 16 rows hold fewer than kk candidates: padded partials
    Dg, ig = SK.sp_knn(c.fit, c.qry, kk, tile=16)
    assert torch.equal(ig.cpu(), it) and torch.equal(Dg.cpu(), Dt)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kk", KKS + [33])
def test_exact_cosine(cases, kk, tile):
    c = cases("exact")
    Dt, it = c.twin(kk, "cosine")
    Dg, ig = SK.sp_knn(c.fit, c.qry, kk, metric="cosine", tile=tile)
    assert torch.equal(ig.cpu(), it)
    err = (Dg.cpu() - Dt).abs()
    assert float(err.max()) <= 8 * U, float(err.max())
    assert (Dg[0] == 1.0).all() and ig[0].tolist() == list(range(kk))   # the empty query


def test_self_query_exact(cases):
    c = cases("exact")
    Dt, it = SK.sp_knn_torch(c.fit_cpu, c.fit_cpu, 6)
    Dg, ig = SK.sp_knn(c.fit, c.fit, 6, tile=TILE)
    assert torch.equal(ig.cpu(), it) and torch.equal(Dg.cpu(), Dt)
    assert ig[TWIN_ROWS[2], :3].tolist() == list(TWIN_ROWS) and (Dg[TWIN_ROWS[2], :3] == 0).all()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("metric,kk", [("euclidean", 10), ("euclidean", 32), ("cosine", 4),
                                       ("cosine", 10)])
def test_random_within_bound(cases, kk, tile, metric):
    """The kk are those at which no query row of the seeded data has an exact
    tie across the kk / kk + 1 boundary (the empty fit rows tie with each
    other, the copies of one row too, and under cosine every fit row that
    shares no column with the query sits at exactly 1)."""
    c = cases("random")
    bound = c.bounds(metric)
    Dt, it = c.twin(kk + 1, metric)
    Dt, it = Dt.numpy(), it.numpy()
    Dg, ig = SK.sp_knn(c.fit, c.qry, kk, metric=metric, tile=tile)
    assert torch.isfinite(Dg).all()
    Dg, ig = Dg.cpu().numpy(), ig.cpu().numpy()
    # the bound at the twin's neighbours; the largest of a row decides its order
    b = np.take_along_axis(bound, it, axis=1)
    rowb = b.max(1, keepdims=True)
    gaps = np.diff(Dt, axis=1)                            # [m, kk]
    # kk vs kk + 1 is decided for every query row (but the empty query under
    # cosine: every distance is exactly 1 on both sides, the bound is 0)
    live = np.ones(M, dtype=bool)
    if metric == "cosine":
        live[0] = False
        assert (Dg[0] == 1.0).all() and ig[0].tolist() == list(range(kk))
    assert (gaps[live, kk - 1] > 2 * rowb[live, 0]).all()
    np.testing.assert_array_equal(np.sort(ig[live], 1), np.sort(it[live, :kk], 1))
    before = np.concatenate([np.full((M, 1), np.inf), gaps[:, :kk - 1]], 1)
    decided = (before > 2 * rowb) & (gaps[:, :kk] > 2 * rowb) & live[:, None]
    assert decided.any(1)[live].all()
    assert (ig[decided] == it[:, :kk][decided]).all()
    # exact ties inside one implementation go by index: the copies of one row
    assert ig[Q_TWIN_ROW, :3].tolist() == list(TWIN_ROWS)
    # distances: the GPU's own neighbour at each position against the twin's
    # distance of the same pair
    Dpair = np.take_along_axis(c_full(c, metric), ig, axis=1)
    err = np.abs(Dg - Dpair)
    bb = np.take_along_axis(bound, ig, axis=1)
    assert (err <= bb).all(), float((err - bb).max())


def c_full(c, metric):
    """The twin's full [m, n] distance block (cached on the case)."""
    key = ("full", metric)
    if key not in c._twin:
        Dt, it = SK.sp_knn_torch(c.fit_cpu, c.qry_cpu, N_FIT, metric)
        full = np.empty((M, N_FIT))
        np.put_along_axis(full, it.numpy(), Dt.numpy(), axis=1)
        c._twin[key] = full
    return c._twin[key]


def test_random_dist_mode_within_bound(cases):
    c = cases("random")
    bound = c.bounds("euclidean")
    Dg, ig = SK.sp_knn(c.fit, c.qry, 40, tile=TILE, rows=32)
    Dg, ig = Dg.cpu().numpy(), ig.cpu().numpy()
    assert (np.diff(Dg, axis=1) >= 0).all()
    err = np.abs(Dg - np.take_along_axis(c_full(c, "euclidean"), ig, axis=1))
    assert (err <= np.take_along_axis(bound, ig, axis=1)).all()


def test_runs_are_bit_identical(cases):
    c = cases("random")
    for metric in ("euclidean", "cosine"):
        a = SK.sp_knn(c.fit, c.qry, 7, metric=metric, tile=TILE)
        b = SK.sp_knn(c.fit, c.qry, 7, metric=metric, tile=TILE)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # another launch geometry: same distances, bit for bit
        w = SK.sp_knn(c.fit, c.qry, 7, metric=metric, tile=100, rows=9)
        assert torch.equal(a[0], w[0]) and torch.equal(a[1], w[1])


def test_estimators_on_gpu_match_cpu(cases):
    c = cases("exact")
    y = np.random.RandomState(0).randint(0, 4, size=N_FIT)
    for metric in ("euclidean", "cosine"):
        kw = dict(n_neighbors=5, metric=metric)
        gpu = KNeighborsClassifier(device="cuda", **kw).fit(c.X, y)
        cpu = KNeighborsClassifier(device="cpu", **kw).fit(c.X, y)
        assert gpu._fit_method == "brute" and gpu.effective_metric_ == metric
        dg, ig = gpu.kneighbors(c.Q)
        dc, ic = cpu.kneighbors(c.Q)
        assert isinstance(dg, np.ndarray) and dg.dtype == np.float64 and ig.dtype == np.int64
        np.testing.assert_array_equal(ig, ic)
        # the root of identical squares (euclidean); 8 * 2^-53 for cosine
        np.testing.assert_allclose(dg, dc, rtol=2.0 ** -51, atol=8 * U)
        np.testing.assert_array_equal(gpu.predict(c.Q), cpu.predict(c.Q))
        np.testing.assert_array_equal(gpu.kneighbors(c.Q.toarray())[1], ic)   # dense query
    nn = NearestNeighbors(n_neighbors=3, device="cuda").fit(c.X)
    ref = NearestNeighbors(n_neighbors=3, device="cpu").fit(c.X)
    dg, ig = nn.kneighbors()
    dc, ic = ref.kneighbors()
    assert ig.shape == (N_FIT, 3)
    np.testing.assert_array_equal(ig, ic)
    np.testing.assert_allclose(dg, dc, rtol=2.0 ** -51, atol=0)
    # the identical rows find each other, never themselves
    assert sorted(ig[TWIN_ROWS[0], :2].tolist()) == [TWIN_ROWS[1], TWIN_ROWS[2]]
    import pickle
    back = pickle.loads(pickle.dumps(nn))
    assert back._sp.device.type == "cpu"
    np.testing.assert_array_equal(back.kneighbors(c.Q)[1], nn.kneighbors(c.Q)[1])
