"""``csrc/knn.hip`` (``knn_topk_kernel``) against ``_dense_ref.topk_ref`` and
the dense device estimators against an fp64 brute force.

The selection kernel only moves values, so every comparison with the
reference is exact, on distances and indices.  The estimator-level bound is
derived: the device forms D = qn + xn - 2 q.x in fp32, so for any summation
order |D_gpu - D_ref| <= 2 gamma_{d+3} (qn + xn) with u = 2^-24.
"""
import numpy as np
import pytest
import torch

import _dense_ref as R
from sq_learn_amd._config import config_context
from sq_learn_amd.models.neighbors import KNeighborsClassifier, NearestNeighbors
from sq_learn_amd.models.neighbors import knn as knn_mod
from sq_learn_amd.models.neighbors.knn import _topk_rows
from sq_learn_amd.ops import _native as nat

pytestmark = pytest.mark.gpu

CANARY_D = -12345.0
CANARY_I = -987654321


def _launch(Dg, nref, kk, col_offset=0, m=None):
    """knn_topk on the first ``nref`` columns of the device tile ``Dg`` (row
    stride = its own), outputs with two canary rows behind them."""
    m = Dg.shape[0] if m is None else m
    rows = max(m, 0) + 2
    od = torch.full((rows, max(kk, 1)), CANARY_D, dtype=torch.float32, device=Dg.device)
    oi = torch.full((rows, max(kk, 1)), CANARY_I, dtype=torch.int64, device=Dg.device)
    nat.native().knn_topk(Dg.data_ptr(), od.data_ptr(), oi.data_ptr(), m, nref, Dg.stride(0), kk,
                          int(col_offset), nat.stream_handle(Dg.device))
    torch.cuda.synchronize()
    return od.cpu().numpy(), oi.cpu().numpy()


def _check(cuda, D, kk, col_offset=0, pad=0):
    m, nref = D.shape
    full = np.full((m, nref + pad), -1.0, dtype=np.float32)     # padding below every real entry
    full[:, :nref] = D
    od, oi = _launch(torch.from_numpy(full).to(cuda), nref, kk, col_offset)
    rd, ri = R.topk_ref(D, kk, col_offset)
    np.testing.assert_array_equal(od[:m], rd)
    np.testing.assert_array_equal(oi[:m], ri)
    assert np.all(od[m:] == CANARY_D) and np.all(oi[m:] == CANARY_I)


@pytest.mark.parametrize("nref", [1, 63, 64, 65, 200, 2100])
@pytest.mark.parametrize("m", [1, 5, 9])
def test_topk_patterns(cuda, m, nref):
    for pattern in R.TOPK_PATTERNS:
        D = R.topk_pattern(pattern, m, nref, seed=m + nref)
        for kk in (1, 5, 31, 32):
            _check(cuda, D, kk)
    # through the estimators' entry point (contiguous tile, offset 0)
    D = R.topk_pattern("ties", m, nref, seed=1)
    gd, gi = _topk_rows(torch.from_numpy(D).to(cuda), 5)
    rd, ri = R.topk_ref(D, 5)
    np.testing.assert_array_equal(gd.cpu().numpy(), rd)
    np.testing.assert_array_equal(gi.cpu().numpy(), ri)


def test_topk_one_lane_supplies_every_round(cuda):
    D = R.topk_pattern("lane7", 5, 2100)
    _, ri = R.topk_ref(D, 32)
    assert np.all(ri % 64 == 7)          # the case is what it claims to be
    _check(cuda, D, 32)


def test_topk_more_than_available(cuda):
    _check(cuda, R.topk_pattern("random", 5, 3), 5)
    _check(cuda, R.topk_pattern("ties", 9, 3), 32)


def test_topk_inf_and_nan(cuda):
    rng = np.random.RandomState(0)
    for nref in (65, 200):
        D = rng.standard_normal((9, nref)).astype(np.float32)
        D[:, rng.permutation(nref)[:nref - 3]] = np.inf     # 3 finite entries per row
        D[1, :] = np.inf
        for kk in (1, 5, 32):
            _check(cuda, D, kk)
        rd, ri = R.topk_ref(D, 5)
        assert np.all(np.isfinite(rd[0, :3])) and np.all(np.isinf(rd[0, 3:])) and np.all(ri >= 0)
        E = rng.standard_normal((9, nref)).astype(np.float32)
        E[rng.random_sample(E.shape) < 0.5] = np.nan
        E[2, :] = np.nan                                     # no candidate at all
        E[3, 4:] = np.nan                                    # fewer candidates than kk
        E[4, ::2] = np.inf
        for kk in (1, 5, 32):
            _check(cuda, E, kk)
        rd, ri = R.topk_ref(E, 5)
        assert np.all(ri[2] == -1) and np.all(ri[3, 4:] == -1) and not np.isnan(rd).any()


@pytest.mark.parametrize("col_offset", [0, 7, 2 ** 31 + 5])
def test_topk_row_stride_and_offset(cuda, col_offset):
    rng = np.random.RandomState(1)
    for m, nref, pad in [(5, 63, 1), (9, 200, 56), (5, 2100, 4)]:
        D = np.abs(rng.standard_normal((m, nref))).astype(np.float32)
        for kk in (1, 32):
            _check(cuda, D, kk, col_offset=col_offset, pad=pad)
    # padded rows keep (inf, -1) whatever the offset
    E = np.abs(rng.standard_normal((5, 3))).astype(np.float32)
    _check(cuda, E, 5, col_offset=col_offset, pad=5)


def test_topk_launcher_limits(cuda):
    Dg = torch.from_numpy(R.topk_pattern("random", 5, 65)).to(cuda)
    for kk in (0, 33):
        od = torch.full((7, 33), CANARY_D, dtype=torch.float32, device=cuda)
        oi = torch.full((7, 33), CANARY_I, dtype=torch.int64, device=cuda)
        with pytest.raises(RuntimeError):
            nat.native().knn_topk(Dg.data_ptr(), od.data_ptr(), oi.data_ptr(), 5, 65, Dg.stride(0),
                                  kk, 0, nat.stream_handle(cuda))
        torch.cuda.synchronize()
        assert bool((od == CANARY_D).all()) and bool((oi == CANARY_I).all())
    od, oi = _launch(Dg, 65, 5, m=0)
    assert np.all(od == CANARY_D) and np.all(oi == CANARY_I)


# --------------------------------------------------------------- estimators
def _check_neighbours(dist, ind, D, bound, k, exclude_self):
    """dist / ind [mq, k] of a device estimator against the fp64 distances."""
    assert dist.shape == ind.shape == (D.shape[0], k)
    got = dist ** 2                                   # fp64 sqrt of the fp32 D, squared back
    pair_ref = np.take_along_axis(D, ind, 1)
    pair_bound = np.take_along_axis(bound, ind, 1)
    err = np.abs(got - pair_ref)
    print("k-NN max |D_gpu - D_ref| / bound:", float((err / pair_bound).max()))
    assert np.all(err <= pair_bound)                  # each returned pair
    rd, ri, safe = R.knn_ref(D, bound, k, exclude_self=exclude_self)
    # rank by rank: the r-th smallest of values within the bound of theirs
    assert np.all(np.abs(got - rd) <= bound.max(1)[:, None])
    assert np.all(np.diff(dist, axis=1) >= 0)
    assert 1.0 - safe.mean() <= 0.05
    np.testing.assert_array_equal(ind[safe], ri[safe])
    if exclude_self:
        assert not np.any(ind == np.arange(D.shape[0])[:, None])


def _fit(est, k, X):
    if est == "nn":
        return NearestNeighbors(n_neighbors=k, device="cuda").fit(X)
    return KNeighborsClassifier(n_neighbors=k, device="cuda").fit(X, np.arange(300) % 3)


@pytest.mark.parametrize("k", [32, 33])               # native selection / torch.topk fallback
@pytest.mark.parametrize("d", [3, 61])
@pytest.mark.parametrize("est", ["nn", "clf"])
def test_kneighbors_device(cuda, est, d, k):
    X, Q = R.knn_data(d)
    D, bound = R.sqdist_ref(Q, X)
    dist, ind = _fit(est, k, X).kneighbors(Q)
    _check_neighbours(dist, ind, D, bound, k, False)


@pytest.mark.parametrize("k", [1, 31, 32])            # kk = k + 1: 32 native, 33 fallback
@pytest.mark.parametrize("d", [3, 61])
def test_kneighbors_self_query_device(cuda, d, k):
    X, _ = R.knn_data(d)
    D, bound = R.sqdist_ref(X, X)
    dist, ind = _fit("nn", k, X).kneighbors()
    _check_neighbours(dist, ind, D, bound, k, True)


@pytest.mark.parametrize("slab", [None, 8])
@pytest.mark.parametrize("d", [3, 61])
@pytest.mark.parametrize("self_query", [False, True], ids=["query", "self"])
def test_kneighbors_chunking_identical(cuda, monkeypatch, self_query, d, slab):
    """``working_memory=0.01`` (8 query rows at n_fit = 300) against the
    default: the small-tile result meets the same bound, and the two results
    must be identical, distances included.

    The library fp32 GEMM does not give that by itself: measured on an
    MI355X at d = 61, an 8-row product ``q @ X.T`` differs from the same rows
    of the 40-row (300-row) product in 81 % of its entries (9760 of 12000,
    72954 of 90000) by one fp32 ulp, the BLAS picking another kernel for
    another M, while the row norms are bit-identical.  ``kneighbors``
    therefore forms the products in fixed slabs of ``_gemm_rows(n_fit)``
    query rows and sizes its tiles in whole slabs.  At n_fit = 300 the slab
    (1024 rows) holds every query of this test, so both settings run one
    tile; ``slab = 8`` shrinks the slab so that the 40 queries run as 5 tiles
    against 1 and the self-query as 38 against 1, by the same GEMM calls
    either way."""
    if slab is not None:
        monkeypatch.setattr(knn_mod, "_gemm_rows", lambda n_fit: slab)
    X, Q = R.knn_data(d)
    D, bound = R.sqdist_ref(X if self_query else Q, X)
    cases = [("nn", 1), ("nn", 31), ("nn", 32)] if self_query else \
        [("nn", 32), ("nn", 33), ("clf", 32), ("clf", 33)]
    for est, k in cases:
        model = _fit(est, k, X)
        args = () if self_query else (Q,)
        dist, ind = model.kneighbors(*args)
        with config_context(working_memory=0.01):
            dist_c, ind_c = model.kneighbors(*args)
        _check_neighbours(dist_c, ind_c, D, bound, k, self_query)
        np.testing.assert_array_equal(ind_c, ind)
        np.testing.assert_array_equal(dist_c, dist)
