"""The fp64 references of ``_dense_ref`` against the project's CPU paths, on
the inputs the GPU tests use: whatever the GPU tests compare a kernel with
is itself checked here, without a GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _dense_ref as R
from sq_learn_amd.models.neighbors.knn import _topk_rows
from sq_learn_amd.models.tree._tree import forest_apply_host
from sq_learn_amd.ops import linalg as L


# ------------------------------------------------------------------- top-k
@pytest.mark.parametrize("pattern", R.TOPK_PATTERNS)
@pytest.mark.parametrize("m,nref", [(1, 1), (5, 63), (9, 65), (5, 200), (9, 2100)])
def test_topk_ref_matches_torch_topk(pattern, m, nref):
    D = R.topk_pattern(pattern, m, nref)
    for kk in (1, 5, 31, 32):
        if kk > nref:
            continue
        rd, ri = R.topk_ref(D, kk, col_offset=11)
        gd, gi = _topk_rows(torch.from_numpy(D), kk, col_offset=11)
        gd, gi = gd.numpy(), gi.numpy()
        np.testing.assert_array_equal(gd, rd)
        # torch.topk breaks ties in no particular order: indices only where
        # the value occurs once in its row
        for r in range(m):
            vals, counts = np.unique(D[r], return_counts=True)
            uniq = np.isin(rd[r], vals[counts == 1])
            np.testing.assert_array_equal(gi[r][uniq], ri[r][uniq])
        # the reference's own order: (value, column) ascending
        for r in range(m):
            key = list(zip(rd[r].tolist(), ri[r].tolist()))
            assert key == sorted(key)


def test_topk_ref_padding_inf_nan():
    D = np.array([[3.0, np.nan, np.inf, 1.0, np.inf],
                  [np.nan, np.nan, np.nan, np.nan, np.nan],
                  [2.0, 2.0, np.nan, 0.5, 2.0]], dtype=np.float32)
    rd, ri = R.topk_ref(D, 5, col_offset=100)
    np.testing.assert_array_equal(ri, [[103, 100, 102, 104, -1], [-1] * 5, [103, 100, 101, 104, -1]])
    np.testing.assert_array_equal(rd[0], np.array([1, 3, np.inf, np.inf, np.inf], dtype=np.float32))
    assert np.all(np.isinf(rd[1]))
    rd, ri = R.topk_ref(np.array([[2.0, 1.0, 3.0]], dtype=np.float32), 5)
    np.testing.assert_array_equal(ri, [[1, 0, 2, -1, -1]])


# --------------------------------------------------------- k-NN estimators
@pytest.mark.parametrize("d", [3, 61])
@pytest.mark.parametrize("self_query", [False, True])
def test_knn_reference_meets_the_index_cap(d, self_query):
    """The committed data leaves at most 5 % of the (query, rank) pairs out
    of the index comparison, by the reference's own gaps."""
    X, Q = R.knn_data(d)
    for k in (1, 31, 32, 33):
        D, bound = R.sqdist_ref(X if self_query else Q, X)
        _, idx, safe = R.knn_ref(D, bound, k, exclude_self=self_query)
        assert 1.0 - safe.mean() <= 0.05
        if self_query:
            assert not np.any(idx == np.arange(X.shape[0])[:, None])


@pytest.mark.parametrize("d", [3, 61])
def test_knn_reference_matches_cpu_estimator(d):
    from sq_learn_amd.models.neighbors import NearestNeighbors
    X, Q = R.knn_data(d)
    D, bound = R.sqdist_ref(Q, X)
    rd, ri, safe = R.knn_ref(D, bound, 32)
    dist, ind = NearestNeighbors(n_neighbors=32, device="cpu").fit(X).kneighbors(Q)
    np.testing.assert_array_equal(ind[safe], ri[safe])
    # the CPU path evaluates the same expansion in fp64
    b64 = bound * (R.gamma(d + 3, R.U64) / R.gamma(d + 3))
    got = dist ** 2
    assert np.all(np.abs(got - np.take_along_axis(D, ind, 1))
                  <= np.take_along_axis(b64, ind, 1) + 4 * R.U64 * got)


# ----------------------------------------------------------------- moments
@pytest.mark.parametrize("n", [1, 7, 8, 9, 255, 257, 600])
def test_col_moments_ref_matches_cpu_path(n):
    rng = np.random.RandomState(n)
    for d in (1, 63, 300):
        Xi = rng.randint(-64, 65, size=(n, d)).astype(np.float32)
        s, ss = L.col_moments_local(torch.from_numpy(Xi))
        rs, rss = R.col_moments_ref(Xi)
        np.testing.assert_array_equal(s.numpy(), rs)
        np.testing.assert_array_equal(ss.numpy(), rss)
        Xr = rng.standard_normal((n, d)).astype(np.float32)
        s, ss = L.col_moments_local(torch.from_numpy(Xr)[:, ::2])
        rs, rss = R.col_moments_ref(Xr[:, ::2])
        a = np.abs(Xr[:, ::2].astype(np.float64))
        assert np.all(np.abs(s.numpy() - rs) <= n * R.U64 * a.sum(0))
        assert np.all(np.abs(ss.numpy() - rss) <= n * R.U64 * (a * a).sum(0))


def test_row_norms_ref_matches_cpu_path():
    rng = np.random.RandomState(0)
    for d in (1, 3, 200, 1027):
        Xi = rng.randint(-16, 17, size=(5, d)).astype(np.float32)
        np.testing.assert_array_equal(L.row_norms_sq(torch.from_numpy(Xi)).numpy(),
                                      R.row_norms_ref(Xi).astype(np.float32))


# ---------------------------------------------------------------------- mu
@pytest.mark.parametrize("d", [5, 9, 40, 129, 513])
@pytest.mark.parametrize("with_mean", [False, True])
def test_mu_ref_matches_cpu_path(d, with_mean):
    for n in (1, 3, 257):
        for rstar in R.mu_rstars(n):
            X, mean = R.mu_data(n, d, rstar, with_mean)
            a = X if mean is None else X - mean
            # the construction the GPU tests rely on
            assert np.all(a * 16 == np.round(a * 16)) and np.abs(X).max() < 8
            zeros = (a == 0).sum(1)
            assert zeros[rstar] == 0 and np.all(np.delete(zeros, rstar) == 1)
            for name, exps in R.MU_EXP_SETS.items():
                rows, _ = R.mu_rowsums_ref(X, exps, mean)
                assert np.all(rows.argmax(1) == rstar), (name, n, d, rstar)
                if n > 1:
                    assert np.all(np.sort(rows, 1)[:, -2] < rows[:, rstar])
                rmax, cols = R.mu_ref(X, exps, mean)
                gm, gc = L.mu_power_sums_local(
                    torch.from_numpy(X), exps, None if mean is None else torch.from_numpy(mean))
                np.testing.assert_allclose(gm.numpy(), rmax, rtol=1e-12)
                np.testing.assert_allclose(gc.numpy(), cols, rtol=1e-12, atol=0)


def test_mu_data_is_exact_in_bf16():
    X, mean = R.mu_data(257, 40, 128, True)
    Xt = torch.from_numpy(X)
    assert torch.equal(Xt.to(torch.bfloat16).double(), Xt)
    assert torch.equal(torch.from_numpy(mean).float().double(), torch.from_numpy(mean))


# ------------------------------------------------------------------ forest
def _as_trees(tab):
    trees = []
    for t, (o, m) in enumerate(zip(tab["offs"], tab["sizes"])):
        sl = slice(int(o), int(o + m))
        trees.append(SimpleNamespace(node_count=int(m), children_left=tab["left"][sl],
                                     children_right=tab["right"][sl], feature=tab["feat"][sl],
                                     threshold=tab["thr"][sl]))
    return trees


@pytest.mark.parametrize("T", [1, 3, 7])
@pytest.mark.parametrize("d", [1, 12])
def test_forest_ref_matches_host_traversal(T, d):
    tab = R.make_forest(R.forest_depths(T), d, 3, seed=T + d)
    for n in (1, 129, 300):
        X = R.forest_rows(n, d, seed=n)
        leaves, sums, _ = R.forest_ref(tab, X)
        np.testing.assert_array_equal(forest_apply_host(_as_trees(tab), X), leaves)
        want = tab["values"][tab["offs"][None, :] + leaves].sum(1)
        np.testing.assert_allclose(sums, want, rtol=1e-13, atol=1e-13)
    # NaN rows without a missing table go right, as the host comparison does
    X = R.forest_rows(129, d, seed=5, nan_frac=0.2)
    np.testing.assert_array_equal(forest_apply_host(_as_trees(tab), X), R.forest_ref(tab, X)[0])


def test_forest_ref_root_leaf_and_cap():
    tab = R.make_forest([0], 4, 2)
    leaves, sums, _ = R.forest_ref(tab, R.forest_rows(5, 4))
    assert np.all(leaves == 0) and np.all(sums == tab["values"][0][None, :])
    bad = R.make_forest([2], 4, 2)
    bad["left"][1] = 0          # a cycle: node 1 points back at the root
    bad["right"][1] = 0
    with pytest.raises(RuntimeError):
        R.forest_ref(bad, np.full((1, 4), -100.0, dtype=np.float32))
