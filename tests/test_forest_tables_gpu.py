"""``csrc/forest.hip`` (``forest_apply``, ``forest_predict<1|4|8|16|32>``) on
node tables built by construction, against the Python walk of
``_dense_ref.forest_ref``.

The kernels loop until they meet a leaf, so no table goes to the device that
the reference has not walked first (``_walked``): the reference caps every
walk at the tree's node count and raises when the cap is hit.

Leaf ids are compared exactly.  A prediction sums T fp64 leaf vectors in
tree order (T - 1 roundings; the scales used here are powers of two, or the
leaf values small integers, so the final product is exact) against a
correctly rounded reference: |got - ref| <= T 2^-53 |scale| sum|v|, and
exactly equal when the leaf values are small integers.
"""
import numpy as np
import pytest
import torch

import _dense_ref as R
from sq_learn_amd.ops.forest import ForestTables, forest_apply

pytestmark = pytest.mark.gpu

S_ALL = [1, 2, 4, 5, 8, 9, 16, 17, 32]       # every template, both sides of each switch


def _walked(tab, X, use_missing=False):
    """The reference walk; only a table it terminates on may be launched."""
    leaves, sums, abs_sums = R.forest_ref(tab, X, use_missing=use_missing)
    assert leaves.shape == (X.shape[0], len(tab["offs"]))
    assert np.all(tab["left"][tab["offs"][None, :] + leaves] == -1)
    return leaves, sums, abs_sums


def _apply(tab, Xg):
    out = forest_apply(Xg, tab["left"], tab["right"], tab["feat"], tab["thr"], tab["offs"])
    assert out.dtype == torch.int32
    return out.cpu().numpy().astype(np.int64)


def _predict(tab, Xg, cuda, scale=1.0, use_missing=False):
    ft = ForestTables(tab["left"], tab["right"], tab["feat"], tab["thr"], tab["offs"],
                      tab["values"], cuda, missing_left=tab["missing"] if use_missing else None)
    out = ft.predict_sum(Xg, scale=scale)
    assert out.dtype == torch.float64 and out.shape == (Xg.shape[0], tab["values"].shape[1])
    return out.cpu().numpy()


@pytest.mark.parametrize("d", [1, 12])
@pytest.mark.parametrize("n", [1, 129, 300])
@pytest.mark.parametrize("T", [1, 3, 7])
def test_forest_tables(cuda, T, n, d):
    X = R.forest_rows(n, d, seed=n + d)
    Xg = torch.from_numpy(X).to(cuda)
    for S in S_ALL:
        tab = R.make_forest(R.forest_depths(T), d, S, seed=S + T)
        leaves, sums, abs_sums = _walked(tab, X)
        if S in (1, 5):
            np.testing.assert_array_equal(_apply(tab, Xg), leaves)
        for scale in (1.0, 0.25):
            got = _predict(tab, Xg, cuda, scale=scale)
            assert np.all(np.abs(got - scale * sums) <= T * R.U64 * scale * abs_sums)
        tab_i = R.make_forest(R.forest_depths(T), d, S, seed=S + T, int_values=True)
        _, sums_i, _ = _walked(tab_i, X)
        np.testing.assert_array_equal(_predict(tab_i, Xg, cuda, scale=3.0), 3.0 * sums_i)


def test_forest_value_width_limit(cuda):
    tab = R.make_forest([1], 4, 33)
    with pytest.raises(ValueError):
        ForestTables(tab["left"], tab["right"], tab["feat"], tab["thr"], tab["offs"],
                     tab["values"], cuda)


@pytest.mark.parametrize("depths", [[0], [4, 0, 4], [0, 0, 3], [3, 0]])
def test_forest_root_leaf(cuda, depths):
    X = R.forest_rows(129, 4, seed=1)
    Xg = torch.from_numpy(X).to(cuda)
    tab = R.make_forest(depths, 4, 5, seed=2, int_values=True)
    leaves, sums, _ = _walked(tab, X)
    for t, dep in enumerate(depths):
        if dep == 0:
            assert np.all(leaves[:, t] == 0)
    np.testing.assert_array_equal(_apply(tab, Xg), leaves)
    np.testing.assert_array_equal(_predict(tab, Xg, cuda), sums)


def _stump(thr, S=2):
    """Root on feature 0 with two leaves; the leaf values name the leaf."""
    val = np.zeros((3, S))
    val[1, 0] = 1.0
    val[2, 1 % S] = 2.0
    return dict(left=np.array([1, -1, -1]), right=np.array([2, -1, -1]),
                feat=np.array([0, -2, -2]), thr=np.array([thr, -2.0, -2.0]), values=val,
                missing=np.zeros(3, dtype=np.uint8))


def test_forest_threshold_equality_is_fp64(cuda):
    x = np.float32(0.1)                       # fp32 value; its fp64 neighbours are not fp32
    x64 = np.float64(x)
    above, below = np.nextafter(x64, np.inf), np.nextafter(x64, -np.inf)
    assert np.float32(above) == x and np.float32(below) == x and below < x64 < above
    tab = R.stack_tables([_stump(t) for t in (x64, above, below, np.inf, -np.inf)])
    X = np.array([[x], [np.nextafter(x, np.float32(1))], [np.nextafter(x, np.float32(-1))],
                  [np.inf], [-np.inf], [3.0e38], [-3.0e38], [0.0]], dtype=np.float32)
    leaves, sums, _ = _walked(tab, X)
    # the reference itself: x == thr goes left; fp64 comparison on both sides of x;
    # thr = +inf takes every row left, thr = -inf only x = -inf
    np.testing.assert_array_equal(leaves[0], [1, 1, 2, 1, 2])
    np.testing.assert_array_equal(leaves[:, 3], np.ones(8))
    np.testing.assert_array_equal(leaves[:, 4], [2, 2, 2, 2, 1, 2, 2, 2])
    Xg = torch.from_numpy(X).to(cuda)
    np.testing.assert_array_equal(_apply(tab, Xg), leaves)
    np.testing.assert_array_equal(_predict(tab, Xg, cuda), sums)


@pytest.mark.parametrize("S", [1, 4, 9])
def test_forest_missing_left(cuda, S):
    d, n = 6, 300
    X = R.forest_rows(n, d, seed=3, nan_frac=0.25)
    nan_rows = np.isnan(X).any(1)
    assert nan_rows.any() and (~nan_rows).any()
    Xg = torch.from_numpy(X).to(cuda)
    base = R.make_forest([4, 0, 3, 2], d, S, seed=S, int_values=True)
    leaves_none, sums_none, _ = _walked(base, X)         # no table: NaN compares false, goes right
    np.testing.assert_array_equal(_apply(base, Xg), leaves_none)
    np.testing.assert_array_equal(_predict(base, Xg, cuda), sums_none)
    results = {}
    for flag in ("zeros", "ones", "random"):
        tab = dict(base)
        if flag != "random":
            tab["missing"] = np.full_like(base["missing"], flag == "ones")
        _, sums, _ = _walked(tab, X, use_missing=True)
        got = _predict(tab, Xg, cuda, use_missing=True)
        np.testing.assert_array_equal(got, sums)
        # rows without a NaN do not see the table
        np.testing.assert_array_equal(got[~nan_rows], sums_none[~nan_rows])
        results[flag] = sums
    np.testing.assert_array_equal(results["zeros"], sums_none)     # all-right = no table
    assert not np.array_equal(results["ones"][nan_rows], results["zeros"][nan_rows])
