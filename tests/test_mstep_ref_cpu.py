"""The numpy references of the fixed-point M-step (``_mstep_ref.py``) checked
on their own: hand-computed cases, the torch twin on dyadic inputs, the
algebra between the references, and the exactness precondition of every
parameter set of ``test_mstep_kernels_gpu.py``."""
import math

import numpy as np
import pytest
import torch

import _mstep_ref as R
from sq_learn_amd.ops import kmeans as K


# 3 rows, 2 clusters, quantum 2^-2: x / 0.25 = [5, 2.5 (tie -> 2)], [-3.5 (tie
# -> -4), 1.2 -> 1], [100, 100] on an out-of-range label
HAND_X = np.array([[1.25, 0.625], [-0.875, 0.3], [25.0, 25.0]], dtype=np.float32)


def test_quanta_hand():
    q = R.quanta_ref(HAND_X, None, -2)
    assert q.dtype == np.int64
    assert q.tolist() == [[5, 2], [-4, 1], [100, 100]]
    # weights: s = fp32(w) * 4; 1.25 * 2 = 2.5 -> 2 (tie), 0.625 * 2 = 1.25 -> 1
    qw = R.quanta_ref(HAND_X, np.array([0.5, 1.0, 0.25], dtype=np.float32), -2)
    assert qw.tolist() == [[2, 1], [-4, 1], [25, 25]]


def test_reduce_hand():
    lab = np.array([1, 1, 2], dtype=np.int32)          # 2 is out of range for k = 2
    S, N, bound = R.reduce_ref(HAND_X, lab, 2, None, -2, 0)
    assert S.tolist() == [[0, 0], [1, 3]] and N.tolist() == [0, 2] and bound == 9
    S, N, _ = R.reduce_ref(HAND_X, np.array([0, 1, -1], dtype=np.int32), 2, None, -2, 0)
    assert S.tolist() == [[5, 2], [-4, 1]] and N.tolist() == [1, 1]
    w = np.array([0.5, 1.0, 0.25], dtype=np.float32)
    S, N, _ = R.reduce_ref(HAND_X, lab, 2, w, -2, -3)   # counts: rint(w * 8) = 4, 8
    assert S.tolist() == [[0, 0], [-2, 2]] and N.tolist() == [0, 12]


def test_qsum_hand():
    # x^2 / 2^-4: 25, 6.25 -> 6 | 12.25 -> 12, 1.44 (fp32 0.3) -> 1
    Q = R.qsum_ref(HAND_X, np.array([1, 1, 2], dtype=np.int32), 2, -4)
    assert Q.tolist() == [0, 25 + 6 + 12 + 1]
    # ties to even in fp64 at quantum 2: x^2 / 2 = 0.5, 4.5, 12.5, 2 -> 0, 4, 12, 2
    X = np.array([[1.0, 3.0, 5.0, 2.0]], dtype=np.float32)
    assert R.qsum_ref(X, np.array([0]), 1, 1).tolist() == [18]


@pytest.mark.parametrize("weighted", [False, True])
def test_reduce_matches_torch_twin_on_dyadic(weighted):
    """Multiples of 2^xexp and unit weights: no quantum is rounded, so the
    rescaled integer sums are the fp64 index_add sums bit for bit."""
    rng = np.random.RandomState(0)
    n, d, k, xexp = 5000, 12, 7, -8
    X = (rng.randint(-4000, 4001, (n, d)) * 2.0 ** xexp).astype(np.float32)
    lab = R.make_labels("with_invalid", n, k)
    w = np.ones(n, dtype=np.float32) if weighted else None
    S, N, bound = R.reduce_ref(X, lab, k, w, xexp, 0)
    assert bound < R.LIMIT
    rs, rc = K.centroid_sums_torch(torch.from_numpy(X).double(), torch.from_numpy(lab), k,
                                   None if w is None else torch.from_numpy(w))
    assert np.array_equal(S.astype(np.float64) * 2.0 ** xexp, rs.numpy())
    assert np.array_equal(N.astype(np.float64), rc.numpy())


def test_delta_from_zero_and_two_steps():
    n, d, k = 3001, 20, 9
    X = R.make_values("normal", n, d, seed=1)
    xexp = K.fixed_point_exp(float(np.abs(X).max()), n)
    qexp = K.fixed_point_exp(float(np.abs(X).max()) ** 2 * d, n)
    steps = R.delta_label_steps(n, k, seed=1)
    zS, zN, zQ = np.zeros((k, d), np.int64), np.zeros(k, np.int64), np.zeros(k, np.int64)
    prev = np.full(n, -1, dtype=np.int32)
    S, N, Q = R.delta_ref(zS, zN, zQ, X, steps[0], prev, k, xexp, qexp)
    rS, rN, _ = R.reduce_ref(X, steps[0], k, None, xexp, 0)
    assert np.array_equal(S, rS) and np.array_equal(N, rN)
    assert np.array_equal(Q, R.qsum_ref(X, steps[0], k, qexp))
    # successive updates (rows leaving to -1 and coming back included) land
    # on the full reduce at the final labels
    for a, b in zip(steps[:-1], steps[1:]):
        S, N, Q = R.delta_ref(S, N, Q, X, b, a, k, xexp, qexp)
        rS, rN, _ = R.reduce_ref(X, b, k, None, xexp, 0)
        assert np.array_equal(S, rS) and np.array_equal(N, rN)
        assert np.array_equal(Q, R.qsum_ref(X, b, k, qexp))
    assert (steps[3] == -1).any() and ((steps[3] == -1) & (steps[4] >= 0)).any()


def test_cluster_parts_match_direct_sum_on_dyadic():
    """Small dyadic data and centroids: Q, S and the direct sum of squared
    differences are all exact, so the identity holds bit for bit."""
    rng = np.random.RandomState(2)
    n, d, k, xexp, qexp = 400, 10, 5, -6, -12
    X = (rng.randint(-200, 201, (n, d)) * 2.0 ** xexp).astype(np.float32)
    C = (rng.randint(-200, 201, (k, d)) * 2.0 ** -5).astype(np.float32)
    lab = R.make_labels("empty_clusters", n, k)
    S, N, _ = R.reduce_ref(X, lab, k, None, xexp, 0)
    Q = R.qsum_ref(X, lab, k, qexp)
    part, mag = R.cluster_parts_ref(S, N, Q, C, xexp, qexp)
    diff = X.astype(np.float64) - C.astype(np.float64)[lab]
    direct = np.zeros(k)
    np.add.at(direct, lab, (diff * diff).sum(1))
    assert np.array_equal(part, direct)
    assert part[k - 1] == 0.0 and mag[k - 1] == 0.0 and (mag >= np.abs(part)).all()


def test_finalize_hand():
    k, d = 3, 2
    # sums [1, 2], [5, 7], [1, -1]; counts 3, 0 (empty), 2.5 (weighted); inertia
    packed = np.array([1.0, 2.0, 5.0, 7.0, 1.0, -1.0, 3.0, 0.0, 2.5, 9.0])
    old = np.array([[0.5, 0.5], [4.0, -4.0], [0.0, 0.0]], dtype=np.float32)
    for policy in (0, 1):
        C, sh = R.finalize_ref(packed, old, k, d, policy)
        assert C.dtype == np.float32
        assert C[0].tolist() == [np.float32(1.0 / 3.0), np.float32(2.0 / 3.0)]
        assert C[1].tolist() == ([4.0, -4.0] if policy == 0 else [0.0, 0.0])
        assert C[2].tolist() == [np.float32(0.4), np.float32(-0.4)]
        assert sh[1] == (0.0 if policy == 0 else 32.0)
        e0 = float(np.float32(1.0 / 3.0)) - 0.5
        e1 = float(np.float32(2.0 / 3.0)) - 0.5
        assert sh[0] == math.fsum([e0 * e0, e1 * e1])


def test_builders():
    n, k = 1000, 37
    assert (R.make_labels("one_cluster", n, k) == k // 2).all()
    assert np.array_equal(R.make_labels("alternating", n, k), np.arange(n) % k)
    inv = R.make_labels("with_invalid", n, k)
    assert (inv == -1).sum() == 100 and inv.max() < k
    assert (R.make_labels("all_invalid", n, k) == -1).all()
    assert R.make_labels("empty_clusters", n, k).max() < k - 2
    assert np.array_equal(R.make_labels("random", n, k), R.make_labels("random", n, k))
    # halves: the engine's rule lands on the builder's exponent, every entry
    # but [0, 0] is an exact tie
    X = R.make_values("halves", 8193, 20)
    assert K.fixed_point_exp(float(np.abs(X).max()), 8193) == R.HALVES_XEXP
    t = X.astype(np.float64) * 2.0 ** -R.HALVES_XEXP
    t[0, 0] = 0.5
    assert np.array_equal(t - np.floor(t), np.full_like(t, 0.5))
    q = R.quanta_ref(X, None, R.HALVES_XEXP)
    assert (q.ravel()[1:] % 2 == 0).all()
    # the clamps: tiny data reaches the lower one
    T = R.make_values("tiny", 8193, 20)
    assert K.fixed_point_exp(float(np.abs(T).max()), 8193) == -120
    # bf16 rounding: representable, ties to even
    b = R.bf16_round(np.array([1.0, 1.00390625, 1.01171875, 3.0e30], dtype=np.float32))
    assert b[:3].tolist() == [1.0, 1.0, 1.015625]
    assert np.array_equal(R.bf16_round(b), b)
    tb = torch.from_numpy(R.make_values("normal", 64, 8))
    assert np.array_equal(R.bf16_round(tb.numpy()), tb.to(torch.bfloat16).float().numpy())


def _max_abs(vp, n, d, bf16, cache={}):
    key = (vp, n, d, bf16)
    if key not in cache:
        cache[key] = float(np.abs(R.make_values(vp, n, d, bf16=bf16)).max())
    return cache[key]


def test_exactness_precondition_of_the_gpu_cases():
    """sum_i |q_i| < 2^53 for every cluster and feature of every parameter
    set of the GPU file, from the bound n (max|x| max w 2^-xexp + 1/2) that
    holds for any labels; the weighted counts and the squared-norm sums
    likewise.  (The GPU tests assert the per-cluster bound of reduce_ref as
    well; this one needs no device.)"""
    for dt, n, d, k, lp, vp, wk in R.reduce_cases():
        mx = _max_abs(vp, n, d, dt == "bf16")
        w = R.make_weights(wk, n)
        mw = None if w is None else float(w.max())
        xexp = K.fixed_point_exp(mx * (mw if mw is not None else 1.0), n)
        assert n * (mx * (mw or 1.0) * 2.0 ** -xexp + 0.5) < R.LIMIT, (dt, n, d, vp, wk)
        if w is not None:
            wexp = K.fixed_point_exp(mw, n)
            assert n * (mw * 2.0 ** -wexp + 0.5) < R.LIMIT
    for n, d in R.delta_shapes() + [R.DELTA_LONG]:
        mx = _max_abs("normal", n, d, False)
        xexp = K.fixed_point_exp(mx, n)
        qexp = K.fixed_point_exp(mx * mx * d, n)
        # (an update adds rows outside the cluster and subtracts members: a
        # row enters any partial sum at most once, so the same bound holds)
        assert n * (mx * 2.0 ** -xexp + 0.5) < R.LIMIT
        assert n * d * (mx * mx * 2.0 ** -qexp + 0.5) < R.LIMIT


def test_reduce_ref_bound_is_attained_by_one_cluster():
    X = R.make_values("normal", 500, 8)
    xexp = K.fixed_point_exp(float(np.abs(X).max()), 500)
    _, _, bound = R.reduce_ref(X, R.make_labels("one_cluster", 500, 5), 5, None, xexp, 0)
    assert bound == int(np.abs(R.quanta_ref(X, None, xexp)).sum(0).max()) < R.LIMIT
