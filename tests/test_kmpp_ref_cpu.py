"""The numpy model of the exact k-means++ (``_kmpp_ref.py``) checked on its
own: a hand-computed run with both kinds of tie, the reference greedy
k-means++ oracle and the CPU path of ``kmeans_plusplus`` on lattice data
(where fixed point and fp64 agree exactly), and the preconditions of every
parameter set of ``test_kmpp_kernels_gpu.py``."""
import numpy as np
import pytest
import torch

import _kmpp_ref as R
import test_kmpp_kernels_gpu as G
from sq_learn_amd.models._data import Data
from sq_learn_amd.models.cluster._init import kmeans_plusplus
from sq_learn_amd.parallel.comm import Comm

# 6 rows, mirror images about the first axis except row 3, which is equally
# far from rows 0 and 1 (and from rows 0 and 4): distances to row 0 are
# 0, 9, 9, 6.25, 25, 25 (sum 74.25), 6 * 25 = 150 -> scale 2^44
HAND_X = np.array([[0, 0, 0, 0], [-3, 0, 0, 0], [3, 0, 0, 0], [-1.5, 2, 0, 0], [-3, 4, 0, 0],
                   [3, 4, 0, 0]], dtype=np.float32)
S44 = 2.0 ** 44


def test_hand_run():
    # step 1: 0.1 * 74.25 = 7.425 -> row 1 (prefix 9), 0.2 * 74.25 = 14.85 -> row 2 (18).
    #   trial 0 (row 1) improves rows 1 (9 -> 0) and 4 (25 -> 16): Delta 18; row 3 is at
    #   6.25 = closest: NO improvement.  Trial 1 (row 2), the mirror image: rows 2 and 5,
    #   Delta 18.  Equal potentials 56.25: the FIRST trial wins.
    # step 2: prefixes 0 0 9 15.25 31.25 56.25; 0.5 -> 28.125 -> row 4, 0.9 -> 50.625 -> row 5.
    #   trial 0 (row 4): row 4 (16 -> 0), row 3 again at exactly 6.25: Delta 16;
    #   trial 1 (row 5): row 5 (25 -> 0): Delta 25 wins.
    out = R.kmpp_ref(HAND_X, 3, 2, 0, [[0.1, 0.2], [0.5, 0.9]], keep_rows=True)
    assert out["scale"] == S44 and out["P0"] == 74.25 * S44
    s1, s2 = out["steps"]
    assert s1["pos"].tolist() == [1, 2]
    assert (s1["delta"] / S44).tolist() == [18.0, 18.0] and s1["best"] == 0
    assert s1["P_after"] == 56.25 * S44
    assert s1["closest"].tolist() == [0, 0, 9, 6.25, 16, 25]
    assert s1["nearest"].tolist() == [0, 1, 0, 0, 1, 0]
    assert s2["vals"].tolist() == [0.5 * 56.25 * S44, 0.9 * 56.25 * S44]
    assert s2["pos"].tolist() == [4, 5]
    assert (s2["delta"] / S44).tolist() == [16.0, 25.0] and s2["best"] == 1
    assert out["ids"].tolist() == [0, 1, 5] and out["P"] == 31.25 * S44
    assert out["closest"].tolist() == [0, 0, 9, 6.25, 16, 0]
    assert out["nearest"].tolist() == [0, 1, 0, 0, 1, 2]
    np.testing.assert_array_equal(out["centres"], HAND_X[[0, 1, 5]])


def test_pieces_hand():
    qv = np.array([0.0, 3, 0, 0, 2, 5, 0])
    assert R.block_totals(qv, 3, 3).tolist() == [3, 7, 0]
    # first row whose inclusive prefix (0 3 3 3 5 10 10) reaches the value; clamped
    pos, ids = R.pick_ref(qv, [0, 3, 3.5, 5, 10, 11], row_offset=2, n_global=8)
    assert pos.tolist() == [0, 1, 4, 4, 5, 6] and ids.tolist() == [2, 3, 6, 6, 7, 7]
    assert R.partition(2048 * 512 + 77) == (513, 2045) and R.partition(70001) == (256, 274)
    assert R.partition(1) == (1, 1) and R.partition(10_000_000) == (4883, 2048)
    cl = np.array([4.0, 5, 6], dtype=np.float32)
    D = np.array([[1, 9, 9], [9, 2, 3]], dtype=np.float32)
    assert R.effective_closest(cl, np.array([1, 2, 2]), D, 1).tolist() == [4, 2, 3]
    assert R.effective_closest(cl, np.array([1, 2, 2]), D, -1).tolist() == [4, 5, 6]
    assert R.q(np.float32(2.5), 1.0, 1.0) == 2.0 and R.q(np.float32(3.5), 0.5, 2.0) == 4.0
    assert R.scale_for(0.0, 10) == 1.0 and R.scale_for(25.0, 6) == S44
    assert R.lattice_limit(4) == 1023 and R.lattice_limit(64) == 255
    assert R.lattice_limit(2112) == 44


def test_quantise_hand():
    X = np.array([[127, -63.5, 0.4, 0], [0, 0, 0, 0]], dtype=np.float32)
    qi, s, e, q2 = R.quantise_rows(X, 64)
    assert qi[0, :4].tolist() == [127, -64, 0, 0] and not qi[:, 4:].any() and not qi[1].any()
    assert s.tolist() == [1.0, 1.0] and q2.tolist() == [127 ** 2 + 64 ** 2, 0]
    assert e[1] == 0.0 and abs(e[0] - np.sqrt(0.25 + np.float64(np.float32(0.4)) ** 2)) < 1e-15
    # s_c = 2: y = (127, -0.25, 50.126): q1 = (127, 0, 50), q2 = rint(254 * (0, -0.25, 0.126))
    C = np.array([[254, -0.5, 100.252, 0]], dtype=np.float32)
    cq, sc, ec, c2 = R.quantise_cands(C, 64)
    assert sc.tolist() == [2.0]
    assert cq[0, 0, :4].tolist() == [127, 0, 50, 0] and cq[1, 0, :4].tolist() == [0, -64, 32, 0]
    assert not cq[:, 1:].any() and not cq[:, :, 4:].any()
    ct = R.cand_tilde(cq, sc, 1)[0, :4]
    assert np.allclose(ct, [254, -128 / 254, 100 + 64 / 254, 0], rtol=1e-15)
    assert abs(ec[0] - np.sqrt(((C[0].astype(np.float64) - ct) ** 2).sum())) < 1e-15
    # the bound is a lower bound of the true distance
    lb = R.bound_lb64(qi, s, e, cq, sc, ec, 1)
    assert (lb[0] <= R.dist2(X.astype(np.float64), C)[0]).all() and lb[0, 0] > 0


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "dyadic"])
@pytest.mark.parametrize("n,d,k,t", [(600, 8, 9, 4), (2500, 20, 17, None)])
def test_lattice_run_equals_oracles(n, d, k, t, weighted):
    """Integer potentials (or multiples of 1 / 8): the fixed-point model, the
    fp64 cumulative sums of the reference algorithm and the CPU path of
    ``kmeans_plusplus`` choose the same rows."""
    X = R.lattice_blobs(n, d, k, R.lattice_limit(d), seed=n)
    w = np.random.RandomState(1).randint(1, 41, n) / 8.0 if weighted else None
    tt = t or 2 + int(np.log(k))
    rs = np.random.RandomState(5)
    fid = int(rs.randint(n))
    ref = R.kmpp_ref(X, k, tt, fid, rs.random_sample((k - 1, tt)), w=w)
    X64 = X.astype(np.float64)
    np.testing.assert_array_equal(ref["ids"], R.kpp_oracle(X64, k, np.random.RandomState(5), t=t,
                                                           w=w))
    data = Data(torch.from_numpy(X64), n, 0, Comm(None), "sharded")
    _, ids = kmeans_plusplus(data, k, np.random.RandomState(5), n_local_trials=t,
                             sample_weight=None if w is None else torch.from_numpy(w))
    np.testing.assert_array_equal(ref["ids"], np.asarray(ids))
    # the potentials agree exactly as well
    D = R.dist2(X64, X64[ref["ids"]]).min(0)
    assert ref["P"] == float((D * (1.0 if w is None else w)).sum()) * ref["scale"]


# ------------------------------------ preconditions of the GPU parameter sets
@pytest.mark.parametrize("name", list(G.E2E_CASES))
def test_e2e_case_preconditions(name):
    n, d, t, k, blobs, wk, dups = G.E2E_CASES[name]
    X, w = G.e2e_data(name)
    L = R.lattice_limit(d)
    assert d * (2 * L) ** 2 < 2 ** 24 and np.abs(X).max() <= L
    assert np.array_equal(X, np.rint(X)) and X.shape == (n, d) and X.dtype == np.float32
    assert 1 <= t <= 16 and (6 <= k <= 12 or n == 1) and d % 4 == 0
    ref = G.e2e_ref(name)
    assert n * ref["max_pot"] * ref["scale"] <= R.LIMIT
    assert ref["P0"] < 2.0 ** 53
    if n > k:
        assert len(set(ref["ids"].tolist())) == k and ref["P"] > 0
    if name in G.SCREEN_CASES:
        assert ref["steps"][-1]["tri_frac"] >= 0.5, ref["steps"][-1]["tri_frac"]
    if dups:
        Rb, _ = R.partition(n)
        assert (G.DUP_ROWS[0] % Rb, G.DUP_ROWS[1] % Rb) == (0, 0)
        assert (ref["closest"][G.DUP_ROWS[0]:G.DUP_ROWS[1]] == 0).all()    # whole zero blocks
    if wk == "dyadic":
        assert np.array_equal(w * 8, np.rint(w * 8))


def test_e2e_shapes_reach_their_paths():
    part = {nm: R.partition(c[0]) for nm, c in G.E2E_CASES.items()}
    assert part["G274"] == (256, 274) and part["R257"][0] == 257 and part["R513"][0] == 513
    assert -(-513 // 256) == 3 and -(-513 // 64) > 2 * 4        # rchunk; batches per wave
    assert {R.pad64(G.E2E_CASES[nm][1]) for nm in ("d68", "d192", "d256", "d260", "d2112")} == {
        128, 192, 256, 320, 2112}
    assert R.pad64(20) == 64 and 68 % 32 == 4
    from sq_learn_amd.ops import kmeans as K
    assert R.pad64(G.E2E_CASES["d2112"][1]) > K.KMPP_BOUND_MAX_DQ >= 320


@pytest.mark.parametrize("n,d,t,weighted", G.STEP_CASES)
def test_step_case_preconditions(n, d, t, weighted):
    X, w = G.step_data(n, d, weighted)
    Rb, Gb = R.partition(n)
    assert Gb >= 5 and (X[Rb:3 * Rb] == X[0]).all()
    cl = R.dist2(X.astype(np.float64), X[0])[0] * (1.0 if w is None else w)
    ng = n + 3
    assert ng * cl.max() * (1 + R.rel_tol(d)) * R.scale_for(cl.max(), ng) <= R.LIMIT * 1.0001
    assert not np.array_equal(X, np.rint(X))


@pytest.mark.parametrize("d,t", G.BOUND_CASES)
def test_bound_case_band(d, t):
    """At most 5 % of the (row, trial) pairs of the bound test lie in the band
    0.999 closest <= lb <= 1.001 closest the test leaves unconstrained, by
    the reference's own quantisation."""
    X, cand_rows, c0 = G.bound_data(d, t)
    dq = R.pad64(d)
    qi, s, e, _ = R.quantise_rows(X, dq)
    cq, sc, ec, _ = R.quantise_cands(X[cand_rows], dq)
    lb = R.bound_lb64(qi, s, e, cq, sc, ec, t)
    X64 = X.astype(np.float64)
    cl = R.dist2(X64, X64[c0])[0]
    band = (lb >= 0.999 * cl[None, :]) & (lb <= 1.001 * cl[None, :])
    assert band.mean() <= 0.05, band.mean()
    assert (lb <= R.dist2(X64, X[cand_rows])).all()
    # both verdicts occur
    assert (lb > 1.001 * cl[None, :]).all(0).any() and (lb < 0.999 * cl[None, :]).any(0).any()
    assert not X[1].any() and X[2, 3] == 1e4 and (X[4] == X[cand_rows[0]]).all()
    assert (X[5] == X[c0]).all() and cand_rows.max() < G.BOUND_N
