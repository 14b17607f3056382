"""The quantum error model pinned to the REFERENCE's own code.

Samples and helper values of the reference's
``sklearn/QuantumUtility/Utility.py``, recorded by
tests/golden/make_pinned_ref.py (tests/golden/quantum_ref.npz,
quantum_ref_helpers.json: the draws the reference made under the seeds noted
there), are compared with

* the NumPy oracle (:mod:`sq_learn_amd.quantum.reference`),
* the device samplers' CPU twins (:mod:`sq_learn_amd.ops.random`,
  :mod:`sq_learn_amd.quantum.device`; the same Philox streams the HIP kernels
  draw, see ``tests/test_native_random_gpu.py`` for the bit-exact twin checks).

Discrete laws (AE, PE, CPE) are compared by a two-sample chi^2 on pooled
categories, continuous ones (Gaussian tomography noise, IPE, tomography
errors) by a two-sample Kolmogorov-Smirnov test.  The reference drew from
python's ``random`` and ``np.random`` (seeded by the recorder) and, inside
``QuantumState.measure``, from an unseeded ``RandomState`` - thresholds are
p > 1e-4 so a correct law fails about once in 10^4 recordings.
"""
import json
import math
import os

import numpy as np
import pytest
import torch
from scipy import stats

from sq_learn_amd.quantum import reference as Q
from sq_learn_amd.quantum import device as QD
from sq_learn_amd.ops import random as R
from sq_learn_amd.runtime.rng import RngKey

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P_MIN = 1e-4


@pytest.fixture(scope="module")
def U():
    """The reference's recorded draws (arrays) and exact helper values."""
    g = dict(np.load(os.path.join(GOLDEN, "quantum_ref.npz")))
    with open(os.path.join(GOLDEN, "quantum_ref_helpers.json")) as f:
        g.update(json.load(f))
    return g


def _chi2_two_sample(a, b):
    """p-value of 'a and b come from the same discrete law' (pools rare values)."""
    a = np.round(np.asarray(a, dtype=np.float64), 12)
    b = np.round(np.asarray(b, dtype=np.float64), 12)
    vals, inv = np.unique(np.concatenate([a, b]), return_inverse=True)
    ca = np.bincount(inv[: len(a)], minlength=len(vals)).astype(float)
    cb = np.bincount(inv[len(a):], minlength=len(vals)).astype(float)
    tot = ca + cb
    big = tot >= 10
    table = np.stack([ca[big], cb[big]], 0)
    rest = np.array([[ca[~big].sum()], [cb[~big].sum()]])
    if rest.sum() > 0:
        table = np.concatenate([table, rest], 1)
    if table.shape[1] < 2:
        return 1.0
    return stats.chi2_contingency(table)[1]


# --------------------------------------------------------------- Q10 / Q11
AE_LAW = [(0.3, 0.05), (0.04, 0.04), (0.81, 0.06)]


@pytest.mark.parametrize("a,eps", AE_LAW)
def test_amplitude_estimation_law_matches_reference(U, a, eps):
    n = 3000
    ref = U[f"ae_law_{AE_LAW.index((a, eps))}"]
    assert ref.shape == (n,)
    rng = np.random.default_rng(2)
    ours = [Q.amplitude_estimation(a, epsilon=eps, random_state=rng) for _ in range(n)]
    assert _chi2_two_sample(ref, ours) > P_MIN
    # device sampler (CPU twin of ae_batch_kernel: same Philox streams)
    dev = R.amplitude_estimation_batch(torch.full((n,), a, dtype=torch.float64),
                                       torch.full((n,), eps, dtype=torch.float64),
                                       RngKey(3, "ae", 0), Q=1).numpy()
    assert _chi2_two_sample(ref, dev) > P_MIN


def test_amplitude_estimation_median_matches_reference(U):
    n = 600
    a, eps = 0.37, 0.08
    ref = U["ae_median"]
    assert ref.shape == (n,)
    rng = np.random.default_rng(5)
    ours = [Q.amplitude_estimation(a, epsilon=eps, gamma=0.1, random_state=rng) for _ in range(n)]
    assert _chi2_two_sample(ref, ours) > P_MIN
    dev = R.amplitude_estimation_batch(torch.full((n,), a, dtype=torch.float64),
                                       torch.full((n,), eps, dtype=torch.float64),
                                       RngKey(6, "ae", 0), Q=13).numpy()
    assert _chi2_two_sample(ref, dev) > P_MIN


def test_median_evaluation_q_matches_reference(U):
    calls = []
    n_ref = U["median_evaluation_calls"]
    Q.median_evaluation(lambda: calls.append(1) or 0.0, gamma=0.1)
    assert n_ref == len(calls) == 13


# ---------------------------------------------------------------- Q12 / Q13
PE_LAW = [(0.3141, 6), (0.05, 7), (0.77777, 5)]


@pytest.mark.parametrize("omega,m", PE_LAW)
def test_phase_estimation_law_matches_reference(U, omega, m):
    n = 4000
    ref = U[f"pe_law_{PE_LAW.index((omega, m))}"]
    assert ref.shape == (n,)
    rng = np.random.default_rng(8)
    ours = [Q.phase_estimation(omega, m=m, random_state=rng) for _ in range(n)]
    assert _chi2_two_sample(ref, ours) > P_MIN
    dev = R.phase_estimation_batch(torch.full((n,), omega, dtype=torch.float64),
                                   torch.full((n,), m, dtype=torch.int32),
                                   RngKey(9, "pe", 0)).numpy()
    assert _chi2_two_sample(ref, dev) > P_MIN


def test_phase_estimation_epsilon_qubits_match_reference(U):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (eps, gamma) in enumerate([(0.01, 0.1), (1e-3, 0.05), (0.2, 0.3)]):
            m_ref, M_ref = U["pe_qubits"][i]
            _, _, m, M = Q.phase_estimation(0.4, epsilon=eps, gamma=gamma, nqubit=True,
                                            random_state=0)
            assert (m_ref, M_ref) == (m, M)


CPE_OMEGA = [0.123, 0.5, 0.9]


@pytest.mark.parametrize("omega", CPE_OMEGA)
def test_consistent_phase_estimation_law_matches_reference(U, omega):
    eps, gamma = 0.05, 0.1
    n = 300
    ref = U[f"cpe_law_{CPE_OMEGA.index(omega)}"]
    assert ref.shape == (n,)
    rng = np.random.default_rng(11)
    ours = [Q.consistent_phase_estimation(omega, eps, gamma, random_state=rng) for _ in range(n)]
    assert _chi2_two_sample(ref, ours) > P_MIN
    # device path: consistent PE on the PE kernel's law
    dev = QD.consistent_phase_estimation_device(torch.full((n,), omega, dtype=torch.float64),
                                                eps, gamma, RngKey(12, "pe", 0)).numpy()
    assert _chi2_two_sample(ref, dev) > P_MIN
    # consistency: the reference returns (almost) one value; so do we
    assert np.mean(np.isclose(ours, np.median(ref))) > 0.9


# ---------------------------------------------------------------------- Q14
@pytest.mark.parametrize("gamma", [None, 0.1])
def test_ipe_law_matches_reference(U, gamma):
    """gamma=None: one AE draw (the Fejer law's spread); 0.1: the reference
    default, median of 13 (concentrated on one or two values)."""
    rs = np.random.RandomState(0)
    x = rs.standard_normal(32)
    y = x + 0.3 * rs.standard_normal(32)
    eps = 0.5
    n = 1500 if gamma is None else 300
    ref = U["ipe_single" if gamma is None else "ipe_median"]
    assert ref.shape == (n,)
    rng = np.random.default_rng(14)
    ours = np.array([Q.ipe(x, y, eps, gamma=gamma, random_state=rng) for _ in range(n)])
    # a discrete law (S (1 - 2 sin^2(pi j / M)) / 2): chi^2 on values rounded
    # past the last-ulp differences of the two formulas
    r8 = lambda v: np.round(v, 8)  # noqa: E731
    assert _chi2_two_sample(r8(ref), r8(ours)) > P_MIN
    if gamma is None:
        assert len(np.unique(r8(ref))) > 3
    # the device sampler's twin (ae_batch_kernel streams) on the same pair
    S = x @ x + y @ y
    a = torch.full((n,), (S - 2 * (x @ y)) / (2 * S), dtype=torch.float64)
    ea = torch.full((n,), eps * max(1.0, abs(x @ y)) / S, dtype=torch.float64)
    at = R.amplitude_estimation_batch(a, ea, RngKey(16, "ipe", 0), Q=1 if gamma is None else 13).numpy()
    dev = S * (1 - 2 * at) / 2
    assert _chi2_two_sample(r8(ref), r8(dev)) > P_MIN
    if gamma is not None:
        # batched oracle of the fused device kernel
        bat = Q.ipe_batch(np.full(n, x @ y), np.full(n, x @ x), np.full(n, y @ y), eps,
                          gamma=gamma, random_state=np.random.default_rng(15))
        assert _chi2_two_sample(r8(ref), r8(bat)) > P_MIN


# ------------------------------------------------------------------ Q3 / Q4
def test_gaussian_tomography_noise_matches_reference(U):
    vec = np.linspace(-1, 1, 4000)
    noise = 0.7
    ref = U["gaussian_est_noise"]
    assert ref.shape == vec.shape
    ours = Q.make_gaussian_est(vec, noise, random_state=18) - vec
    assert stats.ks_2samp(ref, ours).pvalue > P_MIN
    t = torch.tensor(vec, dtype=torch.float32)
    dev = (QD.gaussian_tomography(t, noise, RngKey(19, "tomography", 0)) - t).double().numpy()
    assert stats.ks_2samp(ref, dev).pvalue > P_MIN
    b = noise / math.sqrt(len(vec))
    assert np.abs(dev).max() <= b * (1 + 1e-6)


def test_matrix_tomography_budget_matches_reference(U):
    A = np.arange(60, dtype=np.float64).reshape(6, 10) / 60
    ref = U["matrix_tomography_noise"]
    assert ref.shape == A.shape
    ours = Q.tomography(A, 0.5, true_tomography=False, random_state=21) - A
    assert stats.ks_2samp(ref.ravel(), ours.ravel()).pvalue > P_MIN
    assert np.abs(ref).max() <= 0.5 / math.sqrt(60) and np.abs(ours).max() <= 0.5 / math.sqrt(60)


def _tomo_errors(est_fn, V, reps):
    return np.array([np.linalg.norm(V - np.asarray(est_fn(i))) for i in range(reps)])


TOMO_SINGLE = [(24, 3000), (700, 40000)]


@pytest.mark.parametrize("d,N", TOMO_SINGLE)
def test_real_tomography_single_pass_matches_reference(U, d, N):
    """One pass with N shots (qPCA's default: incremental_measure=False)."""
    rs = np.random.RandomState(22)
    V = rs.standard_normal(d)
    V /= np.linalg.norm(V)
    reps = 150 if d < 100 else 60
    ref = U[f"tomo_single_err_{TOMO_SINGLE.index((d, N))}"]
    assert ref.shape == (reps,)
    rng = np.random.default_rng(23)
    ours = _tomo_errors(lambda i: Q.real_tomography(V, N=N, incremental_measure=False,
                                                    random_state=rng)[N], V, reps)
    assert stats.ks_2samp(ref, ours).pvalue > P_MIN
    # device code path (long-vector algorithm for d + 1 > 512, Philox twin otherwise)
    dev = _tomo_errors(lambda i: QD.tomography_rows_torch(
        torch.tensor(V)[None], None, RngKey(24, "tomography", i), N=N, incremental_measure=False,
        stop_when_reached_accuracy=False)[0].numpy(), V, reps)
    assert stats.ks_2samp(ref, dev).pvalue > P_MIN
    # sign rule: most signs right once N >> d
    est = np.asarray(Q.real_tomography(V, N=N, incremental_measure=False, random_state=1)[N])
    big = np.abs(V) > 1 / math.sqrt(d)
    assert big.any()
    assert np.mean(np.sign(est[big]) == np.sign(V[big])) > 0.9


def test_real_tomography_stopping_rule_matches_reference(U):
    rs = np.random.RandomState(25)
    d, delta = 16, 0.3
    V = rs.standard_normal(d)
    V /= np.linalg.norm(V)
    reps = 60
    ref_n, ref_e = U["tomo_stop_n"], U["tomo_stop_err"]
    assert ref_n.shape == ref_e.shape == (reps,)
    rng = np.random.default_rng(26)
    our_n, our_e = [], []
    for _ in range(reps):
        r = Q.real_tomography(V, delta=delta, random_state=rng)
        n_last = list(r.keys())[-1]
        our_n.append(n_last)
        our_e.append(np.linalg.norm(V - np.asarray(r[n_last])))
    assert max(ref_e) <= delta and max(our_e) <= delta
    assert stats.ks_2samp(np.log(ref_n), np.log(our_n)).pvalue > P_MIN
    dev_e = [np.linalg.norm(V - QD.tomography_rows_torch(torch.tensor(V)[None], delta,
                                                         RngKey(27, "tomography", i))[0].numpy())
             for i in range(reps)]
    assert max(dev_e) <= delta


def test_fake_sign_tomography_matches_reference(U):
    rs = np.random.RandomState(28)
    V = rs.standard_normal(12)
    V /= np.linalg.norm(V)
    ref = U["fake_sign_err"]
    assert ref.shape == (100,)
    rng = np.random.default_rng(29)
    ours = _tomo_errors(lambda i: Q.L2_tomogrphy_fakeSign(V, N=2000, random_state=rng), V, 100)
    assert stats.ks_2samp(ref, ours).pvalue > P_MIN


# ----------------------------------------------------------------------- Q9
def test_best_mu_and_helpers_equal_reference(U):
    rs = np.random.RandomState(30)
    for i, shape in enumerate([(40, 7), (9, 31)]):
        A = rs.standard_normal(shape)
        A[A < -1.2] = 0.0
        assert tuple(U["best_mu"][i]) == Q.best_mu(A)
        assert U["best_mu_step"][i] == pytest.approx(Q.best_mu(A, step=0.1)[1], rel=1e-12)
    for i, (w0, w1) in enumerate([(0.1, 0.95), (0.5, 0.5), (0.99, 0.01)]):
        assert U["amplitude_est_dist"][i] == pytest.approx(Q.amplitude_est_dist(w0, w1))
    arr = np.array([1, 1, 2, 2, 2, 9, 9, 30], dtype=np.int64)
    np.testing.assert_array_equal(U["check_measure"], Q.check_measure(arr, 0))
    for i, (v, j) in enumerate([(10, 3), (7, 7), (100, 6)]):
        assert U["check_division"][i] == Q.check_division(v, j)
    for i, x in enumerate([0.1, 0.7]):
        assert U["wrapper_sv"][i] == Q.wrapper_phase_est_arguments(x)
        assert U["wrapper_distance"][i] == Q.wrapper_phase_est_arguments(x, "distance")
        assert U["unwrap_sv"][i] == Q.unwrap_phase_est_arguments(x, 0.01)


def test_introduce_error_law_matches_reference(U):
    arr = np.zeros(3000)
    ref = U["introduce_error_array"]
    assert ref.shape == arr.shape
    ours = Q.introduce_error_array(arr, 2.0, random_state=32)
    assert stats.ks_2samp(ref, ours).pvalue > P_MIN
    ref1 = U["introduce_error"]
    assert ref1.shape == (2000,)
    ours1 = np.array([Q.introduce_error(0.0, 0.3, random_state=i)[0] for i in range(2000)])
    assert stats.ks_2samp(ref1, ours1).pvalue > P_MIN


def test_quantum_state_and_coupon_match_reference(U):
    regs, amps = ["a", "b", "c"], [0.2, 0.5, 0.84]
    qs = Q.QuantumState(registers=regs, amplitudes=amps, random_state=34)
    assert U["quantum_state"] == pytest.approx(qs.get_state())
    ref = U["quantum_state_measure"]
    assert ref.shape == (6000,)
    ours = list(qs.measure(6000))
    assert _chi2_two_sample(ref, [regs.index(r) for r in ours]) > P_MIN
    cref = U["coupon_collect"]
    assert cref.shape == (300,)
    cours = [Q.coupon_collect(qs) for _ in range(300)]
    assert stats.ks_2samp(cref, cours).pvalue > P_MIN
