"""Record what the REFERENCE's own code draws for the reference-pinned CPU
tests, so that the tests need no copy of the reference:

* ``quantum_ref.npz`` / ``quantum_ref_helpers.json`` - samples and helper
  values of ``sklearn/QuantumUtility/Utility.py`` (tests/test_quantum_pinned_cpu.py);
* ``dmeans_cpu_ref.npz`` - label counts, inertias, M-step means and tomography
  noise of ``labels_estimation`` / ``_centers_update`` of
  ``sklearn/cluster/_dmeans.py`` (tests/test_dmeans_pinned_cpu.py).

Only outputs are stored; the reference's functions are loaded from a checkout
of the reference at generation time (tests/_dmeans_ref.py).  Every block below
seeds python's ``random`` / ``np.random`` and calls the reference exactly as
the test it belongs to did when it still sampled the reference side by side.
It also checks that tests/fixtures/dmeans_ref.npz (the GPU tests' fixture) is
still what the reference produces.

    python tests/golden/make_pinned_ref.py --reference /path/to/reference
"""
import argparse
import json
import os
import random
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)

AE_LAW = [(0.3, 0.05), (0.04, 0.04), (0.81, 0.06)]
PE_LAW = [(0.3141, 6), (0.05, 7), (0.77777, 5)]
PE_QUBITS = [(0.01, 0.1), (1e-3, 0.05), (0.2, 0.3)]
CPE_OMEGA = [0.123, 0.5, 0.9]
TOMO_SINGLE = [(24, 3000), (700, 40000)]


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _tomo_errors(est_fn, V, reps):
    return np.array([np.linalg.norm(V - np.asarray(est_fn(i))) for i in range(reps)])


def ipe_pair():
    rs = np.random.RandomState(0)
    x = rs.standard_normal(32)
    y = x + 0.3 * rs.standard_normal(32)
    return x, y


def unit_vector(seed, d):
    rs = np.random.RandomState(seed)
    V = rs.standard_normal(d)
    return V / np.linalg.norm(V)


def helper_matrices():
    rs = np.random.RandomState(30)
    out = []
    for shape in [(40, 7), (9, 31)]:
        A = rs.standard_normal(shape)
        A[A < -1.2] = 0.0
        out.append(A)
    return out


def quantum(U):
    """(arrays, helper values) of tests/test_quantum_pinned_cpu.py."""
    g, h = {}, {}
    for i, (a, eps) in enumerate(AE_LAW):
        _seed(1)
        g[f"ae_law_{i}"] = np.array([U.amplitude_estimation(a, epsilon=eps) for _ in range(3000)])
    _seed(4)
    g["ae_median"] = np.array([U.amplitude_estimation(0.37, epsilon=0.08, gamma=0.1)
                               for _ in range(600)])
    calls = []
    U.median_evaluation(lambda: calls.append(1) or 0.0, gamma=0.1)
    h["median_evaluation_calls"] = len(calls)
    for i, (omega, m) in enumerate(PE_LAW):
        _seed(7)
        g[f"pe_law_{i}"] = np.array([U.phase_estimation(omega, m=m) for _ in range(4000)])
    h["pe_qubits"] = []
    for eps, gamma in PE_QUBITS:
        _, _, m_ref, M_ref = U.phase_estimation(0.4, epsilon=eps, gamma=gamma, nqubit=True)
        h["pe_qubits"].append([int(m_ref), int(M_ref)])
    for i, omega in enumerate(CPE_OMEGA):
        _seed(10)
        g[f"cpe_law_{i}"] = np.array([U.consistent_phase_estimation(omega, 0.05, 0.1)
                                      for _ in range(300)])
    x, y = ipe_pair()
    for name, gamma, n in (("ipe_single", None, 1500), ("ipe_median", 0.1, 300)):
        _seed(13)
        g[name] = np.array([U.ipe(x, y, 0.5, gamma=gamma) for _ in range(n)])
    vec = np.linspace(-1, 1, 4000)
    np.random.seed(17)
    g["gaussian_est_noise"] = U.make_gaussian_est(vec, 0.7) - vec
    A = np.arange(60, dtype=np.float64).reshape(6, 10) / 60
    np.random.seed(20)
    g["matrix_tomography_noise"] = U.tomography(A, 0.5, true_tomography=False) - A
    for i, (d, N) in enumerate(TOMO_SINGLE):
        V = unit_vector(22, d)
        reps = 150 if d < 100 else 60
        g[f"tomo_single_err_{i}"] = _tomo_errors(
            lambda _: U.real_tomography(V, N=N, incremental_measure=False)[N], V, reps)
    V = unit_vector(25, 16)
    ref_n, ref_e = [], []
    for _ in range(60):
        r = U.real_tomography(V, delta=0.3)
        n_last = list(r.keys())[-1]
        ref_n.append(n_last)
        ref_e.append(np.linalg.norm(V - np.asarray(r[n_last])))
    g["tomo_stop_n"], g["tomo_stop_err"] = np.asarray(ref_n, dtype=np.float64), np.asarray(ref_e)
    V = unit_vector(28, 12)
    g["fake_sign_err"] = _tomo_errors(lambda _: U.L2_tomogrphy_fakeSign(V, N=2000), V, 100)
    # exact helper values
    h["best_mu"], h["best_mu_step"] = [], []
    for A in helper_matrices():
        name, val = U.best_mu(A)
        h["best_mu"].append([name, float(val)])
        h["best_mu_step"].append(float(U.best_mu(A, step=0.1)[1]))
    h["amplitude_est_dist"] = [float(U.amplitude_est_dist(w0, w1))
                               for w0, w1 in [(0.1, 0.95), (0.5, 0.5), (0.99, 0.01)]]
    arr = np.array([1, 1, 2, 2, 2, 9, 9, 30], dtype=np.int64)
    h["check_measure"] = [int(v) for v in U.check_measure(arr.copy(), 0)]
    h["check_division"] = [[int(v) for v in U.check_division(v, j)]
                           for v, j in [(10, 3), (7, 7), (100, 6)]]
    h["wrapper_sv"] = [float(U.wrapper_phase_est_arguments(x)) for x in [0.1, 0.7]]
    h["wrapper_distance"] = [float(U.wrapper_phase_est_arguments(x, "distance")) for x in [0.1, 0.7]]
    h["unwrap_sv"] = [float(U.unwrap_phase_est_arguments(x, 0.01)) for x in [0.1, 0.7]]
    np.random.seed(31)
    g["introduce_error_array"] = np.asarray(U.introduce_error_array(np.zeros(3000), 2.0))
    g["introduce_error"] = np.array([U.introduce_error(0.0, 0.3)[0] for _ in range(2000)])
    regs, amps = ["a", "b", "c"], [0.2, 0.5, 0.84]
    _seed(33)
    qs_ref = U.QuantumState(registers=regs, amplitudes=amps)
    h["quantum_state"] = {str(k): float(v) for k, v in qs_ref.get_state().items()}
    g["quantum_state_measure"] = np.array([regs.index(r) for r in qs_ref.measure(6000)])
    g["coupon_collect"] = np.array([U.coupon_collect(qs_ref) for _ in range(300)], dtype=np.float64)
    return g, h


def dmeans_problem(seed, n, d, k, spread):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((k, d))
    X = C[rng.integers(0, k, n)] + spread * rng.standard_normal((n, d))
    return X, C


def dmeans_labels2():
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 4, 300)
    labels[:4] = np.arange(4)                     # every cluster non-empty
    return labels


IPE_C = np.array([[2.0, 0.0, 0.0, 0.5], [-2.0, 0.0, 0.0, 0.5], [0.0, 2.5, 0.0, -0.5]])
IPE_X = np.array([[0.0, 0.2, 0.1, 0.4], [0.0, -0.3, 0.7, 0.1], [0.04, 0.4, -0.3, 0.2],
                  [-0.15, 0.1, 0.2, -0.1]])


def dmeans(R):
    """Arrays of tests/test_dmeans_pinned_cpu.py."""
    g = {}
    X, C = dmeans_problem(1, 60, 4, 5, 0.9)
    cnt = np.zeros((60, 5))
    inert = []
    for s in range(400):
        _seed(s)
        lab, _, it = R["labels_estimation"](X, C, 1.5, None, False)
        cnt[np.arange(60), np.asarray(lab, dtype=np.int64)] += 1
        inert.append(float(it))
    g["band_counts"], g["band_inertia"] = cnt, np.asarray(inert)
    X, C = dmeans_problem(2, 300, 6, 4, 0.7)
    labels = dmeans_labels2()
    ref = np.asarray(R["_centers_update"](X, labels, 0.0, False, False, True))
    g["mstep_means"] = ref
    noise = []
    for s in range(150):
        _seed(s)
        noise.append((R["_centers_update"](X, labels, 0.8 / 2, True, False, True) - ref).ravel())
    g["mstep_noise"] = np.concatenate(noise)
    cnt = np.zeros((4, 3))
    inert = []
    for s in range(300):
        _seed(s)
        lab, _, it = R["labels_estimation"](IPE_X, IPE_C, 0.5, None, True)
        cnt[np.arange(4), np.asarray(lab, dtype=np.int64)] += 1
        inert.append(float(it))
    g["ipe_counts"], g["ipe_inertia"] = cnt, np.asarray(inert)
    return g


FIXTURE_KEYS = ("cnt1", "inert1", "means2", "cnt3", "inert3")


def fixture_digest(make_dmeans_ref, z):
    """sha256 over the reference outputs stored in tests/fixtures/dmeans_ref.npz."""
    return make_dmeans_ref.digest({key: z[key] for key in FIXTURE_KEYS})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference")
    a = ap.parse_args()
    os.environ["SQ_REFERENCE_ROOT"] = a.reference
    sys.path.insert(0, TESTS)
    sys.path.insert(0, os.path.join(TESTS, "fixtures"))
    import _dmeans_ref
    import make_dmeans_ref
    if not _dmeans_ref.available():
        raise SystemExit("no reference under " + a.reference)
    R, U = _dmeans_ref.load()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g, h = quantum(U)
    np.savez_compressed(os.path.join(HERE, "quantum_ref.npz"), **g)
    with open(os.path.join(HERE, "quantum_ref_helpers.json"), "w") as f:
        json.dump(h, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "dmeans_cpu_ref.npz"), **dmeans(R))
    # the GPU tests' fixture is the reference's output
    _, z = make_dmeans_ref.load()
    got = make_dmeans_ref.generate(R)
    for key in FIXTURE_KEYS:
        np.testing.assert_array_equal(got[key], z[key], err_msg=key)
    # ... and its digest is recorded, so that tests/test_dmeans_pinned_cpu.py
    # can tell that the fixture is still the one verified here
    with open(os.path.join(HERE, "dmeans_fixture.sha256"), "w") as f:
        f.write(fixture_digest(make_dmeans_ref, z) + "\n")
    print("wrote", HERE)


if __name__ == "__main__":
    main()
