"""The tomography reference (``_tomo_ref.py``) on its own, and the
preconditions of the GPU case matrix of ``test_tomography_kernels_gpu.py``.

* the uniform against exact rational arithmetic, 1.0 included;
* the law of ``binomial_ref`` against scipy's exact pmf (chi^2, 2e5 draws per
  cell, Bonferroni over the cells);
* the cancellation-free acceptance bound against 60-digit arithmetic up to
  n = 2^51, to the budget L_ERR of the module docstring; the lgamma form it
  replaces, measured against the same exact values;
* tree invariants;
* the excusal caps of every GPU case: at most 1 % of single draws and 5 % of
  trees / (row, checkpoint) pairs near a decision boundary.

Measured excusal shares (near draws / draws, near trees / trees):

| case | draws | near draws | trees | near trees |
|---|---|---|---|---|
| binomial grid | 3136 | 0 | 4034 | 0 |
| segment trees, m = 1 .. 2048, levels 0 / 4 / 5 / 9 | 18547 | 0 | 66 | 0 |
| host recursion, m = 2049, 4097, 6149 | 21079 | 0 | 15 | 0 |
| tomography, d = 1 .. 511, both norms | 13104 | 0 | 290 | 0 |
| tomography, d = 13, shots to 1e10, both norms | 808 | 0 | 60 | 0 |

(The budgets are a few ulps of quantities of order one, so a near draw has a
probability of order 1e-13 per decision; the largest share comes from the
round-2 trees at 1e10 shots, about 1e-4 per draw.)
"""
from fractions import Fraction

import numpy as np
import pytest
from scipy import stats

import _qrand_ref as Q
import _tomo_ref as R

DRAWS = 200_000
# (n, p): inversion, both BTRS exits, flip, n = 1, n min(p, 1 - p) around 12
LAW_CELLS = [(1, 0.3), (1, 0.9), (7, 0.5), (23, 0.5), (24, 0.5), (25, 0.5), (25, 0.52),
             (100, 0.1199), (100, 0.12), (100, 0.1201), (100, 0.88), (100, 0.8801),
             (4000, 0.002999), (4000, 0.003), (4000, 0.997), (40, 0.45), (300, 0.2),
             (300, 0.8), (1000, 0.5), (100000, 0.0001199), (100000, 0.00012),
             (1000000, 0.7), (3000000000, 0.2), (2 ** 51, 12.5 * 2.0 ** -51)]


def test_uniform_is_the_correctly_rounded_half_offset():
    ctr = np.array([0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 17, 2 ** 63 + 5], dtype=np.uint64)
    seen_top = False
    for pair in (0, 1):
        u = R.u53(R.KEY_B, ctr, pair)
        for c, ui in zip(ctr.tolist(), u.tolist()):
            w = Q.philox4x32_10((c & Q.MASK32, c >> 32, R.KEY_B[2], R.KEY_B[3]), R.KEY_B[:2])
            i = (w[2 * pair] << 21) ^ (w[2 * pair + 1] >> 11)
            assert ui == float(Fraction(2 * i + 1, 1 << 54))
            seen_top |= i >= 1 << 52
    assert seen_top
    # the rounding itself: odd I >= 2^52 goes up, 2^53 - 1 reaches 1.0
    for i, want in ((2 ** 52, 2.0 ** 52), (2 ** 52 + 1, 2.0 ** 52 + 2), (2 ** 53 - 1, 2.0 ** 53),
                    (2 ** 52 - 1, 2.0 ** 52 - 0.5)):
        assert np.float64(i) + 0.5 == want
    assert (np.float64(2 ** 53 - 1) + 0.5) * R.U == 1.0


def test_binomial_law():
    """chi^2 of 2e5 draws per cell against the exact pmf; cells pooled to an
    expected count of at least 10; family-wise level 1e-3."""
    rows = []
    seen = set()
    for ci, (n, p) in enumerate(LAW_CELLS):
        ctr = np.arange(DRAWS, dtype=np.uint64) + np.uint64(ci << 24)
        res = R.binomial_ref(np.full(DRAWS, float(n)), np.full(DRAWS, p), R.KEY_B, ctr)
        c = res["count"]
        assert np.all((c >= 0) & (c <= n) & (c == np.round(c)))
        seen.update(np.unique(res["branch"]).tolist())
        mu, sd = n * p, np.sqrt(n * p * (1 - p))
        lo, hi = int(max(0, np.floor(mu - 12 * sd - 12))), int(min(n, np.ceil(mu + 12 * sd + 12)))
        ks = np.arange(lo, hi + 1)
        exp = stats.binom.pmf(ks, n, p) * DRAWS
        obs = np.bincount((np.clip(c, lo, hi) - lo).astype(np.int64), minlength=ks.size).astype(float)
        exp[0] += stats.binom.cdf(lo - 1, n, p) * DRAWS
        exp[-1] += stats.binom.sf(hi, n, p) * DRAWS
        # pool from both ends to expected >= 10
        order = np.argsort(np.abs(ks - mu))[::-1]
        go, ge, acc_o, acc_e = [], [], 0.0, 0.0
        for j in order:
            acc_o += obs[j]
            acc_e += exp[j]
            if acc_e >= 10.0:
                go.append(acc_o)
                ge.append(acc_e)
                acc_o = acc_e = 0.0
        go[-1] += acc_o
        ge[-1] += acc_e
        go, ge = np.array(go), np.array(ge)
        chi2 = ((go - ge) ** 2 / ge).sum()
        pv = stats.chi2.sf(chi2, go.size - 1)
        z = (c.mean() - mu) / (sd / np.sqrt(DRAWS))
        rows.append((n, p, go.size, chi2, pv, z))
        print(f"n={n} p={p}: bins {go.size} chi2 {chi2:.1f} p-value {pv:.3g} z(mean) {z:+.2f}")
    assert seen == {R.INVERSION, R.SQUEEZE, R.FULL}
    thr = 1e-3 / len(LAW_CELLS)
    bad = [r for r in rows if r[4] < thr or abs(r[5]) > stats.norm.isf(thr / 2)]
    assert not bad, bad


def _accuracy_points():
    pts = []
    for n in (24.0, 100.0, 4000.0, 1e6, 3e9, 5.8e11, 1e12, 1e14, 2.0 ** 51):
        for pp in (1e-13, 1e-6, 0.003, 0.2, 0.3, 0.4999, 0.5, 12.5 / n):
            if not (n * pp >= 12.0 and pp <= 0.5):
                continue
            m = np.floor((n + 1.0) * pp)
            sd = np.sqrt(n * pp * (1 - pp))
            for zz in (-9.0, -4.0, -1.5, -0.3, 0.0, 0.3, 1.5, 4.0, 9.0):
                k = float(np.clip(np.round(m + zz * sd), 0.0, n))
                pts.append((n, pp, k, m))
            pts.append((n, pp, 0.0, m))
            if n <= 100:
                pts.append((n, pp, n, m))
                pts.append((n, pp, 1.0, m))
                pts.append((n, pp, n - 1.0, m))
    return np.array(pts)


def test_acceptance_bound_against_arbitrary_precision():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    pts = _accuracy_points()
    n, pp, k, m = pts.T
    L, Lerr = R.log_pmf_ratio(n, pp, k, m)
    old = R.btrs_rhs_lgamma(n, pp, k, m)

    def lf(n_, p_, x_):
        n_, p_, x_ = mp.mpf(n_), mp.mpf(p_), mp.mpf(x_)
        return (mp.loggamma(n_ + 1) - mp.loggamma(x_ + 1) - mp.loggamma(n_ - x_ + 1)
                + x_ * mp.log(p_) + (n_ - x_) * mp.log1p(-p_))

    worst = 0.0
    worst_old = {}
    for i in range(len(pts)):
        ex = lf(n[i], pp[i], k[i]) - lf(n[i], pp[i], m[i])
        err = abs(float(mp.mpf(float(L[i])) - ex))
        assert np.isfinite(L[i]) and err <= Lerr[i], (pts[i], float(ex), L[i], err, Lerr[i])
        worst = max(worst, err / Lerr[i])
        if k[i] > 0:
            worst_old[n[i]] = max(worst_old.get(n[i], 0.0), abs(float(mp.mpf(float(old[i])) - ex)))
    print(f"largest error / L_ERR: {worst:.3f} over {len(pts)} points")
    print("lgamma form, largest absolute error by n:", {f"{a:g}": f"{b:.2g}" for a, b in worst_old.items()})
    assert n.max() == 2.0 ** 51
    # the form this reference must not be: it is off by far more than the budget
    assert worst_old[1e12] > 1e-4 and worst_old[2.0 ** 51] > 1e-2


def old_formula_disagreement(n, p=0.2, draws=4000):
    """(full tests, wrong decisions of the lgamma form, of those with a
    reference margin above 1): the decisions ``lv <= rhs`` of the first BTRS
    trial that reaches the full test, over ``draws`` streams."""
    nn = np.full(draws, float(n))
    ref = R.binomial_ref(nn, np.full(draws, p), R.KEY_B, np.arange(draws, dtype=np.uint64), detail=True)
    has = np.isfinite(ref["lv"])
    pp = min(p, 1 - p)
    old = R.btrs_rhs_lgamma(nn[has], pp, ref["k"][has], ref["m"][has])
    wrong = (ref["lv"][has] <= old) != (ref["lv"][has] <= ref["L"][has])
    return int(has.sum()), int(wrong.sum()), int((wrong & (ref["margin"][has] > 1.0)).sum())


def test_lgamma_form_flips_decisions_at_production_shot_counts():
    """The measurement behind the kernel's cancellation-free acceptance
    (docs/PARITY.md): the last full test of each of 4000 draws at p = 0.2."""
    out = {}
    for n in (3e9, 5.8e11, 1e12, 1e14, 2.0 ** 51):
        out[n] = old_formula_disagreement(n)
        print(f"n={n:g}: full tests {out[n][0]}, lgamma form wrong on {out[n][1]}, "
              f"clear of the reference budget {out[n][2]}")
    assert out[3e9][1] == 0
    assert out[1e14][2] > 0 and out[2.0 ** 51][2] > 0


def _check_counts(cnt, N, W=None):
    assert np.all(cnt >= 0) and np.all(cnt == np.round(cnt))
    np.testing.assert_array_equal(cnt.sum(-1), N)
    if W is not None:
        assert np.all(cnt[~(W > 0)] == 0)


def test_tree_invariants():
    for m in R.SEG_M:
        c = R.segment_case(m)
        if m > 1:          # a one-outcome segment takes its total whatever its weight
            _check_counts(c["ref"]["cnt"], c["N"], c["W"][c["wrow"], :m])
        else:
            np.testing.assert_array_equal(c["ref"]["cnt"][:, 0], c["N"])
    for m in R.LONG_M:
        c = R.long_case(m)
        _check_counts(c["ref"]["cnt"], c["N"], c["W"][c["wrow"]])
    for d, big in R.tomo_case_list():
        c = R.tomo_case(d, False, big)
        ref = c["ref"]
        N = np.broadcast_to(c["sched"][None, :], ref["err"].shape).astype(float)
        _check_counts(ref["cnt1"], N, np.broadcast_to((c["V"] ** 2)[:, None, :], ref["cnt1"].shape))
        assert np.all(ref["cnt2"] >= 0) and np.all(ref["cnt2"].sum(-1) <= N)
        assert np.all(np.abs(ref["est"]) == np.sqrt(ref["cnt1"] / N[..., None]))
        # a basis vector is measured exactly at every shot count
        if c["r"] >= 2 and d > 1:
            np.testing.assert_array_equal(ref["est"][1], np.broadcast_to(c["V"][1], ref["est"][1].shape))
    # streams: level, sid and segment each change the draws
    a = R.segment_case(257, 0)["ref"]["cnt"]
    for lv in (4, 5, 9):
        assert not np.array_equal(a, R.segment_case(257, lv)["ref"]["cnt"])


def test_exact_rows_are_exact():
    for d in R.TOMO_D:
        V, exact = R.tomo_rows(d, R.TOMO_R[d], 50 + d)
        for v in V[exact]:
            m = v * 4096.0
            assert np.all(m == np.round(m)) and int((m.astype(np.int64) ** 2).sum()) == 1 << 24
        if d > 3:
            assert (V[0] == 0).any() and (V[0] < 0).any()


def test_mode2_cases_stop_early():
    """Precondition of the mode-2 GPU test: with its stop bound some row of
    every case with more than one checkpoint stops before the last one, and
    no row is excused for an error within the device bound of the stop."""
    for d, big in R.tomo_case_list():
        for ninf in (False, True):
            c = R.tomo_case(d, ninf, big)
            t_stop, _, excused = R.mode2_ref(c["ref"], R.mode2_stop(c), ninf)
            assert not excused.any()
            if len(c["sched"]) > 1 and d > 1:
                assert (t_stop < len(c["sched"]) - 1).any(), (d, t_stop)


def test_excusal_caps():
    """At most 1 % of the single draws and 5 % of the trees of every GPU
    case are near a boundary (the caps are fixed; a case that breaks one gets
    a smaller d or another key)."""
    rows = []
    c = R.binomial_case()
    mg = c["ref"]["margin"]
    drawn = c["ref"]["branch"] != R.TRIVIAL
    rows.append(("binomial grid", int(drawn.sum()), int((drawn & (mg <= 1)).sum()), mg.size,
                 int((mg <= 1).sum())))
    assert {R.TRIVIAL, R.INVERSION, R.SQUEEZE, R.FULL} <= set(np.unique(c["ref"]["branch"]).tolist())
    for m in R.SEG_M:
        for lv in (R.SEG_LEVELS if m == 257 else (0,)):
            r = R.segment_case(m, lv)["ref"]
            rows.append((f"segments m={m} level={lv}", r["draws"], r["near"], r["margin"].size,
                         int((r["margin"] <= 1).sum())))
    for m in R.LONG_M:
        r = R.long_case(m)["ref"]
        rows.append((f"host recursion m={m}", r["draws"], r["near"], r["margin"].size,
                     int((r["margin"] <= 1).sum())))
    for d, big in R.tomo_case_list():
        for ninf in (False, True):
            r = R.tomo_case(d, ninf, big)["ref"]
            rows.append((f"tomography d={d} big={big} inf={ninf}", r["draws"], r["near"],
                         r["margin2"].size, int((r["margin2"] <= 1).sum())))
    for name, draws, near, trees, ntrees in rows:
        print(f"{name}: draws {draws} near {near}; trees {trees} near {ntrees}")
        assert near <= 0.01 * max(draws, 1), name
        assert ntrees <= 0.05 * trees, name
