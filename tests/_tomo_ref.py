"""Plain numpy reference of the tomography multinomial kernels
(csrc/tomography.hip: ``binomial``, ``mnom_segments_kernel``,
``tomography_kernel``) and of the host recursion over segments
(quantum/device.py: ``multinomial_long``).  fp64 numpy and Python ints only;
nothing here imports the code under test.  Every sampler is vectorised over
its draws (one Philox call per tree level and trial), results of the case
matrix are cached (``evaluate``) and must not be written to.

Uniform.  A (block, word pair) gives the 53-bit integer
``I = (x << 21) ^ (y >> 11)`` (pair 0: words 0, 1; pair 1: words 2, 3) and
``u = (fp64(I) + 0.5) * 2^-53``.  ``fp64(I)`` is exact.  Below 2^52,
``I + 0.5`` is exact; from 2^52 on it is a tie between I and I + 1 and rounds
to the even one: that rounding is part of the stream's definition (numpy's
fp64 addition performs it), and it makes ``u = 1.0`` reachable
(I = 2^53 - 1).  ``u - 0.5`` and ``0.5 - |u - 0.5|`` are exact in fp64 (every
u is a multiple of 2^-54 below 1/2 and of 2^-53 above), so U, us and V of a
BTRS trial are the same bits on the host and on the device.

Counters.  ``binomial(n, p, key, ctr)`` draws block ``(ctr << 6) + trial``
(inversion: trial 0, pair 0; BTRS trial t: pair 0 -> U, pair 1 -> V).
Segment trees: ``ctr = (((sid * nseg + segment) << 4 | level & 15) << 12) | node``
with heap node ``i`` in [1, P).  Tomography: ``ctr = ((g T + t) 2 + round) << 20
+ (2^l + i)`` for node i of level l of the padded outcome tree, g the global
row.

Budgets.  A draw is *near* when some decision on its path lies closer to its
boundary than a device evaluation in fp64 may differ from this one; a near
draw (and the tree it belongs to) is excused, every other draw must equal
the device bit for bit.  ``margin`` is the minimum over the path of
distance / budget: near means margin <= 1.  With u = 2^-53 (unit roundoff,
half an ulp), the budgets are, term by term:

* The device code is built with ``-O3`` and no ``-ffp-contract`` option
  (sq_learn_amd/_build.py): hipcc then contracts ``a * b + c`` into an fma
  wherever it sees one, across statements.  An fma drops the rounding of the
  product, so each contractible expression may differ from the two-rounding
  value by one ulp of its result.  Divisions and square roots are correctly
  rounded on the device (no fast-math flag), as in numpy.
* Device libm: the ROCm install carries no accuracy table, so the figures
  are assumptions, by name: ``ULP_POW = 2``, ``ULP_LOG = 2``,
  ``ULP_LOG1P = 2`` (ulps of the result; the HIP programming guide's public
  table lists 1 for each of them).
* ``p_abs``: the absolute uncertainty of the probability handed in (0 where
  the device forms it from the same bits by the same operations: the mass
  heap's pairwise sums and a correctly rounded division).  It scales the
  budgets below through d pp = p_abs.
* Flip (``p > 0.5``) and branch (``n pp < 12``): the same operations on the
  same bits; budget ``p_abs`` resp. ``n p_abs``.
* Inversion.  ``q, s, a`` are the same bits; ``r_0 = pow(q, n)`` differs by
  ULP_POW ulps = 2 ULP_POW u relative; step k multiplies by the same
  ``a / k - s`` with one rounding that may fall differently (2 u), so
  ``r_k`` differs by (2 ULP_POW + 2 k) u relative; the running ``u - sum r_j``
  accumulates these weighted by r_j (sum <= 1) plus k subtraction roundings
  of at most u each.  Budget of ``u_k > r_k``:
  ``INV(k) = (2 ULP_POW + 5 k + 4) u + 64 p_abs`` (the mass below any k moves
  by at most n pp p_abs <= 12 p_abs with p; 64 covers pow and the steps).
* BTRS constants.  ``spq = sqrt(n pp q)`` is the same bits.  ``b = 1.15 +
  2.53 spq`` is contractible: 1 ulp.  ``a = -0.0873 + 0.0248 b + 0.01 pp``:
  two contractible sums on top of b's ulp, with a cancellation of at most 2
  (0.0248 b >= 0.18 against 0.0873 once n pp >= 12, pp <= 1/2): 8 ulps.
  ``t = 2 a / us + b``: 9 ulps of the quotient, 1 of b, 1 of the sum: at most
  ``T_ULPS = 12`` ulps of t.  ``alpha = (2.83 + 5.1 / b) spq``: 4 ulps;
  ``vr = 0.92 - 4.2 / b``: absolute 4 * 2^-52.
* Floor.  ``k = floor(t U + c)``, ``c = n pp + 0.5``.  c is contractible: it
  may differ by ulp(c) unless ``n pp`` is exact (checked with an error-free
  product).  The last sum is contractible as well, and near 2^52 its
  rounding to the grid g = ulp(x) decides k: floor(RN(y)) of the real
  ``y = RN(t U) + c`` jumps at ``i - g / 2``.  The reference recovers y with
  an error-free sum and measures its distance to those jumps; the budget is
  ``E = (T_ULPS + 1) 2^-52 |t U| + [n pp inexact] ulp(c) + (n + |t U| / pp) p_abs``
  (t's ulps and the unrounded product; c's ulp; the move of c and t with
  pp).  In ulps of the argument this is a handful at small n and far below
  one at n ~ 2^51, where |t U| << c.
* ``us >= 0.07``: us is exact on both sides, budget 0 (reported for the
  record only).  ``V <= vr``: ``VR = 4 * 2^-52 + p_abs / pp``.
* Acceptance ``lv <= L``, ``lv = log(V alpha / (a / us^2 + b))``: the
  argument carries 4 (alpha) + 10 (denominator) + 2 (product, quotient)
  ulps = 16 * 2^-52 relative, i.e. absolute in lv, plus ULP_LOG ulps of lv.
  L = ln(pmf(k) / pmf(m)) is evaluated without cancellation (``log_pmf``:
  Loader's saddle-point form, ln f(x) = -1/2 ln(2 pi x (n - x) / n) +
  se(n) - se(x) - se(n - x) - bd0(x, n p) - bd0(n - x, n q), with
  ``x - n p`` from an error-free product so that bd0 keeps its relative
  precision at n ~ 2^51; x = 0 and x = n by n log1p(-p), n ln p).  Each
  term is good to ``L_ULPS = 16`` units of u relative (ratio and logarithm:
  4 u + ULP_LOG ulps; bd0: x - n p 1 u, v 3 u, s 5 u, twelve series terms of
  decreasing weight: below 12 u; stirlerr: 5 rounded Horner steps of a
  value below 1/12), so ``L_ERR = L_ULPS u (sum of |terms| of both pmfs + 1)``;
  ``test_tomo_ref_cpu`` holds the evaluation to that bound against 60-digit
  arithmetic up to n = 2^51.  The kernel evaluates the same form with
  device libm and fmas under the same bound, so
  ``ACC = 16 * 2^-52 + ULP_LOG ulp(lv) + 2 L_ERR + (2 |k - m| + 8) p_abs / pp``
  (d ln(p / q) = dp / (p q) per unit of k - m; lv moves by a few dp / pp).
  With p_abs > 0 the mode ``m = floor((n + 1) pp)`` is a decision too:
  budget ``(n + 1) p_abs``.
* After 63 rejected trials the last proposal, clamped to [0, n], is returned
  (branch EXHAUSTED; not reachable by chance: each trial accepts with
  probability > 0.9).

Tomography.  Round 1's prefix ``s += v_i^2`` is contractible: rows flagged
exact (v_i = m_i / 2^12, sum m_i^2 = 2^24: every partial sum is a multiple of
2^-24 below 2) have p_abs = 0, generic rows differ by at most 2 u per step,
``E1 = 2 M u s_M`` on any prefix, p_abs = 2 E1 / tot at a node of mass tot.
Round 2: ``z`` is a sum of 2 d contractible non-negative terms, relative
(2 d + 2) u; ``ap^2 / z`` inherits it, the serial prefix adds M roundings of
at most u: ``E2 = 2 ((2 d + 2) u + M u)``, p_abs = 2 E2 / tot.  The sign rule
and P = sqrt(c / N) use the same bits on both sides.

Error of a checkpoint.  L2: lane l adds its ceil(d / 64) terms
``(v_i - s_i)^2`` in order (contractible), then six butterfly sums (xor 32,
..., 1; every lane ends with the same value because fp64 addition is
commutative).  Both the device's and the reference's value are within
(k + 1) u relative of the exact sum of squares, k = ceil(d / 64) + 6
(non-negative terms); the square root halves that and adds u:
``|err_dev - err_ref| <= (k + 3) u err``.  L-inf takes maxima of exact
differences: bit for bit.
"""
import functools
import math

import numpy as np

from _qrand_ref import MASK32, philox_blocks

U = 2.0 ** -53
ULP_POW = 2
ULP_LOG = 2
ULP_LOG1P = 2
T_ULPS = 12
L_ULPS = 16
SEG = 2048          # outcomes per segment
MAX_M = 512         # padded outcomes of the tomography kernel
TRIALS = 63

TRIVIAL, INVERSION, SQUEEZE, FULL, EXHAUSTED = 0, 1, 2, 3, 4
BRANCH_NAMES = ("trivial", "inversion", "btrs-squeeze", "btrs-full", "btrs-exhausted")

# ln x! - ln(sqrt(2 pi x) (x / e)^x) for x = 0 .. 15 (x = 0: unused placeholder)
SFERR = np.array([
    0.0, 0.08106146679532725821967, 0.04134069595540929409382, 0.02767792568499833914879,
    0.02079067210376509311152, 0.01664469118982119216319, 0.01387612882307074799875,
    0.01189670994589177009506, 0.01041126526197209649748, 0.009255462182712732917729,
    0.008330563433362871256469, 0.007573675487951840794972, 0.006942840107209529865664,
    0.00640899418800420706844, 0.005951370112758847735624, 0.005554733551962801371039])
S0, S1, S2, S3, S4 = 1.0 / 12, 1.0 / 360, 1.0 / 1260, 1.0 / 1680, 1.0 / 1188
HALF_LN_2PI = 0.918938533204672741780329736406


# ------------------------------------------------------------------ uniform
def u53(key, ctr, pair):
    """The 53-bit uniform of word pair ``pair`` of Philox block ``ctr`` (uint64
    array) under ``key = (k0, k1, s0, s1)``: in (0, 1], 1.0 included (module
    docstring)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    k0, k1, s0, s1 = key
    blk = philox_blocks(ctr & np.uint64(MASK32), ctr >> np.uint64(32), s0, s1, k0, k1)
    x, y = blk[..., 2 * pair], blk[..., 2 * pair + 1]
    i = (x << np.uint64(21)) ^ (y >> np.uint64(11))
    return (i.astype(np.float64) + 0.5) * U


# ------------------------------------------------------------------ error-free pieces
def two_prod(a, b):
    """(p, e) with p = RN(a b) and p + e = a b exactly (Veltkamp / Dekker)."""
    p = a * b
    ca = 134217729.0 * a
    ah = ca - (ca - a)
    al = a - ah
    cb = 134217729.0 * b
    bh = cb - (cb - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def two_sum(a, b):
    """(s, e) with s = RN(a + b) and s + e = a + b exactly (Knuth)."""
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    return s, e


# ------------------------------------------------------------------ log pmf
def stirlerr(x):
    x = np.asarray(x, dtype=np.float64)
    xs = np.maximum(x, 16.0)
    x2 = xs * xs
    ser = (S0 - (S1 - (S2 - (S3 - S4 / x2) / x2) / x2) / x2) / xs
    return np.where(x <= 15.0, SFERR[np.clip(x, 0, 15).astype(np.int64)], ser)


def bd0(x, M, d):
    """x ln(x / M) + M - x for x > 0, given d = x - M to full relative
    precision: the series of Loader's bd0 within 10 % of M, the direct form
    (no cancellation there) outside."""
    with np.errstate(all="ignore"):
        v = d / (x + M)
        s = d * v
        ej = 2.0 * x * v
        v2 = v * v
        for j in range(1, 13):
            ej = ej * v2
            s = s + ej / (2 * j + 1)
        far = x * np.log(x / M) - d
    return np.where(np.abs(d) < 0.1 * (x + M), s, far)


def log_pmf(n, pp, x):
    """(ln pmf(x; n, pp), sum of the magnitudes of its terms), 0 <= x <= n,
    0 < pp <= 1/2, without cancellation (module docstring)."""
    n, pp, x = (np.asarray(t, dtype=np.float64) for t in np.broadcast_arrays(n, pp, x))
    hi, lo = two_prod(n, pp)
    nq = (n - hi) - lo
    xs = np.clip(x, 1.0, np.maximum(n - 1.0, 1.0))
    ds = (xs - hi) - lo                     # x - n pp, one rounding
    lead = 0.5 * np.log(2.0 * np.pi * xs * ((n - xs) / n))
    se = stirlerr(n) - stirlerr(xs) - stirlerr(n - xs)
    b1 = bd0(xs, hi, ds)
    b2 = bd0(n - xs, nq, -ds)
    mid = -lead + se - b1 - b2
    mag = np.abs(lead) + np.abs(se) + b1 + b2
    with np.errstate(all="ignore"):
        at0 = n * np.log1p(-pp)
        atn = n * np.log(pp)
    val = np.where(x <= 0.0, at0, np.where(x >= n, atn, mid))
    mag = np.where(x <= 0.0, np.abs(at0), np.where(x >= n, np.abs(atn), mag))
    return val, mag


def log_pmf_ratio(n, pp, k, m):
    """(L, L_ERR): ln(pmf(k) / pmf(m)) and its absolute error bound."""
    a, ma = log_pmf(n, pp, k)
    b, mb = log_pmf(n, pp, m)
    return a - b, L_ULPS * U * (ma + mb + 1.0)


def btrs_rhs_lgamma(n, pp, k, m):
    """The acceptance bound as the kernel formed it before the
    cancellation-free form: h - lgamma(k + 1) - lgamma(n - k + 1) + (k - m) lpq
    in fp64 (host libm); kept to measure that formula against the exact one."""
    from scipy.special import gammaln
    q = 1.0 - pp
    h = gammaln(m + 1.0) + gammaln(n - m + 1.0)
    return h - gammaln(k + 1.0) - gammaln(n - k + 1.0) + (k - m) * np.log(pp / q)


# ------------------------------------------------------------------ binomial
def _ratio(dist, budget):
    with np.errstate(all="ignore"):
        return np.where(budget > 0.0, dist / np.where(budget > 0.0, budget, 1.0), np.inf)


def binomial_ref(n, p, key, ctr, p_abs=0.0, detail=False):
    """Binomial(n, p) draws of the stream ``ctr`` (arrays of one shape).
    Returns dict: ``count``, ``branch`` (TRIVIAL, INVERSION, SQUEEZE, FULL,
    EXHAUSTED), ``margin`` (min over the path of distance / budget; near iff
    <= 1), ``trials`` (BTRS trials used).  ``p_abs``: absolute uncertainty
    of p (module docstring).  With ``detail`` also ``lv``, ``L``, ``k``,
    ``m`` of the last full test (nan elsewhere)."""
    n, p, p_abs = (np.array(t, dtype=np.float64) for t in np.broadcast_arrays(n, p, p_abs))
    shape = n.shape
    n, p, p_abs = n.ravel(), p.ravel(), p_abs.ravel()
    ctr = np.broadcast_to(np.asarray(ctr, dtype=np.uint64), shape).ravel()
    N = n.size
    count = np.zeros(N)
    branch = np.full(N, TRIVIAL, dtype=np.int64)
    margin = np.full(N, np.inf)
    trials = np.zeros(N, dtype=np.int64)
    det = {t: np.full(N, np.nan) for t in ("lv", "L", "k", "m")} if detail else None

    zero = (n <= 0.0) | (p <= 0.0)
    one = ~zero & (p >= 1.0)
    count[one] = n[one]
    act = ~(zero | one)
    flip = p > 0.5
    pp = np.where(flip, 1.0 - p, p)
    margin[act] = np.minimum(_ratio(np.abs(p - 0.5), p_abs), _ratio(np.abs(n * pp - 12.0), n * p_abs))[act]
    inv = act & (n * pp < 12.0)
    bt = act & ~inv

    idx = np.nonzero(inv)[0]
    if idx.size:
        ni, ppi, pa = n[idx], pp[idx], p_abs[idx]
        q = 1.0 - ppi
        s = ppi / q
        a = (ni + 1.0) * s
        r = np.power(q, ni)
        u = u53(key, ctr[idx] << np.uint64(6), 0)
        k = np.zeros(idx.size)
        mg = np.full(idx.size, np.inf)
        live = np.ones(idx.size, dtype=bool)
        for step in range(4097):
            bud = (2 * ULP_POW + 5 * step + 4) * U + 64.0 * pa
            mg = np.where(live, np.minimum(mg, _ratio(np.abs(u - r), bud)), mg)
            go = live & (u > r) & (step < 4096)
            if not go.any():
                break
            u = np.where(go, u - r, u)
            k = np.where(go, k + 1.0, k)
            with np.errstate(all="ignore"):
                r = np.where(go, r * (a / np.maximum(k, 1.0) - s), r)
            live = go
        k = np.minimum(k, ni)
        count[idx] = k
        branch[idx] = INVERSION
        margin[idx] = np.minimum(margin[idx], mg)

    idx = np.nonzero(bt)[0]
    if idx.size:
        ni, ppi, pa = n[idx], pp[idx], p_abs[idx]
        q = 1.0 - ppi
        npp, npe = two_prod(ni, ppi)
        spq = np.sqrt(ni * ppi * q)
        b = 1.15 + 2.53 * spq
        a = -0.0873 + 0.0248 * b + 0.01 * ppi
        c = npp + 0.5
        vr = 0.92 - 4.2 / b
        alpha = (2.83 + 5.1 / b) * spq
        m = np.floor((ni + 1.0) * ppi)
        ec = np.where(npe != 0.0, np.spacing(c), 0.0)
        xm = (ni + 1.0) * ppi
        mg = _ratio(np.minimum(xm - m, m + 1.0 - xm), (ni + 1.0) * pa)
        kk = np.zeros(idx.size)
        br = np.full(idx.size, EXHAUSTED, dtype=np.int64)
        tr = np.full(idx.size, TRIALS, dtype=np.int64)
        pend = np.arange(idx.size)
        for trial in range(TRIALS):
            if pend.size == 0:
                break
            tc = (ctr[idx[pend]] << np.uint64(6)) + np.uint64(trial)
            Uu = u53(key, tc, 0) - 0.5
            Vv = u53(key, tc, 1)
            us = 0.5 - np.abs(Uu)
            t = 2.0 * a[pend] / us + b[pend]
            tU = t * Uu
            x, xe = two_sum(tU, c[pend])
            k = np.floor(x)
            g = np.spacing(np.abs(x))
            fr = x - k
            dist = np.minimum(np.abs(fr + xe + 0.5 * g), np.abs(1.0 - 0.5 * g - fr - xe))
            E = (T_ULPS + 1) * 2.0 * U * np.abs(tU) + ec[pend] + \
                (ni[pend] + np.abs(tU) / ppi[pend]) * pa[pend]
            mloc = _ratio(dist, E)
            inside = (k >= 0.0) & (k <= ni[pend])
            sq_try = inside & (us >= 0.07)
            mloc = np.where(sq_try, np.minimum(mloc, _ratio(np.abs(Vv - vr[pend]),
                                                             8.0 * U + pa[pend] / ppi[pend])), mloc)
            sq = sq_try & (Vv <= vr[pend])
            full = inside & ~sq
            acc = np.zeros(pend.size, dtype=bool)
            if full.any():
                f = np.nonzero(full)[0]
                pf = pend[f]
                lv = np.log(Vv[f] * alpha[pf] / (a[pf] / (us[f] * us[f]) + b[pf]))
                L, Lerr = log_pmf_ratio(ni[pf], ppi[pf], k[f], m[pf])
                bud = 32.0 * U + ULP_LOG * np.spacing(np.abs(lv)) + 2.0 * Lerr + \
                    (2.0 * np.abs(k[f] - m[pf]) + 8.0) * pa[pf] / ppi[pf]
                mloc[f] = np.minimum(mloc[f], _ratio(np.abs(lv - L), bud))
                acc[f] = lv <= L
                if detail:
                    for name, val in (("lv", lv), ("L", L), ("k", k[f]), ("m", m[pf])):
                        det[name][idx[pf]] = val
            mg[pend] = np.minimum(mg[pend], mloc)
            done = sq | acc
            kk[pend] = k
            br[pend[sq]] = SQUEEZE
            br[pend[acc]] = FULL
            tr[pend[done]] = trial + 1
            pend = pend[~done]
        kk = np.clip(kk, 0.0, ni)
        count[idx] = kk
        branch[idx] = br
        trials[idx] = tr
        margin[idx] = np.minimum(margin[idx], mg)

    fl = act & flip
    count[fl] = n[fl] - count[fl]
    out = dict(count=count.reshape(shape), branch=branch.reshape(shape),
               margin=margin.reshape(shape), trials=trials.reshape(shape))
    if detail:
        out.update({t: v.reshape(shape) for t, v in det.items()})
    return out


def _split(n, left, tot, key, ctr, e_abs=0.0):
    """One tree level: nl ~ Binomial(n, clamp(left / tot)) where n > 0 and
    tot > 0, else 0.  ``e_abs``: absolute uncertainty of left and tot.
    Returns (nl, margin, number of draws, number of near draws)."""
    live = (n > 0.0) & (tot > 0.0)
    with np.errstate(all="ignore"):
        pl = np.where(live, left / np.where(live, tot, 1.0), 0.0)
        pa = np.where(live, 2.0 * e_abs / np.where(live, tot, 1.0), 0.0) * np.ones_like(pl)
    pl = np.clip(pl, 0.0, 1.0)
    # an all-zero half gives p = 0 or 1 from equal bits on both sides
    pa = np.where((pl <= 0.0) | (pl >= 1.0), 0.0, pa)
    res = binomial_ref(np.where(live, n, 0.0), pl, key, ctr, pa)
    mg = np.where(live, res["margin"], np.inf)
    mg = np.where(live & (pa > 0.0) & (tot <= 4.0 * e_abs), 0.0, mg)
    drawn = live & (res["branch"] != TRIVIAL)
    return np.where(live, res["count"], 0.0), mg, int(drawn.sum()), int((drawn & (mg <= 1.0)).sum())


# ------------------------------------------------------------------ segment trees
def _segment_block(w, nseg_tot, key, sidj, level):
    """Trees of equal length: w [nb, len], nseg_tot [nb], sidj [nb] =
    sid * nseg + segment (uint64).  Returns (cnt [nb, len], margin [nb],
    draws, near)."""
    nb, ln = w.shape
    P = 1
    while P < ln:
        P <<= 1
    mass = np.zeros((nb, 2 * P))
    mass[:, P:P + ln] = np.where(w > 0.0, w, 0.0)
    width = P >> 1
    while width >= 1:
        mass[:, width:2 * width] = mass[:, 2 * width:4 * width:2] + mass[:, 2 * width + 1:4 * width:2]
        width >>= 1
    cn = np.zeros((nb, 2 * P))
    cn[:, 1] = nseg_tot
    seg_ctr = ((sidj.astype(np.uint64) << np.uint64(4)) | np.uint64(level & 15)) << np.uint64(12)
    margin = np.full(nb, np.inf)
    draws = near = 0
    width = 1
    while width < P:
        i = np.arange(width, 2 * width)
        ctr = seg_ctr[:, None] | i[None, :].astype(np.uint64)
        nl, mg, dr, nr = _split(cn[:, i], mass[:, 2 * i], mass[:, i], key, ctr)
        cn[:, 2 * i] = nl
        cn[:, 2 * i + 1] = cn[:, i] - nl
        margin = np.minimum(margin, mg.min(1))
        draws += dr
        near += nr
        width <<= 1
    return cn[:, P:P + ln], margin, draws, near


def segment_tree_ref(W, wrow, m, Nseg, key, sid, level):
    """Model of ``mnom_segments_kernel``: W [rows, >= m] weights (row b of
    the batch reads W[wrow[b], :m]; negative weights count as 0), Nseg
    [B, nseg] segment totals, sid [B].  Returns dict: ``cnt`` [B, m],
    ``margin`` [B, nseg] (a tree's margin is the minimum over its draws),
    ``draws``, ``near`` (single draws that are not trivial / of those, near)."""
    W = np.asarray(W, dtype=np.float64)
    wrow = np.asarray(wrow, dtype=np.int64)
    sid = np.asarray(sid, dtype=np.int64)
    B = wrow.shape[0]
    nseg = -(-m // SEG)
    Nseg = np.asarray(Nseg, dtype=np.float64).reshape(B, nseg)
    cnt = np.zeros((B, m))
    margin = np.full((B, nseg), np.inf)
    draws = near = 0
    rows = W[wrow, :m]
    nfull = m // SEG
    base = sid.astype(np.uint64) * np.uint64(nseg)
    if nfull:
        w = rows[:, :nfull * SEG].reshape(B * nfull, SEG)
        sj = (base[:, None] + np.arange(nfull, dtype=np.uint64)[None, :]).reshape(-1)
        c, mg, dr, nr = _segment_block(w, Nseg[:, :nfull].reshape(-1), key, sj, level)
        cnt[:, :nfull * SEG] = c.reshape(B, nfull * SEG)
        margin[:, :nfull] = mg.reshape(B, nfull)
        draws += dr
        near += nr
    if nseg > nfull:
        c, mg, dr, nr = _segment_block(rows[:, nfull * SEG:], Nseg[:, nfull], key,
                                       base + np.uint64(nfull), level)
        cnt[:, nfull * SEG:] = c
        margin[:, nfull] = mg
        draws += dr
        near += nr
    return dict(cnt=cnt, margin=margin, draws=draws, near=near)


def multinomial_long_ref(N, W, wrow, key, sid, level=0):
    """Model of the host recursion ``multinomial_long``: the segment totals
    are a multinomial over the segments' masses one level up.  The masses
    must be exact in fp64 in any summation order (the host sums them with a
    library reduction): asserted.  Returns dict: ``cnt`` [B, m], ``margin``
    [B] (minimum over the whole recursion), ``draws``, ``near``."""
    W = np.asarray(W, dtype=np.float64)
    Wr, m = W.shape
    B = len(N)
    if m <= SEG:
        r = segment_tree_ref(W, wrow, m, np.asarray(N, dtype=np.float64)[:, None], key, sid, level)
        return dict(cnt=r["cnt"], margin=r["margin"].min(1), draws=r["draws"], near=r["near"])
    nseg = -(-m // SEG)
    Wc = np.clip(W, 0.0, None)
    Wb = np.zeros((Wr, nseg))
    for j in range(nseg):
        seg = Wc[:, j * SEG:(j + 1) * SEG]
        Wb[:, j] = seg.sum(1)
        assert np.array_equal(Wb[:, j], seg[:, ::-1].sum(1)) and \
            np.all(Wb[:, j] == np.round(Wb[:, j] * 2.0 ** 20) / 2.0 ** 20), "segment masses not exact"
    top = multinomial_long_ref(N, Wb, wrow, key, sid, level + 1)
    r = segment_tree_ref(W, wrow, m, top["cnt"], key, sid, level)
    return dict(cnt=r["cnt"], margin=np.minimum(top["margin"], r["margin"].min(1)),
                draws=top["draws"] + r["draws"], near=top["near"] + r["near"])


# ------------------------------------------------------------------ tomography
def _outcome_tree(pre, M, N, key, base, e_abs):
    """Multinomial over the outcomes with prefix sums pre [np, M + 1] by the
    padded tree: node i of level l covers [i M >> l, (i + 1) M >> l) and
    draws stream base + 2^l + i.  Returns (cnt [np, M], margin [np], draws,
    near)."""
    npair = pre.shape[0]
    lvl = N.reshape(npair, 1).astype(np.float64)
    margin = np.full(npair, np.inf)
    draws = near = 0
    nodes, width = 1, M
    while width > 1:
        i = np.arange(nodes)
        lo, mid, hi = i * width, i * width + width // 2, (i + 1) * width
        tot = pre[:, hi] - pre[:, lo]
        left = pre[:, mid] - pre[:, lo]
        ctr = base[:, None] + (nodes + i)[None, :].astype(np.uint64)
        nl, mg, dr, nr = _split(lvl, left, tot, key, ctr, np.reshape(e_abs, (npair, 1)))
        nxt = np.empty((npair, 2 * nodes))
        nxt[:, 0::2] = nl
        nxt[:, 1::2] = lvl - nl
        lvl = nxt
        margin = np.minimum(margin, mg.min(1))
        draws += dr
        near += nr
        nodes <<= 1
        width >>= 1
    return lvl, margin, draws, near


def err_sum_l2(df2):
    """Sum of df2 [..., d] in the kernel's order: lane l adds i = l, l + 64,
    ... in order, then the butterfly over xor 32, 16, ..., 1."""
    d = df2.shape[-1]
    pad = np.zeros(df2.shape[:-1] + (-(-d // 64) * 64,))
    pad[..., :d] = df2
    pad = pad.reshape(df2.shape[:-1] + (-1, 64))
    e = np.zeros(df2.shape[:-1] + (64,))
    for j in range(pad.shape[-2]):
        e = e + pad[..., j, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        e = e + e[..., lanes ^ o]
    return e[..., 0]


def err_bound(d, err):
    """|device - reference| of an L2 checkpoint error (module docstring)."""
    return (-(-d // 64) + 6 + 3) * U * err


def tomography_ref(V, sched, key, row_offset=0, norm_inf=False, exact=None, T_total=None):
    """Model of ``tomography_kernel`` for the rows V [r, d] (global rows
    row_offset ..) at every checkpoint of ``sched`` [T].  ``exact`` [r]: rows
    whose round-1 prefix sums are exact in any order (p_abs = 0).  Returns
    dict: ``est`` [r, T, d] (what mode 1 writes for first = t), ``err``
    [r, T] (mode 0), ``cnt1``, ``cnt2`` [r, T, d] (round 2: the hidden plus
    counts), ``margin1``, ``margin2`` [r, T] (the rounds' tree margins;
    margin2 includes margin1), ``draws``, ``near``."""
    V = np.asarray(V, dtype=np.float64)
    r, d = V.shape
    sched = np.asarray(sched, dtype=np.int64)
    T = sched.shape[0]
    assert d + 1 <= MAX_M
    M = 1
    while M < d + 1:
        M <<= 1
    exact = np.zeros(r, dtype=bool) if exact is None else np.asarray(exact, dtype=bool)
    npair = r * T
    row = np.repeat(np.arange(r), T)
    tt = np.tile(np.arange(T), r)
    N = sched[tt].astype(np.float64)
    g = (np.uint64(row_offset) + row.astype(np.uint64))
    base = ((g * np.uint64(T) + tt.astype(np.uint64)) * np.uint64(2)) << np.uint64(20)
    v = V[row]
    # round 1
    sq = np.zeros((npair, M))
    sq[:, :d] = v * v
    pre = np.zeros((npair, M + 1))
    pre[:, 1:] = np.cumsum(sq, axis=1)
    e1 = np.where(exact[row], 0.0, 2.0 * M * U * pre[:, M])
    cnt1, m1, dr1, nr1 = _outcome_tree(pre, M, N, key, base, e1)
    cnt1 = cnt1[:, :d]
    P = np.sqrt(cnt1 / N[:, None])
    # round 2
    ap = 0.5 * (v + P)
    am = 0.5 * (v - P)
    z = np.zeros(npair)
    for i in range(d):
        z = z + (ap[:, i] * ap[:, i] + am[:, i] * am[:, i])
    pre = np.zeros((npair, M + 1))
    s = np.zeros(npair)
    for i in range(M):
        pre[:, i] = s
        if i < d:
            s = s + ap[:, i] * ap[:, i] / z
        elif i == d:
            s = s + np.maximum(1.0 - s, 0.0)
    pre[:, M] = s
    e2 = np.full(npair, 2.0 * ((2 * d + 2) * U + M * U))
    cnt2, m2, dr2, nr2 = _outcome_tree(pre, M, N, key, base + np.uint64(1 << 20), e2)
    cnt2 = cnt2[:, :d]
    est = np.where(cnt2 > 0.4 * P * P * N[:, None], P, -P)
    df = v - est
    err = np.abs(df).max(1) if norm_inf else np.sqrt(err_sum_l2(df * df))
    sh = (r, T)
    return dict(est=est.reshape(r, T, d), err=err.reshape(sh), cnt1=cnt1.reshape(r, T, d),
                cnt2=cnt2.reshape(r, T, d), margin1=m1.reshape(sh),
                margin2=np.minimum(m1, m2).reshape(sh), draws=dr1 + dr2, near=nr1 + nr2, d=d)


def mode2_stop(case):
    """The stop bound the mode-2 test uses for a case: just above the median
    checkpoint error, so that rows stop at different checkpoints."""
    errs = np.sort(case["ref"]["err"].ravel())
    return float(errs[errs.size // 2]) * (1 + 2.0 ** -20) + 1e-9


def mode2_ref(ref, stop_err, norm_inf=False):
    """Mode 2 on a ``tomography_ref`` result: (t_stop [r], est [r, d],
    excused [r]).  A row is excused when a checkpoint up to its stop is near,
    or when an error up to there is within the device bound of ``stop_err``."""
    err, est = ref["err"], ref["est"]
    r, T = err.shape
    ok = err <= stop_err
    t_stop = np.where(ok.any(1), ok.argmax(1), T - 1)
    bound = 0.0 if norm_inf else err_bound(ref["d"], err)
    shaky = (ref["margin2"] <= 1.0) | (np.abs(err - stop_err) <= bound)
    upto = np.arange(T)[None, :] <= t_stop[:, None]
    return t_stop, est[np.arange(r), t_stop], (shaky & upto).any(1)


# ------------------------------------------------------------------ cases
KEY_B = (0x452821E6, 0x38D01377, 0x00000007, 0x00020000)
KEY_S = (0xBE5466CF, 0x34E90C6C, 0x0000000B, 0x00020000)
KEY_T = (0xC0AC29B7, 0xC97C50DD, 0x00000003, 0x00020000)

BIN_N = (0.0, 1.0, 7.0, 100.0, 4000.0, 1e6, 3e9, 5.8e11, 1e12, 2.0 ** 51)
BIN_P = (0.0, 1e-13, 1e-6, 0.003, 0.2, 0.5, 0.5 + 2.0 ** -40, 0.7, 1 - 1e-6, 1.0)
BIN_B = 4096


@functools.lru_cache(maxsize=None)
def binomial_case():
    """The one-draw-per-workgroup case: dict with W [B, 2] (own weight row
    per draw: p = w0 / (w0 + w1) as the heap forms it), N [B], sid [B], the
    nominal (n, p) grid cell ``cell`` [B] (-1: extras) and the reference
    ``ref`` (binomial_ref with detail) under KEY_B, level 0."""
    ns, ps = [], []
    for n in BIN_N:
        for p in BIN_P:
            ns.append(n)
            ps.append(p)
    ncell = len(ns)
    # pairs straddling n pp = 12, on both sides of the flip
    for n, pp in ((24.0, 0.5), (25.0, 0.48), (23.0, 0.5), (100.0, 0.12), (100.0, 0.1199),
                  (4000.0, 0.003), (4000.0, 0.002999), (1e6, 12e-6), (1e6, 11.99e-6),
                  (1e12, 12e-12), (1e12, 11.9e-12), (2.0 ** 51, 12 * 2.0 ** -51),
                  (2.0 ** 51, 11.5 * 2.0 ** -51)):
        for p in (pp, 1.0 - pp):
            ns.append(n)
            ps.append(p)
    reps = BIN_B // len(ns)
    n = np.tile(np.array(ns), reps)
    p = np.tile(np.array(ps), reps)
    cell = np.tile(np.where(np.arange(len(ns)) < ncell, np.arange(len(ns)), -1), reps)
    # one row with a negative weight: clamped to 0, p = 1
    W = np.stack([p, 1.0 - p], axis=1)
    W = np.concatenate([W, [[0.25, -3.0], [-1.0, 0.5]]])
    n = np.concatenate([n, [1000.0, 1000.0]])
    cell = np.concatenate([cell, [-1, -1]])
    B = n.shape[0]
    sid = (np.arange(B, dtype=np.int64) * 2654435761) % (1 << 31)
    Wc = np.clip(W, 0.0, None)
    tot = Wc[:, 0] + Wc[:, 1]
    pl = np.clip(Wc[:, 0] / tot, 0.0, 1.0)
    ctr = (((sid.astype(np.uint64) * np.uint64(1)) << np.uint64(4)) << np.uint64(12)) | np.uint64(1)
    ref = binomial_ref(n, pl, KEY_B, ctr, detail=True)
    return dict(W=W, N=n, sid=sid, cell=cell, p=pl, ref=ref, key=KEY_B)


SEG_M = (1, 2, 3, 255, 256, 257, 2047, 2048)
LONG_M = (2049, 4097, 2048 * 3 + 5)
SEG_LEVELS = (0, 4, 5, 9)
SEG_B = 6


def seg_weights(m, rows=4, seed=0):
    """[rows, m + 3] weights with a stride above m: row 0 generic, row 1 with
    runs of zeros (and a negative entry), row 2 a single non-zero weight, row
    3 small integers."""
    rng = np.random.default_rng(1000 + m + seed)
    W = np.zeros((rows, m + 3))
    W[0, :m] = rng.exponential(size=m) ** 2
    w = rng.exponential(size=m)
    w[rng.random(m) < 0.5] = 0.0
    w[m // 3: m // 3 + max(m // 4, 1)] = 0.0
    if m > 2:
        w[m // 2] = -1.5
    if not (w > 0).any():
        w[m - 1] = 1.0
    W[1, :m] = w
    W[2, (2 * m) // 3] = 3.0
    W[3, :m] = rng.integers(0, 9, size=m)
    if not W[3, :m].any():
        W[3, 0] = 1.0
    W[:, m:] = 7.0      # past the row: must not be read
    return W


@functools.lru_cache(maxsize=None)
def segment_case(m, level=0):
    """One-segment trees of length m: dict with W, wrow [B], N [B], sid [B]
    and the reference."""
    W = seg_weights(m)
    wrow = np.array([0, 1, 2, 3, 1, 0])
    N = np.array([1.0, 37.0, 5000.0, 1e6, 3e9, 1e12])
    sid = np.array([0, 5, 2 ** 20 + 3, 77, 1, 2 ** 31 - 1])
    ref = segment_tree_ref(W, wrow, m, N[:, None], KEY_S, sid, level)
    return dict(W=W, wrow=wrow, N=N, sid=sid, ref=ref, key=KEY_S, m=m, level=level)


@functools.lru_cache(maxsize=None)
def long_case(m):
    """Several segments through the host recursion; integer weights, so the
    segment masses are exact in any order."""
    rng = np.random.default_rng(m)
    W = np.zeros((3, m))
    W[0] = rng.integers(0, 17, size=m)
    W[1] = np.where(rng.random(m) < 0.6, 0.0, rng.integers(1, 5, size=m))
    W[1, SEG:] = 0.0
    W[1, m - 1] = 2.0                      # the last, short segment holds one weight
    W[2, m - 1] = 1.0                      # a single non-zero weight, in the last segment
    wrow = np.array([0, 1, 2, 0, 1])
    N = np.array([1000.0, 1e6, 12345.0, 3e9, 40.0])
    sid = np.array([3, 0, 9, 2 ** 18, 1])
    ref = multinomial_long_ref(N, W, wrow, KEY_S, sid, 0)
    return dict(W=W, wrow=wrow, N=N, sid=sid, ref=ref, key=KEY_S, m=m)


TOMO_D = (1, 2, 3, 63, 64, 65, 255, 511)
TOMO_R = {1: 9, 2: 5, 3: 9, 63: 3, 64: 5, 65: 3, 255: 1, 511: 3}
SCHEDULES = {1: (1, 1000, 10 ** 10), 2: (3, 10 ** 10), 3: (1, 7, 100, 5000, 10 ** 6, 10 ** 10),
             63: (1, 40, 100000), 64: (1, 7, 100, 5000, 10 ** 5, 10 ** 6), 65: (2000,),
             255: (1, 300, 10 ** 6), 511: (5, 4000, 10 ** 6)}
BIG_D = 13          # d <= 15 for the schedule that reaches 1e10 shots
BIG_SCHED = (1, 3, 1000, 10 ** 6, 10 ** 8, 10 ** 10)
ROW_OFFSET = 5


def exact_row(d, rng, zeros=True):
    """v = m / 2^12 with integers m (zeros and negative entries among them),
    sum m^2 = 2^24: every partial sum of the v_i^2 is exact."""
    target = 1 << 24
    if d == 1:
        return np.array([-1.0])
    while True:
        a = int(4096 * min(1.0, math.sqrt(3.4 / d)))
        m = rng.integers(-a, a + 1, size=d)
        if zeros and d > 2:
            m[rng.random(d) < 0.25] = 0
        m[-1] = 0
        m[0] = 0
        rest = target - int((m.astype(np.int64) ** 2).sum())
        if rest < 0:
            continue
        # Lagrange by search: two squares for the last and the first entry
        a = int(math.isqrt(rest))
        for x in range(a, max(a - 4000, -1), -1):
            y2 = rest - x * x
            y = int(math.isqrt(y2))
            if y * y == y2:
                m[0], m[-1] = x, -y
                assert int((m.astype(np.int64) ** 2).sum()) == target
                return m / 4096.0


def tomo_rows(d, r, seed):
    """(V [r, d], exact [r]): exact rows, row 1 (if any) a basis vector, the
    last row (r >= 3) a generic Gaussian one."""
    rng = np.random.default_rng(seed)
    V = np.stack([exact_row(d, rng) for _ in range(r)])
    exact = np.ones(r, dtype=bool)
    if r >= 2:
        V[1] = 0.0
        V[1, d // 2] = -1.0 if d > 1 else 1.0
    # generic Gaussian rows: the last one (r >= 3); for d <= 3, where the
    # exact rows are (nearly all) basis vectors, every row from the third on
    for i in range(2 if d <= 3 else r - 1, r if r >= 3 else 0):
        gv = rng.standard_normal(d)
        V[i] = gv / np.linalg.norm(gv)
        exact[i] = False
    return V, exact


@functools.lru_cache(maxsize=None)
def tomo_case(d, norm_inf=False, big=False):
    """A tomography case: dict with V, exact, sched, key, ref (rows at global
    offset ROW_OFFSET)."""
    r = 5 if big else TOMO_R[d]
    sched = BIG_SCHED if big else SCHEDULES[d]
    V, exact = tomo_rows(d, r, 50 + d)
    ref = tomography_ref(V, sched, KEY_T, row_offset=ROW_OFFSET, norm_inf=norm_inf, exact=exact)
    return dict(V=V, exact=exact, sched=np.array(sched, dtype=np.int64), key=KEY_T, ref=ref,
                d=d, r=r, norm_inf=norm_inf)


def tomo_case_list():
    return [(d, False) for d in TOMO_D] + [(BIG_D, True)]
