"""Plain numpy references of the fixed-point M-step (csrc/kmeans.hip), written
from the quantisation rule, not from the kernels:

* every addend of a cluster sum is ``rintf(x * s)`` formed in fp32 with
  ``s = w * 2^-xexp`` (a power of two when unweighted), every addend of a
  squared-norm sum is ``rint(x * x * 2^-qexp)`` in fp64;
* the accumulators are integer-valued fp64, so as long as every partial sum
  stays below 2^53 the device result is the integer sum, in any order.

The references sum in int64; the GPU tests compare with ``equal``.  The
module also holds the seeded input builders and the parameter sets shared by
``test_mstep_ref_cpu.py`` and ``test_mstep_kernels_gpu.py``.
"""
import math
from fractions import Fraction

import numpy as np

LIMIT = 2 ** 53         # integers up to here are exact in fp64


# ------------------------------------------------------------------ quanta
def quanta_ref(X32, w32, xexp):
    """int64 [n, d]: rint(x * s) with the product and the rounding in fp32,
    s = fp32(w) * fp32(2^-xexp) (the power of two alone when unweighted)."""
    X32 = np.asarray(X32, dtype=np.float32)
    p = np.float32(2.0 ** -xexp)
    if w32 is None:
        q = np.rint(X32 * p)
    else:
        s = np.asarray(w32, dtype=np.float32) * p
        q = np.rint(X32 * s[:, None])
    assert q.dtype == np.float32
    return q.astype(np.int64)


def _segment_sum(V, lab, k):
    """out[c] = sum of the rows of V (int64 [m] or [m, d]) with lab == c;
    every lab is in [0, k).  Sort + reduceat."""
    out = np.zeros((k,) + V.shape[1:], dtype=np.int64)
    if lab.size == 0:
        return out
    order = np.argsort(lab, kind="stable")
    ls = lab[order]
    present, starts = np.unique(ls, return_index=True)
    out[present] = np.add.reduceat(V[order], starts, axis=0)
    return out


def _in_range(lab, k):
    lab = np.asarray(lab, dtype=np.int64)
    return (lab >= 0) & (lab < k)


def reduce_ref(X32, labels, k, w32, xexp, wexp):
    """(S int64 [k, d], N int64 [k], bound): the cluster sums of the quanta,
    the member counts (unweighted) or the sums of rint(fp32(w) * fp32(2^-wexp))
    and the largest sum_i |q_i| over all (cluster, feature) - every partial
    sum of any order is bounded by it, so bound < 2^53 is the precondition
    of exactness.  Rows with a label outside [0, k) add nothing."""
    labels = np.asarray(labels, dtype=np.int64)
    ok = _in_range(labels, k)
    q = quanta_ref(X32, w32, xexp)[ok]
    lab = labels[ok]
    S = _segment_sum(q, lab, k)
    np.abs(q, out=q)
    bound = int(_segment_sum(q, lab, k).max()) if lab.size else 0
    if w32 is None:
        N = np.bincount(lab, minlength=k).astype(np.int64)
    else:
        wq = np.rint(np.asarray(w32, dtype=np.float32) * np.float32(2.0 ** -wexp))
        assert wq.dtype == np.float32
        N = _segment_sum(wq.astype(np.int64)[ok], lab, k)
    return S, N, bound


def _row_q2(X32, qexp):
    """int64 [n]: sum_f rint(x_f^2 * 2^-qexp) in fp64 (the square of an fp32
    value and its scaling by a power of two are exact)."""
    x = np.asarray(X32, dtype=np.float64)
    return np.rint(x * x * 2.0 ** -qexp).astype(np.int64).sum(axis=1)


def qsum_ref(X32, labels, k, qexp):
    """Q int64 [k]: per cluster, the sum over members and features of
    rint(x^2 * 2^-qexp)."""
    labels = np.asarray(labels, dtype=np.int64)
    ok = _in_range(labels, k)
    return _segment_sum(_row_q2(np.asarray(X32)[ok], qexp), labels[ok], k)


def delta_ref(S, N, Q, X32, labels, prev, k, xexp, qexp):
    """The statistics after the incremental update: the quanta of the rows
    with labels != prev are added to cluster labels[i] and subtracted from
    cluster prev[i], wherever that label is in [0, k)."""
    labels = np.asarray(labels, dtype=np.int64)
    prev = np.asarray(prev, dtype=np.int64)
    X32 = np.asarray(X32, dtype=np.float32)
    moved = labels != prev
    S, N, Q = S.copy(), N.copy(), Q.copy()
    for lab, sign in ((labels, 1), (prev, -1)):
        sel = moved & _in_range(lab, k)
        rows = X32[sel]
        S += sign * _segment_sum(quanta_ref(rows, None, xexp), lab[sel], k)
        N += sign * np.bincount(lab[sel], minlength=k).astype(np.int64)
        Q += sign * _segment_sum(_row_q2(rows, qexp), lab[sel], k)
    return S, N, Q


# ------------------------------------------------------- inertia / finalize
def _pow2(e):
    return Fraction(2) ** e


def _scaled_ints(v):
    """Exact integers m_f and a shift sh with v_f = m_f / 2^sh."""
    ratios = [float(x).as_integer_ratio() for x in v]
    sh = max([den.bit_length() - 1 for _, den in ratios] + [0])
    return [num << (sh - (den.bit_length() - 1)) for num, den in ratios], sh


def cluster_parts_ref(S, N, Q, C32, xexp, qexp):
    """(part fp64 [k], mag fp64 [k]):
    part_c = Q_c 2^qexp - 2 2^xexp sum_f c_f S_cf + N_c sum_f c_f^2 evaluated
    exactly (integers and one Fraction) and rounded once to fp64;
    mag_c the same with every term replaced by its absolute value."""
    C32 = np.asarray(C32, dtype=np.float32)
    k = C32.shape[0]
    part = np.zeros(k, dtype=np.float64)
    mag = np.zeros(k, dtype=np.float64)
    for c in range(k):
        ci, sh = _scaled_ints(C32[c].tolist())
        Sc = [int(v) for v in S[c].tolist()]
        cs = sum(a * b for a, b in zip(ci, Sc))
        cs_abs = sum(abs(a * b) for a, b in zip(ci, Sc))
        cc = sum(a * a for a in ci)
        q, nc = int(Q[c]), int(N[c])
        cross = 2 * _pow2(xexp) / _pow2(sh)
        sq = Fraction(nc * cc) / _pow2(2 * sh)
        part[c] = float(q * _pow2(qexp) - cross * cs + sq)
        mag[c] = float(abs(q) * _pow2(qexp) + cross * cs_abs + abs(sq))
    return part, mag


def finalize_ref(packed, C_old32, k, d, empty_policy):
    """(C_new fp32 [k, d] without noise, shift fp64 [k]) from the packed
    bucket [sums k*d, counts k, inertia]: fp32(sum / count) (fp64 division,
    one rounding) when count > 0, else C_old (policy 0) or 0 (policy 1);
    shift_j = fsum((fp64(v) - fp64(old))^2)."""
    packed = np.asarray(packed, dtype=np.float64)
    C_old32 = np.asarray(C_old32, dtype=np.float32).reshape(k, d)
    sums = packed[:k * d].reshape(k, d)
    cnt = packed[k * d:k * d + k]
    C_new = np.empty((k, d), dtype=np.float32)
    for j in range(k):
        if cnt[j] > 0:
            C_new[j] = (sums[j] / cnt[j]).astype(np.float32)
        elif empty_policy == 0:
            C_new[j] = C_old32[j]
        else:
            C_new[j] = 0.0
    diff = C_new.astype(np.float64) - C_old32.astype(np.float64)
    shift = np.array([math.fsum(r) for r in diff * diff], dtype=np.float64)
    return C_new, shift


# ------------------------------------------------------------ input builders
LABEL_PATTERNS = ("random", "one_cluster", "alternating", "with_invalid", "all_invalid",
                  "empty_clusters")
VALUE_PATTERNS = ("normal", "halves", "tiny", "huge")
HALVES_XEXP = -30


def make_labels(pattern, n, k, seed=0):
    """int32 [n] labels (seeded)."""
    rng = np.random.RandomState(1000 + seed)
    if pattern == "random":
        lab = rng.randint(0, k, n)
    elif pattern == "one_cluster":
        lab = np.full(n, k // 2)
    elif pattern == "alternating":
        lab = np.arange(n) % k
    elif pattern == "with_invalid":
        lab = rng.randint(0, k, n)
        lab[rng.permutation(n)[:(n + 9) // 10]] = -1
    elif pattern == "all_invalid":
        lab = np.full(n, -1)
    elif pattern == "empty_clusters":
        lab = rng.randint(0, max(k - 2, 1), n)
    else:
        raise ValueError(pattern)
    return lab.astype(np.int32)


def bf16_round(X32):
    """fp32 values rounded to the nearest bf16 (ties to even), as fp32."""
    u = np.ascontiguousarray(X32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(X32))


def make_values(pattern, n, d, seed=0, bf16=False):
    """fp32 [n, d] data (seeded); with ``bf16`` rounded to bf16 values.

    ``halves``: entries (m + 0.5) 2^HALVES_XEXP, |m| <= 1000, so that every
    quantum sits on a round-half-even tie at the exponent HALVES_XEXP; entry
    [0, 0] is the power of two that makes ``fixed_point_exp(max|x|, n)``
    return exactly that exponent."""
    rng = np.random.RandomState(2000 + seed)
    if pattern == "normal":
        X = rng.standard_normal((n, d)) * 3
    elif pattern == "tiny":
        X = rng.standard_normal((n, d)) * 1e-30
    elif pattern == "huge":
        X = rng.standard_normal((n, d)) * 1e30
    elif pattern == "halves":
        m = rng.randint(-1000, 1001, (n, d)).astype(np.float64)
        X = (m + 0.5) * 2.0 ** HALVES_XEXP
        X[0, 0] = 2.0 ** math.floor(math.log2(2.0 ** (52 + HALVES_XEXP) / n))
    else:
        raise ValueError(pattern)
    X = X.astype(np.float32)
    return bf16_round(X) if bf16 else X


def make_weights(kind, n, seed=0):
    """fp32 [n] weights in (0, 1] with w[0] = 1 (``kind`` "rand"), or the
    same power of two on every row ("pow2"); None for "none"."""
    if kind == "none":
        return None
    if kind == "pow2":
        return np.full(n, 0.25, dtype=np.float32)
    rng = np.random.RandomState(3000 + seed)
    w = (1.0 - rng.random_sample(n)).astype(np.float32)
    w[w <= 0] = 1.0
    w[0] = 1.0
    return w


# ------------------------------------------------- parameter sets (GPU file)
K0 = 37
REDUCE_N = (1, 3, 8191, 8192, 8193, 20001)
REDUCE_D = {"f32": (4, 8, 12, 16, 20, 36, 68, 124, 128, 252, 256, 260, 1024),
            "bf16": (8, 16, 24, 40, 72, 136, 248, 12, 256, 260, 512)}
REDUCE_D_ALL_N = (4, 20, 256)
PATTERN_SHAPES = ((8193, 20), (8193, 256))


def reduce_cases():
    """(dtype, n, d, k, label pattern, value pattern, weights) of every
    segmented-reduce comparison of the GPU file."""
    cases = []
    for dt in ("f32", "bf16"):
        shapes = []
        for d in REDUCE_D[dt]:
            for n in ((8193,) if d >= 512 else (8193, 20001)):
                shapes.append((n, d))
        for d in REDUCE_D_ALL_N:
            for n in REDUCE_N:
                if (n, d) not in shapes:
                    shapes.append((n, d))
        for n, d in shapes:
            for wk in ("none", "rand"):
                cases.append((dt, n, d, K0, "random", "normal", wk))
    for n, d in PATTERN_SHAPES:
        for dt in ("f32", "bf16"):
            for lp in LABEL_PATTERNS[1:]:
                for wk in ("none", "rand"):
                    cases.append((dt, n, d, K0, lp, "normal", wk))
            for vp in VALUE_PATTERNS[1:]:
                for wk in ("none", "rand"):
                    cases.append((dt, n, d, K0, "random", vp, wk))
    cases.append(("f32", 8193, 20, K0, "random", "normal", "pow2"))
    cases.append(("bf16", 8193, 256, K0, "random", "normal", "pow2"))
    for k in (1, 63, 64, 65, 1024, 1025):
        cases.append(("f32", 20001, 20, k, "random", "normal", "none"))
    cases.append(("f32", 20001, 4, 16384, "random", "normal", "none"))
    cases.append(("f32", 140001, 4, K0, "random", "normal", "none"))
    return cases


DELTA_N = (1, 3, 5, 8191, 8193, 20001)
DELTA_D = (4, 100, 252, 256, 260, 512, 516, 768, 772, 1024)
DELTA_D_ALL_N = (4, 100, 256)
DELTA_LONG = (530000, 4)


def delta_shapes():
    """(n, d) of the incremental-update sequences of the GPU file."""
    shapes = []
    for d in DELTA_D:
        for n in ((8193,) if d >= 512 else (8193, 20001)):
            shapes.append((n, d))
    for d in DELTA_D_ALL_N:
        for n in DELTA_N:
            if (n, d) not in shapes:
                shapes.append((n, d))
    return shapes


def delta_label_steps(n, k, seed=0):
    """The five label vectors of one incremental sequence (int32 [n] each):
    random start, ~3 % relabelled, unchanged, a tenth to -1 (and, from the
    step after, back), every row in one cluster."""
    rng = np.random.RandomState(4000 + seed)
    l1 = rng.randint(0, k, n).astype(np.int32)
    l2 = l1.copy()
    mv = rng.permutation(n)[:max(1, (3 * n) // 100)]
    l2[mv] = rng.randint(0, k, mv.size)
    l3 = l2.copy()
    l4 = l3.copy()
    out = rng.permutation(n)[:max(1, n // 10)]
    l4[out] = -1
    l4b = l4.copy()                       # earlier -1 rows come back, others leave
    l4b[out] = rng.randint(0, k, out.size)
    out2 = rng.permutation(n)[:max(1, n // 10)]
    l4b[out2] = -1
    l5 = np.full(n, k - 1, dtype=np.int32)
    return [l1, l2, l3, l4, l4b, l5]
