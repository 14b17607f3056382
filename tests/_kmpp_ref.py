"""Plain numpy model of the exact accelerated greedy k-means++
(csrc/kmpp.hip), written from the algorithm the kernel file's header and
``models/cluster/_init.py`` document, not from the kernels:

* a row's potential is the integer ``q = rint(float64(v) * w * scale)`` with
  one power-of-two ``scale`` per run, so every sum of potentials (block
  totals, prefixes, P, the improvement sums Delta_j) is an exact fp64 integer
  in any order as long as it stays below 2^53;
* a step draws t candidates (the first row whose inclusive prefix reaches
  ``draws * P``), a trial improves a row only where ``D_ij < closest_i``, the
  first trial with the smallest ``P - Delta_j`` wins.

Distances here are fp64 direct form.  On the lattice data of
``lattice_blobs`` (integer coordinates, ``d (2 L)^2 < 2^24``) every fp32
difference, square and partial sum of squares is an integer below 2^24 - exact
in any summation order, with or without fma - so the device's fp32 distances
equal these fp64 ones bit for bit and a whole run is reproducible exactly.

The module also holds the int8 quantisation of the certified bound as
specified, and the reference greedy k-means++ oracle shared with
``test_cluster_cpu.py``.
"""
import math

import numpy as np

LIMIT = 2.0 ** 52        # n_global * max potential * scale stays at or below this
U = 2.0 ** -24           # fp32 unit roundoff


def rel_tol(d):
    """First-order bound of the fp32 rounding of a d-term fma sum of squared
    differences, 3 (d + 2) u (about 2x margin over (d + 2) u + the
    subtractions' 2 u)."""
    return 3.0 * (d + 2) * U


# --------------------------------------------------------------- fixed point
def q(v, w, scale):
    """rint(float64(v) * w * scale), in this operation order."""
    v = np.asarray(v, dtype=np.float64)
    if w is None:
        w = 1.0
    return np.rint(v * w * scale)


def scale_for(max_pot, n_global):
    """2^floor(log2(2^52 / (n_global * max_pot))); 1 if max_pot is not positive."""
    mx = float(max_pot)
    if not mx > 0.0:
        return 1.0
    return 2.0 ** math.floor(math.log2(2.0 ** 52 / (max(int(n_global), 1) * mx)))


def partition(n, grid_cap=2048, rows=256):
    """(R, G) of the fixed row partition: G blocks of R rows."""
    g0 = min(max(-(-n // rows), 1), grid_cap)
    R = max(1, -(-n // g0))
    return R, max(1, -(-n // R))


def block_totals(qrow, R, G):
    """fp64 [G]: the sum of the integer potentials of rows [b R, b R + R)."""
    qrow = np.asarray(qrow, dtype=np.float64)
    out = np.zeros(G, dtype=np.float64)
    for b in range(G):
        out[b] = qrow[b * R:(b + 1) * R].sum()
    return out


def pick_ref(qrow, vals, n=None, row_offset=0, n_global=None):
    """(pos, ids): per value the first row whose inclusive prefix of q is >=
    the value (``searchsorted(cumsum, v, 'left')``) clamped to n - 1, and the
    global id pos + row_offset clamped to [0, n_global - 1]."""
    qrow = np.asarray(qrow, dtype=np.float64)
    n = qrow.shape[0] if n is None else int(n)
    n_global = n if n_global is None else int(n_global)
    cs = np.cumsum(qrow[:n])
    pos = np.minimum(np.searchsorted(cs, np.asarray(vals, dtype=np.float64), "left"), n - 1)
    pos = pos.astype(np.int64)
    return pos, np.clip(pos + int(row_offset), 0, n_global - 1)


def effective_closest(closest, mask, D, best):
    """The closest distances after the lazily applied winner: rows whose mask
    has bit ``best`` take D[best] (best < 0 or None: unchanged)."""
    closest = np.array(closest, copy=True)
    if best is None or best < 0:
        return closest
    sel = ((np.asarray(mask).astype(np.int64) >> int(best)) & 1).astype(bool)
    closest[sel] = np.asarray(D)[int(best)][sel]
    return closest


def dist2(X64, C64, chunk=1 << 15, XT=None):
    """fp64 [m, n]: direct-form squared distances sum_f (x_f - c_f)^2 (``XT``: a
    contiguous transpose of X64 the caller keeps across calls)."""
    X64 = np.asarray(X64, dtype=np.float64)
    C64 = np.atleast_2d(np.asarray(C64, dtype=np.float64))
    n, d = X64.shape
    out = np.empty((C64.shape[0], n), dtype=np.float64)
    if d <= 16 and n > chunk:
        # few features, many rows: feature by feature over contiguous columns
        XT = np.ascontiguousarray(X64.T) if XT is None else XT
        tmp = np.empty(n, dtype=np.float64)
        for j in range(C64.shape[0]):
            acc = out[j]
            acc[:] = 0.0
            for f in range(d):
                np.subtract(XT[f], C64[j, f], out=tmp)
                np.multiply(tmp, tmp, out=tmp)
                acc += tmp
        return out
    for r0 in range(0, n, chunk):
        Xc = X64[r0:r0 + chunk]
        for j in range(C64.shape[0]):
            e = Xc - C64[j]
            out[j, r0:r0 + chunk] = np.einsum("ij,ij->i", e, e)
    return out


# ------------------------------------------------------------ the whole run
def kmpp_ref(X, k, t, first_id, draws, w=None, keep_rows=False):
    """Greedy k-means++ in exact fixed point.  ``draws`` fp64 [k - 1, t].
    Returns a dict: ids [k], centres [k, d] (rows of X), scale, P0 and P (the
    first and final potentials), closest / nearest (final), steps: per centre
    c >= 1 a dict with P (before), vals, pos, delta [t], best, P_after,
    tri_frac (share of rows the triangle criterion ccmin[a] > 4.01 closest,
    or a zero potential, leaves out) and, with ``keep_rows``, the effective
    closest / nearest after the step."""
    X = np.asarray(X)
    n, d = X.shape
    X64 = X.astype(np.float64)
    XT = np.ascontiguousarray(X64.T) if d <= 16 else None
    w64 = None if w is None else np.asarray(w, dtype=np.float64)
    draws = np.asarray(draws, dtype=np.float64).reshape(max(k - 1, 0), t)
    ids = np.empty(k, dtype=np.int64)
    ids[0] = int(first_id)
    closest = dist2(X64, X64[ids[0]])[0]
    nearest = np.zeros(n, dtype=np.int32)
    mx = float((closest * (1.0 if w64 is None else w64)).max()) if n else 0.0
    scale = scale_for(mx, n)
    qcl = q(closest, w64, scale)
    P = float(qcl.sum())
    assert n * mx * scale <= LIMIT
    out = dict(scale=scale, P0=P, steps=[], max_pot=mx)
    for c in range(1, k):
        vals = draws[c - 1] * P
        pos, _ = pick_ref(qcl, vals)
        D = dist2(X64, X64[pos], XT=XT)                # [t, n]
        delta = np.zeros(t, dtype=np.float64)
        for j in range(t):
            sel = D[j] < closest                       # strict: a tie improves nothing
            delta[j] = (qcl[sel] - q(D[j][sel], None if w64 is None else w64[sel], scale)).sum()
        best = int(np.argmin(P - delta))               # the first minimum
        cc = dist2(X64[ids[:c]], X64[pos]).min(0)      # [c]: min_j |cand_j - C_m|^2
        tri = (cc[nearest] > 4.01 * closest) | (closest <= 0.0)
        step = dict(P=P, vals=vals, pos=pos, delta=delta, best=best, tri_frac=float(tri.mean()))
        sel = D[best] < closest
        closest = np.where(sel, D[best], closest)
        nearest = np.where(sel, np.int32(c), nearest)
        qcl = q(closest, w64, scale)
        P = P - float(delta[best])
        ids[c] = pos[best]
        step["P_after"] = P
        if keep_rows:
            step["closest"], step["nearest"] = closest.copy(), nearest.copy()
        out["steps"].append(step)
    assert P == float(qcl.sum())
    out.update(ids=ids, centres=X[ids], P=P, closest=closest, nearest=nearest)
    return out


def kpp_oracle(X, k, rs, t=None, w=None):
    """The reference's greedy k-means++ (``cluster/_kmeans.py:153-247``),
    verbatim semantics in numpy fp64 (``w``: the potential of a row is
    w * d^2, the framework's extension)."""
    n = X.shape[0]
    t = t or 2 + int(np.log(k))
    ww = 1.0 if w is None else np.asarray(w, dtype=np.float64)
    xn = (X * X).sum(1)
    idx = [rs.randint(n)]
    closest = np.maximum(xn + xn[idx[0]] - 2 * X @ X[idx[0]], 0)
    pot = (closest * ww).sum()
    for _ in range(1, k):
        vals = rs.random_sample(t) * pot
        cand = np.clip(np.searchsorted(np.cumsum(closest * ww), vals), None, n - 1)
        D = np.maximum(xn[None, :] + xn[cand][:, None] - 2 * X[cand] @ X.T, 0)
        D = np.minimum(closest, D)
        p = (D * ww).sum(1)
        b = int(np.argmin(p))
        pot, closest = p[b], D[b]
        idx.append(cand[b])
    return np.array(idx)


# ------------------------------------------------------------- lattice data
def lattice_limit(d):
    """The largest integer L with d (2 L)^2 < 2^24."""
    L = int(math.isqrt((2 ** 24 - 1) // d)) // 2
    while d * (2 * (L + 1)) ** 2 < 2 ** 24:
        L += 1
    while d * (2 * L) ** 2 >= 2 ** 24:
        L -= 1
    return L


def lattice_blobs(n, d, centres, L, seed, spread=None):
    """fp32 [n, d] integer-valued blobs with |x| <= L: ``centres`` integer
    blob centres, integer noise of about ``spread`` (default L / 64, at
    least 1) around them, clipped to the box."""
    assert L >= 1 and d * (2 * L) ** 2 < 2 ** 24, (d, L)
    rs = np.random.RandomState(seed)
    spread = max(1.0, L / 64.0) if spread is None else float(spread)
    G = rs.randint(-L, L + 1, (centres, d))
    X = G[rs.randint(centres, size=n)] + np.rint(spread * rs.standard_normal((n, d)))
    X = np.clip(X, -L, L).astype(np.float32)
    assert np.array_equal(X, np.rint(X)) and np.abs(X).max() <= L
    return X


# ------------------------------------------------ int8 copies of the bound
def pad64(d):
    return -(-d // 64) * 64


def quantise_rows(X, dq):
    """(q int8 [n, dq], s fp32 [n], e fp64 [n], q2 int64 [n]): s = max|x| / 127
    in fp32 (1 for a zero row), q = rint(x / s) in fp32 clamped to +-127,
    zeros in d .. dq - 1, e = |x - s q| in fp64, q2 = |q|^2."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    mx = np.abs(X).max(1) if d else np.zeros(n, dtype=np.float32)
    s = np.where(mx > 0, mx / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    qv = np.clip(np.rint(X / s[:, None]), -127, 127)
    qi = np.zeros((n, dq), dtype=np.int8)
    qi[:, :d] = qv.astype(np.int8)
    r = X.astype(np.float64) - s.astype(np.float64)[:, None] * qi[:, :d].astype(np.float64)
    e = np.sqrt((r * r).sum(1))
    return qi, s, e, (qi.astype(np.int64) ** 2).sum(1)


def quantise_cands(C, dq):
    """(cq int8 [2, 16, dq], sc fp64 [t], ec fp64 [t], c2 fp64 [t]): the
    two-term copy c~ = s_c (q1 + q2 / 254) with s_c = max|c| / 127 (fp64; 1
    for a zero candidate), q1 = rint(c / s_c), q2 = rint(254 (c / s_c - q1)),
    both clamped to +-127; ec = |c - c~|, c2 = |c~|^2."""
    C = np.asarray(C, dtype=np.float32)
    t, d = C.shape
    assert t <= 16
    C64 = C.astype(np.float64)
    mx = np.abs(C).max(1).astype(np.float64)
    sc = np.where(mx > 0, mx / 127.0, 1.0)
    y = C64 / sc[:, None]
    q1 = np.clip(np.rint(y), -127, 127)
    q2 = np.clip(np.rint((y - q1) * 254.0), -127, 127)
    cq = np.zeros((2, 16, dq), dtype=np.int8)
    cq[0, :t, :d] = q1.astype(np.int8)
    cq[1, :t, :d] = q2.astype(np.int8)
    ct = cand_tilde(cq, sc, t)[:, :d]
    return cq, sc, np.sqrt(((C64 - ct) ** 2).sum(1)), (ct * ct).sum(1)


def cand_tilde(cq, sc, t):
    """fp64 [t, dq]: c~ = s_c (q1 + q2 / 254) from the int8 copy."""
    cq = np.asarray(cq).astype(np.float64)
    return np.asarray(sc, dtype=np.float64)[:t, None] * (cq[0, :t] + cq[1, :t] / 254.0)


def bound_lb64(xq, s, e, cq, sc, ec, t):
    """fp64 [t, n]: the certified lower bound (|x~ - c~| - e_i - ec_j)^2 on
    |x_i - c_j|^2 (0 where the bracket is not positive), from the given
    quantised data: x~ = s q, c~ = s_c (q1 + q2 / 254)."""
    xt = np.asarray(s, dtype=np.float64)[:, None] * np.asarray(xq).astype(np.float64)
    ct = cand_tilde(cq, sc, t)
    g = np.sqrt(dist2(xt, ct))
    r = g - np.asarray(e, dtype=np.float64)[None, :] - np.asarray(ec, dtype=np.float64)[:t, None]
    return np.where(r > 0.0, r * r, 0.0)
