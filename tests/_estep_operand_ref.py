"""Plain numpy reference of the two table producers of the certified E-step
(csrc/estep_f32.hip): ``sq_fast_centroids`` (Hamerly shifts, the nf fastest
centroids, ``smax_rest``, the Elkan table ``cc``) and ``sq_shift_operand``
(snapshot ring, fp16 shift operand, the per-centroid ``dq`` words).  Written
from the comments above those kernels, not from their bodies; nothing here
imports the code under test.

Inputs are the fp32 (fp64 for the shifts) arrays; all arithmetic is
``np.longdouble`` on the widened values (64-bit significand: asserted by
``test_estep_operand_ref_cpu.py``).  A difference of two fp32 values whose
exponents are at most 2^40 apart, and a sum of fewer than 2^16 squares of
such, are then exact or good to 2^-60 relative: "true" S_j, |S_j|, q_j and
|c_j - c_f| are far below every margin the GPU tests check (the smallest is
2^-24 relative).

Rank rule (fast_select_kernel's comment): rank(c) = #{j : s_j > s_c, or
s_j = s_c and j < c}; ``idx[rank] = c`` for rank < nf; ``smax_rest`` is the
shift of rank nf.

Shift operand (shift_operand_kernel's comment): for every valid ring slot s
of base b, S_j = c_j(t+1) - c_j(b) with c(b) from the reference's OWN
snapshot ring (slot ``snew`` takes C_prev and snapshots it); amax = max_f
|S_jf| lies in [2^(ex2-1), 2^ex2) and beta = 2^(14 - ex2) (1 when amax = 0);
the operand is float16(float32(beta S)); q_j = |c_j(t+1)|^2 - |c_j(b)|^2.

The module also builds the inputs of the GPU case matrix, so that the CPU
tests can check their preconditions (kept shares, exponent spreads) without
a device.  Everything returned from a cached builder is read-only.
"""
import functools
import types

import numpy as np

LD = np.longdouble
F32_EPS = LD(2.0) ** -24      # unit roundoff of fp32
DOWN = LD(1.0) - LD(2.0) ** -19   # the documented slack of a value "rounded down" / "up"
UP = LD(1.0) + LD(2.0) ** -19


def wide(a):
    """fp32 / fp64 array -> long double, exactly."""
    return np.asarray(a).astype(LD)


# --------------------------------------------------------------- fast centroids
def rank_order(s):
    """order[rank] = centroid: larger shift first, ties to the lower index."""
    s = [float(v) for v in np.asarray(s).ravel()]
    return np.array(sorted(range(len(s)), key=lambda j: (-s[j], j)), dtype=np.int64)


def rank_of(s):
    """rank[c] by the definition itself (counting), for the hand-worked cases."""
    s = np.asarray(s, dtype=np.float64)
    k = s.size
    return np.array([sum(1 for j in range(k) if s[j] > s[c] or (s[j] == s[c] and j < c))
                     for c in range(k)], dtype=np.int64)


def sqrt_true(shift_sq):
    """sqrt of the fp64 squared shifts, long double."""
    return np.sqrt(wide(shift_sq))


def cc_true(C, idx):
    """|c_j - c_idx[f]| [k][nf] in long double, +inf where j == idx[f]."""
    Cw = wide(np.asarray(C, dtype=np.float32))
    idx = np.asarray(idx, dtype=np.int64)
    k = Cw.shape[0]
    out = np.empty((k, idx.size), dtype=LD)
    for f, jf in enumerate(idx):
        e = Cw - Cw[jf][None, :]
        out[:, f] = np.sqrt((e * e).sum(1))
        out[jf, f] = np.inf
    return out


def fast_centroids_ref(shift, C, nf, shift_sq=None):
    """The documented outputs from the documented inputs: ``shift`` (fp64:
    sqrt(shift_sq) (1 + 1e-12) rounded to nearest when shift_sq is given, so
    the kernel's own value may differ in the last places - the tests rank the
    shifts the kernel wrote), ``idx``, ``smax_rest`` and the true ``cc``."""
    if shift_sq is not None:
        shift = (sqrt_true(shift_sq) * (LD(1.0) + LD(1e-12))).astype(np.float64)
    shift = np.asarray(shift, dtype=np.float64)
    order = rank_order(shift)
    idx = order[:nf]
    return types.SimpleNamespace(shift=shift, order=order, idx=idx,
                                 smax_rest=max(float(shift[order[nf]]), 0.0),
                                 cc=cc_true(C, idx))


# ---------------------------------------------------------------- shift operand
def engine_valid(t, ring, rlo):
    """The engine's rule (models/cluster/_lloyd.py) for the update c(t) ->
    c(t+1): slot t % ring is fresh, the valid bases are max(rlo, t + 2 - ring)
    .. t.  Returns (snew, bitmask, {slot: base})."""
    bases = {b % ring: b for b in range(max(rlo, t + 2 - ring), t + 1)}
    valid = 0
    for s in bases:
        valid |= 1 << s
    return t % ring, valid, bases


def exponent_spread_wide(a, b, limit=29):
    """Per coordinate: a_f and b_f are nonzero fp32 values whose exponents are
    more than ``limit`` apart, so b_f - a_f need not be exact in fp64."""
    ea = np.frexp(np.asarray(a, dtype=np.float64))[1]
    eb = np.frexp(np.asarray(b, dtype=np.float64))[1]
    return (np.abs(ea - eb) > limit) & (np.asarray(a) != 0) & (np.asarray(b) != 0)


def exponent_spread_ok(a, b, limit=29):
    """Per row: b_f - a_f is exact in fp64 for every coordinate."""
    return ~exponent_spread_wide(a, b, limit).any(-1)


class ShiftOperandRef:
    """The operation with its own snapshot ring.  ``update`` returns, per
    valid slot, the true quantities and the exactly defined outputs."""

    def __init__(self, k, d, d_pad, ring, alpha):
        self.k, self.d, self.d_pad, self.ring, self.alpha = k, d, d_pad, ring, alpha
        self.snap = {}      # slot -> float32 [k][d_pad], zero-padded

    def update(self, C_prev, C_new, snew, valid):
        k, d, dp = self.k, self.d, self.d_pad
        pad = lambda C: np.concatenate(                                   # noqa: E731
            [np.asarray(C, dtype=np.float32), np.zeros((k, dp - d), np.float32)], axis=1)
        new = pad(C_new)
        out = {}
        for s in range(self.ring):
            if not (valid >> s) & 1:
                continue
            if s == snew:
                self.snap[s] = pad(C_prev)
            old = self.snap[s]
            a, b = wide(old), wide(new)
            S = b - a
            amax = np.abs(S).max(1)
            ex2 = np.frexp(amax)[1].astype(np.int64)      # amax in [2^(ex2-1), 2^ex2)
            lb = np.where(amax > 0, 14 - ex2, 0)
            beta = np.ldexp(LD(1.0), lb)
            out[s] = types.SimpleNamespace(
                S=S, amax=amax, log2_beta=lb, beta=beta,
                inv=(LD(1.0) / (LD(self.alpha) * beta)).astype(np.float32),
                dsh=(beta[:, None] * S).astype(np.float32).astype(np.float16),
                q=((b - a) * (b + a)).sum(1), nrm=(b * b + a * a).sum(1),
                norm=np.sqrt((S * S).sum(1)), in_range=exponent_spread_ok(old, new),
                # |S| over the coordinates whose fp64 difference may be inexact
                wild_norm=np.sqrt((S * S * exponent_spread_wide(old, new)).sum(1)))
        if snew not in out:     # the fresh slot is always among the engine's valid ones
            raise ValueError("snew is not a valid slot")
        return out


def operand_error(S, dsh, beta):
    """e_j = |S_j - S~_j / beta_j| for a given fp16 operand, long double."""
    r = S - wide(dsh) / beta[:, None]
    return np.sqrt((r * r).sum(1))


# ------------------------------------------- inputs of the GPU case matrix (A)
SHIFT_PATTERNS = ("random", "dup_at_nf", "all_equal", "all_zero", "one_zero")
CENTRE_PATTERNS = ("random", "identical_pair", "offset_1e4")


def shift_sq_pattern(name, k, nf, seed=0):
    """fp64 squared shifts [k].  dup_at_nf: the values of ranks nf-1, nf and
    nf+1 (where they exist) are one duplicated value, spread over the index
    range, so the tie decides both idx[nf-1] and smax_rest."""
    rs = np.random.RandomState(1000 + 17 * k + nf + seed)
    s = rs.uniform(0.01, 2.0, k) ** 2
    if name == "random":
        pass
    elif name == "dup_at_nf":
        order = rank_order(s)
        lo, hi = max(nf - 1, 0), min(nf + 1, k - 1)
        s[order[lo:hi + 1]] = s[order[nf]]
    elif name == "all_equal":
        s[:] = 0.37
    elif name == "all_zero":
        s[:] = 0.0
    elif name == "one_zero":
        s[rs.randint(k)] = 0.0
    else:
        raise KeyError(name)
    return s


def centre_pattern(name, k, d, fast, seed=0):
    """fp32 centres [k][d].  identical_pair: a slow centroid is a bit copy of
    the fast centroid ``fast`` (None when nf = 0: of centroid 0).  offset_1e4:
    every coordinate at 1e4 but one or two, which are one fp32 ulp of 1e4
    (2^-10 ~ 1e-3) off: mutual distances 0 .. 3e-3."""
    rs = np.random.RandomState(2000 + 31 * k + d + seed)
    if name == "offset_1e4":
        C = np.full((k, d), 1e4, np.float32)
        for j in range(k):      # one or two coordinates off by an ulp of 1e4 (2^-10)
            f = rs.permutation(d)[:2]
            C[j, f] += (rs.choice([-1, 1], f.size) * 2.0 ** -10).astype(np.float32)
    else:
        C = rs.randn(k, d).astype(np.float32)
    if name == "identical_pair" and k >= 2:
        src = 0 if fast is None else int(fast)
        C[(src + 1) % k] = C[src]
    return C


# ------------------------------------------- inputs of the GPU case matrix (B)
STILL, ULP, POW2, BELOW, CANCEL, WILD = range(6)
KIND_NAMES = ("still", "one ulp", "amax 2^m (+ tiny coordinates)", "amax below 2^m",
              "small shift (1e-3 at offset 1e4)", "exponent spread 2^35")
T0, N_UPDATES, RLO_JUMP_AT = 5, 6, 8


def _exact_step(a, mag, sign):
    """fp32 b with b - a == sign * mag exactly (mag a power of two), or None."""
    b = np.float32(np.float64(a) + sign * mag)
    return b if LD(b) - LD(a) == LD(sign * mag) else None


@functools.lru_cache(maxsize=None)
def operand_sequence(k, d, seed=0):
    """Centres c(T0) .. c(T0 + N_UPDATES) (fp32 [k][d] each) and the kind of
    every (update, centroid).  Centroid j of update u takes kind (j + u) % 6, so
    every kind occurs in every sequence, for k = 1 too.  Even centroids live at
    offset 1e4 on the lattice 2^-9 Z (there one fp32 ulp is 2^-10 ~ 1e-3, and
    q_j cancels heavily), odd ones on 2^-14 Z within +-4.  With d >= 4 the last
    three coordinates are 'quiet': touched by the POW2 kind only, which moves
    the last two by 2^-30 and 2^-42 of amax (fp16 images: subnormal, and zero)
    and takes the third from -2^-40 to 2^-16 (1 + 2^-11): with amax = 2^-3
    (beta = 2^16) beta S = 1 + 2^-11 + 2^-24 there, which fp32 rounds to the
    fp16 tie 1 + 2^-11 and fp16 to 1, where one rounding gives 1 + 2^-10.

    STILL: no change.  ULP: coordinate 0 one fp32 ulp up.  POW2: coordinate 0
    by exactly +-2^m, the others by less.  BELOW: coordinate 0 by 2^m less one
    ulp of the new value.  CANCEL: every coordinate by a few lattice steps.
    WILD: one coordinate from order one to order 2^-35 (beyond the fp64-exact
    range; with d >= 2 coordinate 0 also moves by an odd multiple of 2^-14 of
    at least 1/8, whose fp16 image is off by 2^-15 of amax or more)."""
    rs = np.random.RandomState(3000 + 101 * k + d + seed)
    offset = (np.arange(k) % 2 == 0)
    nq = 3 if d >= 4 else 0                       # quiet coordinates
    body = d - nq
    C = np.zeros((k, d), np.float64)
    if nq:
        C[:, d - 3] = -2.0 ** -40
    C[:, :body] = np.where(offset[:, None], 1e4 + rs.randint(-64, 65, (k, body)) * 2.0 ** -9,
                           rs.randint(-2 ** 15, 2 ** 15 + 1, (k, body)) * 2.0 ** -14)
    # coordinate 0 is kept away from zero (the exact +-2^m steps move toward it)
    C[~offset, 0] = np.where(C[~offset, 0] >= 0, 1.0, -1.0) * (1.0 + np.abs(C[~offset, 0]) / 4)
    cur = C.astype(np.float32)
    assert (cur == C).all()
    seq, kinds = [cur.copy()], np.zeros((N_UPDATES, k), np.int64)
    for u in range(N_UPDATES):
        new = cur.copy()
        for j in range(k):
            kind = (j + u) % 6
            kinds[u, j] = kind
            lat = 2.0 ** -9 if offset[j] else 2.0 ** -14
            a0 = cur[j, 0]
            if kind == ULP:
                new[j, 0] = np.nextafter(a0, np.float32(np.inf))
            elif kind in (POW2, BELOW):
                m = -3
                b = None
                for sign in (-np.sign(a0) or 1.0, np.sign(a0) or 1.0):
                    b = _exact_step(a0, 2.0 ** m, sign)
                    if b is not None:
                        break
                if b is None:     # a0 has bits far below 2^m (after WILD at d = 1)
                    b = np.float32(np.float64(a0) + 2.0 ** m)
                if kind == BELOW:
                    b = np.nextafter(b, np.float32(a0))
                new[j, 0] = b
                if body > 1:      # the rest well below amax: |step| <= 2^-5
                    st = rs.randint(-8, 9, body - 1) * (lat if offset[j] else 2.0 ** -8)
                    st[np.abs(cur[j, 1:body]) < 2.0 ** -18] = 0     # what WILD left tiny stays
                    new[j, 1:body] = (cur[j, 1:body].astype(np.float64) + st).astype(np.float32)
                if kind == POW2 and nq:
                    new[j, d - 1] = np.float32(np.float64(cur[j, d - 1]) + 2.0 ** (m - 30))
                    new[j, d - 2] = np.float32(np.float64(cur[j, d - 2]) + 2.0 ** (m - 42))
                    if cur[j, d - 3] == np.float32(-2.0 ** -40):
                        new[j, d - 3] = np.float32(2.0 ** -16 * (1 + 2.0 ** -11))
            elif kind == CANCEL:
                st = rs.choice([-2, -1, 1, 2], body) * lat * (1 if offset[j] else 16)
                if body > 1:
                    st[np.abs(cur[j, :body]) < 2.0 ** -18] = 0
                new[j, :body] = (cur[j, :body].astype(np.float64) + st).astype(np.float32)
            elif kind == WILD:
                f = 1 if body > 1 else 0
                a = np.float64(cur[j, f])
                if abs(a) < 2.0 ** -18:      # already tiny: back to order one
                    new[j, f] = np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
                else:                        # 2^35 below its own exponent
                    new[j, f] = np.float32(np.ldexp(1.0 + 2.0 ** -22, int(np.frexp(a)[1]) - 36)
                                           * np.sign(a))
                if f == 1:
                    odd = (2 * rs.randint(2 ** 10, 2 ** 11) + 1) * 2.0 ** -14   # in [1/8, 1/4)
                    odd = odd if not offset[j] else np.round(odd * 2 ** 9) * 2.0 ** -9 + 2.0 ** -9
                    new[j, 0] = np.float32(np.float64(a0) - (np.sign(a0) or 1.0) * odd)
        cur = new
        seq.append(cur.copy())
    for c in seq:
        c.setflags(write=False)
    kinds.setflags(write=False)
    return tuple(seq), kinds


def strided_pair(C_prev, C_new, ldc):
    """C_prev and C_new as column slices [:, :d] of wider buffers (ldc > d)
    filled with a sentinel the kernel must not read as data."""
    k, d = C_prev.shape
    A = np.full((k, ldc), 7.5e7, np.float32)
    B = np.full((k, ldc), -7.5e7, np.float32)
    A[:, :d], B[:, :d] = C_prev, C_new
    return A, B


# --------------------------------------------- inputs of the chains (section C)
def _round_up32(v):
    f = np.asarray(v).astype(np.float32)
    return np.where(wide(f) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def _round_down32(v):
    f = np.asarray(v).astype(np.float32)
    return np.where(wide(f) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def sq_dists(X, C, chunk=512):
    """|x_i - c_j|^2 [n][k] in long double from the fp32 arrays."""
    Xw, Cw = wide(np.asarray(X, np.float32)), wide(np.asarray(C, np.float32))
    out = np.empty((Xw.shape[0], Cw.shape[0]), dtype=LD)
    for s in range(0, Xw.shape[0], chunk):
        e = Xw[s:s + chunk, None, :] - Cw[None, :, :]
        out[s:s + chunk] = (e * e).sum(-1)
    return out


FILTER_CASES = {
    # name: (d, centre scale, delta, fast-centroid shift scale)
    "d8": (8, 4.0, 40.0, 1.0),
    "d64": (64, 2.0, 300.0, 0.15),
}
FILTER_N, FILTER_K, FILTER_FAST = 4096, 40, 6


@functools.lru_cache(maxsize=None)
def filter_geometry(case):
    """Real geometry for the filter chain: fp32 X, C_old, C_new; labels = the
    exact argmin under C_old; ub = the exact label distance rounded up to fp32,
    lb = the exact nearest-other distance rounded down; the exact squared
    shifts rounded to fp64; the exact squared distances under C_new."""
    d, cscale, delta, fscale = FILTER_CASES[case]
    n, k = FILTER_N, FILTER_K
    rs = np.random.RandomState(0)
    centres = cscale * rs.randn(k, d)
    X = (centres[rs.randint(k, size=n)] + 0.7 * rs.randn(n, d)).astype(np.float32)
    C_old = (centres + 0.05 * rs.randn(k, d)).astype(np.float32)
    sh = 0.002 * rs.randn(k, d)
    fast = rs.permutation(k)[:FILTER_FAST]
    sh[fast] = fscale * rs.randn(FILTER_FAST, d)
    C_new = (C_old.astype(np.float64) + sh).astype(np.float32)
    D0 = sq_dists(X, C_old)
    labels = D0.argmin(1)
    ar = np.arange(n)
    d_lab = np.sqrt(D0[ar, labels])
    other = D0.copy()
    other[ar, labels] = np.inf
    d_oth = np.sqrt(other.min(1))
    e = wide(C_new) - wide(C_old)
    g = types.SimpleNamespace(
        X=X, C_old=C_old, C_new=C_new, labels=labels.astype(np.int32), ub=_round_up32(d_lab),
        lb=_round_down32(d_oth), shift_sq=(e * e).sum(1).astype(np.float64), delta=delta,
        D_new=sq_dists(X, C_new), n=n, k=k, d=d)
    for v in vars(g).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


def filter_rule_ref(g, nf):
    """The documented rule of the bounds filter on the REFERENCE's tables (long
    double; cc at the low end of its documented interval): which rows hold.
    u = ub + s_label; w = min(lb - smax_rest, min_f max(cc[l][f] - u, lb -
    s_f)); holds: w > 0 and w^2 - u^2 > delta."""
    r = fast_centroids_ref(None, g.C_new, nf, shift_sq=g.shift_sq)
    s = wide(r.shift)
    u = wide(g.ub) + s[g.labels]
    lb = wide(g.lb)
    w = lb - LD(r.smax_rest)
    if nf:
        cc = np.where(np.isinf(r.cc), r.cc, r.cc * DOWN - LD(2e-30))[g.labels]
        w = np.minimum(w, np.maximum(cc - u[:, None], lb[:, None] - s[r.idx][None, :]).min(1))
    return (w > 0) & (w * w - u * u > LD(g.delta) * (LD(1.0) + LD(1e-9)) + LD(1e-30))


def filter_unsound_rows(g, held, ub_new=None, lb_new=None):
    """Rows of ``held`` (bool [n]) that break the filter's promise under C_new:
    another centroid within delta of the label's squared distance, or (given
    the rewritten bounds) ub below the label distance / lb above the nearest
    other.  Returns three index arrays."""
    ar = np.arange(g.n)
    dl = g.D_new[ar, g.labels]
    other = g.D_new.copy()
    other[ar, g.labels] = np.inf
    do = other.min(1)
    band = held & ~(do - dl > LD(g.delta))
    if ub_new is None:
        return np.flatnonzero(band), np.zeros(0, np.int64), np.zeros(0, np.int64)
    bad_ub = held & ~(wide(ub_new) >= np.sqrt(dl))
    bad_lb = held & ~(wide(lb_new) <= np.sqrt(do))
    return np.flatnonzero(band), np.flatnonzero(bad_ub), np.flatnonzero(bad_lb)


GAP_N, GAP_K, GAP_RING, GAP_T0, GAP_DELTA = 4096, 40, 3, 2, 4.0
GAP_DIMS = {128: 120, 256: 256}     # d_pad -> d


@functools.lru_cache(maxsize=None)
def gap_geometry(d_pad):
    """Real geometry for the gap-screen chain: centres c(2) .. c(5) (three
    updates), fp32 rows between 2 - 4 near centres, and per row a record at a
    base b in {3, 4} (the bases valid after the third update with a ring of 3):
    da, the gaps to the c_r - 1 other nearest centres, err covering the fp32
    rounding of those words (2^-22 of the largest), in the word layout of
    test_gap_screen_dots_gpu.py."""
    d, n, k = GAP_DIMS[d_pad], GAP_N, GAP_K
    rs = np.random.RandomState(500 + d_pad)
    scale = 6.0 / np.sqrt(d)
    C = [(scale * rs.randn(k, d)).astype(np.float32)]
    for _ in range(3):
        C.append((C[-1].astype(np.float64) + 0.03 * scale * rs.randn(k, d)).astype(np.float32))
    # a row: a random mix of 2 - 4 centres + noise
    c_r = rs.randint(2, 5, size=n)
    pick = np.stack([rs.permutation(k)[:4] for _ in range(n)])
    wgt = rs.dirichlet(np.ones(4) * 0.6, size=n) * (np.arange(4)[None, :] < c_r[:, None])
    wgt /= wgt.sum(1, keepdims=True)
    tie = rs.rand(n) < 0.25                      # a quarter near a bisector: small gaps
    wgt[tie, :2] = wgt[tie, :2].mean(1)[:, None]
    X = ((wgt[:, :, None] * C[2].astype(np.float64)[pick]).sum(1)
         + 0.25 * scale * rs.randn(n, d)).astype(np.float32)
    base = 3 + rs.randint(0, 2, size=n)
    Dn = sq_dists(X, C[3])
    D = {3: sq_dists(X, C[1]), 4: sq_dists(X, C[2])}
    rec = np.zeros((n, 8), np.float32)
    ids = rec.view(np.uint32)
    jc = np.zeros((n, 4), np.int64)
    slot = np.zeros(n, np.int64)
    for b in (3, 4):
        rows = np.flatnonzero(base == b)
        near = np.argsort(D[b][rows], axis=1)[:, :4]          # nearest first
        # the argmin's position among the candidates varies
        sl = rs.randint(0, 1 << 16, size=rows.size) % c_r[rows]
        cand = near.copy()
        cand[np.arange(rows.size), 0], cand[np.arange(rows.size), sl] = \
            near[np.arange(rows.size), sl], near[np.arange(rows.size), 0]
        past = np.arange(4)[None, :] >= c_r[rows][:, None]
        cand = np.where(past, cand[:, :1], cand)
        dd = D[b][rows[:, None], cand]
        da = dd[np.arange(rows.size), sl]
        gaps = np.where(past, LD(0), dd - da[:, None])
        rec[rows, 0] = da.astype(np.float32)
        rec[rows, 2:6] = gaps.astype(np.float32)
        rec[rows, 1] = _round_up32(LD(2.0) ** -22 * (da + np.abs(gaps).max(1)))
        jc[rows], slot[rows] = cand, sl
    ids[:, 6] = (jc[:, 0] | slot << 14 | jc[:, 1] << 16 | (c_r - 1) << 30).astype(np.uint32)
    ids[:, 7] = (jc[:, 2] | jc[:, 3] << 16).astype(np.uint32)
    g = types.SimpleNamespace(C=tuple(C), X=X, base=base, c_r=c_r, jc=jc, slot=slot, rec=rec,
                              labels=jc[np.arange(n), slot].astype(np.int32),
                              D_new=Dn, n=n, k=k, d=d, d_pad=d_pad)
    for v in vars(g).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


def gap_true_margin(g):
    """Per row, under the newest centres: (argmin position among the
    candidates, min over the other candidates of D_c - D_argmin)."""
    ar = np.arange(g.n)
    inr = np.arange(4)[None, :] < g.c_r[:, None]
    dd = np.where(inr, g.D_new[ar[:, None], g.jc], np.inf)
    m = dd.argmin(1)
    rest = dd.copy()
    rest[ar, m] = np.inf
    return m, rest.min(1) - dd[ar, m]
