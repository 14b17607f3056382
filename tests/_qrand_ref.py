"""Plain numpy references of the sampling layer (csrc/qrand.hip, csrc/fejer.h),
written from the published Philox4x32-10 definition and the closed form of the
Fejer law, not from the kernels or their torch twins.  fp64 and Python ints
only; nothing here imports the code under test.

Counter layouts (key = (k0, k1), stream = (s0, s1)):

* ``word(e)``: word ``e & 3`` of the block with counter ``(e>>2 lo, e>>2 hi, s0, s1)``;
* the normal of element ``e`` uses words 0, 1 of block ``e >> 1`` (Box-Muller,
  even element -> cos, odd -> sin);
* word ``w`` of the stream of sample ``s``: word ``w & 3`` of the block with counter
  ``(s lo, (s hi & 0xFFFF) | (w >> 2) << 16, s0, s1)``.

Uniforms.  ``u01(w) = ((w >> 8) + 0.5) / 2^24`` is exact in fp64.  An fp32
kernel cannot hold it once ``w >> 8 >= 2^23`` (25 significant bits): k + 0.5 is
a tie and rounds to the even neighbour, so half of the fp32 uniforms are off by
2^-25 and the largest one is 1.0.  ``u01_f32`` is that rounding.  The uniform
kernel is pinned to it bit for bit; the normal and truncated-normal references
are fp64 evaluations of the transform AT the fp32 uniform, because the
sensitivity of either transform to its uniform, 1 / (u r) resp.
sqrt(pi/2) exp(z^2/2), has no bound as u -> 1 and would swamp the fp32 budget
of the transform itself.

The walk margin DELTA.  The kernel walks l = 0, +1, -1, ..., -16 in fp32 and
stops at the first cumulative mass >= u.  With eps = 2^-24, fast sines and
cosines taken as good to 2 ulp (4 eps), and p_l the mass of offset l:

* numerator sin^2(pi phi) / M^2: 3 eps (rounded sine, squared) + 1 (1 / M^2)
  + 1 (product); a term adds 2 e(sine) + 1 (square) + 1 (division):
  K_l = 7 + 2 e_l;
* l = 0, and l = +1 when phi > 1/2 (own angle): e = 1 (angle) + 4 = 5, K = 17;
* recurrence: e(sin t alpha) <= 5 + 7 (t - 1), |err cos t alpha| <= 6 t;
* l = +-t by angle addition: e <= [t (e(sin t alpha) + 5) +
  phi (6 t + 6)] / |t -+ phi| + 1: the (t + phi) / (t - phi) <= 3 blow-up of
  the subtraction (l = +1 is only taken this way for phi <= 1/2);
* 33 additions of a sum <= 1: 33 eps; u rounded to fp32: eps / 2.

``walk_delta`` evaluates sum_l p_l K_l eps + 33.5 eps over a grid of phases
and M; its supremum is below 90 eps, so DELTA = 96 eps = 5.73e-6: a walk draw
whose fp64 uniform lies farther than DELTA from every fp64 boundary must land
on the reference bin, one within DELTA may land on either side.  The small-M
and the tail branch are fp64 on the device; their margin TIGHT = 1e-12 is
relative to the compared quantities.
"""
import functools
import math

import numpy as np

M0 = 0xD2511F53
M1 = 0xCD9E8D57
W0 = 0x9E3779B9
W1 = 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1

WALK = 16
SMALL_M = 2 * WALK + 4
EPS32 = 2.0 ** -24
DELTA = 96 * EPS32
TIGHT = 1e-12

EXACT, SMALL, WALKED, TAIL = 0, 1, 2, 3

# walk order 0, +1, -1, ..., +16, -16
WALK_OFFS = np.array([0] + [s * t for t in range(1, WALK + 1) for s in (1, -1)], dtype=np.int64)


# ------------------------------------------------------------------ Philox
def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds on Python ints: (4 counter words, 2 key
    words) -> 4 words (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in ctr)
    k0, k1 = (int(k) & MASK32 for k in key)
    for r in range(10):
        if r:
            k0 = (k0 + W0) & MASK32
            k1 = (k1 + W1) & MASK32
        p0 = M0 * c0
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
    return c0, c1, c2, c3


def philox_blocks(c0, c1, c2, c3, k0, k1):
    """The same on uint64 arrays (each holding a uint32): uint64 [n, 4]."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))
    m = np.uint64(MASK32)
    sh = np.uint64(32)
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    for r in range(10):
        if r:
            k0 = (k0 + W0) & MASK32
            k1 = (k1 + W1) & MASK32
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & m
    return np.stack([c0, c1, c2, c3], axis=-1)


def _ids(offset, n):
    """uint64 ids offset .. offset + n - 1 modulo 2^64."""
    return np.uint64(int(offset) & MASK64) + np.arange(n, dtype=np.uint64)


def _blocks_of(key, idx):
    k0, k1, s0, s1 = key
    return philox_blocks(idx & np.uint64(MASK32), idx >> np.uint64(32), s0, s1, k0, k1)


def flat_words(key, offset, n):
    """word(e) of the flat elements e = offset .. offset + n - 1."""
    e = _ids(offset, n)
    blk = _blocks_of(key, e >> np.uint64(2))
    return blk[np.arange(n), (e & np.uint64(3)).astype(np.int64)]


def u01(w):
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0


def u01_f32(w):
    """u01 as an fp32 kernel holds it (round to nearest even), as fp64."""
    return u01(w).astype(np.float32).astype(np.float64)


class SampleWords:
    """Word streams of the samples ``ids`` (uint64 array): ``u(w)`` is the
    fp64 uniform of word ``w`` of every sample."""

    def __init__(self, key, ids):
        self.key = key
        self.ids = np.asarray(ids, dtype=np.uint64)
        self._blk = {}

    def words(self, w, sel=None):
        b = w >> 2
        if b not in self._blk:
            k0, k1, s0, s1 = self.key
            lo = self.ids & np.uint64(MASK32)
            hi = ((self.ids >> np.uint64(32)) & np.uint64(0xFFFF)) | np.uint64(b << 16)
            self._blk[b] = philox_blocks(lo, hi, s0, s1, k0, k1)
        col = self._blk[b][:, w & 3]
        return col if sel is None else col[sel]

    def u(self, w, sel=None):
        return u01(self.words(w, sel))


# ------------------------------------------------------------------ normal
@functools.lru_cache(maxsize=8)
def normal_ref(key, offset, n, mean=0.0, std=1.0, exact_u=False):
    """(value, r, u1): fp64 Box-Muller of the fp32 uniforms of block e >> 1
    (of the exact uniforms with ``exact_u``).  Cached: do not write to it.

    The quarter turns are taken off u2 before the angle is formed (u2 - q/4
    is exact in fp64), so the value keeps its relative precision next to a
    zero of the cosine or sine, and is 0 where u2 is a whole quarter turn
    (0.5, 0.75 and 1.0 are fp32 uniforms)."""
    e = _ids(offset, n)
    blk = _blocks_of(key, e >> np.uint64(1))
    uf = u01 if exact_u else u01_f32
    u1, u2 = uf(blk[:, 0]), uf(blk[:, 1])
    r = np.sqrt(-2.0 * np.log(u1))
    q = np.rint(4.0 * u2)
    ang = 2.0 * np.pi * (u2 - 0.25 * q)
    sd, cd = np.sin(ang), np.cos(ang)
    q = q.astype(np.int64) & 3
    c = np.choose(q, [cd, -sd, -cd, sd])
    s = np.choose(q, [sd, cd, -sd, -cd])
    z = np.where((e & np.uint64(1)) == 0, r * c, r * s)
    return mean + std * z, r, u1


def normal_tol(value, r, std):
    """fp32 budget of ``mean + std z``.  The angle 2 pi u2 < 8 is rounded to
    fp32 (half an ulp = 2 * 2^-23 at most) from a rounded 2 pi (1.5 * 2^-23 at
    the far end), both scaled by r; sine/cosine, the logarithm, the square
    root and the product each add about an ulp of a factor <= 1 or of r.  The
    starting budget is 4 * 2^-23 (1 + r) std; the last fp32 rounding of the
    result (and of std z + mean, one fma) adds 2^-24 |value|."""
    return 4 * 2.0 ** -23 * (1.0 + r) * abs(std) + EPS32 * np.abs(value)


def bf16_rne(v):
    """(nearest bf16 of fp64 v, ties to even, as fp64; one bf16 ulp at v)."""
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(v)                      # v = m 2^e, 0.5 <= |m| < 1
    q = np.ldexp(np.rint(np.ldexp(m, 8)), e - 8)
    return q, np.ldexp(1.0, e - 8)


# ------------------------------------------------------------------ truncated normal
def erf(x):
    """erf on fp64 arrays, |x| <= 6: 2/sqrt(pi) e^{-x^2} sum 2^n x^(2n+1)/(2n+1)!!
    (all terms of one sign, no cancellation)."""
    x = np.asarray(x, dtype=np.float64)
    x2 = x * x
    term = x.copy()
    tot = x.copy()
    for n in range(1, 400):
        term = term * (2.0 * x2 / (2 * n + 1))
        tot = tot + term
        if np.all(np.abs(term) <= 1e-18 * np.abs(tot)):
            break
    return 2.0 / math.sqrt(math.pi) * np.exp(-x2) * tot


def erfinv(p):
    """erfinv on fp64 arrays, |p| < 1 - 2^-30: Winitzki's start, Newton on erf."""
    p = np.asarray(p, dtype=np.float64)
    a = 0.147
    ln = np.log1p(-p * p)
    t = 2.0 / (math.pi * a) + ln / 2.0
    x = np.sign(p) * np.sqrt(np.sqrt(t * t - ln / a) - t)
    for _ in range(8):
        d = (erf(x) - p) * (math.sqrt(math.pi) / 2.0) * np.exp(x * x)
        x = x - d
        if np.all(np.abs(d) <= 1e-15 * np.maximum(np.abs(x), 1e-300)):
            break
    return x


def trunc_normal_ref(key, offset, n, b, exact_u=False):
    """sqrt(2) erfinv((2u - 1) erf(b / sqrt 2)) clamped to [-b, b], fp64, at
    the fp32 uniform of word(e) (at the exact one with ``exact_u``).  u = 1.0
    (the largest fp32 uniform) is b."""
    u = (u01 if exact_u else u01_f32)(flat_words(key, offset, n))
    eb = math.erf(b / math.sqrt(2.0))
    p = (2.0 * u - 1.0) * eb
    top = u >= 1.0
    z = math.sqrt(2.0) * erfinv(np.where(top, 0.0, p))
    z = np.where(top, b, z)
    return np.clip(z, -b, b)


# ------------------------------------------------------------------ Fejer law
def ae_bins(eps):
    eps = np.asarray(eps, dtype=np.float64)
    return np.ceil((np.pi / (2.0 * eps)) * (1.0 + np.sqrt(1.0 + 4.0 * eps))).astype(np.int64)


def eps_for_bins(M):
    """An eps with ae_bins(eps) == M, half a bin clear of either neighbour."""
    lo, hi = 1e-9, 10.0
    f = lambda e: (math.pi / (2.0 * e)) * (1.0 + math.sqrt(1.0 + 4.0 * e))
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        if f(mid) > M - 0.5:
            lo = mid
        else:
            hi = mid
    assert int(ae_bins(lo)) == M and abs(f(lo) - (M - 0.5)) < 0.01
    return lo


def ae_omega(a, M):
    return np.asarray(M, dtype=np.float64) * np.arcsin(np.sqrt(np.clip(a, 0.0, 1.0))) / np.pi


def ae_value(j, M):
    return np.sin(np.pi * np.asarray(j, dtype=np.float64) / np.asarray(M, dtype=np.float64)) ** 2


def _masses(phi, Md, offs):
    """P(l) = sin^2(pi phi) / (M^2 sin^2(pi (l - phi) / M)), fp64, with the
    numerator and l = +1 taken from 1 - phi (exact) above 1/2."""
    phi = np.asarray(phi, dtype=np.float64)[..., None]
    Md = np.asarray(Md, dtype=np.float64)[..., None]
    offs = np.asarray(offs, dtype=np.float64)
    near = np.where(phi > 0.5, 1.0 - phi, phi)
    num = np.sin(np.pi * near) ** 2
    x = np.where((offs == 1.0) & (phi > 0.5), 1.0 - phi, offs - phi)
    return num / (Md * Md * np.sin(np.pi * x / Md) ** 2)


def fejer_walk_cdf(omega, M):
    """fp64 cumulative mass over l = 0, +1, -1, ..., +-16: [..., 33]."""
    omega = np.asarray(omega, dtype=np.float64)
    phi = omega - np.floor(omega)
    return np.cumsum(_masses(phi, M, WALK_OFFS), axis=-1)


def walk_delta():
    """Supremum of the fp32 error bound of the walk's cumulative mass (module
    docstring), over a grid of phases and M, in units of 1."""
    worst = 0.0
    phi = np.concatenate([np.linspace(1e-6, 1 - 1e-6, 4001), [0.5, np.nextafter(0.5, 1)],
                          10.0 ** -np.arange(2, 13), 1 - 10.0 ** -np.arange(2, 13)])
    for M in (37, 41, 64, 128, 1000, 314160, 2 ** 20, 2 ** 30, 2 ** 40):
        p = _masses(phi, np.full_like(phi, M), WALK_OFFS)
        K = np.empty_like(p)
        K[:, 0] = 17.0
        for t in range(1, WALK + 1):
            es = 5.0 + 7.0 * (t - 1)
            top = t * (es + 5.0) + phi * (6.0 * t + 6.0)
            ep = top / (t - phi) + 1.0
            if t == 1:
                ep = np.where(phi > 0.5, 5.0, ep)
            K[:, 2 * t - 1] = 7.0 + 2.0 * ep
            K[:, 2 * t] = 7.0 + 2.0 * (top / (t + phi) + 1.0)
        worst = max(worst, float(((p * K).sum(1) + 33.5).max()))
    return worst * EPS32


def fejer_bin(omega, M, words):
    """Bins of one draw per element.  ``omega``, ``M``: arrays [n]; ``words``:
    a SampleWords over the n sample ids.  Returns a dict of arrays [n]:

    * ``bin``: the sampled bin in [0, M);
    * ``branch``: EXACT (phi = 0), SMALL (M <= 36: inverse CDF over the whole
      period), WALKED (first walk offset whose cumulative mass >= u), TAIL
      (rejection with the telescoping proposal);
    * ``ell``: the offset from floor(omega) (0 where SMALL);
    * ``margin``: distance from the uniform(s) to the nearest decision
      boundary (walk: absolute, in cumulative mass; small / tail: relative);
    * ``edge``: the walk boundary nearest to u (k: between walk positions k
      and k + 1; 32: between l = -16 and the tail), -1 elsewhere.
    """
    omega = np.asarray(omega, dtype=np.float64)
    M = np.asarray(M, dtype=np.int64)
    n = omega.shape[0]
    Md = M.astype(np.float64)
    fl = np.floor(omega)
    phi = omega - fl
    base = fl.astype(np.int64)
    out = np.zeros(n, dtype=np.int64)
    ell = np.zeros(n, dtype=np.int64)
    branch = np.full(n, EXACT, dtype=np.int64)
    margin = np.full(n, np.inf)
    edge = np.full(n, -1, dtype=np.int64)

    exact = phi == 0.0
    out[exact] = np.mod(base[exact], M[exact])
    small = ~exact & (M <= SMALL_M)
    big = ~exact & (M > SMALL_M)

    for i in np.nonzero(small)[0]:
        Mi = int(M[i])
        j = np.arange(Mi, dtype=np.float64)
        sn = np.sin(np.pi * (j - omega[i]) / Mi)
        near = 1.0 - phi[i] if phi[i] > 0.5 else phi[i]
        with np.errstate(divide="ignore"):
            p = np.where(sn == 0.0, 1.0, np.sin(np.pi * near) ** 2 / (Mi * Mi * sn * sn))
        cdf = np.cumsum(p)
        u = float(words.u(0, np.array([i]))[0]) * cdf[-1]
        k = int(np.searchsorted(cdf, u, side="left"))      # first cdf >= u
        out[i] = min(k, Mi - 1)
        branch[i] = SMALL
        margin[i] = np.min(np.abs(cdf[:-1] - u)) / cdf[-1] if Mi > 1 else np.inf

    idx = np.nonzero(big)[0]
    if idx.size:
        cdf = np.cumsum(_masses(phi[idx], Md[idx], WALK_OFFS), axis=-1)
        u = words.u(0, idx)
        k = (cdf < u[:, None]).sum(1)
        d = np.abs(cdf - u[:, None])
        edge[idx] = d.argmin(1)
        margin[idx] = d.min(1)
        branch[idx] = np.where(k < WALK_OFFS.size, WALKED, TAIL)
        ell[idx] = WALK_OFFS[np.minimum(k, WALK_OFFS.size - 1)]
        t = idx[k >= WALK_OFFS.size]
        if t.size:
            ell[t], tm = _tail(phi[t], Md[t], words, t)
            margin[t] = np.minimum(margin[t], tm)
        out[idx] = np.mod(base[idx] + ell[idx], M[idx])
    return dict(bin=out, branch=branch, ell=ell, margin=margin, edge=edge)


def _tail(phi, Md, words, sel):
    """Offsets with |l| > 16 (fejer.h, top): proposal q(z) = 1/(z - 1/2) -
    1/(z + 1/2) over z = l - phi (right) or phi - l (left), accepted with
    4 (z^2 - 1/4) / (M^2 sin^2(pi z / M)); words 1 + 3 it .. 3 + 3 it of the
    sample choose the side, the proposal and the acceptance of round it."""
    n = phi.shape[0]
    res = np.zeros(n, dtype=np.int64)
    marg = np.full(n, np.inf)
    lR = np.floor(phi + Md / 2.0)
    lL = lR - Md + 1.0
    zR0, nR = WALK + 1 - phi, np.maximum(lR - WALK, 0.0)
    zL0, nL = WALK + 1 + phi, np.maximum(-WALK - lL, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        SR = np.where(nR > 0, 1.0 / (zR0 - 0.5) - 1.0 / (zR0 + nR - 0.5), 0.0)
        SL = np.where(nL > 0, 1.0 / (zL0 - 0.5) - 1.0 / (zL0 + nL - 0.5), 0.0)
    pend = np.arange(n)
    for it in range(4096):
        if pend.size == 0:
            break
        s = sel[pend]
        ua, ub, uc = (words.u(1 + 3 * it + q, s) for q in range(3))
        sr, sl = SR[pend], SL[pend]
        right = ua * (sr + sl) < sr
        m1 = np.abs(ua * (sr + sl) - sr) / (sr + sl)
        z0 = np.where(right, zR0[pend], zL0[pend])
        S = np.where(right, sr, sl)
        cnt = np.where(right, nR[pend], nL[pend])
        R = 1.0 / (z0 - 0.5) - ub * S
        x = 1.0 / R - 0.5 - z0
        i = np.ceil(x)
        hi = np.maximum(cnt - 1.0, 0.0)
        inside = (x > 0.0) & (x < hi)          # outside, the clamp decides
        m2 = np.where(inside, np.abs(x - np.rint(x)) / np.maximum(np.abs(x), 1.0), np.inf)
        i = np.minimum(np.maximum(i, 0.0), hi)
        z = z0 + i
        acc = 4.0 * (z * z - 0.25) / (Md[pend] ** 2 * np.sin(np.pi * z / Md[pend]) ** 2)
        ok = uc < acc
        m3 = np.abs(uc - acc)
        marg[pend] = np.minimum(marg[pend], np.minimum(m1, np.minimum(m2, m3)))
        l = np.where(right, np.rint(z + phi[pend]), np.rint(phi[pend] - z)).astype(np.int64)
        res[pend[ok]] = l[ok]
        pend = pend[~ok]
    return res, marg


def tail_pmf(phi, M):
    """(offsets, conditional law) of the tail |l| > 16 of one (phi, M)."""
    lR = int(math.floor(phi + M / 2.0))
    lL = lR - M + 1
    offs = np.concatenate([np.arange(WALK + 1, lR + 1), np.arange(lL, -WALK)])
    p = _masses(np.array([phi]), np.array([float(M)]), offs)[0]
    return offs, p / p.sum()


def pe_near_one(w):
    """phase_estimation's rule for omega ~ 1: the top bin, no draw."""
    w = np.asarray(w, dtype=np.float64)
    return (w == 1.0) | (np.abs(w - 1.0) <= 1e-8 + 1e-5)


def median_ref(v):
    """Median over axis 0; an even count averages the two middle values
    (numpy.median, which the reference project's median evaluation calls)."""
    s = np.sort(np.asarray(v, dtype=np.float64), axis=0)
    q = s.shape[0]
    return s[q // 2] if q % 2 else 0.5 * (s[q // 2 - 1] + s[q // 2])


# ------------------------------------------------------------------ cases
# keys: (k0, k1, s0, s1)
KEY_U = (0x9E3779B9, 0x7F4A7C15, 0x0000002A, 0x00010000)
KEY_N = (0x243F6A88, 0x85A308D3, 0x00000005, 0x00090000)
KEY_T = (0x13198A2E, 0x03707344, 0x00000003, 0x00010000)
KEY_F = (0xA4093822, 0x299F31D0, 0x00000001, 0x00040000)
KEY_ZERO = (0, 0, 0, 0)
KEY_ONES = (MASK32,) * 4

# block of KEY_N whose first word is below 2^8: u1 = 0.5 * 2^-24, the smallest
# uniform, r = sqrt(50 ln 2) = 5.887 (elements 2 b and 2 b + 1)
SMALLEST_U1_BLOCK = 7297576

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

FLAT_N = (1, 3, 255, 257, 4099)
FLAT_OFFSETS = (0, 1, 2, 3, 13, 2 ** 32 - 2, 2 ** 34 - 1)
BIG_N = 8192 * 256 + 257          # past the launch's block cap: stride loop + tail
TN_BOUNDS = (1e-3, 0.5, 3.0, 8.0)
NORMAL_PARAMS = ((0.0, 1.0), (-3.5, 0.25))

N_CASE = 4096
PHI_GENERIC = (0.5, (0.3141 * 128) % 1.0, 0.9)
NEAR_LOW = (1e-3, 1e-6, 1e-9, 1e-12)
NEAR_HIGH = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-8)       # 1 - phi
NEAR_M = (41, 1000, 314160, 2 ** 20, 2 ** 40)
AMPLITUDES = (-0.1, 0.0, 1e-12, 0.25, 0.5, 0.75, 1 - 1e-12, 1.0, 1.1)
REP_Q = (1, 3, 13, 31, 2, 4)
REP_OFFSETS = (0, 7, 2 ** 32 - 3)


def _law_case(name, M, j, phi, n=N_CASE, offset=0, sub=0):
    """One (omega = j + phi, M) law, n draws: through phase estimation when M
    is a power of two (omega / M is exact), else through amplitude estimation
    (a = sin^2(pi omega / M); the phase is what fp64 yields on the way back)."""
    key = KEY_F[:2] + (KEY_F[2] + sub, KEY_F[3])
    if M & (M - 1) == 0:
        w = (j + phi) / M
        return dict(name=name, op="pe", key=key, offset=offset, Q=1,
                    x=np.full(n, w), m=np.full(n, M.bit_length() - 1, dtype=np.int32))
    a = math.sin(math.pi * (j + phi) / M) ** 2
    return dict(name=name, op="ae", key=key, offset=offset, Q=1,
                x=np.full(n, a), eps=np.full(n, eps_for_bins(M)))


@functools.lru_cache(maxsize=None)
def fejer_cases():
    """The case matrix of the Fejer tests: a tuple of dicts (name, op 'pe' /
    'ae', key, offset, Q, x = omega or a, m or eps)."""
    cases = []
    sub = 0
    for M in (64, 128, 2 ** 20, 2 ** 30, 2 ** 40):
        for phi in PHI_GENERIC:
            sub += 1
            cases.append(_law_case(f"generic-M{M}-phi{phi:.4f}", M, 40, phi, sub=sub))
    for m in (1, 2, 5):
        sub += 1
        cases.append(dict(name=f"small-m{m}", op="pe", key=KEY_F[:2] + (sub, KEY_F[3]), offset=0, Q=1,
                          x=np.full(N_CASE, 0.3141), m=np.full(N_CASE, m, dtype=np.int32)))
    sub += 1
    cases.append(dict(name="small-ae-eps0.1", op="ae", key=KEY_F[:2] + (sub, KEY_F[3]), offset=0, Q=1,
                      x=np.full(N_CASE, 0.3), eps=np.full(N_CASE, 0.1)))
    for name, w in (("onbin-phi0", 37.0 / 128), ("onbin-omega0", 0.0), ("onbin-one", 1.0),
                    ("onbin-nearone", 1 - 5e-6)):
        sub += 1
        cases.append(dict(name=name, op="pe", key=KEY_F[:2] + (sub, KEY_F[3]), offset=0, Q=1,
                          x=np.full(N_CASE, w), m=np.full(N_CASE, 7, dtype=np.int32)))
    def near(name, M, j, phi):
        # a stream whose first uniforms all clear DELTA: the bin that holds
        # (almost) all the mass decides every draw
        nonlocal sub
        while True:
            sub += 1
            c = _law_case(name, M, j, phi, sub=sub)
            if SampleWords(c["key"], _ids(0, N_CASE)).u(0).min() >= DELTA:
                return c

    for M in NEAR_M:
        for phi in NEAR_LOW:
            cases.append(dict(near(f"nearbin-M{M}-phi{phi:g}", M, 3, phi), phase=("phi", phi)))
        for d in NEAR_HIGH:
            cases.append(dict(near(f"nearbin-M{M}-1mphi{d:g}", M, 3, 1.0 - d), phase=("1-phi", d)))
    # below pi phi = 2^-50 the kernel takes l = 0 without a walk
    cases.append(dict(near("nearbin-M1099511627776-phi1e-17", 2 ** 40, 0, 1e-17), phase=("phi", 1e-17)))
    sub += 1
    cases.append(_law_case("tail-M1048576", 2 ** 20, 40, 0.5, n=65536, sub=sub))
    rng = np.random.default_rng(20)
    sub += 1
    cases.append(dict(name="hetero-m", op="pe", key=KEY_F[:2] + (sub, KEY_F[3]), offset=5, Q=1,
                      x=rng.uniform(0.0, 0.99, N_CASE),
                      m=rng.choice(np.array([1, 5, 7, 20, 33], dtype=np.int32), N_CASE)))
    sub += 1
    cases.append(dict(name="hetero-eps", op="ae", key=KEY_F[:2] + (sub, KEY_F[3]), offset=5, Q=1,
                      x=rng.uniform(0.0, 1.0, N_CASE),
                      eps=rng.choice(np.array([0.1, 0.02, 1e-3, 1e-5]), N_CASE)))
    sub += 1
    cases.append(dict(name="amplitude-edges", op="ae", key=KEY_F[:2] + (sub, KEY_F[3]), offset=0, Q=1,
                      x=np.tile(np.array(AMPLITUDES), N_CASE // len(AMPLITUDES) + 1)[:N_CASE],
                      eps=np.full(N_CASE, 0.01)))
    for Q in REP_Q:
        for off in REP_OFFSETS:
            sub += 1
            cases.append(dict(name=f"reps-Q{Q}-off{off}", op="ae", key=KEY_F[:2] + (sub, KEY_F[3]),
                              offset=off, Q=Q, x=rng.uniform(0.0, 1.0, N_CASE),
                              eps=rng.choice(np.array([0.1, 0.01, 1e-3]), N_CASE)))
    sub += 1
    cases.append(_law_case("launch-tail-n257", 2 ** 20, 40, 0.3, n=257, sub=sub))
    return tuple(cases)


def evaluate_case(c):
    """Reference of one case (a dict as in ``fejer_cases``): dict with, per
    repetition q, the ``fejer_bin`` result plus ``near`` [n] (list ``draws``),
    ``M`` [n], ``omega`` [n], ``skip`` [n] (phase estimation's omega ~ 1
    rule), and per element the value the op returns (``value``) with the band
    [``lo``, ``hi``] the near-boundary draws leave it: lo == hi == value where
    no draw is near a boundary; a near-boundary walk draw may take either bin
    next to its boundary; a draw within DELTA of the end of the walk, or a
    small-M or tail draw within TIGHT of a decision, may take any (``free``)."""
    n = c["x"].shape[0]
    Q = c["Q"]
    if c["op"] == "pe":
        M = np.left_shift(np.int64(1), c["m"].astype(np.int64))
        omega = M.astype(np.float64) * c["x"]
        skip = pe_near_one(c["x"])
    else:
        M = ae_bins(c["eps"])
        omega = ae_omega(c["x"], M)
        skip = np.zeros(n, dtype=bool)
    Md = M.astype(np.float64)
    outmap = (lambda j: j.astype(np.float64) / Md) if c["op"] == "pe" else (lambda j: ae_value(j, M))
    ids = _ids(c["offset"], n) * np.uint64(Q)
    base = np.floor(omega).astype(np.int64)
    draws, vals, los, his = [], [], [], []
    free_any = np.zeros(n, dtype=bool)
    for q in range(Q):
        d = fejer_bin(omega, M, SampleWords(c["key"], ids + np.uint64(q)))
        v = outmap(d["bin"])
        lo, hi = v.copy(), v.copy()
        close = (d["branch"] >= WALKED) & (d["margin"] <= DELTA)
        walk_near = close & (d["edge"] < WALK_OFFS.size - 1)
        free = (close & ~walk_near) | ((d["branch"] == SMALL) & (d["margin"] <= TIGHT)) | \
               ((d["branch"] == TAIL) & (d["margin"] <= TIGHT))
        e = np.clip(d["edge"], 0, WALK_OFFS.size - 2)
        for side in (e, e + 1):
            alt = outmap(np.mod(base + WALK_OFFS[side], M))
            lo = np.where(walk_near, np.minimum(lo, alt), lo)
            hi = np.where(walk_near, np.maximum(hi, alt), hi)
        lo = np.where(free, 0.0, lo)
        hi = np.where(free, 1.0, hi)
        d["near"] = (walk_near | free) & ~skip
        free_any |= free & ~skip
        draws.append(d)
        vals.append(v)
        los.append(lo)
        his.append(hi)
    value, lo, hi = (median_ref(np.stack(t)) for t in (vals, los, his))
    if c["op"] == "pe":
        top = (Md - 1.0) / Md
        value, lo, hi = (np.where(skip, top, t) for t in (value, lo, hi))
    return dict(case=c, M=M, omega=omega, skip=skip, draws=draws, value=value, lo=lo, hi=hi,
                free=free_any)


@functools.lru_cache(maxsize=None)
def evaluate(index):
    """``evaluate_case`` of case ``index`` of ``fejer_cases`` (cached: shared
    by the tests, not to be written to)."""
    return evaluate_case(fejer_cases()[index])


VALUE_TOL = 1e-12     # sin^2(pi j / M) of two libms; k / 2^m is exact


def compare(out, ev):
    """Draw-by-draw rule for the op's output ``out`` [n] against ``ev``.
    Returns (bad, excused, off): indices breaking the rule, the share of
    draws marked near-boundary, the share of elements off the reference value.

    An element none of whose draws is near a boundary must equal the
    reference (exactly for phase estimation).  With Q = 1 a near-boundary walk
    draw must equal one of its two neighbours; otherwise the output lies in
    the band [lo, hi] (the median is monotone in every draw)."""
    out = np.asarray(out, dtype=np.float64)
    tol = 0.0 if ev["case"]["op"] == "pe" else VALUE_TOL
    value, lo, hi = ev["value"], ev["lo"], ev["hi"]
    sure = lo == hi
    ok = np.where(sure, np.abs(out - value) <= tol, (out >= lo - tol) & (out <= hi + tol))
    if ev["case"]["Q"] == 1:
        ends = np.minimum(np.abs(out - lo), np.abs(out - hi)) <= tol
        ok &= sure | ev["free"] | ends
    excused = float(np.mean([d["near"].mean() for d in ev["draws"]]))
    off = float(np.mean(np.abs(out - value) > tol))
    return np.nonzero(~ok)[0], excused, off
