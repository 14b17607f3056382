// Exact O(1)-expected Fejer-kernel sampler for amplitude / phase estimation.
// Same algorithm as sq_learn_amd/quantum/fejer.py (see its docstring):
//   P(l) = sin^2(pi phi) / (M^2 sin^2(pi (l - phi) / M)),  phi = frac(omega)
//   1) inverse-CDF walk over l = 0, 1, -1, 2, -2, ... (|l| <= WALK),
//      sines by angle-addition recurrence (no transcendental per step);
//   2) tails by rejection with the telescoping proposal 1/(z-1/2)-1/(z+1/2).
// Random words come from Philox blocks (sample id s, block b): counter
// (s_lo, s_hi | b << 16, stream_lo, stream_hi) so every sample owns 2^16
// independent blocks.
#pragma once
#include "common.h"

namespace sq {

constexpr int kFejerWalk = 16;
constexpr int kFejerSmallM = 2 * kFejerWalk + 4;

struct WordStream {
  RngKey key;
  uint64_t s;
  uint32_t b = 0;
  u4 cur;
  int used = 4;
  SQ_DEV WordStream(const RngKey& k, uint64_t sid) : key(k), s(sid) {}
  SQ_DEV uint32_t next() {
    if (used == 4) {
      cur = philox4x32_10((uint32_t)s, ((uint32_t)(s >> 32) & 0xFFFFu) | (b << 16),
                          key.s0, key.s1, key.k0, key.k1);
      ++b;
      used = 0;
    }
    uint32_t w = used == 0 ? cur.x : (used == 1 ? cur.y : (used == 2 ? cur.z : cur.w));
    ++used;
    return w;
  }
  SQ_DEV double u() { return u01d(next()); }
};

// The per-law setup (phi, sin^2(pi phi), the walk's rotation constants) is
// computed once; sample() then costs the walk (plus rare tail rejections).
// fejer_sample() below = FejerLaw(omega, M).sample(ws): identical words and
// results to the CPU twin (ops/random.py fejer_sample_torch).
//
// The walk is fp32.  Two things keep it sound at every phase and M <= 2^40:
//  * Scale.  With 2^e <= M < 2^(e+1) the walk carries 2^e sin(.) instead of
//    sin(.) and 2^(2e) / M^2 instead of 1 / M^2.  Powers of two commute with
//    rounding, so every term has the mantissa the unscaled walk gives, but
//    sin^2(pi phi / M) and sin^2(pi phi) / M^2 no longer underflow (unscaled,
//    M = 2^40 with phi = 1e-12 gave 0 / 0).  Below pi phi < 2^-50 the bin
//    l = 0 holds 1 - O(2^-100) of the mass and is taken outright.
//  * l = +1.  sin(alpha - beta) = sin(pi (1 - phi) / M) by angle subtraction
//    loses a factor (1 + phi) / (1 - phi) of its precision.  For phi <= 1/2
//    that is at most 3, the same as every |l| >= 2 ((t + phi) / (t - phi) <= 3),
//    and the subtraction stays.  For phi > 1/2, where this bin takes most of
//    the mass, the sine comes from its own angle gamma = pi (1 - phi) / M,
//    formed in fp64; sin^2(pi phi) is taken as sin^2(pi (1 - phi)) there too
//    (1 - phi is exact, pi phi near pi is not).
struct FejerLaw {
  double omega, phi, Md;
  long long M, base;
  // s = sin^2(pi phi); sin/cos of alpha = pi / M and beta = pi phi / M with
  // sb = 2^e sin(beta), sa_up = 2^e sin(alpha), sa_dn = 2^-e sin(alpha);
  // s1 = 2^e sin(gamma) when phi > 1/2, else 0; inv_m2 = 2^(2e) / M^2
  float s, sa_up, sa_dn, ca, sb, cb, s1, inv_m2;
  SQ_DEV FejerLaw(double omega_, long long M_) : omega(omega_), M(M_) {
    const double PI = 3.14159265358979323846;
    const double fl = floor(omega);
    phi = omega - fl;
    Md = (double)M;
    base = (long long)fl;
    s = 0.f; sa_up = sa_dn = ca = sb = cb = s1 = inv_m2 = 0.f;
    if (phi == 0.0) return;
    const bool upper = phi > 0.5;
    s = (float)sin(PI * (upper ? 1.0 - phi : phi));
    s = s * s;
    if (M <= kFejerSmallM) return;
    if (PI * phi < 0x1p-50) {   // walk_term(sb) == 1: every draw stops at l = 0
      s = sb = cb = inv_m2 = 1.f;
      return;
    }
    const int e = 63 - __builtin_clzll((unsigned long long)M);
    const float up = ldexpf(1.f, e), dn = ldexpf(1.f, -e);
    const float alpha = (float)(PI / Md);
    const float beta = (float)(PI * phi / Md);
    float sa;
    __sincosf(beta, &sb, &cb);
    __sincosf(alpha, &sa, &ca);
    sb *= up;
    sa_up = sa * up;
    sa_dn = sa * dn;
    if (upper) s1 = __sinf((float)(PI * (1.0 - phi) / Md)) * up;
    inv_m2 = (float)(1.0 / (Md * Md)) * up * up;
  }
  // pmf of the walk offset l (bin base + l) given 2^e sin(l alpha - beta)
  SQ_DEV float walk_term(float sn) const { return s * inv_m2 / (sn * sn); }
  // (st, ct) = (2^e sin, cos)(t alpha) -> the same of (t + 1) alpha
  SQ_DEV void walk_step(float& st, float& ct) const {
    const float nst = st * ca + ct * sa_up;
    const float nct = ct * ca - st * sa_dn;
    st = nst; ct = nct;
  }
  // 2^e sin(t alpha - beta): the sine of l = +t
  SQ_DEV float sin_plus(int t, float st, float ct) const {
    return (t == 1 && s1 != 0.f) ? s1 : st * cb - ct * sb;
  }
  // 2^e sin(t alpha + beta): the sine of l = -t, sign dropped
  SQ_DEV float sin_minus(float st, float ct) const { return st * cb + ct * sb; }
  // offset of a draw conditioned on |l| > kFejerWalk (rejection, telescoping proposal)
  SQ_DEV long long tail_ell(WordStream& ws) const {
    const double PI = 3.14159265358979323846;
    long long ell = 0;
    double lR = floor(phi + Md / 2.0);
    double lL = lR - Md + 1.0;
    double zR0 = kFejerWalk + 1 - phi, nR = fmax(lR - kFejerWalk, 0.0);
    double zL0 = kFejerWalk + 1 + phi, nL = fmax(-kFejerWalk - lL, 0.0);
    double SR = nR > 0 ? 1.0 / (zR0 - 0.5) - 1.0 / (zR0 + nR - 0.5) : 0.0;
    double SL = nL > 0 ? 1.0 / (zL0 - 0.5) - 1.0 / (zL0 + nL - 0.5) : 0.0;
    for (int it = 0; it < 4096; ++it) {
      bool right = ws.u() * (SR + SL) < SR;
      double z0 = right ? zR0 : zL0, S = right ? SR : SL, cnt = right ? nR : nL;
      double R = 1.0 / (z0 - 0.5) - ws.u() * S;
      double i = ceil(1.0 / R - 0.5 - z0);
      i = fmin(fmax(i, 0.0), fmax(cnt - 1.0, 0.0));
      double z = z0 + i;
      double sn = sin(PI * z / Md);
      double accp = 4.0 * (z * z - 0.25) / (Md * Md * sn * sn);
      if (ws.u() < accp) {
        ell = right ? (long long)llround(z + phi) : (long long)llround(phi - z);
        break;
      }
    }
    return ell;
  }
  SQ_DEV long long bin_of(long long ell) const {
    long long j = (base + ell) % M;
    if (j < 0) j += M;
    return j;
  }
  // returns the sampled bin in [0, M)
  SQ_DEV long long sample(WordStream& ws) const {
    const double PI = 3.14159265358979323846;
    if (phi == 0.0) {  // the true value sits on a bin: p = 1 there
      long long j = base % M; if (j < 0) j += M; return j;
    }
    if (M <= kFejerSmallM) {
      // enumerate the whole period: bins j = 0..M-1, inverse CDF
      double u = ws.u();
      double acc = 0.0;
      long long pick = M - 1;
      double tot = 0.0;
      for (long long j = 0; j < M; ++j) {
        double d = (double)j - omega;
        double sn = sin(PI * d / Md);
        tot += (sn == 0.0) ? 1.0 : (double)s / (Md * Md * sn * sn);
      }
      u *= tot;
      for (long long j = 0; j < M; ++j) {
        double d = (double)j - omega;
        double sn = sin(PI * d / Md);
        acc += (sn == 0.0) ? 1.0 : (double)s / (Md * Md * sn * sn);
        if (acc >= u) { pick = j; break; }
      }
      return pick;
    }
    // ---- walk
    float u = (float)ws.u();
    float acc = walk_term(sb);   // l = 0 : sin(-beta)
    long long ell = 0;
    bool found = acc >= u;
    float st = 0.f, ct = 1.f;  // 2^e sin / cos(t*alpha)
    for (int t = 1; t <= kFejerWalk && !found; ++t) {
      walk_step(st, ct);
      acc += walk_term(sin_plus(t, st, ct));
      if (acc >= u) { ell = t; found = true; break; }
      acc += walk_term(sin_minus(st, ct));
      if (acc >= u) { ell = -t; found = true; break; }
    }
    if (!found) ell = tail_ell(ws);
    long long j = (base + ell) % M;
    if (j < 0) j += M;
    return j;
  }
};

SQ_DEV long long fejer_sample(double omega, long long M, WordStream& ws) {
  return FejerLaw(omega, M).sample(ws);
}

// amplitude estimation of a in [0,1] with M bins: returns sin^2(pi j / M)
SQ_DEV double ae_sample(double a, long long M, WordStream& ws) {
  const double PI = 3.14159265358979323846;
  double omega = (double)M * asin(sqrt(fmin(fmax(a, 0.0), 1.0))) / PI;
  long long j = fejer_sample(omega, M, ws);
  double sv = sin(PI * (double)j / (double)M);
  return sv * sv;
}

SQ_DEV long long ae_bins(double eps) {
  const double PI = 3.14159265358979323846;
  return (long long)ceil((PI / (2.0 * eps)) * (1.0 + sqrt(1.0 + 4.0 * eps)));
}

// small median (Q <= 31) by insertion sort in registers; an even Q averages
// the two middle values, as the reference's np.median (Utility.py:571)
template <int QMAX>
SQ_DEV double median_of(double* v, int Q) {
  for (int i = 1; i < Q; ++i) {
    double x = v[i]; int j = i - 1;
    while (j >= 0 && v[j] > x) { v[j + 1] = v[j]; --j; }
    v[j + 1] = x;
  }
  return (Q & 1) ? v[Q / 2] : 0.5 * (v[Q / 2 - 1] + v[Q / 2]);
}

}  // namespace sq
