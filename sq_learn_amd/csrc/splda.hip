// CSR latent Dirichlet allocation kernels (the topic model).
//
// Reference semantics: ``decomposition/_online_lda_fast.pyx`` and the
// ``_update_doc_distribution`` loop of ``decomposition/_lda.py``; the law is
// the one of csrc/host/decomposition_host.cpp: sqh_lda_estep, operation by
// operation (same digamma, same EPS, same stopping rule).
//
// MI355X mapping.
//   E-step (sp_lda_estep_kernel): one wave per document.  The operand is the
//     transposed exp_tw table TW[F][k] (fp64), so a stored word is one
//     contiguous k-wide row.  A fixed-point iteration has two phases over the
//     document's words, 64 at a time:
//       ratio       lanes over words: r_t = cnt_t / (sum_j edt_j tw[t][j] + EPS),
//                   j in order, edt broadcast from LDS;
//       accumulate  lanes over topics: acc_j += r_t tw[t][j], t in order, r_t
//                   and the row base broadcast with readlane.
//     Both sums run in the host's order.  dt, edt and acc live in LDS, one
//     lane owning topic j = lane + 64 i of each.  When the document's gathered
//     rows fit SP_LDA_STAGE doubles they are staged in LDS once, with a row
//     stride of k | 1 doubles: odd, so lanes over words (stride apart) and
//     lanes over topics (adjacent) both spread over the banks.  Longer
//     documents re-gather the rows from global memory on every iteration.
//   Statistics: cnt_t edt_j tw[t][j] / norm_phi_t is at most cnt_t.  It is
//     split into an integer number of quanta 2^e and a remainder in quanta
//     2^e_lo, and both go to int64 planes [F][k] by integer vector atomics
//     (the idiom of sp_rows.h: sp_mstep_kernel): integer addition commutes, so
//     the sums depend neither on the arrival order nor on the launch geometry
//     nor on how the rows are split into calls.  The remainder plane is what
//     keeps small entries accurate to fp64 relative precision: the coarse
//     quantum alone is 2^-52 of the column bound, not of the entry.
//   Bound (sp_lda_bound_kernel): one wave per document, lanes over words (the
//     shared 64-pair load), the max-shifted logsumexp over the topics in
//     order, then a wave sum.
#include <cmath>

#include "sp_rows.h"
#include "sq_api.h"

namespace sq {

constexpr int SP_LDA_STAGE = 2048;   // doubles of gathered rows a wave stages in LDS
constexpr int SP_LDA_MAX_K = 4096;   // 3 LDS rows of k doubles + the stage, one wave
constexpr double SP_LDA_EPS = 2.220446049250313e-16;

// the host file's digamma: recurrence up to x >= 6, then the asymptotic series.  The loop runs
// at most 6 times: an argument that is not positive (NaN included) returns NaN at once, where
// the host would walk up from it.
SQ_DEV double lda_psi(double x) {
  if (!(x > 0.0)) return NAN;
  double r = 0.0;
  while (x < 6.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  const double t = f * (-1.0 / 12 + f * (1.0 / 120 + f * (-1.0 / 252 + f * (1.0 / 240 +
                   f * (-1.0 / 132 + f * (691.0 / 32760 + f * (-1.0 / 12)))))));
  return r + log(x) - 0.5 / x + t;
}

// a wave's view of one document
struct LdaDoc {
  const int* indices;
  const float* data;
  const double* TW;   // [F][k]
  long long s, e;     // stored words [s, e)
  int F, k, nj;       // nj: topic tiles of 64
  double* dt;         // LDS rows of 64 nj doubles
  double* edt;
  double* acc;
  double* S;          // staged rows, stride doubles apart
  int stride;
};

// the lane's (col, cnt) of the words [p, p + 64): a column outside [0, F) or past the end
// becomes (0, 0), which adds nothing
SQ_DEV int lda_load(const LdaDoc& D, long long p, int lane, int& col, double& cnt) {
  float v;
  const int n = sp_load_pairs(D.indices, D.data, p, D.e, lane, col, v);
  const bool ok = col >= 0 && col < D.F;
  col = ok ? col : 0;
  cnt = ok ? (double)v : 0.0;
  return n;
}

// r_t = cnt_t / (sum_j edt_j tw[t][j] + EPS) of the lane's word
template <bool STAGED>
SQ_DEV double lda_ratio(const LdaDoc& D, long long p, int lane, int n, int col, double cnt) {
  const double* row = STAGED ? D.S + (size_t)((int)(p - D.s) + (lane < n ? lane : 0)) * D.stride
                             : D.TW + (long long)col * D.k;
  double v = 0.0;
  for (int j = 0; j < D.k; ++j) v += D.edt[j] * row[j];
  return cnt / (v + SP_LDA_EPS);
}

// row q of the chunk at p, wave-uniform
template <bool STAGED>
SQ_DEV const double* lda_row(const LdaDoc& D, long long p, int col, int q) {
  return STAGED ? D.S + (size_t)((int)(p - D.s) + q) * D.stride
                : D.TW + (long long)bcast_i(col, q) * D.k;
}

template <bool STAGED>
SQ_DEV int lda_iterate(const LdaDoc& D, int lane, double prior, int max_iters, double tol) {
  int it = 0;
  while (it < max_iters) {
    for (long long p = D.s; p < D.e; p += 64) {
      int col;
      double cnt;
      const int n = lda_load(D, p, lane, col, cnt);
      const double r = lda_ratio<STAGED>(D, p, lane, n, col, cnt);
      for (int i = 0; i < D.nj; ++i) {
        const int j = 64 * i + lane;
        const int jr = j < D.k ? j : D.k - 1;
        double a = D.acc[j];
        for (int q = 0; q < n; ++q) a += bcast_d(r, q) * lda_row<STAGED>(D, p, col, q)[jr];
        D.acc[j] = a;
      }
    }
    double total = 0.0, diff = 0.0;
    for (int i = 0; i < D.nj; ++i) {
      const int j = 64 * i + lane;
      if (j < D.k) {
        const double nd = D.edt[j] * D.acc[j] + prior;
        diff += fabs(D.dt[j] - nd);
        D.dt[j] = nd;
        total += nd;
      }
      D.acc[j] = 0.0;
    }
    total = wave_sum(total);
    diff = wave_sum(diff);
    const double pt = lda_psi(total);
    sp_wave_sync();   // every lane is done reading the old edt
    for (int i = 0; i < D.nj; ++i) {
      const int j = 64 * i + lane;
      if (j < D.k) D.edt[j] = exp(lda_psi(D.dt[j]) - pt);
    }
    sp_wave_sync();
    ++it;
    if (diff / D.k < tol) break;
  }
  return it;
}

template <bool STAGED>
SQ_DEV void lda_scatter(const LdaDoc& D, int lane, double hi_scale, double hi_unit,
                        double lo_scale, long long* __restrict__ qhi, long long* __restrict__ qlo) {
  for (long long p = D.s; p < D.e; p += 64) {
    int col;
    double cnt;
    const int n = lda_load(D, p, lane, col, cnt);
    const double r = lda_ratio<STAGED>(D, p, lane, n, col, cnt);
    for (int q = 0; q < n; ++q) {
      const double rq = bcast_d(r, q);
      if (rq == 0.0) continue;   // wave-uniform: a skipped column or a zero count
      const double* row = lda_row<STAGED>(D, p, col, q);
      const long long base = (long long)bcast_i(col, q) * D.k;
      for (int i = 0; i < D.nj; ++i) {
        const int j = 64 * i + lane;
        if (j >= D.k) break;
        const double val = rq * D.edt[j] * row[j];
        const long long hi = __double2ll_rn(val * hi_scale);
        const long long lo = __double2ll_rn((val - (double)hi * hi_unit) * lo_scale);
        if (hi != 0)
          atomicAdd(reinterpret_cast<unsigned long long*>(qhi + base + j), (unsigned long long)hi);
        if (lo != 0)
          atomicAdd(reinterpret_cast<unsigned long long*>(qlo + base + j), (unsigned long long)lo);
      }
    }
  }
}

// ---------------------------------------------------------------- E-step
// Documents [q0, q0 + m); doc_topic [m][k] and iters [m] (optional) are indexed from q0.
// qhi / qlo (optional, together): the int64 statistics planes [F][k].
__global__ void __launch_bounds__(256) sp_lda_estep_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const double* __restrict__ TW, double* __restrict__ doc_topic,
    long long q0, long long m, int F, int k, double prior, int max_iters, double tol,
    int* __restrict__ iters, long long* __restrict__ qhi, long long* __restrict__ qlo,
    double hi_scale, double hi_unit, double lo_scale) {
  extern __shared__ unsigned char lda_smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  LdaDoc D;
  D.indices = indices;
  D.data = data;
  D.TW = TW;
  D.F = F;
  D.k = k;
  D.nj = (k + 63) >> 6;
  D.stride = k | 1;
  const int kp = 64 * D.nj;
  D.dt = reinterpret_cast<double*>(lda_smem) + (size_t)wave * (3 * kp + SP_LDA_STAGE);
  D.edt = D.dt + kp;
  D.acc = D.edt + kp;
  D.S = D.acc + kp;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long pos = (long long)blockIdx.x * wpb + wave; pos < m; pos += stride) {
    D.s = sp_uniform_ll(indptr[q0 + pos]);
    D.e = sp_uniform_ll(indptr[q0 + pos + 1]);
    const long long words = D.e - D.s;
    const bool staged = words > 0 && words * D.stride <= SP_LDA_STAGE;   // wave-uniform
    double* row = doc_topic + pos * k;
    double tot = 0.0;
    for (int i = 0; i < D.nj; ++i) {
      const int j = 64 * i + lane;
      const double v = j < k ? row[j] : 0.0;
      D.dt[j] = v;
      D.acc[j] = 0.0;
      tot += v;
    }
    const double pt = lda_psi(wave_sum(tot));
    for (int i = 0; i < D.nj; ++i) {
      const int j = 64 * i + lane;
      D.edt[j] = j < k ? exp(lda_psi(D.dt[j]) - pt) : 0.0;
    }
    if (staged) {
      for (long long p = D.s; p < D.e; p += 64) {
        int col;
        double cnt;
        const int n = lda_load(D, p, lane, col, cnt);
        for (int q = 0; q < n; ++q) {
          const double* src = TW + (long long)bcast_i(col, q) * k;
          double* dst = D.S + (size_t)((int)(p - D.s) + q) * D.stride;
          for (int j = lane; j < k; j += 64) dst[j] = src[j];
        }
      }
    }
    sp_wave_sync();
    const int it = staged ? lda_iterate<true>(D, lane, prior, max_iters, tol)
                          : lda_iterate<false>(D, lane, prior, max_iters, tol);
    for (int j = lane; j < k; j += 64) row[j] = D.dt[j];
    if (iters && lane == 0) iters[pos] = it;
    if (qhi) {
      if (staged) lda_scatter<true>(D, lane, hi_scale, hi_unit, lo_scale, qhi, qlo);
      else lda_scatter<false>(D, lane, hi_scale, hi_unit, lo_scale, qhi, qlo);
    }
    sp_wave_sync();   // the next document overwrites the LDS rows
  }
}

// ---------------------------------------------------------------- bound
// out[pos] = sum_t cnt_t logsumexp_j(ET[pos][j] + EB[idx_t][j]) of document q0 + pos, the
// words 64 at a time, one per lane.  The document's row of ET is read by per-lane loads of
// one address on purpose: they queue behind the lane's EB loads.  Through a wave-uniform
// pointer (scalar loads) or from an LDS copy the kernel measured 28 % and 60 % slower at
// k = 64 and 128 on 200 000 x 50 000 (profiles/lda_device.md).
__global__ void __launch_bounds__(256) sp_lda_bound_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const double* __restrict__ ET, const double* __restrict__ EB,
    long long q0, long long m, int F, int k, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long pos = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); pos < m; pos += stride) {
    const long long s = sp_uniform_ll(indptr[q0 + pos]);
    const long long e = sp_uniform_ll(indptr[q0 + pos + 1]);
    const double* th = ET + pos * k;
    double a = 0.0;
    for (long long p = s; p < e; p += 64) {
      int col;
      float v;
      const int n = sp_load_pairs(indices, data, p, e, lane, col, v);
      if (lane < n && col >= 0 && col < F) {
        const double* row = EB + (long long)col * k;
        double mx = -INFINITY;
        for (int j = 0; j < k; ++j) mx = fmax(mx, th[j] + row[j]);
        double sum = 0.0;
        for (int j = 0; j < k; ++j) sum += exp(th[j] + row[j] - mx);
        a += (double)v * (mx + log(sum));
      }
    }
    a = wave_sum(a);
    if (lane == 0) out[pos] = a;
  }
}

}  // namespace sq

using namespace sq;

extern "C" int sq_sp_lda_stage() { return SP_LDA_STAGE; }
extern "C" int sq_sp_lda_max_k() { return SP_LDA_MAX_K; }

// hexp / lexp: the exponents of the two quanta (qhi null: no statistics)
extern "C" int sq_sp_lda_estep(const void* indptr, const void* indices, const void* data,
                               const void* tw_t, void* doc_topic, long long q0, long long m,
                               int F, int k, double prior, int max_iters, double tol,
                               void* iters, void* qhi, void* qlo, int hexp, int lexp,
                               void* stream) {
  if (k < 1 || k > SP_LDA_MAX_K || F < 1 || q0 < 0 || m < 0 || max_iters < 0 ||
      !(prior > 0.0) || !std::isfinite(prior) || !std::isfinite(tol) || (qhi == nullptr) != (qlo == nullptr))
    return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  const size_t wave_bytes = (size_t)(3 * 64 * ((k + 63) / 64) + SP_LDA_STAGE) * sizeof(double);
  int wpb = 4;
  while (wpb > 1 && wave_bytes * wpb > 160 * 1024) wpb >>= 1;
  if (wave_bytes * wpb > 160 * 1024) return (int)hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    hipError_t rc = hipFuncSetAttribute((const void*)sp_lda_estep_kernel,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (rc != hipSuccess) return (int)rc;
    attr = true;
  }
  hipLaunchKernelGGL(sp_lda_estep_kernel, dim3(sp_grid(m, wpb)), dim3(64 * wpb),
                     wave_bytes * wpb, (hipStream_t)stream, (const long long*)indptr,
                     (const int*)indices, (const float*)data, (const double*)tw_t,
                     (double*)doc_topic, q0, m, F, k, prior, max_iters, tol, (int*)iters,
                     (long long*)qhi, (long long*)qlo, ldexp(1.0, -hexp), ldexp(1.0, hexp),
                     ldexp(1.0, -lexp));
  return (int)hipGetLastError();
}

extern "C" int sq_sp_lda_bound(const void* indptr, const void* indices, const void* data,
                               const void* elog_theta, const void* elog_beta_t, long long q0,
                               long long m, int F, int k, void* out, void* stream) {
  if (k < 1 || k > SP_LDA_MAX_K || F < 1 || q0 < 0 || m < 0) return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  hipLaunchKernelGGL(sp_lda_bound_kernel, dim3(sp_grid(m, 4)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)indptr, (const int*)indices, (const float*)data,
                     (const double*)elog_theta, (const double*)elog_beta_t, q0, m, F, k,
                     (double*)out);
  return (int)hipGetLastError();
}
