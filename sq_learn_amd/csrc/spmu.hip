// mu(A) power sums of a CSR matrix, optionally centred by a column mean that
// is never subtracted in memory (ops/sparse_linalg.py sp_mu_power_sums; the
// mu phase of PCA / qPCA on sparse rows):
//
//   rowmax[i]    = max over rows r of  sum_j |a_rj|^q_i
//   colsum[i, j] =                     sum_r |a_rj|^q_i         a = x - m  (a = x without a mean)
//
// with |0|^q = 0 for every q, q = 0 included (a count of the nonzero a).  The
// centred matrix is dense but its power sums are sums over the stored entries:
//
//   row r:    sum_j |m_j|^q + sum over stored (r, j) of (|x_rj - m_j|^q - |m_j|^q)
//   column j: (n - cnt_j) |m_j|^q + sum over stored (r, j) of |x_rj - m_j|^q
//
// MI355X mapping.  Nothing is scattered and there are no floating-point
// atomics; all arithmetic is fp64.
//   sp_mu_row_kernel: one wave per row of X.  The (col, v) pairs are loaded 64
//     at a time (sp_load_pairs) and every lane keeps its own pair - the work
//     per pair is a log, an exp and a few products, not a row gather, so the
//     pairs are not broadcast: lane l gathers m[col], forms the terms of the
//     pairs l, l + 64, ... in order and an xor-tree adds the lanes.  The first
//     term sum_j |m_j|^q comes from the caller ([nq]).  A wave keeps the
//     maximum over its rows and writes one partial per exponent;
//     sp_mu_rowmax_kernel takes the maximum of the partials (a maximum does
//     not depend on which wave met which row).
//   sp_mu_col_kernel: the same walk over the CSR of X^T, one wave per row
//     SEGMENT of at most `seg` nonzeros (the segment table of spmm.hip), so a
//     column stored in every row is not one wave's serial walk.  m_j and
//     |m_j|^q are wave-uniform.  The only segment of a column writes colsum;
//     a longer column writes one partial per segment (its first segment adds
//     the (n - cnt_j) |m_j|^q term) and sp_mu_col_reduce_kernel adds them in
//     segment order.
//   Every value is a fixed sequence of fp64 operations that depends on `seg`
//     alone - not on the grid, not on which wave picks up which row.
//   Exponents are taken MU_G at a time (accumulators in registers); more
//     exponents re-walk the row.  GRID: the exponents are 0, b, 2b, ... and
//     the powers of one |a| are 1, t, t^2, ... with t = exp(b log |a|), one
//     log and one exp per element; otherwise exp(q_i log |a|) per exponent.
#include "sp_rows.h"
#include "sq_api.h"

namespace sq {

constexpr int MU_G = 12;   // exponents per pass over a row (the default p-grid has 11)

// p[i] = a^q[g0 + i] for i < ng (a >= 0; 0 for a == 0, at q == 0 too); ng, g0, q: wave-uniform
template <bool GRID>
SQ_DEV void mu_powers(double a, const double* __restrict__ q, int g0, int ng, double step,
                      double (&p)[MU_G]) {
  const bool nz = a != 0.0;
  const double lg = log(nz ? a : 1.0);
  if (GRID) {
    const double t = exp(step * lg);
    double cur = g0 == 0 ? 1.0 : exp(q[g0] * lg);
#pragma unroll
    for (int i = 0; i < MU_G; ++i) {
      p[i] = nz ? cur : 0.0;
      cur *= t;
    }
  } else {
#pragma unroll
    for (int i = 0; i < MU_G; ++i) {
      const double qi = i < ng ? q[g0 + i] : 0.0;
      p[i] = !nz ? 0.0 : qi == 0.0 ? 1.0 : exp(qi * lg);
    }
  }
}

// part[w, i] = max over the rows of wave w of base[i] + sum over the stored (r, j) of
// (|x - m_j|^q_i - |m_j|^q_i); without a mean (mean == base == nullptr) of sum |x|^q_i.
// -inf for a wave without rows.  part: [waves of the grid, nq].
template <bool GRID>
__global__ void __launch_bounds__(256) sp_mu_row_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const double* __restrict__ mean,
    const double* __restrict__ base, const double* __restrict__ q, int nq, double step,
    long long n, double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long w = (long long)blockIdx.x * wpb + (threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * wpb;
  for (int g0 = 0; g0 < nq; g0 += MU_G) {
    const int ng = nq - g0 < MU_G ? nq - g0 : MU_G;
    double best[MU_G];
#pragma unroll
    for (int i = 0; i < MU_G; ++i) best[i] = -__builtin_huge_val();
    for (long long r = w; r < n; r += stride) {
      const long long s = sp_uniform_ll(indptr[r]), e = sp_uniform_ll(indptr[r + 1]);
      double acc[MU_G];
#pragma unroll
      for (int i = 0; i < MU_G; ++i) acc[i] = 0.0;
      for (long long p = s; p < e; p += 64) {
        int col;
        float v;
        const int cnt = sp_load_pairs(indices, data, p, e, lane, col, v);
        if (lane < cnt) {
          double pa[MU_G];
          if (mean) {
            const double m = mean[col];
            double pm[MU_G];
            mu_powers<GRID>(fabs((double)v - m), q, g0, ng, step, pa);
            mu_powers<GRID>(fabs(m), q, g0, ng, step, pm);
#pragma unroll
            for (int i = 0; i < MU_G; ++i) acc[i] += pa[i] - pm[i];
          } else {
            mu_powers<GRID>(fabs((double)v), q, g0, ng, step, pa);
#pragma unroll
            for (int i = 0; i < MU_G; ++i) acc[i] += pa[i];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < MU_G; ++i) {
        if (i < ng) {
          const double t = wave_sum(acc[i]);
          best[i] = fmax(best[i], base ? base[g0 + i] + t : t);
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < MU_G; ++i)
        if (i < ng) part[w * nq + g0 + i] = best[i];
    }
  }
}

// rowmax[i] = max over the waves w of part[w, i]: one wave per exponent
__global__ void __launch_bounds__(64) sp_mu_rowmax_kernel(const double* __restrict__ part,
                                                          long long waves, int nq,
                                                          double* __restrict__ rowmax) {
  const int i = blockIdx.x;
  double best = -__builtin_huge_val();
  for (long long w = threadIdx.x; w < waves; w += 64) best = fmax(best, part[w * nq + i]);
  best = wave_max_d(best);
  if (threadIdx.x == 0) rowmax[i] = best;
}

// Segment g of X^T (nonzeros [seg_start[g], min(seg_start[g] + seg, tptr[j + 1])) of its row
// j = seg_row[g], a column of X): t_i = sum of |x - m_j|^q_i over the segment, plus
// (n - cnt_j) |m_j|^q_i in the first segment of the column.  seg_dst[g] < 0: the column's only
// segment, colsum[i, j] = t_i; otherwise scratch[seg_dst[g], i] = t_i.
template <bool GRID>
__global__ void __launch_bounds__(256) sp_mu_col_kernel(
    const long long* __restrict__ tptr, const float* __restrict__ tdata,
    const long long* __restrict__ seg_row, const long long* __restrict__ seg_start,
    const long long* __restrict__ seg_dst, long long nseg, int seg,
    const double* __restrict__ mean, const double* __restrict__ q, int nq, double step,
    long long n, long long d, double* __restrict__ colsum, double* __restrict__ scratch) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long g = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); g < nseg; g += stride) {
    const long long j = sp_uniform_ll(seg_row[g]);
    const long long s = sp_uniform_ll(seg_start[g]);
    const long long dst = sp_uniform_ll(seg_dst[g]);
    const long long r0 = sp_uniform_ll(tptr[j]), r1 = sp_uniform_ll(tptr[j + 1]);
    const long long e = r1 - s > seg ? s + seg : r1;
    const bool first = mean && s == r0;        // this segment adds the unstored rows' term
    const double m = mean ? mean[j] : 0.0;
    const double rest = (double)(n - (r1 - r0));
    for (int g0 = 0; g0 < nq; g0 += MU_G) {
      const int ng = nq - g0 < MU_G ? nq - g0 : MU_G;
      double acc[MU_G], pm[MU_G];
#pragma unroll
      for (int i = 0; i < MU_G; ++i) acc[i] = 0.0;
      for (long long p = s + lane; p < e; p += 64) {
        double pa[MU_G];
        mu_powers<GRID>(fabs((double)tdata[p] - m), q, g0, ng, step, pa);
#pragma unroll
        for (int i = 0; i < MU_G; ++i) acc[i] += pa[i];
      }
      if (first) mu_powers<GRID>(fabs(m), q, g0, ng, step, pm);
#pragma unroll
      for (int i = 0; i < MU_G; ++i) {
        if (i < ng) {
          double t = wave_sum(acc[i]);
          if (first) t = fma(rest, pm[i], t);
          if (lane == 0) {
            if (dst < 0) colsum[(long long)(g0 + i) * d + j] = t;
            else scratch[dst * nq + g0 + i] = t;
          }
        }
      }
    }
  }
}

// colsum[i, long_row[r]] = scratch[long_ptr[r], i] + ... + scratch[long_ptr[r + 1] - 1, i], in order
__global__ void __launch_bounds__(256) sp_mu_col_reduce_kernel(
    const long long* __restrict__ long_row, const long long* __restrict__ long_ptr,
    long long nlong, const double* __restrict__ scratch, int nq, long long d,
    double* __restrict__ colsum) {
  const long long items = nlong * nq;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const long long r = it / nq;
    const int i = (int)(it - r * nq);
    double acc = 0.0;
    for (long long k = long_ptr[r]; k < long_ptr[r + 1]; ++k) acc += scratch[k * nq + i];
    colsum[(long long)i * d + long_row[r]] = acc;
  }
}

}  // namespace sq

using namespace sq;

// waves of the row pass over n rows: the rows of `part`
extern "C" int sq_sp_mu_row_waves(long long n) { return (int)sp_grid(n, 4) * 4; }

extern "C" int sq_sp_mu_sums(const void* indptr, const void* indices, const void* data,
                             const void* tptr, const void* tdata, const void* seg_row,
                             const void* seg_start, const void* seg_dst, long long nseg, int seg,
                             const void* long_row, const void* long_ptr, long long nlong,
                             long long n, long long d, const void* q, int nq, double qstep,
                             const void* mean, const void* base, void* rowmax, void* colsum,
                             void* part, void* scratch, void* stream) {
  if (n < 1 || d < 1 || nq < 1 || seg < 1 || nseg < d || nlong < 0 || !q || !rowmax || !colsum ||
      !part || (nlong > 0 && !scratch) || ((mean == nullptr) != (base == nullptr)) ||
      (qstep != 0.0 && !(qstep > 0.0)))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const unsigned rgrid = sp_grid(n, 4);
  const bool grid = qstep > 0.0;
#define SQ_MU_ROW(G)                                                                          \
  hipLaunchKernelGGL(sp_mu_row_kernel<G>, dim3(rgrid), dim3(256), 0, s,                       \
                     (const long long*)indptr, (const int*)indices, (const float*)data,       \
                     (const double*)mean, (const double*)base, (const double*)q, nq, qstep, n, \
                     (double*)part)
  if (grid) SQ_MU_ROW(true);
  else SQ_MU_ROW(false);
#undef SQ_MU_ROW
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(sp_mu_rowmax_kernel, dim3(nq), dim3(64), 0, s, (const double*)part,
                     (long long)rgrid * 4, nq, (double*)rowmax);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
#define SQ_MU_COL(G)                                                                          \
  hipLaunchKernelGGL(sp_mu_col_kernel<G>, dim3(sp_grid(nseg, 4)), dim3(256), 0, s,            \
                     (const long long*)tptr, (const float*)tdata, (const long long*)seg_row,  \
                     (const long long*)seg_start, (const long long*)seg_dst, nseg, seg,       \
                     (const double*)mean, (const double*)q, nq, qstep, n, d, (double*)colsum, \
                     (double*)scratch)
  if (grid) SQ_MU_COL(true);
  else SQ_MU_COL(false);
#undef SQ_MU_COL
  rc = (int)hipGetLastError();
  if (rc != 0 || nlong == 0) return rc;
  const long long items = nlong * nq;
  hipLaunchKernelGGL(sp_mu_col_reduce_kernel, dim3(sp_grid(items, 256)), dim3(256), 0, s,
                     (const long long*)long_row, (const long long*)long_ptr, nlong,
                     (const double*)scratch, nq, d, (double*)colsum);
  return (int)hipGetLastError();
}
