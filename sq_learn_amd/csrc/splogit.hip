// Logistic-regression loss kernels on CSR rows (ops/sparse_logistic.py): the
// multinomial and the binary loss with their residuals, and the CSR
// matrix-vector product of the binary gradient and decision function.
//
// Reference semantics: ``linear_model/_logistic.py`` (``_multinomial_loss``,
// ``_logistic_loss_and_grad`` on sparse X through ``safe_sparse_dot``).
//
// MI355X mapping.
//   Multinomial (sp_logit_multi_kernel): one wave per CSR row, lanes across
//     classes.  The logits of 64 * SP_T classes are one sp_walk over the row's
//     entries against the transposed, padded weights (a stored entry is one
//     contiguous row gather, four rows in flight per sub-tile); more classes
//     take more passes over the row.  A running maximum and a running sum of
//     exponentials cross the passes.  With one pass the logits stay in
//     registers; with more they are parked in the row's slice of R and a second
//     phase turns them into the residual, every lane reading back what it wrote
//     itself.  loss_i = sw_i (lse_i - z_i[lab_i]), R[i][c] = sw_i (p_ic -
//     [c == lab_i]).
//   Binary (sp_logit_bin_kernel): one wave per row, lanes across the row's
//     stored entries (lane l takes l, l + 64, ... in order, then an xor tree),
//     gathering from the fp64 weight vector.  With t = +-1: loss_i = sw_i
//     softplus(-t z) in the overflow-safe form, r_i = sw_i (sigmoid(t z) - 1) t
//     as -sw_i t / (1 + exp(t z)).
//   Matrix-vector (sp_matvec_kernel): one wave per row SEGMENT of the table of
//     ops/sparse_linalg.py, lanes across the segment's entries; a row of one
//     segment writes y directly, a longer row one partial per segment, which
//     sp_matvec_reduce_kernel adds in segment order.  On the cached transpose
//     this is X^T r, where a common column is a long row.
//   The per-row losses reach one device scalar through sp_logit_sum_kernel: one
//     workgroup, thread t adds rows t, t + 1024, ... in order, then a tree.
//   No floating-point atomics: every value is a fixed sequence of fp64
//   operations that does not depend on the grid (the product on `seg` alone).
#include <cmath>

#include "sp_rows.h"
#include "sq_api.h"

namespace sq {

constexpr int SP_LOGIT_SUM_THREADS = 1024;

// exp out of line: inlined nine times, its constants fill the scalar registers of the multinomial
// kernel past their limit
static __device__ __attribute__((noinline)) double logit_exp(double x) { return exp(x); }

// the lane's share of sum_p data[p] x[indices[p]] over the entries [s, e): entries s + lane,
// s + lane + 64, ... in order in one accumulator, four gathers issued ahead of their sums; a
// column outside [0, cols) adds nothing
SQ_DEV double logit_lane_dot(const int* __restrict__ indices, const float* __restrict__ data,
                             const double* __restrict__ x, int cols, long long s, long long e,
                             int lane) {
  double a = 0.0;
  long long p = s + lane;
  for (; p + 192 < e; p += 256) {
    int c[4];
    float v[4];
    double y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      c[u] = indices[p + 64 * u];
      v[u] = data[p + 64 * u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) y[u] = (c[u] >= 0 && c[u] < cols) ? x[c[u]] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) a = fma((double)v[u], y[u], a);
  }
  for (; p < e; p += 64) {
    const int c = indices[p];
    if (c >= 0 && c < cols) a = fma((double)data[p], x[c], a);
  }
  return a;
}

// ---------------------------------------------------------------- multinomial
// Wt [cols of X][ldw] holds the K classes in its first K columns, zeros up to ldw >= 64 *
// ceil(K / 64); lab [n] in [0, K); R [n][K]; rowloss [n].
__global__ void __launch_bounds__(256) sp_logit_multi_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const double* __restrict__ Wt, long long ldw,
    const double* __restrict__ bias, const int* __restrict__ lab, const double* __restrict__ sw,
    long long n, int K, double* __restrict__ R, double* __restrict__ rowloss) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  const bool one_pass = K <= 64 * SP_T;
  const SpPadded off;
  for (long long i = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); i < n; i += stride) {
    const long long s = sp_uniform_ll(indptr[i]);
    const long long e = sp_uniform_ll(indptr[i + 1]);
    const int li = lab[i];
    double* __restrict__ r = R + i * K;
    double m = -INFINITY, ssum = 0.0, zl = 0.0;
    SpAcc z = 0.0;
    for (int c0 = 0; c0 < K; c0 += 64 * SP_T) {
      const int left = (K - c0 + 63) / 64;
      const int nt = left < SP_T ? left : SP_T;   // wave-uniform
      SpAcc acc = 0.0;
      sp_walk<false>(acc, nt, Wt + c0 + lane, ldw, off, indices, data, s, e, lane);
      double pm = -INFINITY;
#pragma unroll
      for (int t = 0; t < SP_T; ++t) {
        const int c = c0 + lane + 64 * t;
        const bool ok = t < nt && c < K;
        z[t] = ok ? acc[t] + bias[ok ? c : 0] : -INFINITY;
        pm = fmax(pm, z[t]);
        if (ok && c == li) zl = z[t];
      }
      const double mn = fmax(m, wave_max_d(pm));
      double ps = 0.0;
#pragma unroll
      for (int t = 0; t < SP_T; ++t) ps += logit_exp(z[t] - mn);
      ssum = ssum * logit_exp(m - mn) + wave_sum(ps);
      m = mn;
      if (!one_pass) {
#pragma unroll
        for (int t = 0; t < SP_T; ++t) {
          const int c = c0 + lane + 64 * t;
          if (t < nt && c < K) r[c] = z[t];
        }
      }
    }
    const double lse = m + log(ssum);
    const double w = sw[i];
    zl = wave_sum(zl);   // one lane holds it, the others zero
    if (lane == 0) rowloss[i] = w * (lse - zl);
    if (one_pass) {
#pragma unroll
      for (int t = 0; t < SP_T; ++t) {
        const int c = lane + 64 * t;
        if (c < K) r[c] = w * (logit_exp(z[t] - lse) - (c == li ? 1.0 : 0.0));
      }
    } else {
      for (int c = lane; c < K; c += 64) r[c] = w * (logit_exp(r[c] - lse) - (c == li ? 1.0 : 0.0));
    }
  }
}

// --------------------------------------------------------------------- binary
// w [d]; lab [n] 0 / 1 (anything non-zero is the positive class); r [n]; rowloss [n].
__global__ void __launch_bounds__(256) sp_logit_bin_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const double* __restrict__ w, double b,
    const int* __restrict__ lab, const double* __restrict__ sw, long long n, int d,
    double* __restrict__ r, double* __restrict__ rowloss) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long i = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); i < n; i += stride) {
    const long long s = indptr[i], e = indptr[i + 1];
    const double dot = wave_sum(logit_lane_dot(indices, data, w, d, s, e, lane));
    if (lane == 0) {
      const double t = lab[i] != 0 ? 1.0 : -1.0;
      const double tz = t * (dot + b);
      const double wi = sw[i];
      rowloss[i] = wi * (fmax(-tz, 0.0) + log1p(exp(-fabs(tz))));
      r[i] = -wi * t / (1.0 + exp(tz));
    }
  }
}

// -------------------------------------------------------------- matrix-vector
// segment g: entries [seg_start[g], min(seg_start[g] + seg, indptr[seg_row[g] + 1])) of row
// seg_row[g]; seg_dst[g] < 0: the row's only segment, written to y; otherwise the slot of its
// partial in scratch.
__global__ void __launch_bounds__(256) sp_matvec_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const long long* __restrict__ seg_row,
    const long long* __restrict__ seg_start, const long long* __restrict__ seg_dst,
    long long nseg, int seg, const double* __restrict__ x, int cols, double* __restrict__ y,
    double* __restrict__ scratch) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long g = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); g < nseg; g += stride) {
    const long long row = seg_row[g], s = seg_start[g], dst = seg_dst[g];
    long long e = indptr[row + 1];
    if (e - s > seg) e = s + seg;
    const double a = wave_sum(logit_lane_dot(indices, data, x, cols, s, e, lane));
    if (lane == 0) (dst < 0 ? y[row] : scratch[dst]) = a;
  }
}

// y[long_row[r]] = scratch[long_ptr[r]] + ... + scratch[long_ptr[r + 1] - 1], in order
__global__ void __launch_bounds__(256) sp_matvec_reduce_kernel(
    const long long* __restrict__ long_row, const long long* __restrict__ long_ptr,
    long long nlong, const double* __restrict__ scratch, double* __restrict__ y) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < nlong; r += stride) {
    const long long a = long_ptr[r], b = long_ptr[r + 1];
    double acc = 0.0;
    long long q = a;
    for (; q + 4 <= b; q += 4) {     // four loads in flight, one addition chain
      const double p0 = scratch[q], p1 = scratch[q + 1], p2 = scratch[q + 2], p3 = scratch[q + 3];
      acc = (((acc + p0) + p1) + p2) + p3;
    }
    for (; q < b; ++q) acc += scratch[q];
    y[long_row[r]] = acc;
  }
}

// ------------------------------------------------------------------- loss sum
// out[0] = the sum of v [n] in a fixed order (one workgroup): thread t adds the elements t,
// t + 1024, ... in order, eight loads issued ahead of their sums, then a tree over the threads
__global__ void __launch_bounds__(SP_LOGIT_SUM_THREADS) sp_logit_sum_kernel(
    const double* __restrict__ v, long long n, double* __restrict__ out) {
  constexpr int T = SP_LOGIT_SUM_THREADS;
  __shared__ double sh[T];
  double a = 0.0;
  long long i = threadIdx.x;
  for (; i + 7LL * T < n; i += 8LL * T) {
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = v[i + (long long)u * T];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += x[u];
  }
  for (; i < n; i += T) a += v[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

}  // namespace sq

using namespace sq;

static int logit_loss_sum(const void* rowloss, long long n, void* loss, hipStream_t s) {
  hipLaunchKernelGGL(sp_logit_sum_kernel, dim3(1), dim3(SP_LOGIT_SUM_THREADS), 0, s,
                     (const double*)rowloss, n, (double*)loss);
  return (int)hipGetLastError();
}

// classes one pass over a row covers (more classes re-walk the row)
extern "C" int sq_sp_logit_tile_classes() { return 64 * SP_T; }

extern "C" int sq_sp_logit_multi(const void* indptr, const void* indices, const void* data,
                                 const void* Wt, long long ldw, const void* bias, const void* lab,
                                 const void* sw, long long n, int K, void* R, void* rowloss,
                                 void* loss, void* stream) {
  if (K < 1 || n < 0 || ldw < 64LL * ((K + 63) / 64) || !indptr || !Wt || !bias || !loss ||
      (n > 0 && (!lab || !sw || !R || !rowloss)))   // indices / data are null without entries
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    hipLaunchKernelGGL(sp_logit_multi_kernel, dim3(sp_grid(n, 4)), dim3(256), 0, s,
                       (const long long*)indptr, (const int*)indices, (const float*)data,
                       (const double*)Wt, ldw, (const double*)bias, (const int*)lab,
                       (const double*)sw, n, K, (double*)R, (double*)rowloss);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  return logit_loss_sum(rowloss, n, loss, s);
}

extern "C" int sq_sp_logit_bin(const void* indptr, const void* indices, const void* data,
                               const void* w, double b, const void* lab, const void* sw,
                               long long n, int d, void* r, void* rowloss, void* loss,
                               void* stream) {
  if (d < 1 || n < 0 || !indptr || !w || !loss || (n > 0 && (!lab || !sw || !r || !rowloss)))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    hipLaunchKernelGGL(sp_logit_bin_kernel, dim3(sp_grid(n, 4)), dim3(256), 0, s,
                       (const long long*)indptr, (const int*)indices, (const float*)data,
                       (const double*)w, b, (const int*)lab, (const double*)sw, n, d, (double*)r,
                       (double*)rowloss);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  return logit_loss_sum(rowloss, n, loss, s);
}

extern "C" int sq_sp_matvec(const void* indptr, const void* indices, const void* data,
                            const void* seg_row, const void* seg_start, const void* seg_dst,
                            long long nseg, int seg, const void* long_row, const void* long_ptr,
                            long long nlong, const void* x, int cols, void* y, void* scratch,
                            void* stream) {
  if (nseg <= 0) return 0;
  if (seg < 1 || cols < 1 || nlong < 0 || !indptr || !seg_row || !seg_start || !seg_dst || !x ||
      !y || (nlong > 0 && (!scratch || !long_row || !long_ptr)))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sp_matvec_kernel, dim3(sp_grid(nseg, 4)), dim3(256), 0, s,
                     (const long long*)indptr, (const int*)indices, (const float*)data,
                     (const long long*)seg_row, (const long long*)seg_start,
                     (const long long*)seg_dst, nseg, seg, (const double*)x, cols, (double*)y,
                     (double*)scratch);
  const int rc = (int)hipGetLastError();
  if (rc != 0 || nlong == 0) return rc;
  hipLaunchKernelGGL(sp_matvec_reduce_kernel, dim3(sp_grid(nlong, 256)), dim3(256), 0, s,
                     (const long long*)long_row, (const long long*)long_ptr, nlong,
                     (const double*)scratch, (double*)y);
  return (int)hipGetLastError();
}
