// Kernel matrices of CSR queries against a CSR fit set (SURVEY.md E4/E5, K17,
// sparse half): K(q_i, x_j) for the linear, polynomial, rbf and sigmoid
// kernels, written out or applied to vectors without being formed.
//
// Reference semantics: ``metrics/pairwise.py`` linear_kernel /
// polynomial_kernel / rbf_kernel / sigmoid_kernel on sparse input
// (``safe_sparse_dot``, then the elementwise function), as the least-squares
// SVMs of ``svm/_classes.py`` and ``svm/_qSVM.py`` use them.
//
// Operands: those of spknn.hip (CSR queries, the transposed fit set and its
// tile pointer table, the squared row norms of both sides, one fixed-point
// exponent per query row).  The inner products are accumulated by the phase
// the k-NN and radius kernels share (spknn_acc.h): 64-bit integer quanta,
// integer LDS atomics, results independent of arrival order and launch
// geometry.  The kernel functions are those of spgram.h.
//
// MI355X mapping.
//   sp_gram_kernel (matrix mode): one workgroup of four waves per (query row,
//     fit tile of T rows), grid and LDS accumulators as in sp_knn_kernel.
//     After the accumulate phase the threads run across the tile and store
//     K[q, base + j] to out + q * ld + base + j: ld is the caller's row
//     stride, so out may be a view into a larger matrix (the K block of the
//     LS-SVM system).  In a self-join the pair (q, q) is at distance exactly 0
//     for rbf and takes the addend diag_add.
//   sp_gram_matvec_kernel (apply mode): the same grid.  After the accumulate
//     phase every thread sums K[q, base + j] * V[base + j, r] serially over
//     j = tid, tid + 256, ..., a fixed xor butterfly adds the 64 lanes of a
//     wave, the four wave sums pass through LDS and are added in wave order:
//     one partial per (query, tile, r).  The kernel values never reach memory.
//   sp_gram_reduce_kernel: one thread per (query, r) adds the partials of the
//     query in ascending tile order.
//
// No floating-point atomics: results are bit-identical from run to run for a
// given T and independent of how the queries are cut into launches.  LDS:
// 8 T bytes of accumulators plus the four wave sums (128 bytes); T <= 8192
// keeps two workgroups on a CU, as for sp_knn_kernel.
#include "spgram.h"
#include "spknn_acc.h"
#include "sq_api.h"

namespace sq {

// grid: m * ntiles workgroups, workgroup b serves query q0 + b / ntiles and
// tile b % ntiles.  out: row q of the whole result at out + q * ld.
__global__ void __launch_bounds__(64 * SPKNN_WAVES) sp_gram_kernel(
    const long long* __restrict__ qptr, const int* __restrict__ qidx,
    const float* __restrict__ qval, const int* __restrict__ trow, const float* __restrict__ tval,
    const long long* __restrict__ tab, const double* __restrict__ qn,
    const double* __restrict__ xn, const int* __restrict__ qexp, long long q0, long long n, int d,
    int T, long long ntiles, long long nnz_x, int kind, double gamma, double coef0, double degree,
    int self_join, double diag_add, double* __restrict__ out, long long ld) {
  extern __shared__ unsigned char spgram_smem[];
  long long* acc = reinterpret_cast<long long*>(spgram_smem);
  const int tid = threadIdx.x;
  const long long ql = blockIdx.x / ntiles;          // query inside the chunk
  const long long t = blockIdx.x - ql * ntiles;
  const long long q = q0 + ql;
  const long long base = t * T;                      // first fit row of the tile
  const int nv = (int)((n - base) < T ? (n - base) : T);

  const int ex = qexp[q];
  knn_accumulate(acc, qptr, qidx, qval, trow, tval, tab, q, t, base, nv, ex, d, T, ntiles, nnz_x);

  const double quantum = ldexp(1.0, ex);
  const double qi = qn[q];
  const long long own = self_join ? q : -1;           // the fit row that is the query itself
  double* row = out + q * ld + base;
  for (int j = tid; j < nv; j += 64 * SPKNN_WAVES) {
    const bool self = base + j == own;
    double v = (self && kind == 2)
                   ? kernel_rbf(gamma, 0.0)
                   : kernel_value(kind, (double)acc[j] * quantum, qi, xn[base + j], gamma, coef0,
                                  degree);
    if (self) v += diag_add;
    row[j] = v;
  }
}

// grid as above.  V [n, R] row-major; part [m, ntiles, R]: the partial of
// workgroup b at part + b * R.
__global__ void __launch_bounds__(64 * SPKNN_WAVES) sp_gram_matvec_kernel(
    const long long* __restrict__ qptr, const int* __restrict__ qidx,
    const float* __restrict__ qval, const int* __restrict__ trow, const float* __restrict__ tval,
    const long long* __restrict__ tab, const double* __restrict__ qn,
    const double* __restrict__ xn, const int* __restrict__ qexp, long long q0, long long n, int d,
    int T, long long ntiles, long long nnz_x, int kind, double gamma, double coef0, double degree,
    int self_join, const double* __restrict__ V, int R, double* __restrict__ part) {
  extern __shared__ unsigned char spgram_smem[];
  long long* acc = reinterpret_cast<long long*>(spgram_smem);
  double* wsum = reinterpret_cast<double*>(acc + T);    // [WAVES][RMAX]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const long long ql = blockIdx.x / ntiles;
  const long long t = blockIdx.x - ql * ntiles;
  const long long q = q0 + ql;
  const long long base = t * T;
  const int nv = (int)((n - base) < T ? (n - base) : T);

  const int ex = qexp[q];
  knn_accumulate(acc, qptr, qidx, qval, trow, tval, tab, q, t, base, nv, ex, d, T, ntiles, nnz_x);

  const double quantum = ldexp(1.0, ex);
  const double qi = qn[q];
  const long long own = self_join ? q : -1;
  double s[SPGRAM_RMAX] = {0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < nv; j += 64 * SPKNN_WAVES) {
    const double v = (base + j == own && kind == 2)
                         ? kernel_rbf(gamma, 0.0)
                         : kernel_value(kind, (double)acc[j] * quantum, qi, xn[base + j], gamma,
                                        coef0, degree);
    const double* vr = V + (base + j) * R;
#pragma unroll
    for (int r = 0; r < SPGRAM_RMAX; ++r)
      if (r < R) s[r] = __dadd_rn(s[r], __dmul_rn(v, vr[r]));
  }
#pragma unroll
  for (int r = 0; r < SPGRAM_RMAX; ++r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[r] += __shfl_xor(s[r], o, 64);
    if (lane == 0) wsum[wave * SPGRAM_RMAX + r] = s[r];
  }
  __syncthreads();
  if (tid < R) {
    double total = wsum[tid];
#pragma unroll
    for (int w = 1; w < SPKNN_WAVES; ++w) total += wsum[w * SPGRAM_RMAX + tid];
    part[(long long)blockIdx.x * R + tid] = total;
  }
}

// one thread per (query of the chunk, r): the partials in ascending tile order
__global__ void __launch_bounds__(256) sp_gram_reduce_kernel(
    const double* __restrict__ part, long long q0, long long m, long long ntiles, int R,
    double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m * R) return;
  const long long ql = i / R;
  const int r = (int)(i - ql * R);
  const double* p = part + ql * ntiles * R + r;
  double total = 0.0;
  for (long long t = 0; t < ntiles; ++t) total += p[t * R];
  out[(q0 + ql) * R + r] = total;
}

}  // namespace sq

using namespace sq;

static bool sp_gram_args_ok(long long q0, long long m, long long n, int d, int T, long long nnz_x,
                            int kind, int self_join) {
  if (n < 1 || n >= (1LL << 31) || d < 1 || T < 1 || T > sq_sp_knn_tile_max() || q0 < 0 ||
      nnz_x < 0 || kind < 0 || kind >= SPGRAM_KINDS || (self_join && q0 + m > n))
    return false;
  const long long ntiles = (n + T - 1) / T;
  return m * ntiles < (1LL << 31);
}

template <class K>
static hipError_t sp_gram_lds(K kernel, bool* done) {
  if (*done) return hipSuccess;
  hipError_t rc = hipFuncSetAttribute(
      (const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)(SPKNN_TMAX * sizeof(long long) + SPKNN_WAVES * SPGRAM_RMAX * sizeof(double)));
  *done = rc == hipSuccess;
  return rc;
}

// Queries q0 .. q0 + m of the CSR (qptr, qidx, qval) against the transposed
// fit set (trow, tval: nnz_x entries) with its tile table tab [d * ntiles + 1]:
// K[q, j] in fp64 to out + q * ld + j for the rows q of the launch (out is the
// first row of the whole result, ld >= n its row stride in elements).
// self_join: query row i is fit row i, at distance 0 from itself (rbf), and
// K[i, i] takes the addend diag_add.
extern "C" int sq_sp_gram(const void* qptr, const void* qidx, const void* qval, const void* trow,
                          const void* tval, const void* tab, const void* qn, const void* xn,
                          const void* qexp, long long q0, long long m, long long n, int d, int T,
                          long long nnz_x, int kind, double gamma, double coef0, double degree,
                          int self_join, double diag_add, void* out, long long ld, void* stream) {
  if (!sp_gram_args_ok(q0, m, n, d, T, nnz_x, kind, self_join) || ld < n ||
      (diag_add != 0.0 && !self_join))
    return (int)hipErrorInvalidValue;
  if (m <= 0) return 0;
  const long long ntiles = (n + T - 1) / T;
  static bool attr = false;
  hipError_t rc = sp_gram_lds(sp_gram_kernel, &attr);
  if (rc != hipSuccess) return (int)rc;
  const size_t lds = (size_t)T * sizeof(long long) + SPKNN_WAVES * SPGRAM_RMAX * sizeof(double);
  hipLaunchKernelGGL(sp_gram_kernel, dim3((unsigned)(m * ntiles)), dim3(64 * SPKNN_WAVES), lds,
                     (hipStream_t)stream, (const long long*)qptr, (const int*)qidx,
                     (const float*)qval, (const int*)trow, (const float*)tval,
                     (const long long*)tab, (const double*)qn, (const double*)xn,
                     (const int*)qexp, q0, n, d, T, ntiles, nnz_x, kind, gamma, coef0, degree,
                     self_join ? 1 : 0, diag_add, (double*)out, ld);
  return (int)hipGetLastError();
}

// sum_j K[q, j] V[j, r] for the rows q of the launch: V [n, R] row-major fp64,
// part [m, ntiles, R] scratch, out [>= q0 + m, R] (the first row of the whole
// result).
extern "C" int sq_sp_gram_matvec(const void* qptr, const void* qidx, const void* qval,
                                 const void* trow, const void* tval, const void* tab,
                                 const void* qn, const void* xn, const void* qexp, long long q0,
                                 long long m, long long n, int d, int T, long long nnz_x, int kind,
                                 double gamma, double coef0, double degree, int self_join,
                                 const void* V, int R, void* part, void* out, void* stream) {
  if (!sp_gram_args_ok(q0, m, n, d, T, nnz_x, kind, self_join) || R < 1 || R > SPGRAM_RMAX)
    return (int)hipErrorInvalidValue;
  if (m <= 0) return 0;
  const long long ntiles = (n + T - 1) / T;
  static bool attr = false;
  hipError_t rc = sp_gram_lds(sp_gram_matvec_kernel, &attr);
  if (rc != hipSuccess) return (int)rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)T * sizeof(long long) + SPKNN_WAVES * SPGRAM_RMAX * sizeof(double);
  hipLaunchKernelGGL(sp_gram_matvec_kernel, dim3((unsigned)(m * ntiles)), dim3(64 * SPKNN_WAVES),
                     lds, s, (const long long*)qptr, (const int*)qidx, (const float*)qval,
                     (const int*)trow, (const float*)tval, (const long long*)tab,
                     (const double*)qn, (const double*)xn, (const int*)qexp, q0, n, d, T, ntiles,
                     nnz_x, kind, gamma, coef0, degree, self_join ? 1 : 0, (const double*)V, R,
                     (double*)part);
  int err = (int)hipGetLastError();
  if (err != 0) return err;
  hipLaunchKernelGGL(sp_gram_reduce_kernel, dim3((unsigned)((m * R + 255) / 256)), dim3(256), 0, s,
                     (const double*)part, q0, m, ntiles, R, (double*)out);
  return (int)hipGetLastError();
}
