// CSR sparse k-means / q-means kernels (sparse half).
//
// Reference semantics: ``cluster/_k_means_lloyd.pyx`` lloyd_iter_chunked_sparse
// (distances of CSR rows to dense centres, cluster sums of CSR rows); the
// delta-band label rule is the dense engine's (band.h).
//
// MI355X mapping.
//   E-step (sp_estep_kernel): one wave per CSR row, lanes across centroids.
//     The operand is the transposed centre matrix CT[d][k_pad] (fp64, k_pad a
//     multiple of 64, zero padded): a nonzero (col, v) adds v * CT[col][j] to
//     the accumulator of centroid j, i.e. every nonzero is one contiguous
//     8 * k_pad byte row gather.  The row's (col, v) pairs are loaded 64 at a
//     time (coalesced) and broadcast with readlane so the CT row base is
//     wave-uniform; four CT rows are in flight per wave.  A tile covers
//     64 * SP_T centroids; larger k loops over tiles and re-walks the row
//     (the first 64 nonzeros stay in registers).  Distances
//     D_j = max(xn + cn_j - 2 acc_j, 0) go to a per-wave LDS row of k doubles
//     (band mode) or straight to global memory (gram / sqdist modes).
//   M-step (sp_mstep_kernel of sp_rows.h): w_i * v quantised to 64-bit
//     integer quanta of 2^xexp and added with 64-bit integer vector atomics
//     into a k x d int64 buffer; integer addition commutes, so the sums do not
//     depend on the arrival order or the launch geometry.  sp_mstep_finish
//     converts to fp64.
//   Row norms: sp_row_moments_kernel of sp_rows.h without the sum.
#include "band.h"
#include "sp_rows.h"
#include "sq_api.h"

namespace sq {

// ---------------------------------------------------------------- E-step
// mode 0: band (labels, mind, per-wave inertia partials)
// mode 1: gram   out_f[(i - row0) * ldo + j] = (float) x_i . c_j
// mode 2: sqdist out_d[(i - row0) * ldo + j] = D_j
__global__ void __launch_bounds__(256) sp_estep_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const double* __restrict__ CT, const double* __restrict__ cn,
    const double* __restrict__ xn, long long row0, long long row1, int k, int k_pad, int mode,
    double delta, RngKey key, long long row_offset, int* __restrict__ labels,
    double* __restrict__ mind, double* __restrict__ part, float* __restrict__ out_f,
    double* __restrict__ out_d, long long ldo) {
  extern __shared__ unsigned char sp_smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  double* ld = reinterpret_cast<double*>(sp_smem) + (size_t)wave * (mode == 0 ? k : 0);
  const long long stride = (long long)gridDim.x * wpb;
  double inertia = 0.0;
  for (long long i = row0 + (long long)blockIdx.x * wpb + wave; i < row1; i += stride) {
    // wave-uniform row extent in scalar registers
    const long long s = sp_uniform_ll(indptr[i]);
    const long long e = sp_uniform_ll(indptr[i + 1]);
    const double xi = xn[i];
    // the first 64 nonzeros stay in registers across the centroid tiles
    int col0;
    float v0;
    const int cnt0 = sp_load_pairs(indices, data, s, e, lane, col0, v0);
    double mn = INFINITY;
    for (int j0 = 0; j0 < k_pad; j0 += 64 * SP_T) {
      SpAcc acc = 0.0;
      const int nt = (k_pad - j0) >= 64 * SP_T ? SP_T : (k_pad - j0) / 64;   // wave-uniform
      sp_walk<true>(acc, nt, CT + j0 + lane, k_pad, SpPadded(), indices, data, s, e, lane, col0,
                    v0, cnt0);
#pragma unroll
      for (int t = 0; t < SP_T; ++t) {
        const int j = j0 + lane + 64 * t;
        if (t < nt && j < k) {
          if (mode == 1) {
            out_f[(i - row0) * ldo + j] = (float)acc[t];
          } else {
            double D = (xi + cn[j]) - 2.0 * acc[t];
            D = D > 0.0 ? D : 0.0;
            if (mode == 2) {
              out_d[(i - row0) * ldo + j] = D;
            } else {
              ld[j] = D;
              mn = fmin(mn, D);
            }
          }
        }
      }
    }
    if (mode == 0) {
      sp_wave_sync();
      mn = wave_min_d(mn);
      const double thr = mn + delta;
      const float u = band_u(key, row_offset + i);
      const int lab = band_pick_wave<double>([&](int j) { return ld[j]; }, k, thr, u, lane);
      if (lane == 0) {
        labels[i] = lab;
        mind[i] = mn;
      }
      inertia += mn;
      sp_wave_sync();
    }
  }
  if (mode == 0 && lane == 0) part[(long long)blockIdx.x * wpb + wave] = inertia;
}

// ---------------------------------------------------------------- M-step
__global__ void __launch_bounds__(256) sp_mstep_finish_kernel(
    const long long* __restrict__ qsum, const long long* __restrict__ qcnt, long long kd, int k,
    double xq, double wq, double* __restrict__ sums, double* __restrict__ counts) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < kd; t += stride) {
    sums[t] = (double)qsum[t] * xq;
    if (t < k) counts[t] = (double)qcnt[t] * wq;
  }
}

}  // namespace sq

using namespace sq;

extern "C" int sq_sp_row_norms(const void* indptr, const void* data, void* xn, long long n,
                               void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sp_row_moments_kernel<false>, dim3(sp_grid(n, 4)), dim3(256), 0,
                     (hipStream_t)stream, (const long long*)indptr, (const float*)data,
                     (double*)nullptr, (double*)xn, n);
  return (int)hipGetLastError();
}

// waves per workgroup of the band mode for k centroids (0: k too large)
static int sq_sp_estep_wpb(int k) {
  const size_t row = (size_t)k * sizeof(double);
  int wpb = 4;
  while (wpb > 1 && row * wpb > 160 * 1024) wpb >>= 1;
  return row * wpb > 160 * 1024 ? 0 : wpb;
}

// number of per-wave inertia partials the band mode writes for n rows
extern "C" int sq_sp_estep_parts(long long n, int k) {
  const int wpb = sq_sp_estep_wpb(k);
  if (wpb == 0) return 0;
  return (int)sp_grid(n, wpb) * wpb;
}

extern "C" int sq_sp_estep(const void* indptr, const void* indices, const void* data,
                           const void* CT, const void* cn, const void* xn, long long row0,
                           long long row1, int d, int k, int k_pad, int mode, double delta,
                           unsigned k0, unsigned k1, unsigned s0, unsigned s1,
                           long long row_offset, void* labels, void* mind, void* part,
                           void* inertia, void* out, long long ldo, void* stream) {
  if (row1 <= row0) return 0;
  if (k < 1 || d < 1 || k_pad < k || k_pad % 64 != 0 || mode < 0 || mode > 2)
    return (int)hipErrorInvalidValue;
  if (mode != 0 && ldo < k) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  int wpb = 4;
  size_t lds = 0;
  if (mode == 0) {
    wpb = sq_sp_estep_wpb(k);
    if (wpb == 0) return (int)hipErrorInvalidValue;
    lds = (size_t)k * sizeof(double) * wpb;
    static bool attr = false;
    if (!attr) {
      hipError_t rc = hipFuncSetAttribute((const void*)sp_estep_kernel,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (rc != hipSuccess) return (int)rc;
      attr = true;
    }
  }
  const unsigned grid = sp_grid(row1 - row0, wpb);
  const RngKey key{k0, k1, s0, s1};
  hipLaunchKernelGGL(sp_estep_kernel, dim3(grid), dim3(64 * wpb), lds, s,
                     (const long long*)indptr, (const int*)indices, (const float*)data,
                     (const double*)CT, (const double*)cn, (const double*)xn, row0, row1, k, k_pad,
                     mode, delta, key, row_offset, (int*)labels, (double*)mind, (double*)part,
                     mode == 1 ? (float*)out : nullptr, mode == 2 ? (double*)out : nullptr, ldo);
  int rc = (int)hipGetLastError();
  if (rc != 0 || mode != 0) return rc;
  hipLaunchKernelGGL(sp_sum_parts_kernel, dim3(1), dim3(256), 0, s, (const double*)part,
                     (int)grid * wpb, (double*)inertia);
  return (int)hipGetLastError();
}

// qsum [k * d] and qcnt [k] int64, zeroed by the caller on the same stream
extern "C" int sq_sp_mstep(const void* indptr, const void* indices, const void* data,
                           const void* labels, const void* weights, long long n, int d, int k,
                           int xexp, int wexp, void* qsum, void* qcnt, void* sums, void* counts,
                           void* stream) {
  if (k < 1 || d < 1) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    hipLaunchKernelGGL(sp_mstep_kernel<false>, dim3(sp_grid(n, 4)), dim3(256), 0, s,
                       (const long long*)indptr, (const int*)indices, (const float*)data,
                       (const long long*)nullptr, 0LL, (const int*)labels, (const double*)weights,
                       n, n, d, k, ldexp(1.0, -xexp), ldexp(1.0, -wexp), (long long*)qsum,
                       (long long*)qcnt);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  const long long kd = (long long)k * d;
  const long long blocks = (kd + 255) / 256;
  hipLaunchKernelGGL(sp_mstep_finish_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)),
                     dim3(256), 0, s, (const long long*)qsum, (const long long*)qcnt, kd, k,
                     ldexp(1.0, xexp), ldexp(1.0, wexp), (double*)sums, (double*)counts);
  return (int)hipGetLastError();
}
