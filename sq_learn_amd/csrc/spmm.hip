// CSR sparse-times-dense products in fp64: the row passes of
// the randomized SVD on sparse input (ops/sparse_linalg.py).
//
//   out[r, j] = sum over the nonzeros p of row r of (double)data[p] * B[indices[p], j],  j < l
//
// One kernel serves Y = X W (run on X) and Z = X^T Y (run on the CSR of X^T,
// built once per matrix): both are gathers, nothing is scattered and there
// are no floating-point atomics.
//
// MI355X mapping.
//   spmm_seg_kernel: the unit of work is a row SEGMENT of at most `seg`
//     nonzeros (segment table built from indptr by the caller), one wave per
//     segment, lanes across the columns of B: a nonzero (col, v) adds
//     v * B[col][j] to the accumulator of column j, one contiguous row gather.
//     The (col, v) pairs are loaded 64 at a time (coalesced) and broadcast
//     with readlane, so the B row base is wave-uniform; four B rows are in
//     flight per wave.  A pass covers 64 * SP_T columns; wider B loops over
//     column tiles and re-walks the segment.  Lanes past l load column l - 1
//     (in bounds) and store nothing.  A row of one segment writes `out`
//     directly (an empty row writes zeros); a longer row writes one partial
//     per segment into a scratch buffer.
//   spmm_reduce_kernel: one wave per (long row, 64-column tile) adds the
//     row's partials in segment order.
//   The value of every output element is a fixed sequence of fp64 FMAs (inside
//     a segment, in storage order) and additions (across segments, in segment
//     order) that depends on `seg` alone - not on the grid, not on which wave
//     picks up which segment.
//   sp_row_moments_kernel (sp_rows.h): per-row sum and sum of squares; on X^T
//     these are the column moments.
// The segment walk is sp_walk of sp_rows.h with the clamped column offsets.
#include "sp_rows.h"
#include "sq_api.h"

namespace sq {

// segment g: nonzeros [seg_start[g], min(seg_start[g] + seg, indptr[seg_row[g] + 1])) of row
// seg_row[g]; seg_dst[g] < 0: the row's only segment, written to out; otherwise the slot of its
// partial in scratch [slots, l].
__global__ void __launch_bounds__(256) spmm_seg_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const long long* __restrict__ seg_row,
    const long long* __restrict__ seg_start, const long long* __restrict__ seg_dst,
    long long nseg, int seg, const double* __restrict__ B, long long ldb, int l,
    double* __restrict__ out, long long ldo, double* __restrict__ scratch) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long g = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); g < nseg; g += stride) {
    const long long row = sp_uniform_ll(seg_row[g]);
    const long long s = sp_uniform_ll(seg_start[g]);
    const long long dst = sp_uniform_ll(seg_dst[g]);
    long long e = sp_uniform_ll(indptr[row + 1]);
    if (e - s > seg) e = s + seg;
    double* o = dst < 0 ? out + row * ldo : scratch + dst * (long long)l;
    for (int j0 = 0; j0 < l; j0 += 64 * SP_T) {
      SpAcc acc = 0.0;
      SpClamped off;
#pragma unroll
      for (int t = 0; t < SP_T; ++t) {
        const int j = j0 + lane + 64 * t;
        off.off[t] = j < l ? j : l - 1;
      }
      const int left = (l - j0 + 63) / 64;
      const int nt = left < SP_T ? left : SP_T;   // wave-uniform
      sp_walk<false>(acc, nt, B, ldb, off, indices, data, s, e, lane);
#pragma unroll
      for (int t = 0; t < SP_T; ++t) {
        const int j = j0 + lane + 64 * t;
        if (t < nt && j < l) o[j] = acc[t];
      }
    }
  }
}

// out[long_row[r], j] = scratch[long_ptr[r]][j] + ... + scratch[long_ptr[r + 1] - 1][j], in order
__global__ void __launch_bounds__(256) spmm_reduce_kernel(
    const long long* __restrict__ long_row, const long long* __restrict__ long_ptr,
    long long nlong, const double* __restrict__ scratch, int l, double* __restrict__ out,
    long long ldo) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long ctiles = (l + 63) / 64;
  const long long items = nlong * ctiles;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long it = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); it < items; it += stride) {
    const long long r = it / ctiles;
    const int j = (int)(it - r * ctiles) * 64 + lane;
    if (j >= l) continue;
    const long long a = long_ptr[r], b = long_ptr[r + 1];
    const double* __restrict__ src = scratch + j;
    double acc = 0.0;
    long long q = a;
    for (; q + 4 <= b; q += 4) {     // four loads in flight, one addition chain
      const double p0 = src[q * l], p1 = src[(q + 1) * l];
      const double p2 = src[(q + 2) * l], p3 = src[(q + 3) * l];
      acc = (((acc + p0) + p1) + p2) + p3;
    }
    for (; q < b; ++q) acc += src[q * l];
    out[long_row[r] * ldo + j] = acc;
  }
}

}  // namespace sq

using namespace sq;

// columns one pass over a segment covers (wider B re-walks the segment)
extern "C" int sq_spmm_tile_cols() { return 64 * SP_T; }

extern "C" int sq_spmm(const void* indptr, const void* indices, const void* data,
                       const void* seg_row, const void* seg_start, const void* seg_dst,
                       long long nseg, int seg, const void* long_row, const void* long_ptr,
                       long long nlong, const void* B, long long ldb, int l, void* out,
                       long long ldo, void* scratch, void* stream) {
  if (nseg <= 0) return 0;
  if (l < 1 || seg < 1 || ldb < l || ldo < l || nlong < 0 || (nlong > 0 && scratch == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(spmm_seg_kernel, dim3(sp_grid(nseg, 4)), dim3(256), 0, s,
                     (const long long*)indptr, (const int*)indices, (const float*)data,
                     (const long long*)seg_row, (const long long*)seg_start,
                     (const long long*)seg_dst, nseg, seg, (const double*)B, ldb, l, (double*)out,
                     ldo, (double*)scratch);
  int rc = (int)hipGetLastError();
  if (rc != 0 || nlong == 0) return rc;
  const long long items = nlong * ((l + 63) / 64);
  hipLaunchKernelGGL(spmm_reduce_kernel, dim3(sp_grid(items, 4)), dim3(256), 0, s,
                     (const long long*)long_row, (const long long*)long_ptr, nlong,
                     (const double*)scratch, l, (double*)out, ldo);
  return (int)hipGetLastError();
}

extern "C" int sq_sp_row_moments(const void* indptr, const void* data, void* sum, void* sumsq,
                                 long long n, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sp_row_moments_kernel<true>, dim3(sp_grid(n, 4)), dim3(256), 0,
                     (hipStream_t)stream, (const long long*)indptr, (const float*)data,
                     (double*)sum, (double*)sumsq, n);
  return (int)hipGetLastError();
}
