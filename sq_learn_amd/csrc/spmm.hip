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
//     flight per wave.  A pass covers 64 * SPMM_T columns; wider B loops over
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
//   sp_row_moments_kernel: per-row sum and sum of squares (one wave per row,
//     fixed lane partition, xor-tree): on X^T these are the column moments.
#include "common.h"

namespace sq {

constexpr int SPMM_T = 4;   // column sub-tiles of 64 per pass over the segment

SQ_DEV int spmm_bcast_i(int v, int q) { return __builtin_amdgcn_readlane(v, q); }
SQ_DEV float spmm_bcast_f(float v, int q) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), q));
}
// a wave-uniform 64-bit value in scalar registers
SQ_DEV long long spmm_uniform(long long v) {
  return ((long long)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
         (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

// acc[t] += sum over the cnt (<= 64) broadcast nonzeros of v * B[col][off[t]];
// lanes >= cnt hold (col 0, v 0), so the 4-wide unroll may overrun cnt.
template <int NT>
SQ_DEV void spmm_accumulate(double (&acc)[SPMM_T], const double* __restrict__ B, long long ldb,
                            const int (&off)[SPMM_T], int col, float v, int cnt) {
  for (int q = 0; q < cnt; q += 4) {
    const double* r0 = B + (long long)spmm_bcast_i(col, q) * ldb;
    const double* r1 = B + (long long)spmm_bcast_i(col, q + 1) * ldb;
    const double* r2 = B + (long long)spmm_bcast_i(col, q + 2) * ldb;
    const double* r3 = B + (long long)spmm_bcast_i(col, q + 3) * ldb;
    const double v0 = (double)spmm_bcast_f(v, q), v1 = (double)spmm_bcast_f(v, q + 1);
    const double v2 = (double)spmm_bcast_f(v, q + 2), v3 = (double)spmm_bcast_f(v, q + 3);
    double x0[NT], x1[NT], x2[NT], x3[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      x0[t] = r0[off[t]];
      x1[t] = r1[off[t]];
      x2[t] = r2[off[t]];
      x3[t] = r3[off[t]];
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[t] = fma(v0, x0[t], acc[t]);
      acc[t] = fma(v1, x1[t], acc[t]);
      acc[t] = fma(v2, x2[t], acc[t]);
      acc[t] = fma(v3, x3[t], acc[t]);
    }
  }
}

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
    const long long row = spmm_uniform(seg_row[g]);
    const long long s = spmm_uniform(seg_start[g]);
    const long long dst = spmm_uniform(seg_dst[g]);
    long long e = spmm_uniform(indptr[row + 1]);
    if (e - s > seg) e = s + seg;
    double* o = dst < 0 ? out + row * ldo : scratch + dst * (long long)l;
    for (int j0 = 0; j0 < l; j0 += 64 * SPMM_T) {
      double acc[SPMM_T];
      int off[SPMM_T];
#pragma unroll
      for (int t = 0; t < SPMM_T; ++t) {
        acc[t] = 0.0;
        const int j = j0 + lane + 64 * t;
        off[t] = j < l ? j : l - 1;
      }
      const int left = (l - j0 + 63) / 64;
      const int nt = left < SPMM_T ? left : SPMM_T;   // wave-uniform
      for (long long p = s; p < e; p += 64) {
        int col = 0;
        float v = 0.0f;
        if (p + lane < e) {
          col = indices[p + lane];
          v = data[p + lane];
        }
        const int cnt = (int)((e - p) < 64 ? (e - p) : 64);
        if (nt == SPMM_T) spmm_accumulate<SPMM_T>(acc, B, ldb, off, col, v, cnt);
        else if (nt == 3) spmm_accumulate<3>(acc, B, ldb, off, col, v, cnt);
        else if (nt == 2) spmm_accumulate<2>(acc, B, ldb, off, col, v, cnt);
        else spmm_accumulate<1>(acc, B, ldb, off, col, v, cnt);
      }
#pragma unroll
      for (int t = 0; t < SPMM_T; ++t) {
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

__global__ void __launch_bounds__(256) sp_row_moments_kernel(
    const long long* __restrict__ indptr, const float* __restrict__ data,
    double* __restrict__ sum, double* __restrict__ sumsq, long long n) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long i = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); i < n; i += stride) {
    const long long s = indptr[i], e = indptr[i + 1];
    double a = 0.0, b = 0.0;
    for (long long p = s + lane; p < e; p += 64) {
      const double v = (double)data[p];
      a += v;
      b = fma(v, v, b);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
      sum[i] = a;
      sumsq[i] = b;
    }
  }
}

}  // namespace sq

using namespace sq;

// persistent grid: at most ~8 waves per SIMD on 256 CUs
static unsigned spmm_grid(long long waves) {
  const long long blocks = (waves + 3) / 4;
  const long long cap = 256LL * 8;
  return (unsigned)(blocks < cap ? (blocks < 1 ? 1 : blocks) : cap);
}

// columns one pass over a segment covers (wider B re-walks the segment)
extern "C" int sq_spmm_tile_cols() { return 64 * SPMM_T; }

extern "C" int sq_spmm(const void* indptr, const void* indices, const void* data,
                       const void* seg_row, const void* seg_start, const void* seg_dst,
                       long long nseg, int seg, const void* long_row, const void* long_ptr,
                       long long nlong, const void* B, long long ldb, int l, void* out,
                       long long ldo, void* scratch, void* stream) {
  if (nseg <= 0) return 0;
  if (l < 1 || seg < 1 || ldb < l || ldo < l || nlong < 0 || (nlong > 0 && scratch == nullptr))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(spmm_seg_kernel, dim3(spmm_grid(nseg)), dim3(256), 0, s,
                     (const long long*)indptr, (const int*)indices, (const float*)data,
                     (const long long*)seg_row, (const long long*)seg_start,
                     (const long long*)seg_dst, nseg, seg, (const double*)B, ldb, l, (double*)out,
                     ldo, (double*)scratch);
  int rc = (int)hipGetLastError();
  if (rc != 0 || nlong == 0) return rc;
  const long long items = nlong * ((l + 63) / 64);
  hipLaunchKernelGGL(spmm_reduce_kernel, dim3(spmm_grid(items)), dim3(256), 0, s,
                     (const long long*)long_row, (const long long*)long_ptr, nlong,
                     (const double*)scratch, l, (double*)out, ldo);
  return (int)hipGetLastError();
}

extern "C" int sq_sp_row_moments(const void* indptr, const void* data, void* sum, void* sumsq,
                                 long long n, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sp_row_moments_kernel, dim3(spmm_grid(n)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)indptr, (const float*)data, (double*)sum, (double*)sumsq,
                     n);
  return (int)hipGetLastError();
}
