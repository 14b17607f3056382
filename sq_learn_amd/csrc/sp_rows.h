// Wave-per-CSR-row helpers of the gather and scatter kernels: included by
// csrc/spkmeans.hip (contiguous row ranges), csrc/spminibatch.hip (row lists),
// csrc/spmm.hip and csrc/spmu.hip (row segments), csrc/splda.hip, csrc/spnmf.hip and
// csrc/splogit.hip (one wave per row, two phases).  Placement rule: anything two sparse .hip
// files need lives here - the readlane broadcast of a row's (col, v) pairs,
// the row-gather accumulation and the tile walk around it, the fixed-point
// scatter, the per-row moments, the fixed-order sum of per-wave partials and
// the persistent grid size.  The inverted-index kernels (spknn.hip,
// spradius.hip) share their accumulate phase through spknn_acc.h instead.
#pragma once
#include "common.h"

namespace sq {

constexpr int SP_T = 4;   // sub-tiles of 64 operand columns per pass over the row
// a lane's SP_T accumulators of one tile, held as one vector value across the walk
typedef double SpAcc __attribute__((ext_vector_type(SP_T)));

SQ_DEV int bcast_i(int v, int q) { return __builtin_amdgcn_readlane(v, q); }
SQ_DEV float bcast_f(float v, int q) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), q));
}
SQ_DEV double bcast_d(double v, int q) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, q);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), q);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
SQ_DEV double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
SQ_DEV double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
SQ_DEV void sp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// a wave-uniform 64-bit value in scalar registers
SQ_DEV long long sp_uniform_ll(long long v) {
  return ((long long)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
         (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

// Where a lane reads sub-tile t of an operand row.  SpPadded: the operand is
// padded to a multiple of 64 columns and the row pointer already points at the
// lane's first column, so the offset is the immediate 64 t.  SpClamped: an
// unpadded operand; off[t] is the lane's column, clamped into the row.
struct SpPadded {
  SQ_DEV int operator()(int t) const { return 64 * t; }
};
struct SpClamped {
  int off[SP_T];
  SQ_DEV int operator()(int t) const { return off[t]; }
};

// acc[t] += sum over the cnt (<= 64) broadcast nonzeros of v * B[col][off(t)];
// lanes >= cnt hold (col 0, v 0), so the 4-wide unroll may overrun cnt.
template <int NT, class Off>
SQ_DEV void sp_accumulate(SpAcc& acc, const double* __restrict__ B, long long ldb,
                          const Off& off, int col, float v, int cnt) {
  for (int q = 0; q < cnt; q += 4) {
    const double* r0 = B + (long long)bcast_i(col, q) * ldb;
    const double* r1 = B + (long long)bcast_i(col, q + 1) * ldb;
    const double* r2 = B + (long long)bcast_i(col, q + 2) * ldb;
    const double* r3 = B + (long long)bcast_i(col, q + 3) * ldb;
    const double v0 = (double)bcast_f(v, q), v1 = (double)bcast_f(v, q + 1);
    const double v2 = (double)bcast_f(v, q + 2), v3 = (double)bcast_f(v, q + 3);
    double x0[NT], x1[NT], x2[NT], x3[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      x0[t] = r0[off(t)];
      x1[t] = r1[off(t)];
      x2[t] = r2[off(t)];
      x3[t] = r3[off(t)];
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

// the lane's (col, v) of the pairs [p, min(p + 64, e)), (0, 0) past the end; returns their count
SQ_DEV int sp_load_pairs(const int* __restrict__ indices, const float* __restrict__ data,
                         long long p, long long e, int lane, int& col, float& v) {
  col = 0;
  v = 0.0f;
  if (p + lane < e) {
    col = indices[p + lane];
    v = data[p + lane];
  }
  return (int)((e - p) < 64 ? (e - p) : 64);
}

// One tile of nt (1 .. SP_T, wave-uniform) sub-tiles: acc += the products of the nonzeros [s, e)
// with their operand rows, 64 pairs at a time.  HELD: (col, v, cnt) are the first 64 pairs,
// which the caller loaded and keeps in registers across its tiles.
// The dispatch on nt is two-way tests on purpose: an equality chain becomes a switch inside the
// loop, the loop is then not unswitched on nt, and spmm_seg_kernel pays 12 VGPRs and two waves
// per SIMD for it (profiles/sparse_refactor.md).
template <bool HELD, class Off>
SQ_DEV void sp_walk(SpAcc& acc, int nt, const double* __restrict__ B, long long ldb,
                    const Off& off, const int* __restrict__ indices,
                    const float* __restrict__ data, long long s, long long e, int lane,
                    int col = 0, float v = 0.0f, int cnt = 0) {
  for (long long p = s; p < e; p += 64) {
    if (!HELD || p > s) cnt = sp_load_pairs(indices, data, p, e, lane, col, v);
    if (nt > 2) {
      if (nt == SP_T) sp_accumulate<SP_T>(acc, B, ldb, off, col, v, cnt);
      else sp_accumulate<3>(acc, B, ldb, off, col, v, cnt);
    } else {
      if (nt == 2) sp_accumulate<2>(acc, B, ldb, off, col, v, cnt);
      else sp_accumulate<1>(acc, B, ldb, off, col, v, cnt);
    }
  }
}

// Fixed-point scatter, one wave per position: w * v of every stored value of a CSR row in
// quanta of 1 / xscale onto qsum[labels[pos]][col], w in quanta of 1 / wscale onto
// qcnt[labels[pos]], by 64-bit integer vector atomics; a label outside [0, k) is skipped.
// LIST = false (Lloyd M-step): position pos is row pos, m == n.  LIST = true (mini-batch): the
// row is rows[pos] (rows == nullptr: row0 + pos), an id outside [0, n) is skipped, and so is a
// position whose weight quantum rounds to zero.  That last rule is the one difference in what
// the two add.  The mini-batch update consumes and clears only the quanta rows of centres with
// a positive weight sum, so there such a position must add nothing at all: value quanta under
// a zero weight sum would stay behind and leak into a later step.  The Lloyd M-step zeroes its
// buffers before every call and converts every row, so a value quantum that survives the
// rounding of a tiny weight stays in the sum.
template <bool LIST>
static __global__ void __launch_bounds__(256) sp_mstep_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const long long* __restrict__ rows, long long row0,
    const int* __restrict__ labels, const double* __restrict__ weights, long long m, long long n,
    int d, int k, double xscale, double wscale, long long* __restrict__ qsum,
    long long* __restrict__ qcnt) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long pos = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); pos < m; pos += stride) {
    const long long i = !LIST ? pos : rows ? rows[pos] : row0 + pos;
    const int lab = labels[pos];
    if ((LIST && (i < 0 || i >= n)) || lab < 0 || lab >= k) continue;
    const double w = weights ? weights[pos] : 1.0;
    const long long qw = __double2ll_rn(w * wscale);
    if (LIST && qw == 0) continue;
    const long long s = indptr[i], e = indptr[i + 1];
    long long* row = qsum + (long long)lab * d;
    for (long long p = s + lane; p < e; p += 64) {
      const int c = indices[p];
      const long long q = __double2ll_rn(w * (double)data[p] * xscale);
      if (q != 0 && c >= 0 && c < d)
        atomicAdd(reinterpret_cast<unsigned long long*>(row + c), (unsigned long long)q);
    }
    if (lane == 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(qcnt + lab), (unsigned long long)qw);
  }
}

// per-row sum of squares, with SUM also the sum: one wave per row, lane l takes the stored
// values l, l + 64, ... in order, then an xor-tree over the lanes
template <bool SUM>
static __global__ void __launch_bounds__(256) sp_row_moments_kernel(
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
      if (SUM) a += v;
      b = fma(v, v, b);
    }
    if (SUM) a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
      if (SUM) sum[i] = a;
      sumsq[i] = b;
    }
  }
}

// fixed-order sum of the per-wave partials (one workgroup)
static __global__ void __launch_bounds__(256) sp_sum_parts_kernel(const double* __restrict__ part,
                                                                  int m, double* __restrict__ out) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) a += part[i];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

}  // namespace sq

// persistent grid: ~8 waves per SIMD lane group per CU, at most 8192 waves
static inline unsigned sp_grid(long long rows, int wpb) {
  const long long blocks = (rows + wpb - 1) / wpb;
  const long long cap = 256LL * 8 * 4 / wpb;
  return (unsigned)(blocks < cap ? (blocks < 1 ? 1 : blocks) : cap);
}
