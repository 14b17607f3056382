// Wave-per-CSR-row helpers shared by csrc/spkmeans.hip (contiguous row
// ranges) and csrc/spminibatch.hip (row lists): the readlane broadcast of a
// row's (col, v) pairs, the CT[d][k_pad] row-gather accumulation, the
// fixed-order sum of per-wave partials and the persistent grid size.
#pragma once
#include "common.h"

namespace sq {

constexpr int SP_T = 4;   // centroid sub-tiles of 64 per pass over the row

SQ_DEV int bcast_i(int v, int q) { return __builtin_amdgcn_readlane(v, q); }
SQ_DEV float bcast_f(float v, int q) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), q));
}
SQ_DEV double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
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

// acc[t] += sum over the cnt (<= 64) broadcast nonzeros of v * CT[col][j0 + lane + 64 t];
// lanes >= cnt hold (col 0, v 0), so the 4-wide unroll may overrun cnt.
template <int NT>
SQ_DEV void sp_accumulate(double (&acc)[SP_T], const double* __restrict__ CTj, long long k_pad,
                          int col, float v, int cnt) {
  for (int q = 0; q < cnt; q += 4) {
    const double* r0 = CTj + (long long)bcast_i(col, q) * k_pad;
    const double* r1 = CTj + (long long)bcast_i(col, q + 1) * k_pad;
    const double* r2 = CTj + (long long)bcast_i(col, q + 2) * k_pad;
    const double* r3 = CTj + (long long)bcast_i(col, q + 3) * k_pad;
    const double v0 = (double)bcast_f(v, q), v1 = (double)bcast_f(v, q + 1);
    const double v2 = (double)bcast_f(v, q + 2), v3 = (double)bcast_f(v, q + 3);
    double x0[NT], x1[NT], x2[NT], x3[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      x0[t] = r0[64 * t];
      x1[t] = r1[64 * t];
      x2[t] = r2[64 * t];
      x3[t] = r3[64 * t];
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
