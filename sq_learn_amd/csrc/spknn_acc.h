// The accumulate phase of the inverted-index kernels, shared by the sparse
// k-NN kernel (spknn.hip) and the sparse radius-neighbour kernels
// (spradius.hip): the T inner products of one (query row, fit tile) pair as
// 64-bit integer quanta of 2^e in LDS, and the distance epilogue on one of
// them.  Operands and the MI355X mapping are described in spknn.hip.
#pragma once
#include "common.h"

namespace sq {

constexpr int SPKNN_WAVES = 4;
constexpr int SPKNN_TMAX = 8192;
constexpr int SPKNN_LONG = 256;      // slice entries from which the waves share a slice

// metric 0: squared euclidean, metric 1: cosine distance
SQ_DEV double knn_distance(int metric, double dot, double qn, double sq, double xn) {
  if (metric == 0) {
    const double D = (qn + xn) - 2.0 * dot;
    return D > 0.0 ? D : 0.0;
  }
  if (qn == 0.0 || xn == 0.0) return 1.0;
  const double D = 1.0 - dot / (sq * sqrt(xn));
  return D < 0.0 ? 0.0 : (D > 2.0 ? 2.0 : D);
}

// one entry of a column slice: round(v * xv) quanta onto its row's accumulator
SQ_DEV void knn_add(long long* acc, int row, float xv, double v, long long base, int nv) {
  const long long r = (long long)row - base;
  const long long quanta = __double2ll_rn(v * (double)xv);
  if (quanta != 0 && r >= 0 && r < nv)
    atomicAdd(reinterpret_cast<unsigned long long*>(acc + r), (unsigned long long)quanta);
}

// the entries a + first, a + first + STRIDE, ... of the slice [a, b); four
// loads are in flight before their adds
template <int STRIDE>
SQ_DEV void knn_scatter(long long* acc, const int* __restrict__ trow,
                        const float* __restrict__ tval, long long a, long long b, int first,
                        double v, long long base, int nv) {
  long long z = a + first;
  for (; z + 3 * STRIDE < b; z += 4 * STRIDE) {
    const int r0 = trow[z], r1 = trow[z + STRIDE], r2 = trow[z + 2 * STRIDE],
              r3 = trow[z + 3 * STRIDE];
    const float x0 = tval[z], x1 = tval[z + STRIDE], x2 = tval[z + 2 * STRIDE],
                x3 = tval[z + 3 * STRIDE];
    knn_add(acc, r0, x0, v, base, nv);
    knn_add(acc, r1, x1, v, base, nv);
    knn_add(acc, r2, x2, v, base, nv);
    knn_add(acc, r3, x3, v, base, nv);
  }
  for (; z < b; z += STRIDE) knn_add(acc, trow[z], tval[z], v, base, nv);
}

// The inner products of query row q with the nv fit rows of tile t (first
// fit row ``base``) into acc[0 .. T), by the whole workgroup of SPKNN_WAVES
// waves; ends with a barrier.  ``ex`` is the query row's exponent: acc[j] *
// 2^ex is the inner product.
SQ_DEV void knn_accumulate(long long* acc, const long long* __restrict__ qptr,
                           const int* __restrict__ qidx, const float* __restrict__ qval,
                           const int* __restrict__ trow, const float* __restrict__ tval,
                           const long long* __restrict__ tab, long long q, long long t,
                           long long base, int nv, int ex, int d, int T, long long ntiles,
                           long long nnz_x) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // every accumulator of the tile is zeroed, the unused tail of a short last
  // tile included
  for (int j = tid; j < T; j += 64 * SPKNN_WAVES) acc[j] = 0;
  __syncthreads();

  const long long s = qptr[q], e = qptr[q + 1];
  const double scale = ldexp(1.0, -ex);
  // short slices: the waves take the nonzeros round-robin, lanes across the
  // slice.  Long slices (a column present in much of the tile) would leave
  // one wave with the work of the workgroup: all four waves share each.
  for (int pass = 0; pass < 2; ++pass) {
    for (long long p = s + (pass == 0 ? wave : 0); p < e; p += (pass == 0 ? SPKNN_WAVES : 1)) {
      const int c = qidx[p];
      if (c < 0 || c >= d) continue;
      const double v = (double)qval[p] * scale;      // exact: a power of two
      if (v == 0.0) continue;
      long long a = tab[(long long)c * ntiles + t];
      long long b = tab[(long long)c * ntiles + t + 1];
      a = a < 0 ? 0 : a;
      b = b > nnz_x ? nnz_x : b;
      const bool wide = b - a >= SPKNN_LONG;
      if (pass == 0 && !wide)
        knn_scatter<64>(acc, trow, tval, a, b, lane, v, base, nv);
      else if (pass == 1 && wide)
        knn_scatter<64 * SPKNN_WAVES>(acc, trow, tval, a, b, tid, v, base, nv);
    }
  }
  __syncthreads();
}

}  // namespace sq
