// Brute-force k-NN of CSR queries against a CSR fit set (SURVEY.md S11, K18,
// sparse half): sparse-times-sparse inner products through an inverted index.
//
// Reference semantics: ``neighbors/_base.py`` kneighbors with algorithm
// 'brute' on sparse input - ``euclidean_distances`` / ``cosine_distances``
// through ``safe_sparse_dot``, then the k smallest per query row.
//
// Operands.  The queries are CSR rows (int64 indptr, int32 indices, fp32
// values).  The fit set is used through its transpose (column c holds the
// sorted fit rows with a value in c) and a tile pointer table: fit rows are
// cut into tiles of T, and tab[c * ntiles + t] .. tab[c * ntiles + t + 1] is
// the slice of column c that falls into tile t, so the kernel never searches.
//
// MI355X mapping.
//   sp_knn_kernel: one workgroup of four waves per (query row, fit tile).
//     The T inner products of the tile live in LDS as 64-bit integer quanta of
//     2^e (e per query row).  The waves take the query's nonzeros (c, qv)
//     round-robin; the lanes of a wave run across the column slice, and every
//     entry adds round(qv * xv / 2^e) to its row's accumulator with a 64-bit
//     integer LDS atomic.  Slices of 256 entries or more (a column present in
//     much of the tile) are shared by all four waves in a second pass, four
//     loads in flight per lane.  The fp64 product of two fp32 values is exact, and
//     integer addition commutes: the sums do not depend on the arrival order
//     or on the launch geometry.  Work per query is sum_c nnz_x(c) over the
//     query's columns, against nnz(X) for a gather over densified queries.
//     After a barrier the epilogue turns accumulators into distances (fp64)
//     and either writes them out (dist mode) or selects the kk <= 32 smallest
//     by (distance, fit index): per-lane sorted register lists, kk rounds of
//     wave-wide argmin, the four wave lists combined by wave 0 through LDS.
//   sp_knn_merge_kernel: one wave per query row selects the kk best of the
//     ntiles * kk partials by the same order.
//
// LDS: 8 T bytes of accumulators plus 1.5 KiB of wave lists.  T <= 8192
// keeps two workgroups on a CU (160 KiB), which is also what the register
// lists of the selection allow (two waves per SIMD); the default is chosen by
// the caller (profiles/sparse_knn.md).
//
// The accumulate phase and the distance formulae live in spknn_acc.h, shared
// with the radius-neighbour kernels of spradius.hip.
#include "spknn_acc.h"
#include "sq_api.h"

namespace sq {

constexpr int SPKNN_KMAX = 32;
constexpr int SPKNN_NONE = 0x7FFFFFFF;

// (distance, index) order: the smaller distance first, ties to the smaller index
SQ_DEV bool knn_before(double a, int ai, double b, int bi) {
  return a < b || (a == b && ai < bi);
}

SQ_DEV void knn_list_reset(double (&bv)[SPKNN_KMAX], int (&bi)[SPKNN_KMAX]) {
#pragma unroll
  for (int i = 0; i < SPKNN_KMAX; ++i) { bv[i] = INFINITY; bi[i] = SPKNN_NONE; }
}

// insertion into the lane's sorted list of ``depth`` live slots (static
// indices only: the list stays in registers); a pair that beats no slot
// falls through unchanged
SQ_DEV void knn_list_insert(double (&bv)[SPKNN_KMAX], int (&bi)[SPKNN_KMAX], int depth, double v,
                            int ix) {
  double cv = v;
  int ci = ix;
#pragma unroll
  for (int i = 0; i < SPKNN_KMAX; ++i) {
    if (i < depth) {
      const bool lt = knn_before(cv, ci, bv[i], bi[i]);
      const double tv = bv[i];
      const int ti = bi[i];
      bv[i] = lt ? cv : tv;
      bi[i] = lt ? ci : ti;
      cv = lt ? tv : cv;
      ci = lt ? ti : ci;
    }
  }
}

// kk rounds of wave-wide argmin over the heads of the 64 lists; the lane that
// owns the minimum pops it.  emit(t, v, ix) is called by every lane with the
// t-th smallest pair of the wave (+inf / SPKNN_NONE once the lists run dry).
template <class Emit>
SQ_DEV void knn_list_drain(double (&bv)[SPKNN_KMAX], int (&bi)[SPKNN_KMAX], int kk, Emit emit) {
  for (int t = 0; t < kk; ++t) {
    double v = bv[0];
    int ix = bi[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(ix, o, 64);
      if (knn_before(ov, oi, v, ix)) { v = ov; ix = oi; }
    }
    emit(t, v, ix);
    if (bi[0] == ix && bv[0] == v) {
#pragma unroll
      for (int i = 0; i < SPKNN_KMAX - 1; ++i) { bv[i] = bv[i + 1]; bi[i] = bi[i + 1]; }
      bv[SPKNN_KMAX - 1] = INFINITY;
      bi[SPKNN_KMAX - 1] = SPKNN_NONE;
    }
  }
}

// grid: m * ntiles workgroups, workgroup b serves query q0 + b / ntiles and
// tile b % ntiles.  mode 0: partials pd / pi [m, ntiles, kk]; mode 1: the
// distances of the tile into dist [m, n].
__global__ void __launch_bounds__(64 * SPKNN_WAVES) sp_knn_kernel(
    const long long* __restrict__ qptr, const int* __restrict__ qidx,
    const float* __restrict__ qval, const int* __restrict__ trow, const float* __restrict__ tval,
    const long long* __restrict__ tab, const double* __restrict__ qn,
    const double* __restrict__ xn, const int* __restrict__ qexp, long long q0, long long n, int d,
    int T, long long ntiles, long long nnz_x, int kk, int metric, int mode,
    double* __restrict__ pd, int* __restrict__ pi, double* __restrict__ dist) {
  extern __shared__ unsigned char spknn_smem[];
  long long* acc = reinterpret_cast<long long*>(spknn_smem);
  double* wv = reinterpret_cast<double*>(acc + T);                    // [WAVES][KMAX]
  int* wi = reinterpret_cast<int*>(wv + SPKNN_WAVES * SPKNN_KMAX);     // [WAVES][KMAX]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const long long ql = blockIdx.x / ntiles;          // query inside the chunk
  const long long t = blockIdx.x - ql * ntiles;
  const long long q = q0 + ql;
  const long long base = t * T;                      // first fit row of the tile
  const int nv = (int)((n - base) < T ? (n - base) : T);

  const int ex = qexp[q];
  knn_accumulate(acc, qptr, qidx, qval, trow, tval, tab, q, t, base, nv, ex, d, T, ntiles, nnz_x);

  const double quantum = ldexp(1.0, ex);
  const double qi = qn[q];
  const double sq = sqrt(qi);
  if (mode == 1) {
    double* row = dist + ql * n + base;
    for (int j = tid; j < nv; j += 64 * SPKNN_WAVES)
      row[j] = knn_distance(metric, (double)acc[j] * quantum, qi, sq, xn[base + j]);
    return;
  }

  double bv[SPKNN_KMAX];
  int bi[SPKNN_KMAX];
  knn_list_reset(bv, bi);
  // a lane meets at most ceil(T / 256) rows: deeper slots would stay empty
  const int per_lane = (T + 64 * SPKNN_WAVES - 1) / (64 * SPKNN_WAVES);
  const int depth = kk < per_lane ? kk : per_lane;
  for (int j = tid; j < nv; j += 64 * SPKNN_WAVES) {
    const double D = knn_distance(metric, (double)acc[j] * quantum, qi, sq, xn[base + j]);
    knn_list_insert(bv, bi, depth, D, (int)(base + j));
  }
  knn_list_drain(bv, bi, kk, [&](int r, double v, int ix) {
    if (lane == 0) { wv[wave * SPKNN_KMAX + r] = v; wi[wave * SPKNN_KMAX + r] = ix; }
  });
  __syncthreads();
  if (wave != 0) return;
  // the four sorted wave lists hold 4 kk <= 128 pairs: two per lane
  knn_list_reset(bv, bi);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int g = lane + 64 * h;                     // pair g: wave g / kk, slot g % kk
    if (g < SPKNN_WAVES * kk) {
      const int w = g / kk, r = g - w * kk;
      knn_list_insert(bv, bi, 2, wv[w * SPKNN_KMAX + r], wi[w * SPKNN_KMAX + r]);
    }
  }
  double* od = pd + ((long long)blockIdx.x) * kk;
  int* oi = pi + ((long long)blockIdx.x) * kk;
  knn_list_drain(bv, bi, kk, [&](int r, double v, int ix) {
    if (lane == 0) { od[r] = v; oi[r] = ix == SPKNN_NONE ? -1 : ix; }
  });
}

// one wave per query row: the kk best of its ntiles * kk partials
__global__ void __launch_bounds__(256) sp_knn_merge_kernel(
    const double* __restrict__ pd, const int* __restrict__ pi, long long m, long long ntiles,
    int kk, double* __restrict__ outd, long long* __restrict__ outi) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= m) return;
  double bv[SPKNN_KMAX];
  int bi[SPKNN_KMAX];
  knn_list_reset(bv, bi);
  const long long cnt = ntiles * kk;
  const double* rd = pd + r * cnt;
  const int* ri = pi + r * cnt;
  for (long long j = lane; j < cnt; j += 64) {
    const int ix = ri[j];
    if (ix >= 0) knn_list_insert(bv, bi, kk, rd[j], ix);
  }
  knn_list_drain(bv, bi, kk, [&](int t, double v, int ix) {
    if (lane == 0) {
      outd[r * kk + t] = v;
      outi[r * kk + t] = ix == SPKNN_NONE ? -1 : (long long)ix;
    }
  });
}

}  // namespace sq

using namespace sq;

extern "C" int sq_sp_knn_tile_max() { return SPKNN_TMAX; }

// Queries q0 .. q0 + m of the CSR (qptr, qidx, qval) against the transposed
// fit set (trow, tval: nnz_x entries) with its tile table tab [d * ntiles + 1].
// mode 0: pd / pi [m, ntiles, kk] scratch, outd [m, kk] fp64, outi [m, kk]
// int64.  mode 1: dist [m, n] fp64 (pd, pi, outd, outi unused).
extern "C" int sq_sp_knn(const void* qptr, const void* qidx, const void* qval, const void* trow,
                         const void* tval, const void* tab, const void* qn, const void* xn,
                         const void* qexp, long long q0, long long m, long long n, int d, int T,
                         long long nnz_x, int kk, int metric, int mode, void* pd, void* pi,
                         void* dist, void* outd, void* outi, void* stream) {
  if (m <= 0) return 0;
  if (n < 1 || n >= (1LL << 31) || d < 1 || T < 1 || T > SPKNN_TMAX || metric < 0 || metric > 1 ||
      mode < 0 || mode > 1 || q0 < 0 || nnz_x < 0)
    return (int)hipErrorInvalidValue;
  if (mode == 0 && (kk < 1 || kk > SPKNN_KMAX || kk > n)) return (int)hipErrorInvalidValue;
  const long long ntiles = (n + T - 1) / T;
  if (m * ntiles >= (1LL << 31)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)T * sizeof(long long) +
                     (size_t)SPKNN_WAVES * SPKNN_KMAX * (sizeof(double) + sizeof(int));
  static bool attr = false;
  if (!attr) {
    hipError_t rc = hipFuncSetAttribute(
        (const void*)sp_knn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)(SPKNN_TMAX * sizeof(long long) +
              SPKNN_WAVES * SPKNN_KMAX * (sizeof(double) + sizeof(int))));
    if (rc != hipSuccess) return (int)rc;
    attr = true;
  }
  hipLaunchKernelGGL(sp_knn_kernel, dim3((unsigned)(m * ntiles)), dim3(64 * SPKNN_WAVES), lds, s,
                     (const long long*)qptr, (const int*)qidx, (const float*)qval,
                     (const int*)trow, (const float*)tval, (const long long*)tab,
                     (const double*)qn, (const double*)xn, (const int*)qexp, q0, n, d, T, ntiles,
                     nnz_x, kk, metric, mode, (double*)pd, (int*)pi, (double*)dist);
  int rc = (int)hipGetLastError();
  if (rc != 0 || mode == 1) return rc;
  hipLaunchKernelGGL(sp_knn_merge_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s,
                     (const double*)pd, (const int*)pi, m, ntiles, kk, (double*)outd,
                     (long long*)outi);
  return (int)hipGetLastError();
}
