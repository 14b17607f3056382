// Radius neighbours of CSR queries against a CSR fit set (SURVEY.md N24, K18,
// sparse half): {j : D(q_i, x_j) <= thr} for every query row, as CSR lists.
//
// Reference semantics: ``neighbors/_base.py`` radius_neighbors with algorithm
// 'brute' on sparse input, as ``cluster/_dbscan.py`` uses it - the distances of
// ``euclidean_distances`` / ``cosine_distances`` thresholded inclusively.
//
// Operands: those of spknn.hip (CSR queries, the transposed fit set and its
// tile pointer table, the squared row norms of both sides, one fixed-point
// exponent per query row).  The inner products are accumulated by the phase
// both kernels share (spknn_acc.h): 64-bit integer quanta, integer LDS
// atomics, results independent of arrival order and launch geometry.
//
// MI355X mapping.
//   sp_radius_mark_kernel: one workgroup of four waves per (query row, fit
//     tile of T rows), grid and LDS accumulators as in sp_knn_kernel.  After
//     the accumulate phase every wave takes 64-row groups of the tile: a lane
//     turns its accumulator into the fp64 distance, tests D <= thr (inclusive;
//     the pair (q, q) of a self-join is a hit whatever D is), the wave ballots
//     and lane 0 stores the 64-bit word to mask[query, (base + j) / 64]: one
//     bit per pair.  T is a multiple of 64, so a word never straddles two
//     tiles and every word of a mask row is written exactly once, the tail
//     bits of the last word as zeros.  The popcounts of the words add up
//     (integers) to cnt[query, tile].
//   sp_radius_fill_kernel: one wave per (query row, tile).  The lanes read
//     the tile's mask words, an exclusive wave scan of the popcounts places
//     every word, and each lane expands the set bits of its word to fit-row
//     indices behind the (query, tile) offset that the caller's cumulative sum
//     of cnt gives.  Lists are ascending by fit index whatever the geometry.
//
// No floating-point atomics, no per-lane lists.  LDS: 8 T + 16 bytes.
#include "spknn_acc.h"
#include "sq_api.h"

namespace sq {

// grid: m * ntiles workgroups, workgroup b serves query q0 + b / ntiles and
// tile b % ntiles.  mask [m, words] with words = ceil(n / 64); cnt [m, ntiles].
__global__ void __launch_bounds__(64 * SPKNN_WAVES) sp_radius_mark_kernel(
    const long long* __restrict__ qptr, const int* __restrict__ qidx,
    const float* __restrict__ qval, const int* __restrict__ trow, const float* __restrict__ tval,
    const long long* __restrict__ tab, const double* __restrict__ qn,
    const double* __restrict__ xn, const int* __restrict__ qexp, long long q0, long long n, int d,
    int T, long long ntiles, long long nnz_x, int metric, double thr, int self_join,
    long long words, unsigned long long* __restrict__ mask, int* __restrict__ cnt) {
  extern __shared__ unsigned char sprad_smem[];
  long long* acc = reinterpret_cast<long long*>(sprad_smem);
  int* wcnt = reinterpret_cast<int*>(acc + T);        // [WAVES]
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
  const long long own = self_join ? q : -1;           // the fit row that is the query itself
  unsigned long long* row = mask + ql * words + base / 64;
  int hits = 0;
  // g0 is the same for the 64 lanes of a wave: the ballot sees whole waves
  for (int g0 = 64 * wave; g0 < nv; g0 += 64 * SPKNN_WAVES) {
    const int j = g0 + lane;
    bool hit = false;
    if (j < nv) {
      const double D = knn_distance(metric, (double)acc[j] * quantum, qi, sq, xn[base + j]);
      hit = D <= thr || base + j == own;
    }
    const unsigned long long word = __ballot(hit);
    if (lane == 0) row[g0 >> 6] = word;
    hits += __popcll(word);
  }
  if (lane == 0) wcnt[wave] = hits;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < SPKNN_WAVES; ++w) total += wcnt[w];
    cnt[blockIdx.x] = total;
  }
}

// one wave per (query row, tile); cs is the inclusive cumulative sum of cnt
// over the flattened [m, ntiles], ``total`` its last entry (the length of out)
__global__ void __launch_bounds__(256) sp_radius_fill_kernel(
    const unsigned long long* __restrict__ mask, const long long* __restrict__ cs, long long pairs,
    long long ntiles, long long words, int wpt, long long total, int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= pairs) return;
  const long long ql = w / ntiles;
  const long long t = w - ql * ntiles;
  const long long first = t * wpt;                   // first mask word of the tile
  const int nw = (int)((words - first) < wpt ? (words - first) : wpt);
  long long pos = w ? cs[w - 1] : 0;
  const long long end = cs[w];
  if (end == pos) return;
  const unsigned long long* row = mask + ql * words + first;
  for (int w0 = 0; w0 < nw; w0 += 64) {
    const int i = w0 + lane;
    unsigned long long word = i < nw ? row[i] : 0ull;
    const int c = __popcll(word);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    long long at = pos + (incl - c);
    const int col = (int)((first + i) * 64);
    while (word) {
      const int b = __ffsll((long long)word) - 1;
      if (at < end && at < total) out[at] = col + b;
      ++at;
      word &= word - 1;
    }
    pos += __shfl(incl, 63, 64);
  }
}

}  // namespace sq

using namespace sq;

static bool sp_radius_args_ok(long long m, long long n, int T) {
  if (n < 1 || n >= (1LL << 31) || T < 64 || T > SPKNN_TMAX || T % 64 != 0) return false;
  const long long ntiles = (n + T - 1) / T;
  return m * ntiles < (1LL << 31);
}

// Queries q0 .. q0 + m of the CSR (qptr, qidx, qval) against the transposed
// fit set (trow, tval: nnz_x entries) with its tile table tab [d * ntiles + 1]:
// mask [m, ceil(n / 64)] uint64 and cnt [m, ntiles] int32.  self_join: query
// row i is fit row i and is its own neighbour.
extern "C" int sq_sp_radius_mark(const void* qptr, const void* qidx, const void* qval,
                                 const void* trow, const void* tval, const void* tab,
                                 const void* qn, const void* xn, const void* qexp, long long q0,
                                 long long m, long long n, int d, int T, long long nnz_x,
                                 int metric, double thr, int self_join, void* mask, void* cnt,
                                 void* stream) {
  if (m <= 0) return 0;
  if (!sp_radius_args_ok(m, n, T) || d < 1 || metric < 0 || metric > 1 || q0 < 0 || nnz_x < 0 ||
      (self_join && q0 + m > n))
    return (int)hipErrorInvalidValue;
  const long long ntiles = (n + T - 1) / T;
  const long long words = (n + 63) / 64;
  const size_t lds = (size_t)T * sizeof(long long) + SPKNN_WAVES * sizeof(int);
  static bool attr = false;
  if (!attr) {
    hipError_t rc = hipFuncSetAttribute(
        (const void*)sp_radius_mark_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)(SPKNN_TMAX * sizeof(long long) + SPKNN_WAVES * sizeof(int)));
    if (rc != hipSuccess) return (int)rc;
    attr = true;
  }
  hipLaunchKernelGGL(sp_radius_mark_kernel, dim3((unsigned)(m * ntiles)), dim3(64 * SPKNN_WAVES),
                     lds, (hipStream_t)stream, (const long long*)qptr, (const int*)qidx,
                     (const float*)qval, (const int*)trow, (const float*)tval,
                     (const long long*)tab, (const double*)qn, (const double*)xn,
                     (const int*)qexp, q0, n, d, T, ntiles, nnz_x, metric, thr, self_join ? 1 : 0,
                     words, (unsigned long long*)mask, (int*)cnt);
  return (int)hipGetLastError();
}

// The marked pairs of m query rows as fit-row indices: out [total] int32,
// the list of (query, tile) behind cs[query * ntiles + tile - 1].
extern "C" int sq_sp_radius_fill(const void* mask, const void* cs, long long m, long long n, int T,
                                 long long total, void* out, void* stream) {
  if (m <= 0 || total <= 0) return 0;
  if (!sp_radius_args_ok(m, n, T)) return (int)hipErrorInvalidValue;
  const long long ntiles = (n + T - 1) / T;
  const long long words = (n + 63) / 64;
  const long long pairs = m * ntiles;
  hipLaunchKernelGGL(sp_radius_fill_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, (const unsigned long long*)mask, (const long long*)cs,
                     pairs, ntiles, words, T / 64, total, (int*)out);
  return (int)hipGetLastError();
}
