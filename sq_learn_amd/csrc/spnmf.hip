// Non-negative matrix factorisation kernels: the Kullback-
// Leibler ratio over the stored entries of a CSR matrix and the coordinate-
// descent sweep.
//
// Reference semantics: ``decomposition/_nmf.py`` (``_special_sparse_dot``,
// ``_multiplicative_update_w / _h``, ``_beta_divergence`` on sparse X) and
// ``decomposition/_cdnmf_fast.pyx``; the law of the sweep is the one of
// csrc/host/decomposition_host.cpp: sqh_cdnmf_update, operation by operation.
//
// MI355X mapping.
//   Ratio (sp_nmf_kl_kernel): one wave per CSR row, the shape of splda.hip.
//     The row of P sits in LDS.  The stored entries go 64 at a time through
//     two phases:
//       ratio       lanes over entries: wh_t = sum_j P[i][j] Q[c_t][j], j in
//                   order, 0 -> EPS; r_t = x_t / wh_t; with DIV also the
//                   lane's x_t log(x_t / wh_t) of the entries above EPS;
//       accumulate  lanes over components: acc_j += r_t Q[c_t][j], t in order,
//                   r_t and the row base broadcast with readlane.
//     acc lives in LDS, one lane owning component j = lane + 64 i.  A row
//     whose gathered Q rows fit SP_NMF_STAGE doubles stages them in LDS once
//     (row stride k | 1: odd, so lanes over entries and lanes over components
//     both spread over the banks); a longer row gathers them twice from global
//     memory.  One wave owns an output row: no atomics, and the result does
//     not depend on the launch geometry or on how the rows are split into
//     calls.
//   Sweep (nmf_cd_kernel): one lane per row of W, one wave per workgroup.  A
//     tile of R rows of W and of XHt is staged in LDS with row stride k | 1
//     (coalesced global accesses, conflict-free LDS accesses of lanes a row
//     apart); R is 64 while the two tiles fit and shrinks above that, the
//     lanes past R idle.  HHt[t][.] is wave-uniform: from LDS up to
//     NMF_CD_HHT_K components, through a uniform pointer (scalar loads) above.
//     The sum over r runs ascending in every lane, as on the host.  A row's
//     sum of |projected gradient| goes to viol[row]; sp_sum_parts_kernel adds
//     them in a fixed order.
#include <cmath>

#include "sp_rows.h"
#include "sq_api.h"

namespace sq {

constexpr int SP_NMF_STAGE = 1024;        // doubles of gathered rows a wave stages in LDS
constexpr int SP_NMF_STAGE_MIN_ROW = 4;   // a staged entry counts as at least this many doubles
constexpr int SP_NMF_MAX_K = 1024;
constexpr int SP_NMF_LDS = 64 * 1024;     // per workgroup of the ratio kernel
constexpr int NMF_CD_MAX_K = 1024;
constexpr int NMF_CD_HHT_K = 64;          // HHt in LDS up to this k
constexpr int NMF_CD_LDS = 128 * 1024;    // per workgroup (one wave) of the sweep

static inline int nmf_kl_wave_doubles(int k) { return 2 * 64 * ((k + 63) / 64) + SP_NMF_STAGE; }
static inline int nmf_kl_wpb(int k) {
  int wpb = 4;
  while (wpb > 1 && (size_t)nmf_kl_wave_doubles(k) * sizeof(double) * wpb > (size_t)SP_NMF_LDS)
    wpb >>= 1;
  return wpb;
}
static inline int nmf_cd_rows(int k) {
  const size_t hht = k <= NMF_CD_HHT_K ? (size_t)k * k * sizeof(double) : 0;
  const size_t r = ((size_t)NMF_CD_LDS - hht) / (2 * (size_t)(k | 1) * sizeof(double));
  return (int)(r < 64 ? r : 64);
}

// sum_j a[j] b[j], j ascending in one accumulator; the loads of eight terms are issued before
// their products are added, so one memory latency covers eight steps of the chain (left to
// the compiler the loop waits for every load: profiles/nmf_device.md)
SQ_DEV double nmf_dot(const double* a, const double* b, int k, double s = 0.0) {
  int j = 0;
  for (; j + 8 <= k; j += 8) {
    double x[8], y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      x[u] = a[j + u];
      y[u] = b[j + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += x[u] * y[u];
  }
  for (; j < k; ++j) s += a[j] * b[j];
  return s;
}

// a wave's view of one row
struct NmfRow {
  const int* indices;
  const float* data;
  const double* Q;   // [cols][k]
  long long s, e;    // stored entries [s, e)
  int cols, k, nj;   // nj: component tiles of 64
  double* p;         // LDS rows of 64 nj doubles
  double* acc;
  double* S;         // staged rows, stride doubles apart
  int stride;
};

// the lane's (col, x) of the entries [p, p + 64): a column outside [0, cols) or past the end
// becomes (0, 0), which adds nothing
SQ_DEV int nmf_load(const NmfRow& D, long long p, int lane, int& col, double& x) {
  float v;
  const int n = sp_load_pairs(D.indices, D.data, p, D.e, lane, col, v);
  const bool ok = col >= 0 && col < D.cols;
  col = ok ? col : 0;
  x = ok ? (double)v : 0.0;
  return n;
}

template <bool STAGED>
SQ_DEV const double* nmf_q_row(const NmfRow& D, long long p, int col, int q) {
  return STAGED ? D.S + (size_t)((int)(p - D.s) + q) * D.stride
                : D.Q + (long long)bcast_i(col, q) * D.k;
}

// num (optional) and the lane's share of div of one row
template <bool STAGED, bool DIV>
SQ_DEV double nmf_row(const NmfRow& D, int lane, double eps, bool want_num) {
  double dv = 0.0;
  for (long long p = D.s; p < D.e; p += 64) {
    int col;
    double x;
    const int n = nmf_load(D, p, lane, col, x);
    const double* mine = STAGED ? D.S + (size_t)((int)(p - D.s) + (lane < n ? lane : 0)) * D.stride
                                : D.Q + (long long)col * D.k;
    double wh = nmf_dot(D.p, mine, D.k);
    if (wh == 0.0) wh = eps;
    const double r = lane < n ? x / wh : 0.0;
    if (DIV && lane < n && x > eps) dv += x * log(x / wh);
    if (!want_num) continue;   // wave-uniform
    for (int i = 0; i < D.nj; ++i) {
      const int j = 64 * i + lane;
      const int jr = j < D.k ? j : D.k - 1;
      double a = D.acc[j];
      int q = 0;
      for (; q + 4 <= n; q += 4) {   // four rows in flight, added in order
        const double x0 = nmf_q_row<STAGED>(D, p, col, q)[jr];
        const double x1 = nmf_q_row<STAGED>(D, p, col, q + 1)[jr];
        const double x2 = nmf_q_row<STAGED>(D, p, col, q + 2)[jr];
        const double x3 = nmf_q_row<STAGED>(D, p, col, q + 3)[jr];
        a += bcast_d(r, q) * x0;
        a += bcast_d(r, q + 1) * x1;
        a += bcast_d(r, q + 2) * x2;
        a += bcast_d(r, q + 3) * x3;
      }
      for (; q < n; ++q) a += bcast_d(r, q) * nmf_q_row<STAGED>(D, p, col, q)[jr];
      D.acc[j] = a;
    }
  }
  return dv;
}

// ---------------------------------------------------------------- ratio
// Rows [q0, q0 + m); P [m][k], num [m][k] (optional) and div [m] (with DIV) are indexed from q0.
template <bool DIV>
__global__ void __launch_bounds__(256) sp_nmf_kl_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const double* __restrict__ P, const double* __restrict__ Q,
    long long q0, long long m, int cols, int k, double eps, double* __restrict__ num,
    double* __restrict__ div) {
  extern __shared__ unsigned char nmf_smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  NmfRow D;
  D.indices = indices;
  D.data = data;
  D.Q = Q;
  D.cols = cols;
  D.k = k;
  D.nj = (k + 63) >> 6;
  D.stride = k | 1;
  const int kp = 64 * D.nj;
  D.p = reinterpret_cast<double*>(nmf_smem) + (size_t)wave * (2 * kp + SP_NMF_STAGE);
  D.acc = D.p + kp;
  D.S = D.acc + kp;
  const int per = D.stride > SP_NMF_STAGE_MIN_ROW ? D.stride : SP_NMF_STAGE_MIN_ROW;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long pos = (long long)blockIdx.x * wpb + wave; pos < m; pos += stride) {
    D.s = sp_uniform_ll(indptr[q0 + pos]);
    D.e = sp_uniform_ll(indptr[q0 + pos + 1]);
    const long long entries = D.e - D.s;
    const bool staged = entries > 0 && entries * per <= SP_NMF_STAGE;   // wave-uniform
    const double* prow = P + pos * k;
    for (int i = 0; i < D.nj; ++i) {
      const int j = 64 * i + lane;
      D.p[j] = j < k ? prow[j] : 0.0;
      D.acc[j] = 0.0;
    }
    if (staged) {
      for (long long p = D.s; p < D.e; p += 64) {
        int col;
        double x;
        const int n = nmf_load(D, p, lane, col, x);
        for (int q = 0; q < n; ++q) {
          const double* src = Q + (long long)bcast_i(col, q) * k;
          double* dst = D.S + (size_t)((int)(p - D.s) + q) * D.stride;
          for (int j = lane; j < k; j += 64) dst[j] = src[j];
        }
      }
    }
    sp_wave_sync();
    const bool want_num = num != nullptr;
    double dv = staged ? nmf_row<true, DIV>(D, lane, eps, want_num)
                       : nmf_row<false, DIV>(D, lane, eps, want_num);
    if (want_num)
      for (int j = lane; j < k; j += 64) num[pos * k + j] = D.acc[j];
    if (DIV) {
      dv = wave_sum(dv);
      if (lane == 0) div[pos] = dv;
    }
    sp_wave_sync();   // the next row overwrites the LDS rows
  }
}

// ---------------------------------------------------------------- sweep
// Rows [row0, row0 + m) of W [.][k] and XHt [.][k]; viol [m] is indexed from row0.  One wave
// per workgroup, lane l < R owns row l of the tile.  An entry of perm outside [0, k) is skipped.
template <bool HLDS>
__global__ void __launch_bounds__(64) nmf_cd_kernel(
    double* __restrict__ W, const double* __restrict__ HHt, const double* __restrict__ XHt,
    const long long* __restrict__ perm, long long row0, long long m, int k, int R,
    double* __restrict__ viol) {
  extern __shared__ unsigned char nmf_smem[];
  const int lane = threadIdx.x;
  const int stride = k | 1;
  double* Wt = reinterpret_cast<double*>(nmf_smem);
  double* Xt = Wt + (size_t)R * stride;
  double* Hs = Xt + (size_t)R * stride;
  if (HLDS) {
    for (int idx = lane; idx < k * k; idx += 64) Hs[idx] = HHt[idx];
  }
  const long long tiles = (m + R - 1) / R;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long base = tile * R;
    const int cnt = (int)(m - base < R ? m - base : R);
    const long long g0 = (row0 + base) * k;
    const int total = cnt * k;
    for (int idx = lane; idx < total; idx += 64) {
      const int r = idx / k, j = idx - r * k;
      Wt[r * stride + j] = W[g0 + idx];
      Xt[r * stride + j] = XHt[g0 + idx];
    }
    __syncthreads();
    if (lane < cnt) {
      double* w = Wt + lane * stride;
      const double* x = Xt + lane * stride;
      double v = 0.0;
      for (int s = 0; s < k; ++s) {
        const long long tl = sp_uniform_ll(perm[s]);
        if (tl < 0 || tl >= k) continue;
        const int t = (int)tl;
        const double* h = HLDS ? Hs + (size_t)t * k : HHt + (long long)t * k;
        const double grad = nmf_dot(h, w, k, -x[t]);
        const double wt = w[t];
        const double pg = wt == 0.0 ? fmin(0.0, grad) : grad;
        v += fabs(pg);
        const double hess = h[t];
        if (hess != 0.0) w[t] = fmax(wt - grad / hess, 0.0);
      }
      viol[base + lane] = v;
    }
    __syncthreads();
    for (int idx = lane; idx < total; idx += 64) {
      const int r = idx / k, j = idx - r * k;
      W[g0 + idx] = Wt[r * stride + j];
    }
    __syncthreads();
  }
}

}  // namespace sq

using namespace sq;

extern "C" int sq_sp_nmf_stage() { return SP_NMF_STAGE; }
extern "C" int sq_sp_nmf_stage_min_row() { return SP_NMF_STAGE_MIN_ROW; }
extern "C" int sq_sp_nmf_max_k() { return SP_NMF_MAX_K; }
extern "C" int sq_sp_nmf_wpb(int k) { return k < 1 || k > SP_NMF_MAX_K ? 0 : nmf_kl_wpb(k); }
extern "C" int sq_nmf_cd_max_k() { return NMF_CD_MAX_K; }
extern "C" int sq_nmf_cd_hht_k() { return NMF_CD_HHT_K; }
extern "C" int sq_nmf_cd_rows(int k) { return k < 1 || k > NMF_CD_MAX_K ? 0 : nmf_cd_rows(k); }

extern "C" int sq_sp_nmf_kl(const void* indptr, const void* indices, const void* data,
                            const void* P, const void* Q, long long q0, long long m, int cols,
                            int k, double eps, void* num, void* div, void* stream) {
  if (k < 1 || k > SP_NMF_MAX_K || cols < 1 || q0 < 0 || m < 0 || !(eps > 0.0) ||
      !std::isfinite(eps) || (num == nullptr && div == nullptr) || !indptr || !Q ||
      (m > 0 && !P))   // indices / data are null for a matrix without stored entries
    return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  const int wpb = nmf_kl_wpb(k);
  const size_t bytes = (size_t)nmf_kl_wave_doubles(k) * sizeof(double) * wpb;
  if (bytes > (size_t)SP_NMF_LDS) return (int)hipErrorInvalidValue;
  const dim3 grid(sp_grid(m, wpb)), block(64 * wpb);
  if (div)
    hipLaunchKernelGGL(sp_nmf_kl_kernel<true>, grid, block, bytes, (hipStream_t)stream,
                       (const long long*)indptr, (const int*)indices, (const float*)data,
                       (const double*)P, (const double*)Q, q0, m, cols, k, eps, (double*)num,
                       (double*)div);
  else
    hipLaunchKernelGGL(sp_nmf_kl_kernel<false>, grid, block, bytes, (hipStream_t)stream,
                       (const long long*)indptr, (const int*)indices, (const float*)data,
                       (const double*)P, (const double*)Q, q0, m, cols, k, eps, (double*)num,
                       (double*)div);
  return (int)hipGetLastError();
}

// W [.][k] in place over the rows [row0, row0 + m); rowviol [m] scratch, violation [1]
extern "C" int sq_nmf_cd_sweep(void* W, const void* HHt, const void* XHt, const void* perm,
                               long long row0, long long m, int k, void* rowviol,
                               void* violation, void* stream) {
  if (k < 1 || k > NMF_CD_MAX_K || row0 < 0 || m < 0 || m >= (1LL << 31) || !W || !HHt || !XHt ||
      !perm || !rowviol || !violation)
    return (int)hipErrorInvalidValue;
  const int R = nmf_cd_rows(k);
  if (R < 1) return (int)hipErrorInvalidValue;
  const bool hlds = k <= NMF_CD_HHT_K;
  const size_t bytes = (2 * (size_t)R * (k | 1) + (hlds ? (size_t)k * k : 0)) * sizeof(double);
  if (bytes > (size_t)NMF_CD_LDS) return (int)hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    hipError_t rc = hipFuncSetAttribute((const void*)nmf_cd_kernel<true>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, NMF_CD_LDS);
    if (rc == hipSuccess)
      rc = hipFuncSetAttribute((const void*)nmf_cd_kernel<false>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, NMF_CD_LDS);
    if (rc != hipSuccess) return (int)rc;
    attr = true;
  }
  if (m > 0) {
    const long long tiles = (m + R - 1) / R;
    const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);
    if (hlds)
      hipLaunchKernelGGL(nmf_cd_kernel<true>, dim3(grid), dim3(64), bytes, (hipStream_t)stream,
                         (double*)W, (const double*)HHt, (const double*)XHt,
                         (const long long*)perm, row0, m, k, R, (double*)rowviol);
    else
      hipLaunchKernelGGL(nmf_cd_kernel<false>, dim3(grid), dim3(64), bytes, (hipStream_t)stream,
                         (double*)W, (const double*)HHt, (const double*)XHt,
                         (const long long*)perm, row0, m, k, R, (double*)rowviol);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return (int)rc;
  }
  hipLaunchKernelGGL(sp_sum_parts_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                     (const double*)rowviol, (int)m, (double*)violation);
  return (int)hipGetLastError();
}
