// Row-list CSR kernels of the sparse mini-batch k-means step.
//
// Reference semantics: ``cluster/_kmeans.py`` _mini_batch_step,
// ``_k_means_fast.pyx`` _mini_batch_update_csr and ``utils/sparsefuncs_fast``
// assign_rows_csr.  A mini-batch is a list of CSR row ids drawn with
// replacement; nothing is copied or densified per step.
//
// MI355X mapping.
//   sp_list_estep_kernel: one wave per list position, the tile walk of
//     sp_estep_kernel (sp_walk of sp_rows.h) against CT[d][k_pad]; the label
//     is the plain argmin (lowest index on exact ties), kept in registers and
//     reduced across the wave - no LDS row, always 4 waves per workgroup.
//   Scatter: sp_mstep_kernel of sp_rows.h over the list, with the rule that a
//     position of zero weight quantum adds nothing.
//   mb_update_kernel: one pass over the dense k x d state in 64 x 64 tiles:
//     c' = (c n_c + sum) / (n_c + w_c) for the centres the batch touched,
//     written to C (rows along features) and, through an LDS tile transpose,
//     to CT (rows along centres), so both global writes are coalesced; the
//     consumed quanta are zeroed and per-tile partials of |c'|^2 and
//     |c' - c|^2 go to two [k][d / 64] arrays that mb_finish_kernel and
//     mb_record_kernel sum in a fixed order.
//   sp_rows_dense_kernel: one wave per list entry, zero fill then scatter.
#include "sp_rows.h"
#include "sq_api.h"

namespace sq {

// ---------------------------------------------------------------- E-step
// position pos reads CSR row rows[pos] (rows == nullptr: row0 + pos); an id
// outside [0, n) gets label -1 and distance 0.
__global__ void __launch_bounds__(256) sp_list_estep_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const double* __restrict__ CT, const double* __restrict__ cn,
    const double* __restrict__ xn, const long long* __restrict__ rows, long long row0,
    long long m, long long n, int k, int k_pad, const double* __restrict__ weights,
    int* __restrict__ labels, double* __restrict__ mind, double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  double inertia = 0.0;
  for (long long pos = (long long)blockIdx.x * wpb + wave; pos < m; pos += stride) {
    const long long i = sp_uniform_ll(rows ? rows[pos] : row0 + pos);
    if (i < 0 || i >= n) {
      if (lane == 0) {
        labels[pos] = -1;
        mind[pos] = 0.0;
      }
      continue;
    }
    const long long s = sp_uniform_ll(indptr[i]);
    const long long e = sp_uniform_ll(indptr[i + 1]);
    const double xi = xn[i];
    // the first 64 nonzeros stay in registers across the centroid tiles
    int col0;
    float v0;
    const int cnt0 = sp_load_pairs(indices, data, s, e, lane, col0, v0);
    double bd = INFINITY;
    int bj = 0x7fffffff;
    for (int j0 = 0; j0 < k_pad; j0 += 64 * SP_T) {
      SpAcc acc = 0.0;
      const int nt = (k_pad - j0) >= 64 * SP_T ? SP_T : (k_pad - j0) / 64;   // wave-uniform
      sp_walk<true>(acc, nt, CT + j0 + lane, k_pad, SpPadded(), indices, data, s, e, lane, col0,
                    v0, cnt0);
      // a lane meets its centroids in increasing j: strict < keeps the lowest
#pragma unroll
      for (int t = 0; t < SP_T; ++t) {
        const int j = j0 + lane + 64 * t;
        if (t < nt && j < k) {
          double D = (xi + cn[j]) - 2.0 * acc[t];
          D = D > 0.0 ? D : 0.0;
          if (D < bd) {
            bd = D;
            bj = j;
          }
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(bd, o, 64);
      const int oj = __shfl_xor(bj, o, 64);
      if (od < bd || (od == bd && oj < bj)) {
        bd = od;
        bj = oj;
      }
    }
    if (lane == 0) {
      labels[pos] = bj < k ? bj : -1;
      mind[pos] = bd;
    }
    inertia += (weights ? weights[pos] : 1.0) * bd;
  }
  if (lane == 0) part[(long long)blockIdx.x * wpb + wave] = inertia;
}

// ---------------------------------------------------------------- update
// the dense mini-batch formula with one rounding per operation
SQ_DEV double mb_mean(double c, double n, double s, double w) {
#pragma clang fp contract(off)
  const double a = c * n;
  const double b = a + s;
  const double t = n + w;
  return b / t;
}

constexpr int MB_TILE = 64;

__global__ void __launch_bounds__(256) mb_update_kernel(
    double* __restrict__ C, double* __restrict__ CT, const double* __restrict__ counts,
    long long* __restrict__ qsum, const long long* __restrict__ qcnt, int k, int d, int k_pad,
    double xq, double wq, double* __restrict__ pcn, double* __restrict__ pshift) {
  __shared__ double tile[MB_TILE][MB_TILE + 1];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int c0 = blockIdx.x * MB_TILE, f0 = blockIdx.y * MB_TILE;
  const bool mine = c0 + lane < k && qcnt[c0 + lane] > 0;
  const unsigned long long upd = __ballot(mine);   // the same in all four waves
  if (upd == 0) return;                            // nothing to do in this tile
  const int f = f0 + lane;
  const int nft = gridDim.y;
  // a wave owns the tile rows wave + 4 i; four rows per round so that their
  // loads are in flight together
  for (int cb = wave; cb < MB_TILE; cb += 16) {
    double cv[4], nc[4], wc[4];
    long long q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cc = cb + 4 * r;
      cv[r] = 0.0;
      nc[r] = 0.0;
      wc[r] = 1.0;
      q[r] = 0;
      if (((upd >> cc) & 1) && f < d) {            // the first test is wave-uniform
        const long long idx = (long long)(c0 + cc) * d + f;
        cv[r] = C[idx];
        q[r] = qsum[idx];
        nc[r] = counts[c0 + cc];
        wc[r] = (double)qcnt[c0 + cc] * wq;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cc = cb + 4 * r;
      if (!((upd >> cc) & 1)) continue;            // wave-uniform
      const int c = c0 + cc;
      double nv = 0.0;
      if (f < d) {
        const long long idx = (long long)c * d + f;
        nv = mb_mean(cv[r], nc[r], (double)q[r] * xq, wc[r]);
        C[idx] = nv;
        qsum[idx] = 0;
      }
      tile[cc][lane] = nv;
      const double df = nv - cv[r];
      const double s1 = wave_sum(nv * nv), s2 = wave_sum(df * df);
      if (lane == 0) {
        pcn[(long long)c * nft + blockIdx.y] = s1;
        pshift[(long long)c * nft + blockIdx.y] = s2;
      }
    }
  }
  __syncthreads();
  if (mine) {
    for (int ff = wave; ff < MB_TILE && f0 + ff < d; ff += 4)
      CT[(long long)(f0 + ff) * k_pad + c0 + lane] = tile[lane][ff];
  }
}

// one wave per centre: cn and the squared shift from the [k][nft] partials
// (lanes stride over the tiles, then a wave sum: a fixed order),
// counts' = counts + w_c; clears qcnt
__global__ void __launch_bounds__(256) mb_finish_kernel(
    double* __restrict__ counts, long long* __restrict__ qcnt, double* __restrict__ cn,
    const double* __restrict__ pcn, const double* __restrict__ pshift, int k, int nft, double wq,
    double* __restrict__ shift) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= k) return;
  const long long q = qcnt[c];
  double a = 0.0, b = 0.0;
  if (q > 0) {
    for (int t = lane; t < nft; t += 64) {
      a += pcn[(long long)c * nft + t];
      b += pshift[(long long)c * nft + t];
    }
    a = wave_sum(a);
    b = wave_sum(b);
  }
  if (lane == 0) {
    if (q > 0) {
      cn[c] = a;
      counts[c] = counts[c] + (double)q * wq;
    }
    shift[c] = b;
    if (q != 0) qcnt[c] = 0;
  }
}

// rec[1] = sum of shift[k] in a fixed order, rec[2] = min of counts[k]
__global__ void __launch_bounds__(256) mb_record_kernel(const double* __restrict__ shift,
                                                        const double* __restrict__ counts, int k,
                                                        double* __restrict__ rec) {
  __shared__ double sh[256], mn[256];
  double a = 0.0, b = INFINITY;
  for (int i = threadIdx.x; i < k; i += 256) {
    a += shift[i];
    b = fmin(b, counts[i]);
  }
  sh[threadIdx.x] = a;
  mn[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[threadIdx.x] += sh[threadIdx.x + o];
      mn[threadIdx.x] = fmin(mn[threadIdx.x], mn[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    rec[1] = sh[0];
    rec[2] = mn[0];
  }
}

// ---------------------------------------------------------------- densify
// out[(dst ? dst[pos] : pos)][:] = X[rows[pos]][:]; an id outside [0, n) or a
// destination outside [0, m_out) is skipped.
__global__ void __launch_bounds__(256) sp_rows_dense_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const float* __restrict__ data, const long long* __restrict__ rows,
    const long long* __restrict__ dst, long long m, long long n, long long m_out, int d,
    double* __restrict__ out, long long ld) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const long long stride = (long long)gridDim.x * wpb;
  for (long long pos = (long long)blockIdx.x * wpb + (threadIdx.x >> 6); pos < m; pos += stride) {
    const long long i = rows[pos];
    const long long o = dst ? dst[pos] : pos;
    if (i < 0 || i >= n || o < 0 || o >= m_out) continue;
    double* row = out + o * ld;
    for (int c = lane; c < d; c += 64) row[c] = 0.0;
    // the zero fill has reached memory before any lane scatters over it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const long long s = indptr[i], e = indptr[i + 1];
    for (long long p = s + lane; p < e; p += 64) {
      const int c = indices[p];
      if (c >= 0 && c < d) row[c] = (double)data[p];
    }
  }
}

}  // namespace sq

using namespace sq;

// labels [m] int32, mind [m] fp64, part [8192] fp64 (one per wave of the grid),
// inertia [1] = sum_t w_t mind[t] in a fixed order
extern "C" int sq_sp_list_estep(const void* indptr, const void* indices, const void* data,
                                const void* CT, const void* cn, const void* xn, const void* rows,
                                long long row0, long long m, long long n, int d, int k, int k_pad,
                                const void* weights, void* labels, void* mind, void* part,
                                void* inertia, void* stream) {
  if (k < 1 || d < 1 || k_pad < k || k_pad % 64 != 0 || m < 0) return (int)hipErrorInvalidValue;
  if (!rows && (row0 < 0 || row0 + m > n)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = sp_grid(m, 4);
  if (m > 0) {
    hipLaunchKernelGGL(sp_list_estep_kernel, dim3(grid), dim3(256), 0, s,
                       (const long long*)indptr, (const int*)indices, (const float*)data,
                       (const double*)CT, (const double*)cn, (const double*)xn,
                       (const long long*)rows, row0, m, n, k, k_pad, (const double*)weights,
                       (int*)labels, (double*)mind, (double*)part);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(sp_sum_parts_kernel, dim3(1), dim3(256), 0, s, (const double*)part,
                     m > 0 ? (int)grid * 4 : 0, (double*)inertia);
  return (int)hipGetLastError();
}

// qsum [k * d] and qcnt [k] int64 accumulate; the caller zeroes them once
extern "C" int sq_sp_list_mstep(const void* indptr, const void* indices, const void* data,
                                const void* rows, long long row0, const void* labels,
                                const void* weights, long long m, long long n, int d, int k,
                                int xexp, int wexp, void* qsum, void* qcnt, void* stream) {
  if (k < 1 || d < 1 || m < 0) return (int)hipErrorInvalidValue;
  if (!rows && (row0 < 0 || row0 + m > n)) return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  hipLaunchKernelGGL(sp_mstep_kernel<true>, dim3(sp_grid(m, 4)), dim3(256), 0,
                     (hipStream_t)stream, (const long long*)indptr, (const int*)indices,
                     (const float*)data, (const long long*)rows, row0, (const int*)labels,
                     (const double*)weights, m, n, d, k, ldexp(1.0, -xexp), ldexp(1.0, -wexp),
                     (long long*)qsum, (long long*)qcnt);
  return (int)hipGetLastError();
}

// C [k][d], CT [d][k_pad], cn [k], counts [k] are updated in place; qsum and
// qcnt are consumed and left zero; pcn and pshift are [k][ceil(d / 64)]
// scratch, shift is [k] scratch; rec[1] = squared shift, rec[2] = min count.
extern "C" int sq_mb_update(void* C, void* CT, void* cn, void* counts, void* qsum, void* qcnt,
                            int k, int d, int k_pad, int xexp, int wexp, void* pcn, void* pshift,
                            void* shift, void* rec, void* stream) {
  if (k < 1 || d < 1 || k_pad < k || k_pad % 64 != 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int nct = (k + MB_TILE - 1) / MB_TILE, nft = (d + MB_TILE - 1) / MB_TILE;
  if (nft > 65535) return (int)hipErrorInvalidValue;
  const double wq = ldexp(1.0, wexp);
  hipLaunchKernelGGL(mb_update_kernel, dim3(nct, nft), dim3(256), 0, s, (double*)C, (double*)CT,
                     (const double*)counts, (long long*)qsum, (const long long*)qcnt, k, d, k_pad,
                     ldexp(1.0, xexp), wq, (double*)pcn, (double*)pshift);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(mb_finish_kernel, dim3((k + 3) / 4), dim3(256), 0, s, (double*)counts,
                     (long long*)qcnt, (double*)cn, (const double*)pcn, (const double*)pshift, k,
                     nft, wq, (double*)shift);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(mb_record_kernel, dim3(1), dim3(256), 0, s, (const double*)shift,
                     (const double*)counts, k, (double*)rec);
  return (int)hipGetLastError();
}

extern "C" int sq_sp_rows_dense(const void* indptr, const void* indices, const void* data,
                                const void* rows, const void* dst, long long m, long long n,
                                long long m_out, int d, void* out, long long ld, void* stream) {
  if (d < 1 || ld < d || m < 0 || !rows) return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  hipLaunchKernelGGL(sp_rows_dense_kernel, dim3(sp_grid(m, 4)), dim3(256), 0,
                     (hipStream_t)stream, (const long long*)indptr, (const int*)indices,
                     (const float*)data, (const long long*)rows, (const long long*)dst, m, n,
                     m_out, d, (double*)out, ld);
  return (int)hipGetLastError();
}
