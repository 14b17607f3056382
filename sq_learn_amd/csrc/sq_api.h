// The native boundary: the one declaration of every extern "C" sq_* entry
// point of the .hip translation units.  Each .hip file that defines or calls
// one includes this header, so a definition that disagrees with it is a
// compile error (conflicting C-linkage declarations); module.cpp includes it
// with SQ_API defined as a weak attribute (a variant build may lack a
// translation unit and must still load) and derives each binding's argument
// parsing from the prototype.  Pointers are device pointers unless noted,
// ``stream`` is a hipStream_t; every launcher returns a hipError_t as int
// unless noted.
#pragma once

#ifndef SQ_API
#define SQ_API
#endif

extern "C" {

// qrand.hip
SQ_API int sq_trunc_normal_add(void* x, int dtype, long long n, double b, unsigned k0, unsigned k1,
                               unsigned s0, unsigned s1, unsigned long long offset, void* stream);
SQ_API int sq_philox_normal(void* out, int dtype, long long n, double mean, double stdv,
                            unsigned k0, unsigned k1, unsigned s0, unsigned s1,
                            unsigned long long offset, void* stream);
SQ_API int sq_philox_uniform(void* out, long long n, unsigned k0, unsigned k1, unsigned s0,
                             unsigned s1, unsigned long long offset, void* stream);
SQ_API int sq_ae_batch(const void* a, const void* eps, void* out, long long n, int Q, unsigned k0,
                       unsigned k1, unsigned s0, unsigned s1, unsigned long long offset,
                       void* stream);
// out[i] = k / 2^m[i].  0 <= m[i] <= 40: the fp32 walk of fejer.h is scaled to
// stay clear of underflow through M = 2^40 at every phase; the launcher does
// not read m (device memory), ops/random.py phase_estimation_batch rejects
// values outside the range.
SQ_API int sq_pe_batch(const void* omega, const void* m, void* out, long long n, unsigned k0,
                       unsigned k1, unsigned s0, unsigned s1, unsigned long long offset,
                       void* stream);

// tomography.hip
SQ_API int sq_tomography(const void* V, int r, int d, const void* sched, int T, int mode,
                         const void* first, void* err, void* out, int norm_inf, unsigned k0,
                         unsigned k1, unsigned s0, unsigned s1, long long row_offset, void* stream,
                         double stop_err);
SQ_API int sq_mnom_segments(const void* W, long long ldw, const void* wrow, long long m,
                            long long B, const void* Nseg, void* cnt, long long ldc, unsigned k0,
                            unsigned k1, unsigned s0, unsigned s1, const void* sid, int level,
                            void* stream);

// tsgemm64.hip (sq_xtx_geometry: host out-parameters, returns 0)
SQ_API int sq_xtx_geometry(int da, int db, int sym, int* TM, int* TN, int* n_pairs);
SQ_API int sq_xtx(const void* A, int ta, long long lda, const void* mua, int da, const void* B,
                  int tb, long long ldb, const void* mub, int db, long long n, int sym,
                  int n_splits, void* part, void* C, int accumulate, void* stream);
SQ_API int sq_xw(const void* A, int ta, long long lda, const void* mu, long long n, int d,
                 const void* W, long long ldw, int l, int upper, void* Y, int to, long long ldy,
                 void* stream);

// ipe.hip
SQ_API int sq_ipe_fused(const void* X, long long ldx, const void* Cf, const void* C,
                        const void* hint_labels, const void* xn, const void* cn, void* labels,
                        void* mind, long long n, int d, int d_pad, int k, int k_pad, double eps,
                        int Q, unsigned k0, unsigned k1, unsigned s0, unsigned s1, unsigned t0,
                        unsigned t1, unsigned ts0, unsigned ts1, unsigned q0, unsigned q1,
                        unsigned qs0, unsigned qs1, long long row_offset, int prune, void* stats,
                        void* scratch, void* stream, const void* rlist, const void* rcount,
                        long long list_n, const void* ext_thr_in, const void* ext_hj_in);

// ipe16.hip (ia / da: host argument arrays of the op)
SQ_API int sq_ipe16(int op, const long long* ia, const double* da, void* stream);

// pairwise_fast.hip
SQ_API int sq_pairwise_reduce(const void* X, const void* Y, void* out, int n, int m, int d, int op,
                              double p, int dtype, void* stream);

// forest.hip
SQ_API int sq_forest_apply(const void* left, const void* right, const void* feature,
                           const void* thr, const void* offs, int T, const void* X, long long n,
                           int d, void* out, void* stream);
SQ_API int sq_forest_predict(const void* left, const void* right, const void* feature,
                             const void* thr, const void* missing_left, const void* offs, int T,
                             const void* value, int s_act, const void* X, long long n, int d,
                             double scale, void* out, void* stream);

// elkan.hip
SQ_API int sq_elkan_step(const void* X, const void* C, const void* hcc, const void* snext,
                         const void* shift, void* labels, void* upper, void* lower, long long n,
                         int d, int k, int dtype, int init, void* stream);

// spkmeans.hip (sq_sp_estep_parts: the partial count, not an error code)
SQ_API int sq_sp_row_norms(const void* indptr, const void* data, void* xn, long long n,
                           void* stream);
SQ_API int sq_sp_estep_parts(long long n, int k);
SQ_API int sq_sp_estep(const void* indptr, const void* indices, const void* data, const void* CT,
                       const void* cn, const void* xn, long long row0, long long row1, int d,
                       int k, int k_pad, int mode, double delta, unsigned k0, unsigned k1,
                       unsigned s0, unsigned s1, long long row_offset, void* labels, void* mind,
                       void* part, void* inertia, void* out, long long ldo, void* stream);
SQ_API int sq_sp_mstep(const void* indptr, const void* indices, const void* data,
                       const void* labels, const void* weights, long long n, int d, int k,
                       int xexp, int wexp, void* qsum, void* qcnt, void* sums, void* counts,
                       void* stream);

// spminibatch.hip
SQ_API int sq_sp_list_estep(const void* indptr, const void* indices, const void* data,
                            const void* CT, const void* cn, const void* xn, const void* rows,
                            long long row0, long long m, long long n, int d, int k, int k_pad,
                            const void* weights, void* labels, void* mind, void* part,
                            void* inertia, void* stream);
SQ_API int sq_sp_list_mstep(const void* indptr, const void* indices, const void* data,
                            const void* rows, long long row0, const void* labels,
                            const void* weights, long long m, long long n, int d, int k, int xexp,
                            int wexp, void* qsum, void* qcnt, void* stream);
SQ_API int sq_mb_update(void* C, void* CT, void* cn, void* counts, void* qsum, void* qcnt, int k,
                        int d, int k_pad, int xexp, int wexp, void* pcn, void* pshift, void* shift,
                        void* rec, void* stream);
SQ_API int sq_sp_rows_dense(const void* indptr, const void* indices, const void* data,
                            const void* rows, const void* dst, long long m, long long n,
                            long long m_out, int d, void* out, long long ld, void* stream);

// spmm.hip (sq_spmm_tile_cols: the column count, not an error code)
SQ_API int sq_spmm_tile_cols();
SQ_API int sq_spmm(const void* indptr, const void* indices, const void* data, const void* seg_row,
                   const void* seg_start, const void* seg_dst, long long nseg, int seg,
                   const void* long_row, const void* long_ptr, long long nlong, const void* B,
                   long long ldb, int l, void* out, long long ldo, void* scratch, void* stream);
SQ_API int sq_sp_row_moments(const void* indptr, const void* data, void* sum, void* sumsq,
                             long long n, void* stream);

// spmu.hip (sq_sp_mu_row_waves: the rows of `part`, not an error code).  mu(A) power sums
// of the CSR matrix (indptr, indices, data) [n, d] with the CSR of its transpose (tptr, tdata)
// and that transpose's segment table: rowmax [nq], colsum [nq, d], q [nq] fp64, qstep > 0:
// q is 0, qstep, 2 qstep, ...; mean [d] and base [nq] = sum_j |mean_j|^q (both or neither);
// part [sq_sp_mu_row_waves(n), nq], scratch [slots of the table, nq]
SQ_API int sq_sp_mu_row_waves(long long n);
SQ_API int sq_sp_mu_sums(const void* indptr, const void* indices, const void* data,
                         const void* tptr, const void* tdata, const void* seg_row,
                         const void* seg_start, const void* seg_dst, long long nseg, int seg,
                         const void* long_row, const void* long_ptr, long long nlong, long long n,
                         long long d, const void* q, int nq, double qstep, const void* mean,
                         const void* base, void* rowmax, void* colsum, void* part, void* scratch,
                         void* stream);

// spknn.hip (sq_sp_knn_tile_max: the tile size, not an error code)
SQ_API int sq_sp_knn_tile_max();
SQ_API int sq_sp_knn(const void* qptr, const void* qidx, const void* qval, const void* trow,
                     const void* tval, const void* tab, const void* qn, const void* xn,
                     const void* qexp, long long q0, long long m, long long n, int d, int T,
                     long long nnz_x, int kk, int metric, int mode, void* pd, void* pi, void* dist,
                     void* outd, void* outi, void* stream);

// spradius.hip
SQ_API int sq_sp_radius_mark(const void* qptr, const void* qidx, const void* qval, const void* trow,
                             const void* tval, const void* tab, const void* qn, const void* xn,
                             const void* qexp, long long q0, long long m, long long n, int d, int T,
                             long long nnz_x, int metric, double thr, int self_join, void* mask,
                             void* cnt, void* stream);
SQ_API int sq_sp_radius_fill(const void* mask, const void* cs, long long m, long long n, int T,
                             long long total, void* out, void* stream);

// splda.hip (sq_sp_lda_stage: the doubles of gathered rows a wave stages in LDS,
// sq_sp_lda_max_k: the largest topic count; neither is an error code)
SQ_API int sq_sp_lda_stage();
SQ_API int sq_sp_lda_max_k();
SQ_API int sq_sp_lda_estep(const void* indptr, const void* indices, const void* data,
                           const void* tw_t, void* doc_topic, long long q0, long long m, int F,
                           int k, double prior, int max_iters, double tol, void* iters, void* qhi,
                           void* qlo, int hexp, int lexp, void* stream);
SQ_API int sq_sp_lda_bound(const void* indptr, const void* indices, const void* data,
                           const void* elog_theta, const void* elog_beta_t, long long q0,
                           long long m, int F, int k, void* out, void* stream);

// spnmf.hip (the first seven return a limit or a launch geometry, not an error code:
// the doubles of gathered rows a wave stages in LDS and the least doubles a staged
// entry counts as, the largest component count and the waves per workgroup of the
// ratio kernel at k; the largest component count of the sweep, the k up to which it
// keeps HHt in LDS and its rows per wave at k)
SQ_API int sq_sp_nmf_stage();
SQ_API int sq_sp_nmf_stage_min_row();
SQ_API int sq_sp_nmf_max_k();
SQ_API int sq_sp_nmf_wpb(int k);
SQ_API int sq_nmf_cd_max_k();
SQ_API int sq_nmf_cd_hht_k();
SQ_API int sq_nmf_cd_rows(int k);
SQ_API int sq_sp_nmf_kl(const void* indptr, const void* indices, const void* data, const void* P,
                        const void* Q, long long q0, long long m, int cols, int k, double eps,
                        void* num, void* div, void* stream);
SQ_API int sq_nmf_cd_sweep(void* W, const void* HHt, const void* XHt, const void* perm,
                           long long row0, long long m, int k, void* rowviol, void* violation,
                           void* stream);

// splogit.hip (sq_sp_logit_tile_classes: the classes one pass over a row covers, not
// an error code; b of sq_sp_logit_bin: the intercept, a host value)
SQ_API int sq_sp_logit_tile_classes();
SQ_API int sq_sp_logit_multi(const void* indptr, const void* indices, const void* data,
                             const void* Wt, long long ldw, const void* bias, const void* lab,
                             const void* sw, long long n, int K, void* R, void* rowloss,
                             void* loss, void* stream);
SQ_API int sq_sp_logit_bin(const void* indptr, const void* indices, const void* data,
                           const void* w, double b, const void* lab, const void* sw, long long n,
                           int d, void* r, void* rowloss, void* loss, void* stream);
SQ_API int sq_sp_matvec(const void* indptr, const void* indices, const void* data,
                        const void* seg_row, const void* seg_start, const void* seg_dst,
                        long long nseg, int seg, const void* long_row, const void* long_ptr,
                        long long nlong, const void* x, int cols, void* y, void* scratch,
                        void* stream);

// spgram.hip (kind: 0 linear, 1 poly, 2 rbf, 3 sigmoid; out: the first row of the
// whole result, row q at out + q * ld)
SQ_API int sq_sp_gram(const void* qptr, const void* qidx, const void* qval, const void* trow,
                      const void* tval, const void* tab, const void* qn, const void* xn,
                      const void* qexp, long long q0, long long m, long long n, int d, int T,
                      long long nnz_x, int kind, double gamma, double coef0, double degree,
                      int self_join, double diag_add, void* out, long long ld, void* stream);
SQ_API int sq_sp_gram_matvec(const void* qptr, const void* qidx, const void* qval,
                             const void* trow, const void* tval, const void* tab, const void* qn,
                             const void* xn, const void* qexp, long long q0, long long m,
                             long long n, int d, int T, long long nnz_x, int kind, double gamma,
                             double coef0, double degree, int self_join, const void* V, int R,
                             void* part, void* out, void* stream);

// failure.hip
SQ_API int sq_failure_inject(void* labels, long long n, int k, double p, int R, unsigned k0,
                             unsigned k1, unsigned s0, unsigned s1, unsigned t0, unsigned t1,
                             unsigned u0, unsigned u1, long long row_offset, void* counters,
                             void* lb, void* corr, void* mind, const void* X, long long ldx,
                             const void* C, int ldc, int d, void* stream);

// kmeans.hip
SQ_API int sq_estep_bf16(const void* X, const void* C, void* part, const void* cn, const void* xn,
                         void* labels, void* mind, void* ovf_rows, void* ovf_count, void* inertia,
                         long long n, int d, int k, int k_pad, double delta, int part_cap,
                         unsigned k0, unsigned k1, unsigned s0, unsigned s1, long long row_offset,
                         int ovf_cap, void* stream);
SQ_API int sq_band_select(const void* D, const void* rows, const void* xn, void* labels, void* mind,
                          long long m, int k, long long ldD, double delta, unsigned k0, unsigned k1,
                          unsigned s0, unsigned s1, long long row_offset, void* stream);
SQ_API int sq_band_select_rows(const void* X, const void* C, const void* cn, const void* xn,
                               const void* rows, const void* count, void* labels, long long cap,
                               int d_pad, int k, int k_pad, double delta, unsigned k0, unsigned k1,
                               unsigned s0, unsigned s1, long long row_offset, void* stream);
SQ_API int sq_centroid_accumulate(const void* X, int xdtype, const void* labels,
                                  const void* weights, void* sums, void* counts, long long n, int d,
                                  int k, int chunk, void* stream);
SQ_API int sq_centroid_reduce(const void* X, int xdtype, const void* labels, const void* weights,
                              void* sums, void* counts, long long n, int d, int k, int xexp,
                              int wexp, void* ws_hist, void* ws_cursor, void* ws_perm, void* mind,
                              const void* Cold, void* stream);
SQ_API int sq_centroid_delta(const void* X, const void* labels, const void* prev, void* sums,
                             void* counts, void* qsum, long long n, int d, int k, int xexp,
                             int qexp, void* ws_hist, void* ws_cursor, void* ws_perm, void* stream);
SQ_API int sq_centroid_delta_lists(const void* X, const void* labels, const void* prev, void* sums,
                                   void* counts, void* qsum, long long n, int d, int k, int xexp,
                                   int qexp, void* ws_hist, void* ws_cursor, void* ws_perm,
                                   const void* L0, const void* c0, const void* L1, const void* c1,
                                   const void* L2, const void* c2, void* stream);
SQ_API int sq_cluster_inertia(const void* sums, const void* counts, const void* qsum, const void* C,
                              int k, int d, int xexp, int qexp, void* part, void* stream);
SQ_API int sq_pack_stats(const void* sums, const void* counts, const void* inertia, void* packed,
                         int k, int d, int xexp, int wexp, void* stream);
SQ_API int sq_mstep_stats(const void* sums, const void* counts, const void* qsum, const void* C,
                          int k, int d, int xexp, int qexp, const void* corr, long long n,
                          void* part, void* inertia, void* packed, void* stream);
SQ_API int sq_sum_partials(const void* part, int n, void* out, void* stream);
SQ_API int sq_centroid_finalize(const void* packed, const void* C_old, void* C_new, void* C_bf16,
                                void* shift_part, void* cn, void* shift, int k, int d, int k_pad,
                                double noise_b, unsigned k0, unsigned k1, unsigned s0, unsigned s1,
                                int empty_policy, void* scalars, void* ovf_count, void* C_f16,
                                double alpha, void* cmax2, const void* kept, void* stream);
SQ_API int sq_ipe_estep(const void* G, const void* xn, const void* cn, void* labels, void* mind,
                        long long m, int k, long long ldG, double eps, int Q, unsigned k0,
                        unsigned k1, unsigned s0, unsigned s1, long long row_offset, void* stream);

// kmpp.hip (sq_kmpp_grid: the grid size, not an error code; ia: a host
// argument array of the op)
SQ_API int sq_kmpp_grid(long long n);
SQ_API int sq_kmpp_init(const void* X, long long ldx, int d, long long n, const void* c0,
                        const void* w, void* closest, void* nearest, void* bmax, void* Xq, int dq,
                        void* srow, void* erow, void* q2row, void* stream);
SQ_API int sq_kmpp_block_totals(const void* closest, const void* w, long long n, long long R, int G,
                                double scale, void* block_tot, void* stream);
SQ_API int sq_kmpp_cc(const void* cand, const void* C, int c, int d, int t, void* cc, int ldcc,
                      void* cinfo, void* candq, int dq, void* delta_part, long long ndp,
                      void* counters, void* stream);
SQ_API int sq_kmpp_screen(void* closest, void* nearest, const void* mask_prev, const void* Dprev,
                          const void* best_prev, int c_prev, const void* cc, int ldcc, int t,
                          long long n, long long R, int G, void* mask_out, void* surv, void* exact,
                          void* scount, void* ecount, int prune, void* stream);
SQ_API int sq_kmpp_bound(const void* Xq, int dq, const void* srow, const void* erow,
                         const void* xq2, const void* closest, const void* candq,
                         const void* cinfo, int t, int d, long long n, long long R, int G,
                         const void* surv, const void* scount, void* exact, void* ecount,
                         void* stream);
SQ_API int sq_kmpp_dots(const void* Xq, int dq, long long n, const void* candq, void* out,
                        void* stream);
SQ_API int sq_kmpp_exact(const void* X, long long ldx, int d, long long n, int t, const void* cand,
                         const void* closest, const void* w, double scale, const void* exact,
                         const void* ecount, void* mask_out, void* Dout, void* delta_part,
                         long long R, int G, void* stream);
SQ_API int sq_kmpp_pick(const void* block_tot, int G, long long R, long long n, const void* vals,
                        int t, const void* closest, const void* mask, const void* D,
                        const void* best, const void* w, double scale, void* pos, const void* X,
                        long long ldx, int d, void* cands, void* cand_ids, long long row_offset,
                        long long n_global, void* stream);
SQ_API int sq_kmpp_finish(const void* delta_part, int G, int t, void* block_tot, void* P,
                          const void* draws_next, void* vals, const void* cands,
                          const void* cand_ids, int d, void* centers, void* ids, int c,
                          void* best_out, void* stream);
SQ_API int sq_kmpp_batch(int op, const long long* ia, void* stream);

// estep_f32.hip
// The gap records of a certified E-step (rec null / rec_on 0: off): the
// screen writes a row's record with base it_now (rec_mflag = 2 + base), the
// filter lists rows whose base is in [it_lo, it_now - 1] in mrows_b / count_b,
// the gap screen moves them by the shift operand of their base (dsh / dq,
// slot base % ring) and lists the rows that can have moved in mrows_mv /
// count_mv (optional).  ovf2_rows / ovf2_count (optional): the second
// overflow list of the dense-row 3-pass kernel.
SQ_API int sq_bounds_filter(const void* labels, void* ub, void* lb, const void* shift,
                            const void* smax, long long n, double delta, void* rlist, void* rcount,
                            const void* mflag, void* mrows, void* multi_count, const void* cc,
                            const void* fidx, int nf, int k, void* stream, void* corr,
                            void* rec_count, int rec_on, int it_now, int it_lo, void* mrows_b,
                            void* count_b);
SQ_API int sq_fast_centroids(void* shift, const void* shift_sq, const void* C, int k, int d, int nf,
                             void* idx, void* smax_rest, void* cc, void* stream);
SQ_API int sq_shift_operand(const void* Cprev, const void* Cnew, int ldc, int d, int d_pad, int k,
                            double alpha, void* snap, void* dsh, void* dq, int ring, int snew,
                            unsigned valid, void* stream);
SQ_API int sq_estep_f32(const void* X, const void* C, const void* xn, void* labels, void* mind,
                        void* ovf_rows, void* ovf_count, void* part, int part_cap, void* inertia,
                        long long n, int d_pad, int k_pad, double alpha, double delta, unsigned k0,
                        unsigned k1, unsigned s0, unsigned s1, long long row_offset, int ovf_cap,
                        void* stream);
SQ_API int sq_estep_x64(const void* Xh, const void* X, const void* C, const void* Cm,
                        const void* xn, const void* cmax2, void* labels, void* mind,
                        void* dense_rows, void* ovf_rows, void* mrows, void* mcand, void* corr,
                        void* rlist, void* rcount, void* ub, void* lb, void* mflag, void* xflag,
                        void* counts, void* part, int part_cap, long long n, int d, int d_pad,
                        int k, int k_pad, double alpha, double delta, unsigned k0, unsigned k1,
                        unsigned s0, unsigned s1, long long row_offset, int list_rs, void* stream,
                        void* rec, void* rec_mflag, int it_now, int it_lo, int ring,
                        const void* dsh, const void* dq, long long dsh_stride, void* mrows_b,
                        void* count_b, void* n_done, void* mrows_mv, void* count_mv,
                        void* ovf2_rows, void* ovf2_count);
// The gap screen of sq_estep_x64 alone, on the caller's buffers (n: capacity
// of the lists).  grid_blocks (0: the default grid) and ydbg (null: off; float
// [n][4], the scaled x.S per list position and candidate slot) are for tests
// and timing (ops/kmeans.py calls it through ctypes: the module's method table
// lists what the estimators call).
SQ_API int sq_gap_screen(const void* Xh, const void* xn, const void* mrows_b, const void* count_b,
                         const void* dsh, const void* dq, long long dsh_stride, int ring,
                         double alpha, double delta, void* labels, void* rec, void* rec_mflag,
                         int it_now, void* mrows, void* multi_count, void* n_done, void* mrows_mv,
                         void* count_mv, long long n, int d_pad, int grid_blocks, void* ydbg,
                         void* stream);
// (diagnostic builds with -DSQ_X64_STAMP=1 only; host: a host buffer)
SQ_API int sq_x64_stamps(void* host, int n_waves);
SQ_API int sq_x64_stamps_clear();
SQ_API int sq_fill_mind(const void* X, int ldx, const void* Cm, int d, const void* labels,
                        void* mind, long long n, void* stream);
SQ_API int sq_sum_f32(const void* v, long long n, void* part, int extra, void* out, void* stream);
SQ_API int sq_centers_f16_operand(const void* Cm, void* op, int k, int d, int d_pad, int k_pad,
                                  double alpha, void* stream);

// rows_f64.hip
SQ_API int sq_rows_f64(const void* X, long long ldx, const void* C, long long ldc, int d, int k,
                       const void* rows, const void* count, long long n_direct, long long cap,
                       void* labels, void* mind, void* corr, void* ub, double delta, unsigned k0,
                       unsigned k1, unsigned s0, unsigned s1, long long row_offset, int grid,
                       void* stream);

// linalg.hip
SQ_API int sq_mu_sums(const void* X, int xdtype, long long ldx, const void* qs, int nq,
                      void* rowmax, void* colsum, void* part, int part_wgs, void* rowacc,
                      long long n, int d, const void* mean, float qstep, void* stream);
SQ_API int sq_col_moments(const void* X, int xdtype, long long ldx, long long n, int d, void* part,
                          int part_wgs, void* stream);
SQ_API int sq_row_norms(const void* X, int xdtype, void* out, long long n, int d, void* stream);

// knn.hip
SQ_API int sq_knn_topk(const void* D, void* outd, void* outi, long long m, int nref, long long ldD,
                       int kk, long long col_offset, void* stream);

}  // extern "C"
