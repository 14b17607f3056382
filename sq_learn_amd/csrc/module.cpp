// CPython extension module ``sq_learn_amd._C``: argument marshalling to the
// extern "C" launchers declared in sq_api.h.  One template (``bind``) derives
// a binding from the launcher's prototype: the argument format string, the
// storage, the pointer conversion and the call, so a binding takes exactly
// the C function's parameters in the C function's order and cannot disagree
// with it.  Pointers arrive as integers (tensor.data_ptr()), the HIP stream
// as the integer handle of torch.cuda.current_stream(), so every launch is
// stream-ordered with torch and capturable in a hipGraph.  No torch C++
// headers: the native layer is ABI-independent of the torch build.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <tuple>

// weak: a variant build may lack a translation unit and must still load
#define SQ_API __attribute__((weak))
#include "sq_api.h"

// One parameter type of a launcher: its format character, the
// type parsed into, the conversion to the parameter.
template <class T, char C>
struct Scalar {
  using store = T;
  static constexpr char fmt = C;
  static T get(T v) { return v; }
};
template <class T> struct Slot;
template <> struct Slot<int> : Scalar<int, 'i'> {};
template <> struct Slot<long long> : Scalar<long long, 'L'> {};
template <> struct Slot<double> : Scalar<double, 'd'> {};
template <> struct Slot<float> : Scalar<float, 'f'> {};
template <> struct Slot<unsigned> : Scalar<unsigned, 'I'> {};
template <> struct Slot<unsigned long long> : Scalar<unsigned long long, 'K'> {};
template <class T>
struct Slot<T*> {   // every pointer: an integer address
  using store = unsigned long long;
  static constexpr char fmt = 'K';
  static T* get(store v) { return (T*)(uintptr_t)v; }
};

template <class F> struct Format;
template <class... A>
struct Format<int (*)(A...)> {
  static constexpr char str[sizeof...(A) + 1] = {Slot<A>::fmt..., '\0'};
};

static PyObject* ret(int rc) {
  if (rc != 0) {
    PyErr_Format(PyExc_RuntimeError, "sq_learn_amd native launch failed: %s (%d)",
                 hipGetErrorString((hipError_t)rc), rc);
    return nullptr;
  }
  Py_RETURN_NONE;
}

enum : unsigned {
  NOGIL = 1,   // release the GIL around the call
  VALUE = 2,   // the int is the result, not an error code
};

template <unsigned FLAGS, class... A>
static PyObject* bind(const char* symbol, int (*fn)(A...), PyObject* args) {
  std::tuple<typename Slot<A>::store...> v{};
  if (!std::apply([&](auto&... s) {
        return PyArg_ParseTuple(args, Format<int (*)(A...)>::str, &s...);
      }, v))
    return nullptr;
  if (!fn) {
    PyErr_Format(PyExc_RuntimeError, "native symbol %s not built", symbol);
    return nullptr;
  }
  auto call = [&] { return std::apply([&](auto... s) { return fn(Slot<A>::get(s)...); }, v); };
  int rc;
  if constexpr (FLAGS & NOGIL) {
    Py_BEGIN_ALLOW_THREADS
    rc = call();
    Py_END_ALLOW_THREADS
  } else {
    rc = call();
  }
  if constexpr (FLAGS & VALUE) return PyLong_FromLong(rc);
  return ret(rc);
}

// doc + "\n\nargs: " + format, as one static string
template <size_t N, size_t M>
constexpr std::array<char, N + M + 8> doc_args(const char (&doc)[N], const char (&fmt)[M]) {
  constexpr char sep[] = "\n\nargs: ";
  std::array<char, N + M + 8> out{};
  size_t o = 0;
  for (size_t i = 0; i + 1 < N; ++i) out[o++] = doc[i];
  for (size_t i = 0; i + 1 < sizeof(sep); ++i) out[o++] = sep[i];
  for (size_t i = 0; i < M; ++i) out[o++] = fmt[i];
  return out;
}

// volatile: the weak symbol's null test survives inlining
#define SQ_FN(name, flags, doc)                                                          \
  {#name,                                                                                \
   [](PyObject*, PyObject* args) -> PyObject* {                                          \
     decltype(&sq_##name) volatile fn = &sq_##name;                                      \
     return bind<flags>("sq_" #name, fn, args);                                          \
   },                                                                                    \
   METH_VARARGS, [] {                                                                    \
     static constexpr auto text = doc_args(doc, Format<decltype(&sq_##name)>::str);      \
     return text.data();                                                                 \
   }()}

static PyObject* py_xtx_geometry(PyObject*, PyObject* a) {
  int da, db, sym, TM, TN, np;
  if (!PyArg_ParseTuple(a, "iii", &da, &db, &sym)) return nullptr;
  if (!sq_xtx_geometry) {
    PyErr_SetString(PyExc_RuntimeError, "native symbol sq_xtx_geometry not built");
    return nullptr;
  }
  sq_xtx_geometry(da, db, sym, &TM, &TN, &np);
  return Py_BuildValue("(iii)", TM, TN, np);
}

static PyObject* py_device_arch(PyObject*, PyObject*) {
  hipDeviceProp_t prop;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
    Py_RETURN_NONE;
  return Py_BuildValue("(siii)", prop.gcnArchName, prop.multiProcessorCount,
                       (int)prop.maxSharedMemoryPerMultiProcessor, prop.warpSize);
}

static PyMethodDef methods[] = {
    SQ_FN(forest_apply, 0, "leaf ids of (row, tree) pairs"),
    SQ_FN(forest_predict, 0, "sum of leaf values over trees"),
    SQ_FN(trunc_normal_add, NOGIL, "x += TN(-b,b) (Philox keyed)"),
    SQ_FN(philox_normal, 0, "fill with mean+std*N(0,1)"),
    SQ_FN(philox_uniform, 0, "fill with U(0,1)"),
    SQ_FN(ae_batch, 0, "batched median-of-Q amplitude estimation"),
    SQ_FN(pe_batch, 0, "batched phase estimation"),
    SQ_FN(estep_bf16, 0, "fused MFMA distance + delta-band E-step"),
    SQ_FN(band_select, 0, "delta-band selection over distance rows"),
    SQ_FN(band_select_rows, 0, "device-driven overflow fallback"),
    SQ_FN(pairwise_reduce, 0, "L1 / chi2 / chebyshev / minkowski tiles"),
    SQ_FN(elkan_step, 0, "Elkan bounded k-means assignment"),
    SQ_FN(sp_row_norms, 0, "CSR squared row norms (fp64)"),
    SQ_FN(sp_estep, NOGIL, "CSR E-step: delta-band labels / gram / distances"),
    SQ_FN(sp_mstep, 0, "CSR cluster sums (64-bit fixed-point atomics)"),
    SQ_FN(sp_list_estep, 0, "CSR row-list argmin E-step"),
    SQ_FN(sp_list_mstep, 0, "CSR row-list fixed-point scatter"),
    SQ_FN(mb_update, 0, "fused mini-batch centre update"),
    SQ_FN(sp_rows_dense, 0, "CSR rows to dense fp64 rows"),
    SQ_FN(spmm_tile_cols, VALUE, "columns per pass of the CSR x dense kernel"),
    SQ_FN(spmm, NOGIL, "CSR x dense fp64 product over row segments"),
    SQ_FN(sp_row_moments, 0, "CSR per-row sum and sum of squares (fp64)"),
    SQ_FN(sp_knn_tile_max, VALUE, "largest fit tile of the sparse k-NN kernel"),
    SQ_FN(sp_knn, 0, "CSR x CSR brute k-NN through an inverted index"),
    SQ_FN(sp_radius_mark, 0, "CSR x CSR radius test: one bit per pair"),
    SQ_FN(sp_radius_fill, 0, "marked pairs to ascending index lists"),
    SQ_FN(failure_inject, 0, "Bernoulli estimation failure + resampling"),
    SQ_FN(tomography, 0, "batched shot-based vector tomography"),
    SQ_FN(mnom_segments, 0, "segmented multinomial (long vectors)"),
    SQ_FN(xtx, 0, "fp64 MFMA (A-mu_a)^T (B-mu_b), split-K + fixed-order finalize"),
    {"xtx_geometry", py_xtx_geometry, METH_VARARGS, "xtx tile sizes and pair count"},
    SQ_FN(xw, 0, "fp64 MFMA (A-mu) W"),
    SQ_FN(bounds_filter, 0, "Hamerly pruning -> active row list"),
    SQ_FN(shift_operand, 0, "fp16 centroid-shift operand (gap screen)"),
    SQ_FN(fast_centroids, 0, "fastest centroids + Elkan distances"),
    SQ_FN(centroid_delta, 0, "incremental fixed-point cluster stats"),
    SQ_FN(centroid_delta_lists, 0, "incremental cluster stats over a filtered E-step's row lists"),
    SQ_FN(cluster_inertia, 0, "per-cluster inertia from the stats"),
    SQ_FN(ipe_fused, 0, "fused fp32-MFMA + amplitude-estimation IPE E-step"),
    SQ_FN(ipe16, 0, "certified fp16 screen of the IPE E-step (op per phase)"),
    SQ_FN(kmpp_batch, 0, "batched k-means++ restarts (op per phase)"),
    SQ_FN(centroid_accumulate, 0, "label-segmented row sums"),
    SQ_FN(centroid_reduce, 0, "counting-sort segmented row sums"),
    SQ_FN(centroid_finalize, 0, "centroid average + noise + shift"),
    SQ_FN(mstep_stats, 0, "incremental M-step inertia + packed bucket"),
    SQ_FN(estep_f32, 0, "fp32-faithful fused E-step (fp16 hi/lo MFMA)"),
    SQ_FN(estep_x64, 0, "certified filter E-step + fp64 re-check"),
    SQ_FN(fill_mind, 0, "exact distance to the label for marked rows"),
    SQ_FN(sum_f32, 0, "deterministic sum of a float vector"),
    SQ_FN(kmpp_grid, VALUE, "k-means++ trial pass grid size"),
    SQ_FN(kmpp_init, 0, "k-means++ first centre distances"),
    SQ_FN(kmpp_block_totals, 0, "k-means++ fixed-point block totals"),
    SQ_FN(kmpp_cc, 0, "k-means++ candidate-centre distances"),
    SQ_FN(kmpp_screen, 0, "k-means++ triangle screen + lazy update"),
    SQ_FN(kmpp_bound, 0, "k-means++ certified int8 bound"),
    SQ_FN(kmpp_exact, 0, "k-means++ exact fp32 trial distances"),
    SQ_FN(kmpp_dots, 0, "int8 MFMA dots of the k-means++ bound (test hook)"),
    SQ_FN(kmpp_finish, 0, "k-means++ winner of one centre (one rank)"),
    SQ_FN(kmpp_pick, 0, "k-means++ two-level potential sampling"),
    SQ_FN(rows_f64, 0, "exact fp64 E-step over a row list (fp64 MFMA)"),
    SQ_FN(centers_f16_operand, 0, "fp16-split centroid operand"),
    SQ_FN(pack_stats, 0, "pack M-step statistics into one fp64 bucket"),
    SQ_FN(ipe_estep, 0, "IPE-noised distance argmin"),
    SQ_FN(col_moments, 0, "fp64 column sums and sums of squares"),
    SQ_FN(mu_sums, 0, "mu(A) power sums for a p-grid"),
    SQ_FN(row_norms, 0, "squared row norms"),
    SQ_FN(knn_topk, 0, "per-row k smallest"),
    {"device_arch", py_device_arch, METH_NOARGS, "(arch, CUs, LDS/CU, wave size)"},
    {nullptr, nullptr, 0, nullptr}};

// splda.hip: the submodule ``_C.lda``.  Its format table is
// tests/golden/native_formats_lda.json.
static PyMethodDef lda_methods[] = {
    SQ_FN(sp_lda_stage, VALUE, "doubles of gathered rows the LDA E-step stages per wave"),
    SQ_FN(sp_lda_max_k, VALUE, "largest topic count of the LDA E-step"),
    SQ_FN(sp_lda_estep, NOGIL, "CSR LDA variational E-step + fixed-point statistics"),
    SQ_FN(sp_lda_bound, NOGIL, "CSR LDA per-document logsumexp term of the bound"),
    {nullptr, nullptr, 0, nullptr}};

// spnmf.hip: the submodule ``_C.nmf``.  Its format table is
// tests/golden/native_formats_nmf.json.
static PyMethodDef nmf_methods[] = {
    SQ_FN(sp_nmf_stage, VALUE, "doubles of gathered rows the NMF ratio kernel stages per wave"),
    SQ_FN(sp_nmf_stage_min_row, VALUE, "least doubles a staged entry counts as"),
    SQ_FN(sp_nmf_max_k, VALUE, "largest component count of the NMF ratio kernel"),
    SQ_FN(sp_nmf_wpb, VALUE, "waves per workgroup of the NMF ratio kernel at k components"),
    SQ_FN(nmf_cd_max_k, VALUE, "largest component count of the NMF sweep"),
    SQ_FN(nmf_cd_hht_k, VALUE, "component count up to which the NMF sweep keeps HHt in LDS"),
    SQ_FN(nmf_cd_rows, VALUE, "rows per wave of the NMF sweep at k components"),
    SQ_FN(sp_nmf_kl, NOGIL, "CSR NMF Kullback-Leibler ratio products and divergence term"),
    SQ_FN(nmf_cd_sweep, NOGIL, "NMF coordinate-descent sweep over rows, in place"),
    {nullptr, nullptr, 0, nullptr}};

// splogit.hip: the submodule ``_C.logistic``.  Its format table is
// tests/golden/native_formats_logistic.json.
static PyMethodDef logistic_methods[] = {
    SQ_FN(sp_logit_tile_classes, VALUE, "classes per pass of the multinomial loss kernel"),
    SQ_FN(sp_logit_multi, NOGIL, "CSR multinomial logistic loss and residual"),
    SQ_FN(sp_logit_bin, NOGIL, "CSR binary logistic loss and residual"),
    SQ_FN(sp_matvec, NOGIL, "CSR x fp64 vector product over row segments"),
    {nullptr, nullptr, 0, nullptr}};

// spgram.hip: the submodule ``_C.gram``.  Its format table is
// tests/golden/native_formats_gram.json.
static PyMethodDef gram_methods[] = {
    SQ_FN(sp_gram, 0, "CSR x CSR kernel matrix through an inverted index"),
    SQ_FN(sp_gram_matvec, 0, "CSR x CSR kernel matrix applied to vectors, never formed"),
    {nullptr, nullptr, 0, nullptr}};

// spmu.hip: the submodule ``_C.mu``.  Its format table is
// tests/golden/native_formats_mu.json.
static PyMethodDef mu_methods[] = {
    SQ_FN(sp_mu_row_waves, VALUE, "row partials of the CSR mu(A) kernel"),
    SQ_FN(sp_mu_sums, 0, "mu(A) power sums of a (centred) CSR matrix (fp64)"),
    {nullptr, nullptr, 0, nullptr}};

static struct PyModuleDef moddef ={PyModuleDef_HEAD_INIT, "_C",
                                    "sq_learn_amd native HIP kernels (gfx950)", -1, methods};
static struct PyModuleDef lda_moddef = {PyModuleDef_HEAD_INIT, "sq_learn_amd._C.lda",
                                        "latent Dirichlet allocation kernels (splda.hip)", -1,
                                        lda_methods};
static struct PyModuleDef nmf_moddef = {PyModuleDef_HEAD_INIT, "sq_learn_amd._C.nmf",
                                        "non-negative matrix factorisation kernels (spnmf.hip)",
                                        -1, nmf_methods};
static struct PyModuleDef logistic_moddef = {PyModuleDef_HEAD_INIT, "sq_learn_amd._C.logistic",
                                             "logistic-regression loss kernels (splogit.hip)", -1,
                                             logistic_methods};
static struct PyModuleDef gram_moddef = {PyModuleDef_HEAD_INIT, "sq_learn_amd._C.gram",
                                         "sparse kernel-matrix kernels (spgram.hip)", -1,
                                         gram_methods};
static struct PyModuleDef mu_moddef = {PyModuleDef_HEAD_INIT, "sq_learn_amd._C.mu",
                                       "sparse mu(A) power-sum kernels (spmu.hip)", -1,
                                       mu_methods};

static bool add_submodule(PyObject* m, const char* name, PyModuleDef* def) {
  PyObject* sub = PyModule_Create(def);
  if (!sub || PyModule_AddObject(m, name, sub) < 0) {
    Py_XDECREF(sub);
    return false;
  }
  return true;
}

PyMODINIT_FUNC PyInit__C(void) {
  PyObject* m = PyModule_Create(&moddef);
  if (!m) return nullptr;
  if (!add_submodule(m, "lda", &lda_moddef) || !add_submodule(m, "nmf", &nmf_moddef) ||
      !add_submodule(m, "logistic", &logistic_moddef) ||
      !add_submodule(m, "gram", &gram_moddef) || !add_submodule(m, "mu", &mu_moddef)) {
    Py_DECREF(m);
    return nullptr;
  }
  return m;
}
