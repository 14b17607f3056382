// The kernel functions of the sparse kernel-matrix kernels (spgram.hip) on one
// inner product: the operation order of the reference's metrics/pairwise.py
// (multiply by gamma, add coef0, then the function), which the torch twin
// (ops/sparse_kernel.py) repeats.  The multiply and the add are written as
// separately rounded operations, so the compiler cannot contract them into
// one fused multiply-add that the twin does not have.
#pragma once
#include "common.h"

namespace sq {

constexpr int SPGRAM_KINDS = 4;      // 0 linear, 1 poly, 2 rbf, 3 sigmoid
constexpr int SPGRAM_RMAX = 4;       // right-hand sides of one apply

// rbf on a squared distance
SQ_DEV double kernel_rbf(double gamma, double D) { return exp(__dmul_rn(-gamma, D)); }

// dot: the inner product; qn, xn: the squared norms of the two rows
SQ_DEV double kernel_value(int kind, double dot, double qn, double xn, double gamma, double coef0,
                           double degree) {
  if (kind == 0) return dot;
  if (kind == 2) {
    const double D = __dadd_rn(__dadd_rn(qn, xn), -__dmul_rn(2.0, dot));
    return kernel_rbf(gamma, D > 0.0 ? D : 0.0);
  }
  const double arg = __dadd_rn(__dmul_rn(gamma, dot), coef0);
  return kind == 1 ? pow(arg, degree) : tanh(arg);
}

}  // namespace sq
