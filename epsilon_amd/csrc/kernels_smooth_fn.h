// The smooth separable functions (reference prox/sum_exp.cc, sum_logistic.cc, sum_neg_entr.cc,
// sum_inv_pos.cc, sum_neg_log.cc) and their prox for one element, shared by the generic operators
// (kernels_segprox.hip) and the row side of the fused ZERO-term sweep (kernels_fused.hip).  Both
// files are compiled with -ffp-contract=off, so the same input gives the same bits in each.
#pragma once

#include <hip/hip_runtime.h>

namespace eps {
namespace k {
namespace {

struct FnExp {
  static constexpr bool kImplicit = false, kClosedForm = false, kNoEasy = false;
  __device__ static double f(double x) { return exp(x); }
  __device__ static double g(double x) { return exp(x); }
  __device__ static double h(double x) { return exp(x); }
  __device__ static double proj(double x) { return x; }
};
struct FnLogistic {
  static constexpr bool kImplicit = false, kClosedForm = false, kNoEasy = false;
  __device__ static double f(double x) { return x > 0 ? x + log1p(exp(-x)) : log1p(exp(x)); }
  __device__ static double g(double x) { return 1 / (1 + exp(-x)); }
  __device__ static double h(double x) {
    const double s = 1 / (1 + exp(-x));
    return s * (1 - s);
  }
  __device__ static double proj(double x) { return x; }
};
struct FnNegEntr {
  static constexpr bool kImplicit = true, kClosedForm = false, kNoEasy = false;
  __device__ static double f(double x) { return x <= 0 ? 0.0 : x * log(x); }
  __device__ static double g(double x) { return 1 + log(x); }
  __device__ static double h(double x) { return 1 / x; }
  __device__ static double proj(double x) { return fmax(x, 1e-6); }
};
struct FnInvPos {
  static constexpr bool kImplicit = false, kClosedForm = false, kNoEasy = false;
  __device__ static double f(double x) { return 1 / x; }
  __device__ static double g(double x) { return -1 / (x * x); }
  __device__ static double h(double x) { return 2 / (x * x * x); }
  __device__ static double proj(double x) { return fmax(x, 1e-6); }
};
struct FnNegLog {  // closed-form prox (sum_neg_log.cc:9-24); epigraph without the easy case
  static constexpr bool kImplicit = true, kClosedForm = true, kNoEasy = true;
  __device__ static double f(double x) { return -log(x); }
  __device__ static double g(double x) { return -1 / x; }
  __device__ static double h(double x) { return 1 / (x * x); }
  __device__ static double proj(double x) { return x; }
};

// argmin_x lam f(x) + 1/2 (x - v)^2 for one element: the damped Newton of newton.cc:49-103
// specialised to n = 1 (same step, same Armijo test on |x - v + lam f'(x)|).
template <class Fn> __device__ inline double ProxElem(double v, double lam) {
  if constexpr (Fn::kClosedForm) {
    const double z = sqrt(v * v + 4 * lam);
    return v >= 0 ? (v + z) / 2 : 2 * lam / (-v + z);
  } else {
    const double eps = 1e-14;
    double x = Fn::proj(v);
    double res = x - v + lam * Fn::g(x);
    for (int it = 0; it < 100; ++it) {
      if (fabs(res) < eps * (1 + fabs(v))) break;
      const double dx = res / (1 + lam * Fn::h(x));
      double theta = 1;
      bool moved = false;
      while (theta > 1e-12) {
        const double nx = Fn::proj(x - theta * dx);
        const double nres = nx - v + lam * Fn::g(nx);
        if (fabs(nres) <= (1 - 0.001 * theta) * fabs(res)) {
          x = nx;
          res = nres;
          moved = true;
          break;
        }
        theta *= 0.5;
      }
      if (!moved) break;
    }
    return x;
  }
}

}  // namespace
}  // namespace k
}  // namespace eps
