// Per-column arithmetic of the fused lasso sweep shared by the single pass (kernels_fused.hip)
// and the batched pass (kernels_fused_batch.hip): both files are compiled with -ffp-contract=off,
// so the same expressions give the same bits in either.
#pragma once

#include <hip/hip_runtime.h>

namespace eps {
namespace k {
namespace {

// ---- the same pass in either precision (the f64 form serves the fp64 mode: the reference's own
// arithmetic type, linear/linear_map.h:35) ---------------------------------------------------------
template <class T> struct FusedScalarsT {
  T kappa, Bs, Cs, a1, lam, alpha, beta, M;
  T a0, inv_aa;        // two-block form: constraint a0 x0 + a1 x1 = 0, 1 / (a0^2 + a1^2)
  const T* alpha_v;    // per-column alpha / beta of the scaled zone (nullptr: the uniform values)
  const T* beta_v;
};

template <class T> __device__ inline T WaveSumT(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <class T> __device__ inline T ScaledZoneOneT(T xi, T lam, T alpha, T beta, T M) {
  // reference prox/scaled_zone.cc:90-101 with C = 0
  if (fabs(xi) <= M) return xi;
  if (xi > M + lam * alpha) return xi - lam * alpha;
  if (xi < -M - lam * beta) return xi + lam * beta;
  if (xi > T(0)) return M;
  return -M;
}

// One column's elementwise chain (see ChainOne in kernels_fused.hip for the line-by-line
// correspondence).
template <class T>
__device__ inline T ChainOneT(T d, const FusedScalarsT<T>& c, T u, T y0p, T y1p, T* x0o, T* x1o,
                              T* y0o, T* y1o, T* uo) {
  const T v0 = ((u - y0p) - y1p) + y0p;
  const T x0 = c.kappa * d + v0;
  const T y0 = x0;
  const T u1 = v0 - y0;
  const T u2 = u1 + y1p;
  const T vin = c.Bs * u2;
  const T xz = ScaledZoneOneT<T>(vin, c.lam, c.alpha, c.beta, c.M);
  const T x1 = c.Cs * xz;
  const T y1 = c.a1 * x1;
  const T u3 = u2 - y1;
  *x0o = x0;
  *x1o = x1;
  *y0o = y0;
  *y1o = y1;
  *uo = u3;
  return ((u3 - y0) - y1) + y0;
}

}  // namespace
}  // namespace k
}  // namespace eps
