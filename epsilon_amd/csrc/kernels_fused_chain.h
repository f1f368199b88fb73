// Per-column arithmetic of the fused lasso sweep shared by the single pass (kernels_fused.hip)
// and the batched passes (kernels_fused_batch.hip, kernels_fused_wide.hip): these files are
// compiled with -ffp-contract=off, so the same expressions give the same bits in each.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "kernels.h"
#include "kernels_smooth_fn.h"

namespace eps {
namespace k {
namespace {

template <class T> struct Chunk;  // one 16-byte load: R rows
template <> struct Chunk<float> {
  static constexpr int R = 4;
  typedef float V __attribute__((ext_vector_type(4)));
};
template <> struct Chunk<double> {
  static constexpr int R = 2;
  typedef double V __attribute__((ext_vector_type(2)));
};

// One 16-byte load of the streamed matrix (the single pass and the batched pass).  `resident`:
// the default policy, so the line stays in the Infinity Cache for the next sweep; otherwise
// non-temporal, which passes through without displacing what is resident (DESIGN.md 3.7,
// "Residency").  `resident` must be uniform over the workgroup, and the disassembly must show
// both an `nt` and a plain global_load_dwordx4 behind scalar control flow.  Written as two loads
// of one pointer, the compiler merges them into a single plain load and the hint is lost (as it
// did once with the guarded load: kernels_fused.hip, `const V zero`).  So the resident load reads
// through a pointer to the constant address space: the matrix is read-only for the whole launch,
// a per-lane address gives the same global_load instruction, and loads of two pointer types are
// not merged.
template <class T> __device__ inline typename Chunk<T>::V LoadMatrixChunk(const T* p, bool resident) {
  typedef typename Chunk<T>::V V;
  typedef const V __attribute__((address_space(4))) * ConstV;
  if (resident) return *(ConstV)(p);
  return __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
}

// ---- the same pass in either precision (the f64 form serves the fp64 mode: the reference's own
// arithmetic type, linear/linear_map.h:35) ---------------------------------------------------------
template <class T> struct FusedScalarsT {
  T kappa;  // x0 = v0 + kappa * d
  T Bs, Cs, a1, lam, alpha, beta, M;
  T a0, inv_aa;        // two-block form: constraint a0 x0 + a1 x1 = 0, 1 / (a0^2 + a1^2)
  const T* alpha_v;    // per-column alpha / beta of the scaled zone (nullptr: the uniform values)
  const T* beta_v;
};

// The host's records (scalars as double) are narrowed to the compute type T here alone.
template <class T> T* OptT(const DVec& v) { return v.n > 0 ? v.as<T>() : nullptr; }

// The zone of a record as the chains read it, with the caller's kappa and two-block scalars.
template <class T> FusedScalarsT<T> ScalarsOf(const ZoneParams& z, double kappa, double a0, double inv_aa) {
  return {static_cast<T>(kappa), static_cast<T>(z.Bs), static_cast<T>(z.Cs), static_cast<T>(z.a1),
          static_cast<T>(z.lam), static_cast<T>(z.alpha), static_cast<T>(z.beta), static_cast<T>(z.M),
          static_cast<T>(a0), static_cast<T>(inv_aa), OptT<T>(z.alpha_vec), OptT<T>(z.beta_vec)};
}

// The seven state pointers into a device record's own fields (y_zero_prev: nullptr if empty).
template <class T>
void NarrowState(const ConsensusState& s, T** u, T** var, T** copy, T** y_term, T** y_zero, T** y_term_prev,
                 T** y_zero_prev) {
  *u = s.u.as<T>();
  *var = s.var.as<T>();
  *copy = s.copy.as<T>();
  *y_term = s.y_term.as<T>();
  *y_zero = s.y_zero.as<T>();
  *y_term_prev = s.y_term_prev.as<T>();
  *y_zero_prev = OptT<T>(s.y_zero_prev);
}

// One instance in the compute type T, as the kernels read it: the single pass takes its
// arguments from it, the batched passes upload it as it is.
template <class T> LassoBatchInst<T> Narrow(const LassoInstance& s) {
  LassoBatchInst<T> d;
  d.w = s.w.as<T>();
  d.tpart = s.tpart.as<T>();
  NarrowState<T>(s.state, &d.u, &d.x1, &d.x0, &d.y1, &d.y0, &d.y1prev, &d.e0);
  const ZoneParams& z = s.zone;
  d.alpha_v = OptT<T>(z.alpha_vec);
  d.beta_v = OptT<T>(z.beta_vec);
  d.p = s.p.as<T>();
  d.rhs = OptT<T>(s.rhs);
  d.kappa = static_cast<T>(s.kappa);
  d.pkappa = static_cast<T>(s.pkappa);
  d.Bs = static_cast<T>(z.Bs);
  d.Cs = static_cast<T>(z.Cs);
  d.a1 = static_cast<T>(z.a1);
  d.lam = static_cast<T>(z.lam);
  d.alpha = static_cast<T>(z.alpha);
  d.beta = static_cast<T>(z.beta);
  d.M = static_cast<T>(z.M);
  d.zg = OptT<T>(s.zg);
  d.zrhs = OptT<T>(s.zrhs);
  d.zd = OptT<T>(s.zd);
  d.zfarg = OptT<T>(s.zfarg);
  d.ke = static_cast<T>(s.ke);
  d.dinv = static_cast<T>(s.dinv);
  return d;
}

// The records of a batch's members in order into `table` (device; grown as needed).
template <class Inst> void UploadRecords(const std::vector<Inst>& host, DVec* table) {
  const size_t bytes = host.size() * sizeof(Inst);
  const int64_t words = static_cast<int64_t>((bytes + 7) / 8);
  if (table->n < words || table->dt != F64) *table = DVec::Empty(words < 1 ? 1 : words, F64);
  if (bytes == 0) return;
  Runtime& rt = Runtime::Get();
  EPS_HIP(hipMemcpyAsync(table->data(), host.data(), bytes, hipMemcpyHostToDevice, rt.stream()));
  rt.Sync();  // `host` goes out of scope with the caller
}

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

// One column's elementwise chain in two halves around the threshold step, so that a threshold
// that couples several instances (GroupShrinkT) can sit between them.
template <class T> struct ChainHeadT {
  T x0, u2, vin;  // x0 = y0; u after "term 1: u += y_1"; the threshold's input B v
};
// sweep start: u -= y0; u -= y1; then term 0: u += y0         (prox_admm.cc:137-142)
template <class T> __device__ inline T ChainStartT(T u, T y0p, T y1p) { return ((u - y0p) - y1p) + y0p; }
// From term 0's result x0 on (the tall lasso sweep has it from the inverse apply as it is,
// kernels_fused_tall.hip).
template <class T> __device__ inline ChainHeadT<T> ChainHeadFromT(T v0, T x0, const FusedScalarsT<T>& c, T y1p) {
  const T y0 = x0;                // y_0 = A_ x_0 with A_(c0,x) = I
  const T u1 = v0 - y0;           // u -= y_0
  const T u2 = u1 + y1p;          // term 1: u += y_1
  const T vin = c.Bs * u2;        // VectorProx: B v (+ g = 0)      (vector_prox.cc:141)
  return {x0, u2, vin};
}
template <class T>
__device__ inline ChainHeadT<T> ChainHeadOfT(T d, const FusedScalarsT<T>& c, T u, T y0p, T y1p) {
  const T v0 = ChainStartT<T>(u, y0p, y1p);
  const T x0 = c.kappa * d + v0;  // back substitution epilogue: alpha*acc + 1*y
  return ChainHeadFromT<T>(v0, x0, c, y1p);
}
// From the threshold's result xz on.  Returns v0' (input of the next sweep's forward pass).
template <class T>
__device__ inline T ChainTailT(const ChainHeadT<T>& h, T xz, const FusedScalarsT<T>& c, T* x0o, T* x1o,
                               T* y0o, T* y1o, T* uo) {
  const T y0 = h.x0;
  const T x1 = c.Cs * xz;         // C (x - g)                       (vector_prox.cc:145)
  const T y1 = c.a1 * x1;         // y_1 = A_ x_1
  const T u3 = h.u2 - y1;         // u -= y_1
  *x0o = h.x0;
  *x1o = x1;
  *y0o = y0;
  *y1o = y1;
  *uo = u3;
  // next sweep's prox-0 input
  return ((u3 - y0) - y1) + y0;
}

// One column's elementwise chain.  Returns v0' (input of the next sweep's forward pass).
template <class T>
__device__ inline T ChainOneT(T d, const FusedScalarsT<T>& c, T u, T y0p, T y1p, T* x0o, T* x1o,
                              T* y0o, T* y1o, T* uo) {
  const ChainHeadT<T> h = ChainHeadOfT<T>(d, c, u, y0p, y1p);
  const T xz = ScaledZoneOneT<T>(h.vin, c.lam, c.alpha, c.beta, c.M);
  return ChainTailT<T>(h, xz, c, x0o, x1o, y0o, y1o, uo);
}

// ---- ZERO-term problems: per constraint row the sweep is
//   u -= y_s; u -= y_q;  separable term: u += y_s, s = Cs (zone(Bs u + g) - g), y_s = a1 s, u -= y_s;
//   ZERO term: u += y_q, v = u, q = v + (factor) * (product with w), y_q = q, u -= y_q
// (prox_admm.cc:135-147 with the separable term before the ZERO term).  The head runs up to v and
// needs the boundary state alone; the tail needs this sweep's w.
// Fn (kernels_smooth_fn.h): a smooth separable term in place of the zone, its prox the fp64 Newton
// of SmoothProxKernel on the rounded input with the operator's own weight `lam64`.
// RidgeStep in the Fn slot (kHeadRidge, the x side alone): the term is a scalar least-squares prox
// (ScalarLeastSquaresDesc) and its variable the block solve's two scalar-map
// applies on the prox input, s = Cs (Bs ub): no offset, no zone, one rounding per multiply.
// LinearStep in the Fn slot (kHeadLinear, the x side alone): the term is linear (SeparableDesc::kLinear)
// and its variable the block solve's forward step on the row that holds the
// constant and the pivot, s = Cs (Bs ub + g): `g` is the per-element constant -alpha c_j, passed where
// the offset goes.  NonNegStep (kHeadNonNeg, the z side alone): the non-negative cone in the zone's
// place, max(vin, 0) as MaxZeroKernel computes it (kernels_prox.hip), with the zone's offset handling.
struct RidgeStep {};
struct LinearStep {};
struct NonNegStep {};
// A head as the type in the Fn slot: `void` the zone, FnLogistic the smooth term (the one smooth
// function the fused kernels take).  WithHead calls f(HeadTag<Fn>()) for the head's type, so that a
// launcher names its instantiation once, behind `if constexpr` on the tables of kernels.h.
template <class Fn> struct HeadTag { typedef Fn type; };
template <class Fn> constexpr Head HeadOf() {
  return std::is_same<Fn, RidgeStep>::value    ? kHeadRidge
         : std::is_same<Fn, LinearStep>::value ? kHeadLinear
         : std::is_same<Fn, NonNegStep>::value ? kHeadNonNeg
         : std::is_void<Fn>::value             ? kHeadZone
                                               : kHeadSmooth;
}
template <class F> void WithHead(Head h, F f) {
  switch (h) {
    case kHeadZone: return f(HeadTag<void>());
    case kHeadRidge: return f(HeadTag<RidgeStep>());
    case kHeadLinear: return f(HeadTag<LinearStep>());
    case kHeadNonNeg: return f(HeadTag<NonNegStep>());
    case kHeadSmooth: return f(HeadTag<FnLogistic>());
  }
}
// The same for a chain: f(std::integral_constant<Chain, c>()).
template <class F> void WithChain(Chain c, F f) {
  switch (c) {
    case kChainLasso: return f(std::integral_constant<Chain, kChainLasso>());
    case kChainTwoBlock: return f(std::integral_constant<Chain, kChainTwoBlock>());
    case kChainZeroCols: return f(std::integral_constant<Chain, kChainZeroCols>());
    case kChainZeroTall: return f(std::integral_constant<Chain, kChainZeroTall>());
    case kChainZeroTallDot: return f(std::integral_constant<Chain, kChainZeroTallDot>());
    case kChainZeroTallAcc: return f(std::integral_constant<Chain, kChainZeroTallAcc>());
  }
}
template <class T> struct ZeroHeadT {
  T s, ys, v;  // the separable term's variable and y; the ZERO prox's input on this row
};
template <class T, class Fn = void>
__device__ inline ZeroHeadT<T> ZeroHeadOfT(const FusedScalarsT<T>& c, T g, T u, T ysp, T yqp, double lam64 = 0) {
  const T ub = ((u - ysp) - yqp) + ysp;  // sweep start, then the separable term's u += y_s
  T s;
  if constexpr (std::is_same<Fn, RidgeStep>::value) {
    const T t = c.Bs * ub;               // forward substitution: -L(var, constraint) v   (block.cc Substitute)
    s = c.Cs * t;                        // the pivot: Dinv(var) t
  } else if constexpr (std::is_same<Fn, LinearStep>::value) {
    const T t = c.Bs * ub + g;           // forward substitution onto the row of g_: -L(var, constraint) v + g_j
    s = c.Cs * t;                        // the pivot: Dinv(var) t
  } else {
    const T vin = c.Bs * ub + g;         // VectorProx: B v + g            (vector_prox.cc:141)
    T xz;
    if constexpr (std::is_void<Fn>::value) xz = ScaledZoneOneT<T>(vin, c.lam, c.alpha, c.beta, c.M);
    else if constexpr (std::is_same<Fn, NonNegStep>::value) xz = vin > T(0) ? vin : T(0);  // non_negative.cc:8
    else xz = static_cast<T>(ProxElem<Fn>(static_cast<double>(vin), lam64));
    s = c.Cs * (xz - g);                 // C (x - g)                      (vector_prox.cc:145)
  }
  const T ys = c.a1 * s;                 // y_s = A_ s
  const T uc = ub - ys;                  // u -= y_s
  return {s, ys, uc + yqp};              // ZERO term: u += y_q
}
// Finishes the sweep from the product `d` with this sweep's w (q = kappa d + v), writes the
// boundary state and returns the NEXT sweep's v, computed in registers from that state.
template <class T, class Fn = void>
__device__ inline T ZeroChainT(T d, const FusedScalarsT<T>& c, T g, T u, T ysp, T yqp, T* so, T* qo, T* yso,
                               T* yqo, T* uo) {
  const ZeroHeadT<T> h = ZeroHeadOfT<T, Fn>(c, g, u, ysp, yqp);
  const T q = c.kappa * d + h.v;  // back substitution epilogue: alpha*acc + 1*y
  const T un = h.v - q;           // y_q = q (its constraint map is I); u -= y_q
  *so = h.s;
  *qo = q;
  *yso = h.ys;
  *yqo = q;
  *uo = un;
  return ZeroHeadOfT<T, Fn>(c, g, un, h.ys, q).v;
}

// ---- tall ZERO-term problems ("Tall C"): the block LDL^T eliminates
// [constraints, z', arg, x'], so the arg row is a scalar pivot between the two copies and the
// sample side of a sweep is, per sample i with d = C[i,:] . x' of this sweep,
//   f_arg = rhs - e v        forward substitution          (block.cc Substitute: alpha*(e v) + rhs)
//   g_arg = Dinv_arg f_arg   the scalar pivot              (D_inv_ * b)
//   arg   = kappa d + g_arg  back substitution through L(x', arg)^T  (GEMV epilogue alpha*acc + y)
//   q     = v - e arg        back substitution through L(arg, z')
// with v the ZERO prox's input on the sample's row (ZeroHeadOfT), then y_q = q, u = v - q.
// The scalars beside the zone's: c.kappa scales d (-scale of L(x', arg)), `ke` = -e, `dinv` =
// Dinv(arg)'s scalar.
template <class T> struct ZeroTallScalarsT {
  const T* g;    // the z term's offset (nullptr: none)
  const T* rhs;  // the constant on the arg row (nullptr: none)
  T ke, dinv;
};
// The next sweep's f_arg from the ZERO prox's input v: the weight of the forward product.
template <class T> __device__ inline T ZeroTallForwardT(T v, T rhs, T ke) { return ke * v + rhs; }
// Finishes the sample's sweep from the product `d`, writes the boundary state and returns the
// NEXT sweep's f_arg, computed in registers from that state.
template <class T, class Fn = void>
__device__ inline T ZeroTallChainT(T d, const FusedScalarsT<T>& c, T ke, T dinv, T g, T rhs, T u, T ysp, T yqp,
                                   T* so, T* qo, T* yso, T* yqo, T* uo) {
  const ZeroHeadT<T> h = ZeroHeadOfT<T, Fn>(c, g, u, ysp, yqp);
  const T farg = ZeroTallForwardT<T>(h.v, rhs, ke);
  const T garg = dinv * farg;
  const T arg = c.kappa * d + garg;
  const T q = ke * arg + h.v;
  const T un = h.v - q;  // y_q = q (its constraint map is I); u -= y_q
  *so = h.s;
  *qo = q;
  *yso = h.ys;
  *yqo = q;
  *uo = un;
  return ZeroTallForwardT<T>(ZeroHeadOfT<T, Fn>(c, g, un, h.ys, q).v, rhs, ke);
}
// The x side of the same sweep: x'_j comes from the apply of Dinv(x') as it is (q = x'_j, no
// product on top), y_q = q, u = v - q; returns the NEXT sweep's v_x.
template <class T, class Fn = void>
__device__ inline T ZeroTallColsChainT(T q, const FusedScalarsT<T>& c, T g, T u, T ysp, T yqp, T* so, T* yso,
                                       T* uo) {
  const ZeroHeadT<T> h = ZeroHeadOfT<T, Fn>(c, g, u, ysp, yqp);
  const T un = h.v - q;
  *so = h.s;
  *yso = h.ys;
  *uo = un;
  return ZeroHeadOfT<T, Fn>(c, g, un, h.ys, q).v;
}

// The group threshold of one row of a matrix variable (NORM_2 with axis = 1): SegNorm2Kernel's
// expressions (kernels_segprox.hip) on the sum of squares `ss` of the row's threshold inputs,
// accumulated in fp64 in member order.  Returns the factor of xz_i = T(scale * double(vin_i)).
__device__ inline double GroupScale(double ss, double lam) {
  const double nv = sqrt(ss);
  return (nv >= lam && nv > 0) ? 1.0 - lam / nv : 0.0;
}

// One column of the TWO-BLOCK driver's sweep (reference algorithms/prox_admm_two_block.cc:97-112):
//   zu = z - u ;  x0 = prox_0(zu)_0 = v0 + kappa d ;  x1 = prox_1(zu)_1 (scaled zone) ;
//   z = projection of x + u onto {a0 z0 + a1 z1 = 0} ;  u += x - z.
// Returns the next sweep's prox-0 input z0' - u0'.
template <class T>
__device__ inline T ChainTwoBlockT(T d, const FusedScalarsT<T>& c, T z0p, T z1p, T u0p, T u1p, T* x0o,
                                   T* x1o, T* z0o, T* z1o, T* u0o, T* u1o) {
  const T v0 = z0p - u0p;
  const T v1 = z1p - u1p;
  const T x0 = c.kappa * d + v0;
  const T x1 = c.Cs * ScaledZoneOneT<T>(c.Bs * v1, c.lam, c.alpha, c.beta, c.M);
  const T w0 = x0 + u0p;
  const T w1 = x1 + u1p;
  const T t = (c.a0 * w0 + c.a1 * w1) * c.inv_aa;
  const T z0 = w0 - c.a0 * t;
  const T z1 = w1 - c.a1 * t;
  const T u0 = u0p + (x0 - z0);
  const T u1 = u1p + (x1 - z1);
  *x0o = x0;
  *x1o = x1;
  *z0o = z0;
  *z1o = z1;
  *u0o = u0;
  *u1o = u1;
  return z0 - u0;
}

}  // namespace
}  // namespace k
}  // namespace eps
