// Proximal-operator plugin interface and registry.
//
// Same plugin point as the reference (src/epsilon/prox/prox.h:11-77): a ProxOperator is
// created by (ProxFunction::Type, epigraph), initialised once with the function's affine
// argument H and the constraint map A, then applied every sweep:
//     Apply(v) = argmin_x f(H x + g) + 1/2 ||A x - v||^2 .
// Operators register themselves with REGISTER_PROX_OPERATOR / REGISTER_EPIGRAPH_OPERATOR.
#pragma once

#include <functional>
#include <memory>
#include <string>

#include "affine.h"
#include "block.h"
#include "kernels.h"
#include "wire.h"

namespace eps {

class ProxOperatorArg {  // reference prox/prox.h:11-35
 public:
  ProxOperatorArg(const pb::ProxFunction& f, DataMap* data, const AffineOperator& affine_arg,
                  const AffineOperator& affine_constraint)
      : f_(f), data_(data), H_(affine_arg), A_(affine_constraint) {}
  const pb::ProxFunction& prox_function() const { return f_; }
  DataMap* data_map() const { return data_; }
  const AffineOperator& affine_arg() const { return H_; }
  const AffineOperator& affine_constraint() const { return A_; }

 private:
  const pb::ProxFunction& f_;
  DataMap* data_;
  const AffineOperator& H_;
  const AffineOperator& A_;
};

// What a fused route (fused_route.cc) needs to know about an operator to replace its Apply by a
// fused kernel; an operator that cannot be described this way keeps the generic path.
struct LeastSquaresDesc {  // SumSquareProx after block elimination [constraint, variable, arg]
  std::string var_key, arg_key, constraint_key;
  std::shared_ptr<const DenseMatrixImpl> L_arg_var;  // L(arg, var): lazily scaled data matrix
  std::shared_ptr<const DenseMatrixImpl> Dinv_arg;   // cached explicit inverse (with its sign)
  DVec rhs_arg;                                      // constant part of the rhs on the arg row
  // Matrix variable (n x cols, column-major): the maps are I_cols (x) L_arg_var and
  // I_cols (x) Dinv_arg; the descriptors above are the dense factors with the scalar factor of the
  // Kronecker product folded into their scale, rhs_arg has m * cols entries (column c at c * m).
  int64_t cols = 1;
  // The tall form (more rows than columns): the order is [constraint, arg, variable], arg a scalar
  // pivot.  L_arg_var then holds L(var, arg) (transposed: its buffer is the data matrix, rows x
  // cols), Dinv_arg the dense symmetric Dinv(var), dinv_arg Dinv(arg)'s scalar, and
  // Solve(b_ + v)[var] = Dinv(var) (v_c - L(var,arg) rhs_arg).  Vector variables alone (cols == 1).
  bool tall = false;
  double dinv_arg = 0;
};
// A separable term in scalar form (scalar H and A, one weight for every element): with v the prox
// input of the term's constraint row,
//   x = Cs * (f(Bs*v + g) - g),
// f by `kind`.  Each operator answers one kind; which kinds a route takes on which side, and whether
// it takes an offset g, is the route's decision (fused_route.cc).
struct SeparableDesc {
  enum Kind {
    kZone,       // ScaledZoneProx with uniform or per-element alpha / beta: f the scaled zone's prox
    kSmooth,     // SmoothProxOp (SUM_LOGISTIC alone answers): f = prox_{lam fn}
    kRowGroups,  // Norm2Prox with axis = 1 on a rows x cols argument: f the group shrinkage of each row
    kRidge,      // SumSquareProx with a scalar argument map: f the identity, x = Cs * (Bs*v) (below)
    kLinear,     // AffineProx with one dense 1 x n argument map: f the identity, x = Cs * (Bs*v + g) (below)
    kNonNegative,  // NonNegativeProx: f = max(., 0) as k::MaxZero computes it
  };
  Kind kind = kZone;
  std::string var_key, constraint_key;
  double Bs = 0, Cs = 0;  // v' = Bs*v ; x = Cs*x'
  double lam = 0;         // (kRidge: not set, the weight is in Bs and Cs)
  double alpha = 1, beta = 1, M = 0;       // kZone
  DVec alpha_vec, beta_vec;                // kZone: per-element alpha / beta (SUM_QUANTILE with data vectors); empty: uniform
  DVec g;                                  // kZone, kSmooth, kNonNegative: constant offset of the argument (empty: none)
                                           // kLinear: the var row of the solve's constant, -alpha c (n entries)
  k::SmoothFn fn = k::SMOOTH_LOGISTIC;     // kSmooth
  int64_t rows = 0, cols = 0;              // kRowGroups
};
// kRidge: SumSquareProx with a scalar argument map, no offset and one variable, in the order the fill
// model gives this system, [arg, constraint, var], every block of the factorisation a scalar matrix.
// Nothing reaches the var row in the forward substitution but the constraint row, and the back
// substitution starts from it, so Solve(v)[var] is two scalar-map applies on the prox input,
//   t = (-1 * L(var, constraint)) v_c ;  x = (1 * Dinv(var)) t
// (block.cc Substitute, then D_inv *): each factor the product a scalar map's Apply narrows to the
// compute type, one rounding per multiply; Bs and Cs are these two factors, the scalars as the
// factorisation holds them.  In exact arithmetic x = a v / (a^2 + 2 alpha).
// kLinear: AffineProx of an AFFINE function c^T x with one dense 1 x n argument map on one variable
// and one constraint row with a scalar map a and no constant.  The KKT matrix [[0, a], [a, -I]] has no
// diagonal block on var, so the fill model (BlockCholesky: a key without a pivot has no bound) can
// only give the order [constraint, var], both blocks of the factorisation and both pivots scalar
// matrices.  The right-hand side is g_ + v with g_ = -alpha c on the var row and v on the constraint
// row, so Solve(g_ + v)[var] is
//   t = (-1 * L(var, constraint)) v_c + g_j ;  x = (1 * Dinv(var)) t
// (block.cc Substitute: the scalar map's Apply adds its product to the row that holds g, then D_inv *;
// the back substitution writes the constraint row, which no constraint map reads): one rounding per
// multiply and per add.  Bs and Cs are these two factors, the scalars as the factorisation holds them,
// g the var row of g_ in the compute type.  In exact arithmetic x = (a v - alpha c) / a^2.

// ZeroProx after block elimination: the projection onto {C x' + e z' + d = 0} of the graph-form
// problems, in one of two orders; v is the prox input.
// Fat C, [constraints and copies (scalar pivots) ..., arg] (tall = false):
//   w = Dinv (rhs_arg - e v_z - s C v_x),  x' = v_x - s C^T w,  z' = v_z - e w
// with L = L(arg, x') = s C (lazily scaled) and Dinv = Dinv(arg) = -(C C^T + e^2 I)^-1 as the
// factorisation holds it.
// Tall C (more rows than columns): the fill model eliminates [constraint, constraint, z', arg, x'],
// so arg is a scalar pivot and x' the only dense one ("Tall C"; tall = true).  With
// f_arg = rhs_arg - e v_z:
//   x' = Dinv (v_x - L f_arg),  arg = dinv_arg f_arg - L^T x',  z' = v_z - e arg
// with L = L(x', arg) = -C^T / e^2 as the factorisation holds it (transposed, lazily scaled) and
// Dinv = Dinv(x') = (I + C^T C / e^2)^-1.
// Free x (x_free, with tall; DESIGN.md 3.11 "x in the ZERO term alone"): x is no copy - it lives in
// the ZERO term alone, with no constraint row - and the order is [constraint, z', arg, x].  With
// f_arg as above:
//   x = Dinv (-L f_arg),  arg = dinv_arg f_arg - L^T x,  z' = v_z - e arg
// with L = L(x, arg) as above and Dinv = Dinv(x) = (C^T C / e^2)^-1: no "+ I", so C must have full
// column rank (the factorisation has the same order for fat C: the route asks for m > n itself).
// x_constraint_key is empty.
struct ZeroProjectionDesc {
  bool tall = false;
  bool x_free = false;
  std::string x_key, z_key, arg_key;             // z_key empty: no z block (basis pursuit)
  std::string x_constraint_key, z_constraint_key;
  std::shared_ptr<const DenseMatrixImpl> L;     // the dense map: lazily scaled data matrix (tall: trans() set)
  std::shared_ptr<const DenseMatrixImpl> Dinv;  // cached explicit inverse of the dense pivot (with its sign)
  double dinv_arg = 0;                           // tall: Dinv(arg)'s scalar
  double e = 0;                                  // L(arg, z')
  DVec rhs_arg;                                  // constant part of the rhs on the arg row
};

class ProxOperator {  // reference prox/prox.h:37-43
 public:
  virtual ~ProxOperator() {}
  virtual void Init(const ProxOperatorArg& arg) {}
  virtual BlockVector Apply(const BlockVector& v) = 0;
  virtual bool DescribeLeastSquares(LeastSquaresDesc* d) const { return false; }
  virtual bool DescribeSeparable(SeparableDesc* d) const { return false; }
  virtual bool DescribeZeroProjection(ZeroProjectionDesc* d) const { return false; }
};

std::unique_ptr<ProxOperator> CreateProxOperator(int type, bool epigraph);
bool RegisterProxOperatorFactory(int type, bool epigraph,
                                 std::function<std::unique_ptr<ProxOperator>()> factory);

template <class T> bool RegisterProxOperator(int type, bool epigraph) {
  return RegisterProxOperatorFactory(type, epigraph,
                                     [] { return std::unique_ptr<ProxOperator>(new T); });
}

#define EPS_REGISTER_VAR(prefix, type, T) prefix##_##type##_##T
#define REGISTER_PROX_OPERATOR(type, T) \
  static bool EPS_REGISTER_VAR(prox, type, T) = ::eps::RegisterProxOperator<T>(pb::ProxFunction::type, false)
#define REGISTER_EPIGRAPH_OPERATOR(type, T) \
  static bool EPS_REGISTER_VAR(epi, type, T) = ::eps::RegisterProxOperator<T>(pb::ProxFunction::type, true)

// ---- VectorProx: prox with scalar / diagonal H and A reduced to a plain vector prox ------------
// reference prox/vector_prox.{h,cc}

// Slices of argument `arg` (n entries) the reference's axis loop visits (vector_prox.cc:150-177):
// columns for axis 0, rows for axis 1, the whole argument when the function has no axis.
k::Segs SegsOf(const pb::ProxFunction& f, int arg, int64_t n);

class VectorProxInput {
 public:
  double lambda() const;                       // scalar case only
  bool elementwise() const { return elementwise_; }
  const DVec& lambda_vec() const { return lambda_dev_; }
  const DVec& value_vec(int i) const;          // whole argument i (device)
  const pb::ProxFunction& prox_function() const { return f_; }

 private:
  friend class VectorProx;
  bool elementwise_ = false;
  double lambda_ = 0;
  std::vector<double> lambda_host_;
  DVec lambda_dev_;
  BlockVector v_;
  pb::ProxFunction f_;
};

class VectorProxOutput {
 public:
  void set_value(int i, DVec x);

 private:
  friend class VectorProx;
  BlockVector x_;
};

class VectorProx : public ProxOperator {
 public:
  void Init(const ProxOperatorArg& arg) override;
  BlockVector Apply(const BlockVector& v) override;

 protected:
  // Applied to whole arguments.  When the function has an axis (per-row / per-column
  // application, reference vector_prox.cc:150-177) the operator sees the full m x n argument
  // and handles the axis itself; elementwise operators are axis-agnostic.
  virtual void ApplyVector(const VectorProxInput& input, VectorProxOutput* output) = 0;

  // For DescribeSeparable: true iff B_, C_ are single scalar blocks and lambda is a scalar; fills the
  // keys, Bs, Cs, lam and g.  `offset`: a constant on the argument row is accepted and handed out in
  // d->g (empty: there is none); without it any constant is refused.
  bool ScalarForm(SeparableDesc* d, bool offset) const;

 private:
  BlockMatrix B_, C_, D_;
  BlockVector g_;
  VectorProxInput input_;
  VectorProxOutput output_;
};

}  // namespace eps
