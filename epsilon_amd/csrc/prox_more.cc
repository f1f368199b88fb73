// Remaining proximal / epigraph operators of the reference's library:
// sort-based vector functions, the smooth Newton family, log-sum-exp, KL divergence and the
// second-order cone (the orthogonally invariant matrix functions are in prox_matrix.cc).  Each
// class keeps the reference's plugin interface (prox/prox.h:37-77) and cites the file it
// restates; the numeric work is in kernels_segprox.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "comm.h"
#include "kernels.h"
#include "options.h"
#include "prox.h"

namespace eps {
namespace {

DVec NewLike(const DVec& v) { return DVec::Empty(v.n, v.dt); }

// ---- functions of the segments of one argument ---------------------------------------------------
// The prox x = prox(v) and the epigraph projection (x, t) of (v, s) have one body each; K names
// the segment kernels that do the work (K::Prox, K::Epigraph) and gets the call in one record.
struct SegCall {
  const DVec &x, &t, &v, &s;  // t, s: epigraph only
  double lam;                 // prox only
  const pb::ProxFunction& f;
  k::Segs S;
};

template <class K> class SegProxOp final : public VectorProx {
 protected:
  void ApplyVector(const VectorProxInput& input, VectorProxOutput* output) override {
    const DVec& v = input.value_vec(0);
    DVec x = NewLike(v), none;
    K::Prox({x, none, v, none, input.lambda(), input.prox_function(), SegsOf(input.prox_function(), 0, v.n)});
    output->set_value(0, x);
  }
};

template <class K> class SegEpigraphOp final : public VectorProx {
 protected:
  void ApplyVector(const VectorProxInput& input, VectorProxOutput* output) override {
    const DVec& v = input.value_vec(0);
    const DVec& s = input.value_vec(1);
    DVec x = NewLike(v), t = NewLike(s);
    K::Epigraph({x, t, v, s, 0.0, input.prox_function(), SegsOf(input.prox_function(), 0, v.n)});
    output->set_value(0, x);
    output->set_value(1, t);
  }
};

struct MaxK {  // reference prox/max.cc
  static void Prox(const SegCall& c) { k::SegMaxProx(c.x, c.v, c.lam, c.S); }
  static void Epigraph(const SegCall& c) { k::SegMaxEpigraph(c.x, c.t, c.v, c.s, c.S); }
};
struct SumLargestK {  // reference prox/sum_largest.cc; epigraph: BisectionEpigraph newton.cc:239-288
  static void Prox(const SegCall& c) { k::SegSumLargestProx(c.x, c.v, c.lam, c.f.sum_largest_k, c.S); }
  static void Epigraph(const SegCall& c) { k::SegSumLargestEpigraph(c.x, c.t, c.v, c.s, c.f.sum_largest_k, c.S); }
};
struct LogSumExpK {  // reference prox/log_sum_exp.cc
  static void Prox(const SegCall& c) { k::SegLogSumExpProx(c.x, c.v, c.lam, c.S); }
  static void Epigraph(const SegCall& c) { k::SegLogSumExpEpigraph(c.x, c.t, c.v, c.s, c.S); }
};
template <k::SmoothFn FN> struct SmoothK {  // the prox is elementwise: SmoothProxOp below
  static void Epigraph(const SegCall& c) { k::SegSmoothEpigraph(FN, c.x, c.t, c.v, c.s, c.S); }
};

using MaxProx = SegProxOp<MaxK>;
using MaxEpigraph = SegEpigraphOp<MaxK>;
using SumLargestProx = SegProxOp<SumLargestK>;
using SumLargestEpigraph = SegEpigraphOp<SumLargestK>;
using LogSumExpProx = SegProxOp<LogSumExpK>;
using LogSumExpEpigraph = SegEpigraphOp<LogSumExpK>;
REGISTER_PROX_OPERATOR(MAX, MaxProx);
REGISTER_EPIGRAPH_OPERATOR(MAX, MaxEpigraph);
REGISTER_PROX_OPERATOR(SUM_LARGEST, SumLargestProx);
REGISTER_EPIGRAPH_OPERATOR(SUM_LARGEST, SumLargestEpigraph);
REGISTER_PROX_OPERATOR(LOG_SUM_EXP, LogSumExpProx);
REGISTER_EPIGRAPH_OPERATOR(LOG_SUM_EXP, LogSumExpEpigraph);

// ---- smooth separable family (reference prox/newton.cc + sum_exp.cc, sum_logistic.cc,
//      sum_neg_entr.cc, sum_inv_pos.cc, sum_neg_log.cc) --------------------------------------------------

template <k::SmoothFn FN> class SmoothProxOp final : public VectorProx {
 public:
  // SUM_LOGISTIC alone: the domain projections of the others and the closed form of SUM_NEG_LOG
  // have no fused row chain.
  bool DescribeSeparable(SeparableDesc* d) const override {
    if (FN != k::SMOOTH_LOGISTIC) return false;
    d->kind = SeparableDesc::kSmooth;
    d->fn = FN;
    return ScalarForm(d, /*offset=*/true);
  }

 protected:
  void ApplyVector(const VectorProxInput& input, VectorProxOutput* output) override {
    const DVec& v = input.value_vec(0);
    DVec x = NewLike(v);
    if (input.elementwise()) {
      EPS_CHECK_MSG(input.lambda_vec().n == v.n, "elementwise lambda does not match the argument");
      k::SmoothProx(FN, x, v, 0.0, &input.lambda_vec());
    } else {
      k::SmoothProx(FN, x, v, input.lambda(), nullptr);
    }
    output->set_value(0, x);
  }
};

template <k::SmoothFn FN> using SmoothEpigraphOp = SegEpigraphOp<SmoothK<FN>>;

using SumExpProx = SmoothProxOp<k::SMOOTH_EXP>;
using SumExpEpigraph = SmoothEpigraphOp<k::SMOOTH_EXP>;
using SumLogisticProx = SmoothProxOp<k::SMOOTH_LOGISTIC>;
using SumLogisticEpigraph = SmoothEpigraphOp<k::SMOOTH_LOGISTIC>;
using SumNegEntrProx = SmoothProxOp<k::SMOOTH_NEG_ENTR>;
using SumNegEntrEpigraph = SmoothEpigraphOp<k::SMOOTH_NEG_ENTR>;
using SumInvPosProx = SmoothProxOp<k::SMOOTH_INV_POS>;
using SumInvPosEpigraph = SmoothEpigraphOp<k::SMOOTH_INV_POS>;
using SumNegLogProx = SmoothProxOp<k::SMOOTH_NEG_LOG>;
using SumNegLogEpigraph = SmoothEpigraphOp<k::SMOOTH_NEG_LOG>;
REGISTER_PROX_OPERATOR(SUM_EXP, SumExpProx);
REGISTER_EPIGRAPH_OPERATOR(SUM_EXP, SumExpEpigraph);
REGISTER_PROX_OPERATOR(SUM_LOGISTIC, SumLogisticProx);
REGISTER_EPIGRAPH_OPERATOR(SUM_LOGISTIC, SumLogisticEpigraph);
REGISTER_PROX_OPERATOR(SUM_NEG_ENTR, SumNegEntrProx);
REGISTER_EPIGRAPH_OPERATOR(SUM_NEG_ENTR, SumNegEntrEpigraph);
REGISTER_PROX_OPERATOR(SUM_INV_POS, SumInvPosProx);
REGISTER_EPIGRAPH_OPERATOR(SUM_INV_POS, SumInvPosEpigraph);
REGISTER_PROX_OPERATOR(SUM_NEG_LOG, SumNegLogProx);
REGISTER_EPIGRAPH_OPERATOR(SUM_NEG_LOG, SumNegLogEpigraph);

// ---- SUM_KL_DIV (reference prox/sum_kl_div.cc) ----------------------------------------------------------

class SumKLDivProx final : public VectorProx {
 protected:
  void ApplyVector(const VectorProxInput& input, VectorProxOutput* output) override {
    const DVec& u = input.value_vec(0);
    const DVec& v = input.value_vec(1);
    DVec x = NewLike(u), y = NewLike(v);
    if (input.elementwise()) {
      // lambda_vec() covers both arguments (vector_prox.cc:108-116); the kernel wants the first
      EPS_CHECK_MSG(input.lambda_vec().n >= u.n, "elementwise lambda shorter than the argument");
      DVec lv = input.lambda_vec().Slice(0, u.n);
      k::KlDivProx(x, y, u, v, 0.0, &lv);
    } else {
      k::KlDivProx(x, y, u, v, input.lambda(), nullptr);
    }
    output->set_value(0, x);
    output->set_value(1, y);
  }
};
REGISTER_PROX_OPERATOR(SUM_KL_DIV, SumKLDivProx);

class SumKLDivEpigraph final : public VectorProx {
 protected:
  void ApplyVector(const VectorProxInput& input, VectorProxOutput* output) override {
    const DVec& u = input.value_vec(0);
    const DVec& v = input.value_vec(1);
    const DVec& s = input.value_vec(2);
    DVec x = NewLike(u), y = NewLike(v), t = NewLike(s);
    k::SegKlDivEpigraph(x, y, t, u, v, s, SegsOf(input.prox_function(), 0, u.n));
    output->set_value(0, x);
    output->set_value(1, y);
    output->set_value(2, t);
  }
};
REGISTER_EPIGRAPH_OPERATOR(SUM_KL_DIV, SumKLDivEpigraph);

// ---- EXP epigraph, elementwise (reference prox/exp.cc) -----------------------------------------------
// Not a SegEpigraphOp: no segments, and SegsOf must not be asked for any.

class ExpEpigraph final : public VectorProx {
 protected:
  void ApplyVector(const VectorProxInput& input, VectorProxOutput* output) override {
    const DVec& v = input.value_vec(0);
    const DVec& s = input.value_vec(1);
    DVec x = NewLike(v), t = NewLike(s);
    k::ExpEpigraph(x, t, v, s);
    output->set_value(0, x);
    output->set_value(1, t);
  }
};
REGISTER_EPIGRAPH_OPERATOR(EXP, ExpEpigraph);

// ---- SECOND_ORDER_CONE (reference prox/second_order_cone.cc:21-124) ------------------------------------
// ||ax*X_i + bx||_2 <= at*t_i + bt_i for the rows X_i of the m x n argument; "t" is argument 0.

class SecondOrderConeProx final : public ProxOperator {
 public:
  void Init(const ProxOperatorArg& arg) override {
    const pb::ProxFunction& f = arg.prox_function();
    EPS_CHECK_MSG(f.arg_size.size() == 2 && f.arg_size[1].dim.size() == 2,
                  "SECOND_ORDER_CONE needs two sized arguments");
    m_ = f.arg_size[1].dim[0];
    n_ = f.arg_size[1].dim[1];
    const DType dt = arg.data_map()->dtype();
    // InitArgs (:90-107)
    const BlockMatrix& H = arg.affine_arg().A;
    for (const auto& col : H.data()) {  // GetArgKeys (:6-19)
      for (const auto& row : col.second) {
        if (row.first == affine::arg_key(0)) t_key_ = col.first;
        else if (row.first == affine::arg_key(1)) x_key_ = col.first;
        else EPS_FATAL("Unknown row key " << row.first);
      }
    }
    EPS_CHECK_MSG(!t_key_.empty() && !x_key_.empty(), "SECOND_ORDER_CONE: missing argument");
    const double at = GetScalar(H(affine::arg_key(0), t_key_));
    const double ax = GetScalar(H(affine::arg_key(1), x_key_));
    const BlockVector& g = arg.affine_arg().b;
    a_ = at / std::fabs(ax);
    // bx_ = g(arg 1) / ax ; bt_/a_ = g(arg 0) / |ax| / a_   (zeros when absent, block_vector.cc:62-67)
    bx_ = DVec::Zeros(m_ * n_, dt);
    if (g.has_key(affine::arg_key(1))) k::Axpby(bx_, 1 / ax, g(affine::arg_key(1)), 0.0);
    bt_over_a_ = DVec::Zeros(m_, dt);
    if (g.has_key(affine::arg_key(0)))
      k::Axpby(bt_over_a_, 1 / std::fabs(ax) / a_, g(affine::arg_key(0)), 0.0);
    // InitConstraints (:109-122): A'A must be one scalar
    const BlockMatrix& A = arg.affine_constraint().A;
    AT_ = A.Transpose();
    BlockMatrix ATA = AT_ * A;
    const double alphat = GetScalar(ATA(t_key_, t_key_));
    const double alphax = GetScalar(ATA(x_key_, x_key_));
    EPS_CHECK_MSG(alphat == alphax, "A'A not scalar matrix");
    BlockMatrix D;
    D(x_key_, x_key_) = LinearMap::Scalar(1 / alphat, m_ * n_);
    D(t_key_, t_key_) = LinearMap::Scalar(1 / alphat, m_);
    AT_ = D * AT_;
  }

  BlockVector Apply(const BlockVector& v) override {  // :46-56
    BlockVector u = AT_ * v;
    DVec X = u(x_key_).Clone();
    k::Axpby(X, 1.0, bx_, 1.0);
    DVec t = u(t_key_).Clone();
    k::Axpby(t, 1.0, bt_over_a_, 1.0);
    EPS_CHECK(X.n == m_ * n_ && t.n == m_);
    k::Segs S;  // rows of the column-major m x n matrix
    S.count = m_;
    S.len = n_;
    S.seg_stride = 1;
    S.elem_stride = m_;
    DVec Xo = NewLike(X), to = NewLike(t);
    k::SegSocProject(Xo, to, X, t, a_, S);
    k::Axpby(Xo, -1.0, bx_, 1.0);
    k::Axpby(to, -1.0, bt_over_a_, 1.0);
    BlockVector x;
    x.Set(x_key_, Xo);
    x.Set(t_key_, to);
    return x;
  }

 private:
  BlockMatrix AT_;
  double a_ = 1;
  DVec bx_, bt_over_a_;
  std::string t_key_, x_key_;
  int64_t m_ = 0, n_ = 0;
};
REGISTER_PROX_OPERATOR(SECOND_ORDER_CONE, SecondOrderConeProx);

}  // namespace
}  // namespace eps
