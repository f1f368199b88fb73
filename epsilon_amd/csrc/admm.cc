#include "admm.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "comm.h"
#include "fused_route.h"
#include "options.h"

namespace eps {

double Now() {
  using clock = std::chrono::steady_clock;
  return std::chrono::duration<double>(clock::now().time_since_epoch()).count();
}

namespace {

// Sharded solves: the "arg:<k>" rows of a prox operator's H are private to that operator.  An
// arg row fed from a sharded variable through an elementwise map is itself sharded; through a
// dense / Kronecker map it is a contraction into a replicated row (comm.h).
std::set<std::string> InferShardedArgs(const BlockMatrix& H) {
  std::set<std::string> out;
  const ShardSpec& sh = ShardSpec::Get();
  if (!sh.active()) return out;
  if (sh.consensus_terms() && !H.data().empty()) {
    // consensus form: a term over sharded variables only is this rank's own term, and so are
    // its argument rows, whatever the type of the maps into them
    bool all_sharded = true;
    for (const auto& col : H.data()) all_sharded = all_sharded && sh.IsSharded(col.first);
    if (all_sharded) return H.row_keys();
  }
  std::map<std::string, int> vote;  // 1 sharded, 2 replicated
  for (const auto& col : H.data()) {
    if (!sh.IsSharded(col.first)) continue;
    for (const auto& row : col.second) {
      const ImplType t = row.second.impl().type();
      const int v = (t == SCALAR_MATRIX || t == DIAGONAL_MATRIX) ? 1 : 2;
      int& cur = vote[row.first];
      EPS_CHECK_MSG(cur == 0 || cur == v, "row " << row.first
                                                  << " mixes elementwise and dense maps of sharded variables");
      cur = v;
    }
  }
  for (const auto& kv : vote)
    if (kv.second == 1) out.insert(kv.first);
  return out;
}

// Global row / column counts of a block matrix whose sharded keys hold per-rank slices.
void GlobalDims(const BlockMatrix& A, int64_t* m, int64_t* n) {
  const ShardSpec& sh = ShardSpec::Get();
  if (!sh.active()) {
    *m = A.m();
    *n = A.n();
    return;
  }
  double loc[2] = {0, 0}, rep[2] = {0, 0};
  std::set<std::string> seen;
  for (const auto& col : A.data()) {
    const int64_t cn = col.second.begin()->second.impl().n();
    (sh.IsSharded(col.first) ? loc : rep)[1] += cn;
    for (const auto& row : col.second)
      if (seen.insert(row.first).second)
        (sh.IsSharded(row.first) ? loc : rep)[0] += row.second.impl().m();
  }
  DVec d = DVec::FromHost(loc, 2, F64);
  Runtime::Get().comm()->AllReduceSum(d);
  std::vector<double> g = d.ToHost();
  *m = static_cast<int64_t>(g[0] + rep[0] + 0.5);
  *n = static_cast<int64_t>(g[1] + rep[1] + 0.5);
}

}  // namespace

Solver::Solver(pb::Problem problem, std::shared_ptr<DataMap> data, pb::SolverParams params)
    : problem_(std::move(problem)), data_(std::move(data)), params_(params) {}
Solver::~Solver() {}

FusedRoute* Solver::batch_route() const { return initialized_ && !finished_ && iter_ == 0 ? route_.get() : nullptr; }
// (a route without a check of its own - the ZERO-term route unless "fused_zero_check" is "1" -
// launches nothing ahead: its member runs the driver's generic check, waited for, when it is asked
// for the outcome)
void Solver::BatchLaunchCheck(int iter) {
  iter_ = iter;
  if (route_->HasCheck()) route_->LaunchNorms();
}
bool Solver::BatchFinishCheck() {
  if (route_->HasCheck()) FinishRouteCheck();
  else ComputeResiduals();
  finished_ = status_.state == pb::SolverStatus::OPTIMAL;
  return finished_;
}
void Solver::BatchFinishMaxIterations(int iter) {  // what Run() does when the sweeps run out
  iter_ = iter;
  ComputeResiduals();
  status_.state = pb::SolverStatus::MAX_ITERATIONS_REACHED;
  finished_ = true;
}
void Solver::BatchAddLoopTime(double seconds) {
  loop_seconds_ += seconds;
  status_.init_time = init_seconds_;
  status_.total_time = init_seconds_ + loop_seconds_;
}

void Solver::LogStatus() {  // reference prox_admm.cc:219-230
  if (!params_.verbose || !log_) return;
  char buf[256];
  std::snprintf(buf, sizeof(buf), "iter=%d residuals primal=%.2e [%.2e] dual=%.2e [%.2e]",
                status_.num_iterations, status_.r_norm, status_.epsilon_primal, status_.s_norm,
                status_.epsilon_dual);
  log_(buf);
}

void Solver::FinishResiduals(double r, double s, double eps_pri, double eps_dual) {
  status_.r_norm = r;
  status_.s_norm = s;
  status_.epsilon_primal = eps_pri;
  status_.epsilon_dual = eps_dual;
  if (r <= eps_pri && s <= eps_dual && !params_.ignore_stopping_criteria)
    status_.state = pb::SolverStatus::OPTIMAL;
  else
    status_.state = pb::SolverStatus::RUNNING;
  status_.num_iterations = iter_;
}

int Solver::Run(int max_sweeps) {
  EPS_CHECK_MSG(initialized_, "Solver::Run before Init");
  SetCurrentDType(data_->dtype());
  const double t0 = Now();
  int done = 0;
  const int epoch = params_.epoch_iterations > 0 ? params_.epoch_iterations : 1;
  const int log_every = params_.log_iterations > 0 ? params_.log_iterations : 1;
  // the sweeps from iteration `it` up to and including the next one that is followed by a host
  // decision (residual check; log line when verbose), clipped to the limits; 0 = none left
  auto batch_size = [&](int it, int done_so_far) {
    if (it >= params_.max_iterations || (max_sweeps >= 0 && done_so_far >= max_sweeps)) return 0;
    int batch = 1;
    while ((it + batch - 1) % epoch != 0 && !(params_.verbose && (it + batch - 1) % log_every == 0))
      ++batch;
    if (batch > params_.max_iterations - it) batch = params_.max_iterations - it;
    if (max_sweeps >= 0 && batch > max_sweeps - done_so_far) batch = max_sweeps - done_so_far;
    return batch;
  };
  int speculated = 0;  // sweeps of the NEXT batch already enqueued behind a pending check
  // A speculative batch is wasted work when its check says OPTIMAL, so none is started once the
  // last check was within a factor 4 of both tolerances (the residuals fall geometrically, the
  // next check is then likely the last): the steady state gets the overlap, the time to OPTIMAL
  // does not pay for it.
  auto far_from_optimal = [&] {
    if (status_.epsilon_primal <= 0 || status_.epsilon_dual <= 0) return true;  // no check yet
    return status_.r_norm > 4 * status_.epsilon_primal || status_.s_norm > 4 * status_.epsilon_dual;
  };
  while (!finished_ && iter_ < params_.max_iterations && (max_sweeps < 0 || done < max_sweeps)) {
    int batch = speculated;
    if (batch == 0) {
      batch = batch_size(iter_, done);
      SweepBatch(batch);
    }
    speculated = 0;
    done += batch;
    iter_ += batch - 1;  // index of the last sweep of the batch
    if (iter_ % epoch == 0) {
      const int next = (PipelinedChecks() && (params_.ignore_stopping_criteria || far_from_optimal()))
                           ? batch_size(iter_ + 1, done)
                           : 0;
      if (next > 0) {
        BeginResiduals();
        SaveSnapshot();
        SweepBatch(next);  // runs on the device while the host waits for the check's scalars
        speculated = next;
        EndResiduals();
        if (status_.state == pb::SolverStatus::OPTIMAL) {
          RestoreSnapshot();  // the speculative sweeps are discarded (and were never counted)
          finished_ = true;
          break;
        }
      } else {
        ComputeResiduals();
        if (status_.state == pb::SolverStatus::OPTIMAL) {
          finished_ = true;
          break;
        }
      }
    }
    if (iter_ % log_every == 0) LogStatus();
    ++iter_;
  }
  if (!finished_ && iter_ == params_.max_iterations) {
    ComputeResiduals();
    status_.state = pb::SolverStatus::MAX_ITERATIONS_REACHED;
    finished_ = true;
  }
  Runtime::Get().Sync();
  if (Runtime::Get().peer()) Runtime::Get().peer()->CheckError();
  loop_seconds_ += Now() - t0;
  if (finished_) LogStatus();
  status_.init_time = init_seconds_;
  status_.total_time = init_seconds_ + loop_seconds_;
  return done;
}

void Solver::Solve() {
  const double t0 = Now();
  Init();
  Runtime::Get().Sync();
  init_seconds_ = Now() - t0;
  Run(-1);
}

// ---------------------------------------------------------------------------------------------------
// ProxADMMSolver (reference algorithms/prox_admm.cc)
// ---------------------------------------------------------------------------------------------------

class ProxADMMSolver final : public Solver {
 public:
  using Solver::Solver;
  ~ProxADMMSolver() override { ResetGraph(); }

  void Init() override {  // :110-129
    SetCurrentDType(data_->dtype());
    const double t0 = Now();
    if (op_cache_.size() > 64) op_cache_.Clear();
    OpCacheScope cache_scope(InitCache());
    static const bool trace = opt::IsSet(opt::kInitTrace);  // any value, 0 included
    auto mark = [&](const char* what) {  // host wall clock + device drain, debugging aid only
      if (!trace) return;
      const double th = Now();
      Runtime::Get().Sync();
      std::fprintf(stderr, "[init] %-16s host %.2f ms  drained %.2f ms\n", what, 1e3 * (th - t0),
                   1e3 * (Now() - t0));
    };
    InitConstraints();
    mark("constraints");
    InitProxOperators();
    mark("prox operators");
    if (!params_.warm_start || !vars_initialized_) {
      InitVariables();
      vars_initialized_ = true;
    }
    iter_ = 0;
    finished_ = false;
    status_ = pb::SolverStatus();
    initialized_ = true;
    ResetGraph();
    route_.reset();  // (its state lives on in the views for as long as they are needed)
    route_ = RecogniseMultiBlockRoute({static_cast<int>(problem_.constraint.size()), A_, b_, prox_, data_.get(),
                                       shared_cache_, u_, x_, y_, y_prev_});
    mark("fused state");
    if (params_.verbose && log_) {
      char buf[128];
      std::snprintf(buf, sizeof(buf), "constraints, m = %lld, variables, n = %lld",
                    static_cast<long long>(m_), static_cast<long long>(n_));
      log_(buf);
    }
    Runtime::Get().Sync();
    init_seconds_ = Now() - t0;
  }

  BlockVector GetSolution() override {  // :171-176
    BlockVector r;
    for (int i = 0; i < N_; ++i) r += x_[i];
    return r;
  }

 protected:
  void InitConstraints() {  // :25-43
    A_ = BlockMatrix();
    b_ = BlockVector();
    for (size_t i = 0; i < problem_.constraint.size(); ++i) {
      const pb::Expression& constr = problem_.constraint[i];
      EPS_CHECK_MSG(constr.expression_type == pb::Expression::INDICATOR, "constraint is not an indicator");
      EPS_CHECK_MSG(constr.cone_type == 1, "constraint cone is not ZERO");
      EPS_CHECK(constr.arg.size() == 1);
      affine::BuildAffineOperator(constr.arg[0], data_.get(), affine::constraint_key(i), &A_, &b_);
    }
    AT_ = A_.Transpose();
    GlobalDims(A_, &m_, &n_);
  }

  void InitProxOperators() {  // :45-94
    EPS_CHECK_MSG(problem_.objective.expression_type == pb::Expression::ADD, "objective is not ADD");
    N_ = static_cast<int>(problem_.objective.arg.size());
    EPS_CHECK_MSG(params_.rho == 1, "rho != 1 is not supported (reference prox_admm.cc:50)");
    const double sqrt_rho = std::sqrt(params_.rho);
    prox_.clear();
    AiT_.clear();
    arg_shards_.clear();
    term_per_rank_.clear();
    std::set<std::string> constr_vars = A_.col_keys();
    for (int i = 0; i < N_; ++i) {
      const pb::Expression& f_expr = problem_.objective.arg[i];
      EPS_CHECK_MSG(f_expr.expression_type == pb::Expression::PROX_FUNCTION,
                    "objective term " << i << " is not a PROX_FUNCTION");
      AffineOperator H;
      for (size_t k = 0; k < f_expr.arg.size(); ++k)
        affine::BuildAffineOperator(f_expr.arg[k], data_.get(), affine::arg_key(k), &H.A, &H.b);
      AffineOperator A;
      std::map<std::string, const pb::Expression*> vars;
      GetVariables(f_expr, &vars);
      for (const auto& var : vars) {
        if (constr_vars.find(var.first) == constr_vars.end()) continue;
        for (const auto& it : A_.col(var.first)) A.A(it.first, var.first) = sqrt_rho * it.second;
      }
      prox_.emplace_back(CreateProxOperator(f_expr.prox_function.prox_function_type,
                                            f_expr.prox_function.epigraph));
      arg_shards_.push_back(InferShardedArgs(H.A));
      {
        // consensus form: is this one of the per-rank terms f_g(x_g)?
        const ShardSpec& sh = ShardSpec::Get();
        bool own = sh.active() && sh.consensus_terms() && !vars.empty();
        for (const auto& var : vars) own = own && sh.IsSharded(var.first);
        term_per_rank_.push_back(own);
      }
      {
        LocalShardScope scope(arg_shards_.back());
        prox_.back()->Init(ProxOperatorArg(f_expr.prox_function, data_.get(), H, A));
      }
      AiT_.push_back(A.A.Transpose());
    }
  }

  void InitVariables() {  // :96-108
    x_.assign(N_, BlockVector());
    y_.assign(N_, BlockVector());
    u_ = BlockVector();
    for (size_t i = 0; i < problem_.constraint.size(); ++i) {
      u_.Set(affine::constraint_key(i),
             DVec::Zeros(GetDimension(problem_.constraint[i].arg[0]), data_->dtype()));
    }
  }

  void ResetGraph() {
    if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    graph_exec_ = nullptr;
    graph_ = nullptr;
    graph_len_ = 0;
  }

  // The sweeps between two residual checks replayed from one hipGraph: a sharded sweep is 3
  // short dependent launches (~60 us of kernels at 8 ranks), so the host's per-launch cost and
  // jitter would otherwise sit on the critical path.  Iterates are bit-identical to the eager
  // launches (same kernels, same arguments; the exchange tags come from a device counter).
  void SweepBatch(int count) override {
    // EPSILON_HIP_GRAPH: 0 never, 1 always (fused), default: peer mode
    static const int mode = opt::Int(opt::kGraph, -1);
    Runtime& rt = Runtime::Get();
    const bool want = route_ && route_->Capturable() && (mode == 1 || (mode != 0 && route_->CaptureByDefault()));
    if (!want || count < 2 || rt.profiling()) {
      for (int i = 0; i < count; ++i) Sweep();
      return;
    }
    if (graph_exec_ == nullptr || graph_len_ != count) {
      ResetGraph();
      hipStream_t s = rt.stream();
      EPS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      rt.set_capturing(true);
      try {
        for (int i = 0; i < count; ++i) route_->Sweep();
      } catch (...) {
        rt.set_capturing(false);
        hipGraph_t dead = nullptr;
        (void)hipStreamEndCapture(s, &dead);
        if (dead) (void)hipGraphDestroy(dead);
        throw;
      }
      rt.set_capturing(false);
      EPS_HIP(hipStreamEndCapture(s, &graph_));
      EPS_HIP(hipGraphInstantiate(&graph_exec_, graph_, nullptr, nullptr, 0));
      graph_len_ = count;
    }
    EPS_HIP(hipGraphLaunch(graph_exec_, rt.stream()));
  }

  void Sweep() override {  // :135-147
    if (route_) {
      route_->Sweep();
      return;
    }
    y_prev_ = y_;  // shallow: blocks are replaced, never mutated, below
    u_ -= b_;
    for (int i = 0; i < N_; ++i) u_ -= y_[i];
    for (int i = 0; i < N_; ++i) {
      u_ += y_[i];
      {
        LocalShardScope scope(arg_shards_[i]);
        x_[i] = prox_[i]->Apply(u_);
      }
      y_[i] = A_ * x_[i];
      u_ -= y_[i];
    }
  }

  // ---- residual check of a route that has its own: splittable for pipelining -------------------
  bool PipelinedChecks() const override { return route_ && route_->PipelineChecks(); }
  void BeginResiduals() override {
    Runtime& rt = Runtime::Get();
    rt.ResetSlots();
    route_->LaunchNorms();
    rt.FetchSlotsAsync();
  }
  void EndResiduals() override {
    Runtime::Get().WaitSlots();
    FinishRouteCheck();
  }
  void FinishRouteCheck() override {
    const FusedRoute::Check c = route_->FinishCheck();
    const double rho = params_.rho;
    FinishResiduals(c.r, rho * c.s,
                    params_.abs_tol * std::sqrt(static_cast<double>(m_)) + params_.rel_tol * c.max_norm,
                    params_.abs_tol * std::sqrt(static_cast<double>(n_)) + params_.rel_tol * rho * c.atu);
  }
  void SaveSnapshot() override { route_->SaveSnapshot(); }
  void RestoreSnapshot() override { route_->RestoreSnapshot(); }

  void ComputeResiduals() override {  // :178-217
    if (route_ && route_->HasCheck()) {
      BeginResiduals();
      EndResiduals();
      return;
    }
    Runtime& rt = Runtime::Get();
    rt.ResetSlots();
    const int s_b = b_.NormSqAsync();
    std::vector<int> s_Ax(N_);
    BlockVector Ax_b = b_;
    for (int i = 0; i < N_; ++i) {
      // A_*x_[i] is y_[i], computed by the sweep (the reference recomputes it, :186)
      s_Ax[i] = y_[i].NormSqAsync();
      Ax_b += y_[i];
    }
    const int s_r = Ax_b.NormSqAsync();
    std::vector<int> s_s;
    BlockVector Ax_diff;
    for (int i = N_ - 2; i >= 0; --i) {
      Ax_diff += y_[i + 1] - y_prev_[i + 1];
      s_s.push_back((AiT_[i] * Ax_diff).NormSqAsync());
    }
    const int s_u = (AT_ * u_).NormSqAsync();
    rt.FetchSlots();
    if (rt.peer()) rt.peer()->CheckError();

    double max_norm = std::sqrt(rt.SlotValue(s_b));
    double own_max = -1;
    for (int i = 0; i < N_; ++i) {
      if (term_per_rank_[i])  // one term per rank: the reference's max runs over all of them
        own_max = std::fmax(own_max, std::sqrt(rt.SlotLocalValue(s_Ax[i])));
      else
        max_norm = std::fmax(max_norm, std::sqrt(rt.SlotValue(s_Ax[i])));
    }
    if (ShardSpec::Get().active() && ShardSpec::Get().consensus_terms())
      max_norm = std::fmax(max_norm, rt.comm()->AllReduceMaxHost(own_max));
    double s2 = 0;
    for (int s : s_s) {
      const double si = std::sqrt(rt.SlotValue(s));
      s2 += si * si;
    }
    const double rho = params_.rho;
    FinishResiduals(std::sqrt(rt.SlotValue(s_r)), rho * std::sqrt(s2),
                    params_.abs_tol * std::sqrt(static_cast<double>(m_)) + params_.rel_tol * max_norm,
                    params_.abs_tol * std::sqrt(static_cast<double>(n_)) +
                        params_.rel_tol * rho * std::sqrt(rt.SlotValue(s_u)));
  }

 private:
  int64_t m_ = 0, n_ = 0;
  int N_ = 0;
  bool vars_initialized_ = false;
  BlockMatrix A_, AT_;
  BlockVector b_;
  std::vector<BlockMatrix> AiT_;
  std::vector<std::unique_ptr<ProxOperator>> prox_;
  std::vector<std::set<std::string>> arg_shards_;
  std::vector<bool> term_per_rank_;
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t graph_exec_ = nullptr;
  int graph_len_ = 0;
  BlockVector u_;
  std::vector<BlockVector> x_, y_, y_prev_;
};

// ---------------------------------------------------------------------------------------------------
// ProxADMMTwoBlockSolver (reference algorithms/prox_admm_two_block.cc)
// ---------------------------------------------------------------------------------------------------

class ProxADMMTwoBlockSolver final : public Solver {
 public:
  using Solver::Solver;

  void Init() override {  // :21-94
    SetCurrentDType(data_->dtype());
    const double t0 = Now();
    if (op_cache_.size() > 64) op_cache_.Clear();
    OpCacheScope cache_scope(InitCache());
    const double sqrt_rho = std::sqrt(params_.rho);
    const DType dt = data_->dtype();
    AffineOperator H, A;
    BlockVector z0;
    for (size_t i = 0; i < problem_.constraint.size(); ++i) {
      const pb::Expression& constr = problem_.constraint[i];
      EPS_CHECK_MSG(constr.expression_type == pb::Expression::INDICATOR, "constraint is not an indicator");
      EPS_CHECK_MSG(constr.cone_type == 1, "constraint cone is not ZERO");
      EPS_CHECK(constr.arg.size() == 1);
      affine::BuildAffineOperator(constr.arg[0], data_.get(), affine::constraint_key(i), &H.A, &H.b);
      std::map<std::string, const pb::Expression*> vars;
      GetVariables(constr, &vars);
      for (const auto& var : vars) {
        const int64_t dim = GetDimension(*var.second);
        A.A(var.first, var.first) = sqrt_rho * LinearMap::Identity(dim);
        z0.Set(var.first, DVec::Zeros(dim, dt));
      }
    }
    constr_prox_ = CreateProxOperator(pb::ProxFunction::ZERO, false);
    zero_f_ = pb::ProxFunction();
    constr_prox_->Init(ProxOperatorArg(zero_f_, data_.get(), H, A));
    GlobalDims(H.A, &m_, &n_);
    constr_H_ = H;

    EPS_CHECK_MSG(problem_.objective.expression_type == pb::Expression::ADD, "objective is not ADD");
    N_ = static_cast<int>(problem_.objective.arg.size());
    prox_.clear();
    arg_shards_.clear();
    for (int i = 0; i < N_; ++i) {
      const pb::Expression& f_expr = problem_.objective.arg[i];
      EPS_CHECK_MSG(f_expr.expression_type == pb::Expression::PROX_FUNCTION,
                    "objective term " << i << " is not a PROX_FUNCTION");
      AffineOperator Hi, Ai;
      for (size_t k = 0; k < f_expr.arg.size(); ++k)
        affine::BuildAffineOperator(f_expr.arg[k], data_.get(), affine::arg_key(k), &Hi.A, &Hi.b);
      std::map<std::string, const pb::Expression*> vars;
      GetVariables(f_expr, &vars);
      for (const auto& var : vars)
        Ai.A(var.first, var.first) = sqrt_rho * LinearMap::Identity(GetDimension(*var.second));
      prox_.emplace_back(CreateProxOperator(f_expr.prox_function.prox_function_type,
                                            f_expr.prox_function.epigraph));
      arg_shards_.push_back(InferShardedArgs(Hi.A));
      LocalShardScope scope(arg_shards_.back());
      prox_.back()->Init(ProxOperatorArg(f_expr.prox_function, data_.get(), Hi, Ai));
    }
    if (!params_.warm_start || !vars_initialized_) {
      z_ = z0;
      u_ = BlockVector();
      x_ = BlockVector();
      vars_initialized_ = true;
    }
    iter_ = 0;
    finished_ = false;
    status_ = pb::SolverStatus();
    initialized_ = true;
    route_.reset();
    route_ = RecogniseTwoBlockRoute({static_cast<int>(problem_.constraint.size()), constr_H_, prox_, data_.get(), x_,
                                     z_, u_, z_prev_});
    Runtime::Get().Sync();
    init_seconds_ = Now() - t0;
  }

  BlockVector GetSolution() override { return x_; }

 protected:
  void Sweep() override {  // :97-112
    if (route_) {
      route_->Sweep();
      return;
    }
    z_prev_ = z_;
    BlockVector zu = z_ - u_;
    x_ = BlockVector();
    for (int i = 0; i < N_; ++i) {
      LocalShardScope scope(arg_shards_[i]);
      x_ += prox_[i]->Apply(zu);
    }
    z_ = constr_prox_->Apply(x_ + u_);
    u_ += x_ - z_;
  }

  void ComputeResiduals() override {  // :135-156
    Runtime& rt = Runtime::Get();
    rt.ResetSlots();
    const int s_r = DiffNormSqAsync(x_, z_);
    const int s_s = DiffNormSqAsync(z_, z_prev_);
    const int s_x = x_.NormSqAsync();
    const int s_z = z_.NormSqAsync();
    const int s_u = u_.NormSqAsync();
    rt.FetchSlots();
    const double rho = params_.rho;
    const double sq_n = std::sqrt(static_cast<double>(n_));
    FinishResiduals(std::sqrt(rt.SlotValue(s_r)), rho * std::sqrt(rt.SlotValue(s_s)),
                    params_.abs_tol * sq_n + params_.rel_tol * std::fmax(std::sqrt(rt.SlotValue(s_x)),
                                                                         std::sqrt(rt.SlotValue(s_z))),
                    params_.abs_tol * sq_n + params_.rel_tol * rho * std::sqrt(rt.SlotValue(s_u)));
  }

 private:
  int64_t m_ = 0, n_ = 0;
  int N_ = 0;
  bool vars_initialized_ = false;
  pb::ProxFunction zero_f_;
  std::vector<std::unique_ptr<ProxOperator>> prox_;
  std::vector<std::set<std::string>> arg_shards_;
  std::unique_ptr<ProxOperator> constr_prox_;
  AffineOperator constr_H_;
  BlockVector x_, z_, u_, z_prev_;
};

std::unique_ptr<Solver> CreateSolver(pb::Problem problem, std::shared_ptr<DataMap> data,
                                     pb::SolverParams params) {  // solvemodule.cc:74-87
  if (params.solver == pb::SolverParams::PROX_ADMM)
    return std::unique_ptr<Solver>(new ProxADMMSolver(std::move(problem), std::move(data), params));
  if (params.solver == pb::SolverParams::PROX_ADMM_TWO_BLOCK)
    return std::unique_ptr<Solver>(
        new ProxADMMTwoBlockSolver(std::move(problem), std::move(data), params));
  EPS_FATAL("Unknown solver: " << params.solver);
}

BlockVector EvalProx(const pb::Expression& f_expr, double lambda, DataMap* data,
                     const BlockVector& v_in) {  // solvemodule.cc:189-242
  EPS_CHECK_MSG(f_expr.expression_type == pb::Expression::PROX_FUNCTION,
                "eval_prox: expression is not a PROX_FUNCTION");
  SetCurrentDType(data->dtype());
  AffineOperator H, A;
  for (size_t i = 0; i < f_expr.arg.size(); ++i)
    affine::BuildAffineOperator(f_expr.arg[i], data, affine::arg_key(i), &H.A, &H.b);
  std::map<std::string, const pb::Expression*> vars;
  GetVariables(f_expr, &vars);
  int i = 0;
  for (const auto& var : vars) {
    A.A(affine::constraint_key(i++), var.first) =
        (1 / std::sqrt(lambda)) * LinearMap::Identity(GetDimension(*var.second));
  }
  BlockVector v = A.A * v_in;
  std::unique_ptr<ProxOperator> op = CreateProxOperator(f_expr.prox_function.prox_function_type,
                                                        f_expr.prox_function.epigraph);
  op->Init(ProxOperatorArg(f_expr.prox_function, data, H, A));
  return op->Apply(v);
}

}  // namespace eps
