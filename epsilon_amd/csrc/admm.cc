#include "admm.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "comm.h"
#include "kernels.h"

namespace eps {

GraphStats& GraphStats::Get() {
  static GraphStats g;
  return g;
}


namespace {

double Now() {
  using clock = std::chrono::steady_clock;
  return std::chrono::duration<double>(clock::now().time_since_epoch()).count();
}

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
// The generic operator path's sweeps between two residual checks as ONE hipGraph (small problems
// are bound by launch latency: 30-60 launches of a few microseconds per sweep).  BlockVector
// blocks are replaced, never mutated, so a sweep ends in other buffers than it started from; the
// capture therefore runs on CANONICAL copies of the state (shared with this object, hence
// copy-on-write keeps the sweep from writing into them) and ends with device-to-device copies of
// the final blocks back into them: every replay starts and ends at the same addresses.  All
// buffers the captured launches touch are fenced off by a Runtime hold for the graph's life.
// Only for problems whose operators are all ProxOperator::CaptureSafe and whose state is small.
// ---------------------------------------------------------------------------------------------------
class SweepGraph {
 public:
  ~SweepGraph() { Reset(); }

  void Reset() {
    if (exec_) (void)hipGraphExecDestroy(exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    exec_ = nullptr;
    graph_ = nullptr;
    len_ = 0;
    if (!held_.empty()) Runtime::Get().ReturnHeld(&held_);  // (stream order keeps the reuse safe)
    canon_.clear();
  }
  void ClearFailure() { failed_ = false; }

  // MEASURED, AND OFF BY DEFAULT (round 3, ROCm 7.2, MI355X): replaying the generic sweeps from a
  // graph is bit-identical to the eager launches (tests) and buys nothing - 1000 sweeps of the
  // reference's lasso_sparse / mnist / mv_lasso problems take 0.102 / 0.312 / 0.104 s replayed
  // against 0.093 / 0.320 / 0.104 s eager: the host already runs far ahead of the stream, and the
  // gap between two dependent kernels is the same inside a graph - while capturing and
  // instantiating a batch costs 4-5 ms, more than most solves of these problems take in all.
  // EPSILON_HIP_GRAPH_GENERIC (option "graph_generic") = 1: once a run has lasted kEagerFirst
  // sweeps; = 2: after the first sweep (tests); 0 / unset: never.  Read per call.
  static constexpr int kEagerFirst = 50;
  static int Mode() {
    const char* e = std::getenv("EPSILON_HIP_GRAPH_GENERIC");
    return e ? std::atoi(e) : 0;
  }
  static int EagerSweepsFirst() { return Mode() >= 2 ? 1 : kEagerFirst; }

  bool Wanted(int count, const std::vector<BlockVector*>& state) const {
    const int gmode = Mode();
    Runtime& rt = Runtime::Get();
    if (gmode == 0 || count < 2 || failed_) return false;
    if (rt.profiling() || rt.capturing() || rt.holding() || ShardSpec::Get().active()) return false;
    // launch-bound problems only: the copies back cost a pass over the state per batch
    int64_t bytes = 0;
    for (const BlockVector* v : state)
      for (const auto& kv : v->data()) bytes += static_cast<int64_t>(kv.second.bytes());
    return bytes <= (int64_t(64) << 20);
  }

  // Replays `count` sweeps (capturing first when there is no graph of that length, or when
  // somebody re-bound the state since).  false: nothing was enqueued - the caller launches eagerly.
  // The first `n_prev` handles are "previous iterate" copies that every sweep overwrites before it
  // reads them (y_prev = y): their layout before the capture does not matter.
  template <class SweepFn>
  bool Run(int count, const std::vector<BlockVector*>& state, size_t n_prev, SweepFn sweep) {
    if (exec_ == nullptr || len_ != count || !IsCanonical(state)) Capture(count, state, n_prev, sweep);
    if (exec_ == nullptr) return false;
    EPS_HIP(hipGraphLaunch(exec_, Runtime::Get().stream()));
    GraphStats::Get().replayed_sweeps += count;
    return true;
  }

 private:
  static bool SameBuffers(const BlockVector& a, const BlockVector& b) {
    if (a.data().size() != b.data().size()) return false;
    auto ia = a.data().begin();
    auto ib = b.data().begin();
    for (; ia != a.data().end(); ++ia, ++ib)
      if (ia->first != ib->first || ia->second.data() != ib->second.data() || ia->second.n != ib->second.n)
        return false;
    return true;
  }
  static BlockVector CloneBlocks(const BlockVector& v) {
    BlockVector c;
    for (const auto& kv : v.data()) c.Set(kv.first, kv.second.Clone());
    return c;
  }
  // dst (canonical) <- src, block by block, on the stream; false: the layouts differ
  static bool CopyBlocksBack(const BlockVector& dst, const BlockVector& src) {
    if (dst.data().size() != src.data().size()) return false;
    hipStream_t s = Runtime::Get().stream();
    auto id = dst.data().begin();
    auto is = src.data().begin();
    for (; id != dst.data().end(); ++id, ++is) {
      if (id->first != is->first || id->second.n != is->second.n || id->second.dt != is->second.dt) return false;
      if (id->second.data() == is->second.data() || id->second.n == 0) continue;
      EPS_HIP(hipMemcpyAsync(const_cast<void*>(static_cast<const void*>(id->second.data())), is->second.data(),
                             id->second.bytes(), hipMemcpyDeviceToDevice, s));
    }
    return true;
  }
  bool IsCanonical(const std::vector<BlockVector*>& state) const {
    if (state.size() != canon_.size()) return false;
    for (size_t i = 0; i < state.size(); ++i)
      if (!SameBuffers(*state[i], canon_[i])) return false;
    return true;
  }

  // `state`: every BlockVector a sweep reads from the one before it, "previous iterate" handles
  // FIRST (a block the last sweep left alone may still be the canonical buffer of its successor,
  // which the copies back overwrite afterwards).
  template <class SweepFn>
  void Capture(int count, const std::vector<BlockVector*>& state, size_t n_prev, SweepFn sweep) {
    Runtime& rt = Runtime::Get();
    hipStream_t s = rt.stream();
    Reset();
    std::vector<BlockVector> saved;  // the handles as they are, should the capture be abandoned
    for (BlockVector* v : state) {
      saved.push_back(*v);
      canon_.push_back(CloneBlocks(*v));
    }
    rt.BeginHold();
    for (size_t i = 0; i < state.size(); ++i) *state[i] = canon_[i];
    bool ok = hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess;
    hipGraph_t graph = nullptr;
    std::string why;
    if (ok) {
      rt.set_capturing(true);
      try {
        for (int i = 0; i < count; ++i) sweep();
        for (size_t i = 0; i < state.size() && ok; ++i) {
          ok = CopyBlocksBack(canon_[i], *state[i]);
          if (!ok && i < n_prev) {  // written before read: its canonical buffers take today's layout
            BlockVector fresh;
            for (const auto& kv : state[i]->data()) fresh.Set(kv.first, DVec::Empty(kv.second.n, kv.second.dt));
            canon_[i] = fresh;
            ok = CopyBlocksBack(canon_[i], *state[i]);
          }
          if (!ok) {
            why = "the block layout of state handle " + std::to_string(i) + " changed during the sweeps: had";
            for (const auto& kv : canon_[i].data()) why += " " + kv.first + ":" + std::to_string(kv.second.n);
            why += "; has";
            for (const auto& kv : state[i]->data()) why += " " + kv.first + ":" + std::to_string(kv.second.n);
          }
        }
      } catch (const std::exception& e) {
        ok = false;
        why = e.what();
      } catch (...) {
        ok = false;
        why = "exception";
      }
      rt.set_capturing(false);
      const hipError_t ee = hipStreamEndCapture(s, &graph);
      if (ee != hipSuccess || graph == nullptr) {
        if (ok) why = std::string("hipStreamEndCapture: ") + hipGetErrorString(ee);
        ok = false;
      }
    } else {
      why = "hipStreamBeginCapture failed";
    }
    if (ok) {
      const hipError_t ei = hipGraphInstantiate(&exec_, graph, nullptr, nullptr, 0);
      if (ei != hipSuccess) {
        ok = false;
        why = std::string("hipGraphInstantiate: ") + hipGetErrorString(ei);
      }
    }
    if (!ok) {
      static const bool trace = std::getenv("EPSILON_HIP_GRAPH_TRACE") != nullptr;
      if (trace) std::fprintf(stderr, "[graph] capture of %d generic sweeps abandoned: %s\n", count, why.c_str());
      (void)hipGetLastError();
      if (graph) (void)hipGraphDestroy(graph);
      exec_ = nullptr;
      for (size_t i = 0; i < state.size(); ++i) *state[i] = saved[i];  // nothing ran: the state is where it was
      std::vector<std::pair<size_t, void*>> held = rt.EndHold();
      rt.ReturnHeld(&held);
      Reset();
      failed_ = true;
      return;
    }
    graph_ = graph;
    len_ = count;
    ++GraphStats::Get().captures;
    for (size_t i = 0; i < state.size(); ++i) *state[i] = canon_[i];  // the last sweep's handles go to the held pool
    saved.clear();
    held_ = rt.EndHold();
  }

  hipGraph_t graph_ = nullptr;
  hipGraphExec_t exec_ = nullptr;
  int len_ = 0;
  bool failed_ = false;  // a capture did not work out: the solver stays on eager launches
  std::vector<std::pair<size_t, void*>> held_;
  std::vector<BlockVector> canon_;
};


namespace {

int BatchWideMin();  // (with the batched solves below)

// Matrix variables X (n x k) under the data map I_k (x) A: the k columns run as k members of the
// batched kernels inside one solve (ProxADMMSolver::TryEnableFused).  Below this many rows of A
// the solve keeps the generic operator path (a constant: no crossover was measured).
constexpr int64_t kMatrixFusedMinRows = 256;

// EPSILON_HIP_FUSED_MATRIX (eps_set_option "fused_matrix"), read at every Init.
enum MatrixRoute { kMatrixOff, kMatrixAuto, kMatrixPass, kMatrixWide };
MatrixRoute FusedMatrixMode() {
  const char* e = std::getenv("EPSILON_HIP_FUSED_MATRIX");
  if (e == nullptr || std::strcmp(e, "auto") == 0) return kMatrixAuto;
  if (std::strcmp(e, "0") == 0) return kMatrixOff;
  if (std::strcmp(e, "pass") == 0) return kMatrixPass;
  if (std::strcmp(e, "wide") == 0) return kMatrixWide;
  EPS_FATAL("fused_matrix must be 0, pass, wide or auto, got " << e);
}

// ZERO-term problems (basis pursuit, hinge / deadzone + l1 in graph form) on the fused sweep
// (ProxADMMSolver::TryEnableZeroFused).  Below this many rows of the data matrix
// the solve keeps the generic operator path (a constant: no crossover was measured).
constexpr int64_t kZeroFusedMinRows = 256;

// EPSILON_HIP_FUSED_ZERO (eps_set_option "fused_zero"), read at every Init.
bool FusedZeroAuto() {
  const char* e = std::getenv("EPSILON_HIP_FUSED_ZERO");
  if (e == nullptr || std::strcmp(e, "auto") == 0) return true;
  if (std::strcmp(e, "0") == 0) return false;
  EPS_FATAL("fused_zero must be 0 or auto, got " << e);
}

// One sweep of a panel of up to 64 f32 members on the wide route (kernels_fused_wide.hip): back
// product + chain, forward product, reduction and - unless whitened - the cached inverse times
// the panel.  The workspaces depend on (m, n) alone and serve every panel in turn.
struct WideSweep {
  static constexpr int PW = k::kLassoWidePanel;
  int64_t m = 0, n = 0, lda = 0, ldv = 0, panel_len = 0;
  DVec A;
  bool whiten = false;
  const DenseMatrixImpl* D = nullptr;  // the cached inverse (not whitened)
  DVec V, T, apart;
  int64_t akc = 0, afull = 0, arem = 0, aparts = 0;

  void Init(int64_t m_, int64_t n_, const DVec& A_, int64_t lda_, bool whiten_, const DenseMatrixImpl* D_) {
    m = m_;
    n = n_;
    A = A_;
    lda = lda_;
    whiten = whiten_;
    D = D_;
    ldv = (n + 63) / 64 * 64;
    panel_len = static_cast<int64_t>(PW) * m;
    V = DVec::Zeros(static_cast<int64_t>(PW) * ldv, F32);
    T = DVec::Empty(static_cast<int64_t>(k::LassoWideSlabs(m, n)) * panel_len, F32);
    // ranges of the inverse apply's contraction: at most 64, each a multiple of 32 rows
    akc = std::max<int64_t>(32, ((m + 63) / 64 + 31) / 32 * 32);
    afull = m / akc;
    arem = m - afull * akc;
    aparts = afull + (arem > 0 ? 1 : 0);
    apart = whiten ? DVec() : DVec::Empty(aparts * panel_len, F32);
  }

  // Wp = Dinv Pp: always PW columns - the product kernel and its contraction order must not
  // depend on the number of members.  The contraction is split into `aparts` ranges of `akc`
  // rows whose products are summed by ReducePartials: one chain over all m rows would carry the
  // rounding of an m-term sequential sum into w.
  void ApplyInverse(const DVec& Pp, const DVec& Wp) const {
    const int64_t sA = D->trans() ? akc : akc * D->rows();
    k::GemmBatched(D->trans(), false, m, PW, akc, D->scale(), D->data(), D->rows(), sA, Pp, m, akc, 0.0, apart, m,
                   panel_len, afull);
    if (arem > 0) {
      const int64_t oA = afull * sA, oB = afull * akc;
      k::GemmBatched(D->trans(), false, m, PW, arem, D->scale(), D->data().Slice(oA, D->data().n - oA), D->rows(),
                     0, Pp.Slice(oB, Pp.n - oB), m, 0, 0.0, apart.Slice(afull * panel_len, panel_len), m, 0, 1);
    }
    k::ReducePartials(panel_len, static_cast<int>(aparts), apart, 1.0, 0.0, Wp);
  }

  // slots [first, first + nk) of `table`, `live` as LassoWideBack's mask; Wp / Pp: the panel's w
  // and p (Pp unused when whitened: the reduction writes w_hat into Wp through the descriptors)
  void Run(const DVec& table, int first, int nk, uint64_t live, const DVec& Wp, const DVec& Pp,
           const double* group_lam = nullptr) const {
    k::LassoWideBack(m, n, lda, A, table, first, nk, live, Wp, m, V, ldv, group_lam);
    k::LassoWideForward(m, n, lda, A, nk, V, ldv, T, m);
    k::LassoWideReduce(m, n, table, first, nk, live, T, m);
    if (!whiten) ApplyInverse(Pp, Wp);
  }
};

}  // namespace

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
    static const bool trace = std::getenv("EPSILON_HIP_INIT_TRACE") != nullptr;
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
    TryEnableFused();
    TryEnableZeroFused();
    mark("fused state");
    capture_safe_ = true;
    for (const auto& op : prox_) capture_safe_ = capture_safe_ && op->CaptureSafe();
    eager_sweeps_ = 0;
    gg_.ClearFailure();
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

  // ---- batched solves (RunFusedBatches) -------------------------------------------------------
  // A fresh fused solve whose pass the batched one mirrors: its instance for the batched kernels
  // and the key of the group it can join (same data matrix, inverse, dtype and shape).
  bool BatchView(k::LassoInstance* mem, std::vector<uint64_t>* key) const {
    if (!initialized_ || finished_ || iter_ != 0 || !fused_ || fs_.use_peer || ShardSpec::Get().active()) return false;
    const FusedState& f = fs_;
    if (f.cols > 1) return false;  // a matrix variable is a batch of its own: it runs alone
    const DenseMatrixImpl& L = *f.ls.L_arg_var;
    const DenseMatrixImpl& D = *f.ls.Dinv_arg;
    const DType dt = data_->dtype();
    if (L.dtype() != dt || k::LassoBatchWidth(f.m, f.n, dt) == 0) return false;
    *mem = f.pass.inst;
    auto bits = [](double v) {
      uint64_t b;
      std::memcpy(&b, &v, 8);
      return b;
    };
    *key = {reinterpret_cast<uintptr_t>(L.data().data()), static_cast<uint64_t>(L.rows()),
            static_cast<uint64_t>(f.m), static_cast<uint64_t>(f.n), static_cast<uint64_t>(dt),
            bits(L.scale()), reinterpret_cast<uintptr_t>(D.data().data()), bits(D.scale()),
            reinterpret_cast<uintptr_t>(f.symv_packed.data()), f.symv_work.n > 0 ? 1u : 0u,
            static_cast<uint64_t>(params_.max_iterations), static_cast<uint64_t>(params_.epoch_iterations),
            f.whiten ? 1u : 0u, reinterpret_cast<uintptr_t>(f.Ahat.data())};
    return true;
  }
  const DVec& batch_packed_inverse() const { return fs_.symv_packed; }
  double batch_inverse_scale() const { return fs_.ls.Dinv_arg->scale(); }
  const DenseMatrixImpl& batch_inverse() const { return *fs_.ls.Dinv_arg; }
  int batch_grid() const { return fs_.grid; }
  bool batch_whitened() const { return fs_.whiten; }
  const DVec& batch_matrix(int64_t* lda) const {
    *lda = fs_.pass.lda;
    return fs_.pass.A;
  }
  void BatchApplyInverse() { ApplyInverseFixed(); }
  // the residual check at sweep `iter`: its scalars into the next slots, then (after the fetch)
  // the status; true if the instance stops here
  void BatchLaunchNorms(int iter) {
    iter_ = iter;
    LaunchFusedNorms();
  }
  bool BatchFinishCheck() {
    FinishFusedCheck();
    finished_ = status_.state == pb::SolverStatus::OPTIMAL;
    return finished_;
  }
  // what Run() does when the sweeps run out
  void BatchFinishMaxIterations(int iter) {
    iter_ = iter;
    ComputeResiduals();
    status_.state = pb::SolverStatus::MAX_ITERATIONS_REACHED;
    finished_ = true;
  }
  void BatchSetLoopTime(double seconds) {
    loop_seconds_ += seconds;
    status_.init_time = init_seconds_;
    status_.total_time = init_seconds_ + loop_seconds_;
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

  // ---- fused sweep: "least squares + separable threshold" (kernels_fused.hip) ------------------
 private:
  struct FusedState;  // (below)

 protected:
  // Recognised structure (the compiled lasso): two terms [SUM_SQUARE with a dense
  // argument map, scaled-zone prox with scalar maps], one consensus constraint a0 x' + a1 x = 0
  // with a0 = 1 and no constant.  The sweep is then: one fused pass over A (back substitution of
  // this sweep, elementwise chain, forward substitution of the next sweep), a partial-sum
  // reduction (+ the all-reduce when sharded) and the apply of the cached inverse.
  void TryEnableFused() {
    fused_ = false;
    ResetGraph();
    const char* env = std::getenv("EPSILON_HIP_FUSED");
    if (env && env[0] == '0') return;
    if (N_ != 2 || problem_.constraint.size() != 1) return;
    if (!b_.data().empty()) return;
    // consensus form: the threshold step averages over the ranks, which the fused pass does not
    if (ShardSpec::Get().active() && ShardSpec::Get().consensus_terms()) return;
    FusedState f;
    if (!prox_[0]->DescribeLeastSquares(&f.ls)) return;
    f.cols = f.ls.cols;
    const MatrixRoute matrix_mode = f.cols > 1 ? FusedMatrixMode() : kMatrixAuto;
    if (f.cols > 1 && (matrix_mode == kMatrixOff || ShardSpec::Get().active())) return;
    if (!prox_[1]->DescribeScaledZone(&f.sz)) {
      // group lasso: one group per row of the n x cols variable
      GroupNorm2Desc gn;
      if (f.cols == 1 || !prox_[1]->DescribeGroupNorm2(&gn) || gn.cols != f.cols) return;
      f.group = true;
      f.group_rows = gn.rows;
      f.sz = ScaledZoneDesc();
      f.sz.var_key = gn.var_key;
      f.sz.constraint_key = gn.constraint_key;
      f.sz.Bs = gn.Bs;
      f.sz.Cs = gn.Cs;
      f.sz.lam = gn.lam;
    }
    if ((f.sz.alpha_vec.n > 0 && f.sz.alpha_vec.dt != data_->dtype()) ||
        (f.sz.beta_vec.n > 0 && f.sz.beta_vec.dt != data_->dtype()))
      return;
    const std::string ck = affine::constraint_key(0);
    if (f.ls.constraint_key != ck || f.sz.constraint_key != ck) return;
    if (A_.data().size() != 2 || !A_.has_key(ck, f.ls.var_key) || !A_.has_key(ck, f.sz.var_key))
      return;
    const LinearMap& A0 = A_(ck, f.ls.var_key);
    const LinearMap& A1 = A_(ck, f.sz.var_key);
    if (A0.impl().type() != SCALAR_MATRIX || A1.impl().type() != SCALAR_MATRIX) return;
    if (GetScalar(A0) != 1.0) return;
    f.a1 = GetScalar(A1);
    const DenseMatrixImpl& L = *f.ls.L_arg_var;
    if (L.trans()) return;
    f.m = L.rows();
    f.n = L.cols();
    const int64_t nx = f.n * f.cols;  // entries of the variable (a matrix variable: column c at c * n)
    if (A0.impl().n() != nx || A1.impl().n() != nx) return;
    if (!k::LassoFusedSupported(f.m, f.n, L.data(), L.rows())) return;
    if (f.ls.rhs_arg.n != 0 && f.ls.rhs_arg.n != f.m * f.cols) return;
    const DType dt = data_->dtype();
    if (f.cols > 1 && !ChooseMatrixRoute(&f, matrix_mode)) return;
    // the six state vectors are slices of ONE buffer, so that a residual check can snapshot the
    // iterates with a single copy (pipelined checks, Solver::Run)
    const int64_t npad = (nx + 63) / 64 * 64;
    f.state_all = DVec::Zeros(6 * npad, dt);
    f.snapshot = DVec::Empty(6 * npad, dt);
    f.norm_work = DVec::Zeros(64 * 5 + 1, F64);
    int next_slice = 0;
    auto state = [&](const BlockVector& src, const std::string& key) {
      DVec v = f.state_all.Slice(static_cast<int64_t>(next_slice++) * npad, nx);
      if (src.has_key(key)) k::Copy(v, src(key));
      return v;
    };
    f.x0 = state(x_[0], f.ls.var_key);
    f.x1 = state(x_[1], f.sz.var_key);
    f.y0 = state(y_[0], ck);
    f.y1 = state(y_[1], ck);
    f.u = state(u_, ck);
    f.y1prev = state(BlockVector(), ck);
    f.grid = k::LassoFusedGrid(f.m, f.n, dt);
    // a matrix variable: column c's p and w at c * m (the wide route's instance-major panels,
    // whole panels of 64), its partials at c * grid * m
    const int64_t wlen = f.wide ? (f.cols + WideSweep::PW - 1) / WideSweep::PW * WideSweep::PW * f.m : f.cols * f.m;
    f.p = DVec::Zeros(wlen, dt);
    if (!f.wide) f.tpart = DVec::Empty(static_cast<int64_t>(f.grid) * f.m * f.cols, dt);
    if (f.cols > 1) {
      f.w = DVec::Zeros(wlen, dt);
    } else {
      Comm* comm = Runtime::Get().comm();
      PeerExchange* px = Runtime::Get().peer();
      const ShardSpec& sh = ShardSpec::Get();
      const bool sharded = sh.active() && sh.IsSharded(f.ls.var_key);
      // one-shot peer-write exchange inside the sweep's own kernels (kernels_peer.hip) when the
      // ranks share a window and the m-float message fits its slots; RCCL collectives otherwise
      // (a granule carries 32 value bits: an f64 value takes two)
      f.use_peer = sharded && px != nullptr && f.m * (dt == F64 ? 2 : 1) <= px->slot() && f.ls.Dinv_arg != nullptr &&
                   !f.ls.Dinv_arg->trans() && f.ls.Dinv_arg->rows() == f.m;
      const int G = f.use_peer ? px->view().G : (comm ? comm->size() : 1);
      f.slab = ((f.m + G - 1) / G + 3) / 4 * 4;
      f.wpad = DVec::Zeros(f.slab * G, dt);
      f.wslice = DVec::Zeros(f.slab, dt);
      f.w = f.wpad.Slice(0, f.m);  // the gathered vector IS w (first m entries)
      // the inverse is applied by row slabs + all-gather from 3 ranks up; with 2 ranks the
      // symmetric apply of the whole matrix reads the same m^2/2 entries and needs no exchange
      const char* e = std::getenv("EPSILON_HIP_SHARDED_APPLY");
      const bool want_slab = e ? e[0] != 'r' : G >= 3;
      f.peer_slab = f.use_peer && want_slab &&
                    k::PeerSlabApplySupported(px->view(), f.m, f.slab, f.ls.Dinv_arg->data(), f.m);
    }
    {
      const DenseMatrixImpl& D = *f.ls.Dinv_arg;
      if (!f.use_peer && !ShardSpec::Get().active() && EnableWhiten(&f)) {
        // no inverse apply in the sweep: no workspace, no packed copy
      } else if (f.wide) {
        // the inverse times the panel is a product of its own (WideSweep::ApplyInverse)
      } else if (D.symmetric() && D.rows() == f.m && D.rows() >= 1024 && !D.trans()) {
        f.symv_work = DVec::Empty(f.cols * k::SymvWorkspace(f.m), dt);
        // the apply reads a tile-packed copy of the lower tiles (EPSILON_HIP_SYMV_PACKED=0: the
        // matrix as it lies): +m^2/2 values of memory for a tenth of a millisecond at Init
        static const bool packed = [] {
          const char* e = std::getenv("EPSILON_HIP_SYMV_PACKED");
          return !(e && e[0] == '0');
        }();
        if (packed) f.symv_packed = PackInverse(D, f.m);
      }
    }
    if (f.wide) f.ws.Init(f.m, f.n, f.whiten ? f.Ahat : L.data(), f.whiten ? f.m : L.rows(), f.whiten, f.ls.Dinv_arg.get());
    ResetGraph();
    fs_ = f;
    BuildPass();
    // the generic containers become views of the fused state
    x_[0] = BlockVector();
    x_[0].Set(fs_.ls.var_key, fs_.x0);
    x_[1] = BlockVector();
    x_[1].Set(fs_.sz.var_key, fs_.x1);
    y_[0] = BlockVector();
    y_[0].Set(ck, fs_.y0);
    y_[1] = BlockVector();
    y_[1].Set(ck, fs_.y1);
    u_ = BlockVector();
    u_.Set(ck, fs_.u);
    y_prev_.assign(2, BlockVector());
    y_prev_[1].Set(ck, fs_.y1prev);
    fused_ = true;
    FusedForward(/*from_state=*/true);
  }

  // Route of a matrix-variable solve: the batched pass (f32 / f64) or the wide
  // kernels (f32).  The group threshold needs all columns in one launch (pass) or one panel (wide).
  bool ChooseMatrixRoute(FusedState* f, MatrixRoute mode) {
    const DenseMatrixImpl& L = *f->ls.L_arg_var;
    const DenseMatrixImpl& D = *f->ls.Dinv_arg;
    const DType dt = data_->dtype();
    if (f->m < kMatrixFusedMinRows || L.dtype() != dt || D.dtype() != dt) return false;
    if (f->group && f->group_rows != f->n) return false;
    if (f->sz.alpha_vec.n > 0 && f->sz.alpha_vec.n != f->n * f->cols) return false;
    if (f->sz.beta_vec.n > 0 && f->sz.beta_vec.n != f->n * f->cols) return false;
    if (D.rows() != f->m || D.cols() != f->m) return false;
    const int width = k::LassoBatchWidth(f->m, f->n, dt);
    const bool pass_ok = width > 0 && (!f->group || f->cols <= width);
    const bool wide_ok = dt == F32 && k::LassoWideSupported(f->m, f->n, L.data(), L.rows()) &&
                         (!f->group || f->cols <= WideSweep::PW);
    if (mode == kMatrixPass) f->wide = false;
    else if (mode == kMatrixWide) f->wide = true;
    else f->wide = wide_ok && (f->cols >= BatchWideMin() || !pass_ok);
    return f->wide ? wide_ok : pass_ok;
  }

  // The whitened route.  With Dinv_arg = c X^T X, where X = L^-1 is the inverse Cholesky factor
  // kept by DenseMatrixImpl::Inverse, the forward product of a sweep is
  //   d = A^T Dinv p = c (X A)^T (X p),   X p = X rhs - s_L (X A) v,
  // so the pass streams A_hat = X A (same shape as A, formed once at Init) and its partials reduce
  // to w_hat = X p directly: no m x m matrix is read in the sweep.  f32, one GPU, m >= 2048, n >= 2m.
  bool EnableWhiten(FusedState* f) {
    const DenseMatrixImpl& L = *f->ls.L_arg_var;
    const DenseMatrixImpl& D = *f->ls.Dinv_arg;
    OpCache* cache = CurrentOpCache();
    if (!FusedWhitenEnabled() || cache == nullptr || data_->dtype() != F32 || L.dtype() != F32 ||
        f->m < kWhitenMinRows)
      return false;
    // wide data only: A_hat is formed on the split-f16 matrix cores (about 4x the f32 rounding), and
    // a nearly square A amplifies that in the iterates (10244 x 10260: 4e-5 off the generic path
    // after 200 sweeps, twice the fused path's parity tolerance)
    if (f->n < 2 * f->m) return false;
    if (D.id() == 0 || D.trans() || D.rows() != f->m || D.cols() != f->m || L.rows() != f->m) return false;
    // X belongs to exactly this inverse: the cached entry under D's key holds D's own buffer
    const auto inv = cache->Find(D.id());
    const auto X = cache->Find(FactorInverseKey(D.id()));
    if (!inv || !X || inv->data().data() != D.data().data() || X->rows() != f->m || X->cols() != f->m)
      return false;
    // A_hat is shared like the packed inverse: a warm re-Init and the members of a batch find it
    const uint64_t key = HashCombine(HashCombine(HashCombine(HashCombine(X->id(), 0x3a7),
                                                             reinterpret_cast<uintptr_t>(L.data().data())),
                                                 L.id()),
                                     static_cast<uint64_t>(f->n));
    DVec Ahat;
    if (auto hit = cache->Find(key)) {
      Ahat = hit->data();
    } else {
      Ahat = DVec::Empty(f->m * f->n, F32);
      // X is lower triangular: each tile of the product runs over its own k range
      if (!k::GemmSplitF16KRange(4, f->m, f->n, f->m, 1.0, X->data(), f->m, L.data(), f->m, Ahat, f->m))
        k::Gemm(false, false, f->m, f->n, f->m, 1.0, X->data(), f->m, L.data(), f->m, 0.0, Ahat, f->m);
      cache->Put(key, std::make_shared<DenseMatrixImpl>(Ahat, f->m, f->n, false, 1.0, key));
    }
    if (!k::LassoFusedSupported(f->m, f->n, Ahat, f->m)) return false;
    // X rhs on every Init: parameters re-bind the rhs
    if (f->ls.rhs_arg.n != 0 && f->cols > 1) {  // all columns in one product
      f->rhat = DVec::Empty(f->m * f->cols, F32);
      k::Gemm(false, false, f->m, f->cols, f->m, 1.0, X->data(), f->m, f->ls.rhs_arg, f->m, 0.0, f->rhat, f->m);
    } else if (f->ls.rhs_arg.n != 0) {
      f->rhat = DVec::Empty(f->m, F32);
      k::Gemv(false, f->m, f->m, 1.0, X->data(), f->m, f->ls.rhs_arg, 0.0, f->rhat);
    }
    f->X = X->data();
    f->Ahat = Ahat;
    f->wscale = D.scale();
    f->whiten = true;
    return true;
  }
  // kappa of the pass: x0 = v0 + kappa A^T w (whitened: c A_hat^T w_hat)
  double PassKappa() const { return -fs_.ls.L_arg_var->scale() * (fs_.whiten ? fs_.wscale : 1.0); }

  // The tile-packed copy of the cached inverse; instances of a batch (shared cache) that share
  // the inverse share one copy.
  DVec PackInverse(const DenseMatrixImpl& D, int64_t m) {
    uint64_t key = 0;
    if (shared_cache_ != nullptr) {
      key = HashCombine(HashCombine(reinterpret_cast<uintptr_t>(D.data().data()), 0x9ac4ed), m);
      if (auto hit = shared_cache_->Find(key)) return hit->data();
    }
    DVec P = k::SymvPack(m, D.data(), m);
    if (key) shared_cache_->Put(key, std::make_shared<DenseMatrixImpl>(P, P.n, 1, false, 1.0, key));
    return P;
  }

  // p = rhs_arg - L(arg,var) v0 (all-reduced when sharded), w = Dinv_arg p.
  void FusedForward(bool from_state) {
    FusedState& f = fs_;
    const DenseMatrixImpl& L = *f.ls.L_arg_var;
    if (f.cols > 1) {
      EPS_CHECK(from_state);  // (a sweep's own tail: MatrixSweep)
      // column by column what the vector form does below
      DVec v0 = f.u.Clone();
      k::Axpby(v0, -1.0, f.y0, 1.0);
      k::Axpby(v0, -1.0, f.y1, 1.0);
      k::Axpby(v0, 1.0, f.y0, 1.0);
      const int64_t mk = f.m * f.cols;
      DVec p = f.whiten ? DVec::Empty(mk, v0.dt) : f.p.Slice(0, mk);
      for (int64_t c = 0; c < f.cols; ++c) L.Apply(-1.0, v0.Slice(c * f.n, f.n), 0.0, p.Slice(c * f.m, f.m));
      if (f.ls.rhs_arg.n != 0) k::Axpby(p, 1.0, f.ls.rhs_arg, 1.0);
      if (f.whiten) {
        for (int64_t c = 0; c < f.cols; ++c)
          k::Gemv(false, f.m, f.m, 1.0, f.X, f.m, p.Slice(c * f.m, f.m), 0.0, f.w.Slice(c * f.m, f.m));
      } else {
        ApplyInverseFixed();
      }
      return;
    }
    if (f.whiten) {
      if (from_state) {
        // w_hat = X (rhs - L v0) once, from the current state
        DVec v0 = f.u.Clone();
        k::Axpby(v0, -1.0, f.y0, 1.0);
        k::Axpby(v0, -1.0, f.y1, 1.0);
        k::Axpby(v0, 1.0, f.y0, 1.0);
        L.Apply(-1.0, v0, 0.0, f.p);
        if (f.ls.rhs_arg.n != 0) k::Axpby(f.p, 1.0, f.ls.rhs_arg, 1.0);
        k::Gemv(false, f.m, f.m, 1.0, f.X, f.m, f.p, 0.0, f.w);
      } else {
        k::ReducePartials(f.m, f.grid, f.tpart, -L.scale(), 0.0, f.w, f.rhat.n != 0 ? &f.rhat : nullptr);
      }
      return;
    }
    if (from_state) {
      // v0 = ((u - y0) - y1) + y0 of the current state, then the generic forward product
      DVec v0 = f.u.Clone();
      k::Axpby(v0, -1.0, f.y0, 1.0);
      k::Axpby(v0, -1.0, f.y1, 1.0);
      k::Axpby(v0, 1.0, f.y0, 1.0);
      L.Apply(-1.0, v0, 0.0, f.p);
    }
    const ShardSpec& sh = ShardSpec::Get();
    const bool sharded = sh.active() && sh.IsSharded(f.ls.var_key);
    bool rhs_added = false;
    if (!from_state) {
      // the constant part of the rhs rides in the reduction kernel (same rounding order as the
      // separate axpy: sum first, then + rhs); in a sharded run rank 0 alone contributes it to
      // the sum over ranks - one launch less in a sweep that is launch-latency-bound at N = 8
      const bool have_rhs = f.ls.rhs_arg.n != 0;
      const bool fold = have_rhs && (!sharded || Runtime::Get().comm()->rank() == 0);
      k::ReducePartials(f.m, f.grid, f.tpart, -L.scale(), 0.0, f.p, fold ? &f.ls.rhs_arg : nullptr);
      rhs_added = have_rhs;  // folded here, or by rank 0 into the all-reduced sum
    }
    if (sharded) Runtime::Get().comm()->AllReduceSum(f.p);
    if (f.ls.rhs_arg.n != 0 && !rhs_added) k::Axpby(f.p, 1.0, f.ls.rhs_arg, 1.0);
    const DenseMatrixImpl& D = *f.ls.Dinv_arg;
    Comm* comm = Runtime::Get().comm();
    // EPSILON_HIP_SHARDED_APPLY=replicated: every rank applies the whole inverse instead (no
    // all-gather; m^2 bytes per rank) - the cheaper form when the collective's latency exceeds
    // the apply, to be decided on the machine
    static const bool replicated_apply = [] {
      const char* e = std::getenv("EPSILON_HIP_SHARDED_APPLY");
      return e && e[0] == 'r';
    }();
    if (sharded && comm->size() > 1 && !D.trans() && D.rows() == f.m && !replicated_apply) {
      // The cached inverse is replicated and symmetric: each rank applies only its slab of rows
      // (= columns, read contiguously) and the slices are all-gathered, so the m^2 bytes of the
      // apply are split over the ranks like the data matrix is.
      const int G = comm->size();
      const int64_t per = f.slab;  // multiple of 4, G*per >= m
      const int64_t lo = std::min<int64_t>(f.m, comm->rank() * per);
      const int64_t cnt = std::min<int64_t>(f.m, lo + per) - lo;
      DVec mine = f.wslice;
      if (cnt < per) k::Fill(mine, 0.0);
      if (cnt > 0) {
        DVec slab = D.data().Slice(lo * f.m, cnt * f.m);
        k::Gemv(true, f.m, cnt, D.scale(), slab, f.m, f.p, 0.0, mine.Slice(0, cnt));
      }
      comm->AllGather(mine.data(), f.wpad.data(), static_cast<size_t>(per), f.wpad.dt);
      (void)G;
    } else {
      ApplyInverseFixed();
    }
  }

  // The sharded sweep's tail on the peer window: 2 launches, no collective call.
  void FusedForwardPeer() {
    FusedState& f = fs_;
    const DenseMatrixImpl& L = *f.ls.L_arg_var;
    const DenseMatrixImpl& D = *f.ls.Dinv_arg;
    const PeerView& pv = Runtime::Get().peer()->view();
    k::PeerReduceExchange(pv, f.m, f.grid, f.tpart, -L.scale(),
                          f.ls.rhs_arg.n != 0 ? &f.ls.rhs_arg : nullptr, f.p);
    if (f.peer_slab) {
      const int64_t lo = std::min<int64_t>(f.m, static_cast<int64_t>(pv.rank) * f.slab);
      k::PeerSlabApplyExchange(pv, f.m, f.slab, lo, D.data(), f.m, D.scale(), f.p, f.wpad);
    } else {
      ApplyInverseFixed();
    }
  }

  // w = Dinv p with every buffer at a fixed address (what a captured launch needs)
  void ApplyInverseFixed() {
    FusedState& f = fs_;
    const DenseMatrixImpl& D = *f.ls.Dinv_arg;
    if (f.wide) {
      for (int64_t q = 0; q * f.ws.panel_len < f.w.n; ++q)
        f.ws.ApplyInverse(f.p.Slice(q * f.ws.panel_len, f.ws.panel_len), f.w.Slice(q * f.ws.panel_len, f.ws.panel_len));
      return;
    }
    if (f.cols > 1 && f.symv_packed.n > 0) {
      k::SymvPackedBatch(f.m, D.scale(), f.symv_packed, f.table, static_cast<int>(f.cols), f.symv_work);
      return;
    }
    for (int64_t c = 0; f.cols > 1 && c < f.cols; ++c) {
      DVec pc = f.p.Slice(c * f.m, f.m), wc = f.w.Slice(c * f.m, f.m);
      if (f.symv_work.n > 0) {
        DVec work = f.symv_work.Slice(c * k::SymvWorkspace(f.m), k::SymvWorkspace(f.m));
        k::Symv(f.m, D.scale(), D.data(), f.m, pc, 0.0, wc, &work);
      } else {
        D.Apply(1.0, pc, 0.0, wc);
      }
    }
    if (f.cols > 1) return;
    if (f.symv_packed.n > 0) k::SymvPacked(f.m, D.scale(), f.symv_packed, f.p, 0.0, f.w, &f.symv_work);
    else if (f.symv_work.n > 0) k::Symv(f.m, D.scale(), D.data(), f.m, f.p, 0.0, f.w, &f.symv_work);
    else D.Apply(1.0, f.p, 0.0, f.w);
  }

  // ---- fused sweep of ZERO-term problems --------------------------------------
  // Recognised structure: the last term is a ZERO term over private copies (x', and z' unless the
  // problem has no z: basis pursuit) whose block LDL^T is the projection ZeroProx describes; the
  // other terms are one scaled-zone term on x and at most one on z (which may carry an offset),
  // each tied to its copy by a consensus constraint copy + a var = 0 without a constant.  The
  // sweep is then: the pass over the data matrix (chain 2: back product, column chain, forward
  // product), the row kernel (row chain, the partials' sum, r) - basis pursuit: the partials'
  // reduction alone - and the apply of the cached inverse.  The residual check is the generic one
  // on views of the fused state.  One GPU, every dtype the compute type.
  void TryEnableZeroFused() {
    zfused_ = false;
    const bool mode_auto = FusedZeroAuto();
    const char* env = std::getenv("EPSILON_HIP_FUSED");
    if (fused_ || !mode_auto || (env && env[0] == '0')) return;
    if (ShardSpec::Get().active() || !b_.data().empty()) return;
    const int nc = static_cast<int>(problem_.constraint.size());
    if (nc < 1 || nc > 2 || N_ != nc + 1) return;
    ZeroFusedState f;
    if (!prox_[N_ - 1]->DescribeZeroProjection(&f.zp)) return;
    f.has_z = !f.zp.z_key.empty();
    if (f.has_z != (nc == 2)) return;
    f.ix = f.iz = -1;
    for (int i = 0; i + 1 < N_; ++i) {
      ScaledZoneDesc d;
      if (!prox_[i]->DescribeScaledZoneOffset(&d)) return;
      if (f.ix < 0 && d.constraint_key == f.zp.x_constraint_key && d.g.n == 0) {
        f.sx = d;
        f.ix = i;
      } else if (f.has_z && f.iz < 0 && d.constraint_key == f.zp.z_constraint_key) {
        f.sz = d;
        f.iz = i;
      } else {
        return;
      }
    }
    if (f.ix < 0 || (f.has_z && f.iz < 0)) return;
    const DenseMatrixImpl& L = *f.zp.L_arg_x;
    const DenseMatrixImpl& D = *f.zp.Dinv_arg;
    const DType dt = data_->dtype();
    f.m = L.rows();
    f.n = L.cols();
    if (f.m < kZeroFusedMinRows || L.dtype() != dt || D.dtype() != dt) return;
    if (D.rows() != f.m || D.cols() != f.m) return;
    if (!k::LassoFusedSupported(f.m, f.n, L.data(), L.rows())) return;
    // the consensus constraints: copy + a var = 0, scalar maps, nothing else in their rows
    if (static_cast<int>(A_.data().size()) != 2 * nc) return;
    auto tie = [&](const std::string& ck, const std::string& copy, const std::string& var, int64_t len, double* a) {
      if (copy == var || !A_.has_key(ck, copy) || !A_.has_key(ck, var)) return false;
      if (A_.col(copy).size() != 1 || A_.col(var).size() != 1) return false;
      const LinearMap& A0 = A_(ck, copy);
      const LinearMap& A1 = A_(ck, var);
      if (A0.impl().type() != SCALAR_MATRIX || A1.impl().type() != SCALAR_MATRIX) return false;
      if (GetScalar(A0) != 1.0 || A0.impl().n() != len || A1.impl().n() != len) return false;
      *a = GetScalar(A1);
      return true;
    };
    if (!tie(f.zp.x_constraint_key, f.zp.x_key, f.sx.var_key, f.n, &f.ax)) return;
    if (f.has_z && !tie(f.zp.z_constraint_key, f.zp.z_key, f.sz.var_key, f.m, &f.az)) return;
    auto fits = [&](const DVec& v, int64_t len) { return v.n == 0 || (v.n == len && v.dt == dt); };
    if (!fits(f.zp.rhs_arg, f.m) || !fits(f.sx.alpha_vec, f.n) || !fits(f.sx.beta_vec, f.n)) return;
    if (!fits(f.sz.alpha_vec, f.m) || !fits(f.sz.beta_vec, f.m) || !fits(f.sz.g, f.m)) return;

    // state: u, var, copy, y of the separable term, y of the ZERO term, their previous values -
    // per constraint row, taken over from the generic containers (warm start)
    auto side = [&](int64_t len, const std::string& ck, int term, const std::string& var, const std::string& copy,
                    DVec* all, DVec (&v)[7]) {
      const int64_t pad = (len + 63) / 64 * 64;
      *all = DVec::Zeros(7 * pad, dt);
      for (int q = 0; q < 7; ++q) v[q] = all->Slice(q * pad, len);
      auto take = [&](const DVec& dst, const BlockVector& src, const std::string& key) {
        if (src.has_key(key)) {
          EPS_CHECK(src(key).n == dst.n);
          k::Copy(dst, src(key));
        }
      };
      take(v[0], u_, ck);
      take(v[1], x_[term], var);
      take(v[2], x_[N_ - 1], copy);
      take(v[3], y_[term], ck);
      take(v[4], y_[N_ - 1], ck);
    };
    side(f.n, f.zp.x_constraint_key, f.ix, f.sx.var_key, f.zp.x_key, &f.state_n, f.sn);
    if (f.has_z) side(f.m, f.zp.z_constraint_key, f.iz, f.sz.var_key, f.zp.z_key, &f.state_m, f.sm);
    f.grid = k::LassoFusedGrid(f.m, f.n, dt);
    f.w = DVec::Zeros(f.m, dt);
    f.p = DVec::Zeros(f.m, dt);
    f.tpart = DVec::Empty(static_cast<int64_t>(f.grid) * f.m, dt);
    if (D.symmetric() && f.m >= 1024 && !D.trans()) {
      f.symv_work = DVec::Empty(k::SymvWorkspace(f.m), dt);
      f.symv_packed = PackInverse(D, f.m);
    }
    {
      k::LassoFusedArgs& a = f.pass;
      a.m = f.m;
      a.n = f.n;
      a.lda = L.rows();
      a.A = L.data();
      a.chain = 2;
      a.e0 = f.sn[6];
      k::LassoInstance& s = a.inst;
      s.w = f.w;
      s.tpart = f.tpart;
      s.p = f.p;
      s.rhs = f.zp.rhs_arg;
      s.u = f.sn[0];
      s.x1 = f.sn[1];
      s.x0 = f.sn[2];
      s.y1 = f.sn[3];
      s.y0 = f.sn[4];
      s.y1prev = f.sn[5];
      s.alpha_vec = f.sx.alpha_vec;
      s.beta_vec = f.sx.beta_vec;
      s.kappa = s.pkappa = -L.scale();
      s.Bs = f.sx.Bs;
      s.Cs = f.sx.Cs;
      s.a1 = f.ax;
      s.lam = f.sx.lam;
      s.alpha = f.sx.alpha;
      s.beta = f.sx.beta;
      s.M = f.sx.M;
    }
    if (f.has_z) {
      k::ZeroRowsArgs& r = f.rows;
      r.m = f.m;
      r.nparts = f.grid;
      r.w = f.w;
      r.tpart = f.tpart;
      r.r = f.p;
      r.rhs = f.zp.rhs_arg;
      r.g = f.sz.g;
      r.u = f.sm[0];
      r.z = f.sm[1];
      r.zq = f.sm[2];
      r.yz = f.sm[3];
      r.yq = f.sm[4];
      r.yzprev = f.sm[5];
      r.yqprev = f.sm[6];
      r.alpha_vec = f.sz.alpha_vec;
      r.beta_vec = f.sz.beta_vec;
      r.e = f.zp.e;
      r.pkappa = -L.scale();
      r.Bs = f.sz.Bs;
      r.Cs = f.sz.Cs;
      r.a1 = f.az;
      r.lam = f.sz.lam;
      r.alpha = f.sz.alpha;
      r.beta = f.sz.beta;
      r.M = f.sz.M;
    }
    ResetGraph();
    zs_ = f;
    // the generic containers become views of the fused state
    const std::string &ckx = zs_.zp.x_constraint_key, &ckz = zs_.zp.z_constraint_key;
    x_.assign(N_, BlockVector());
    y_.assign(N_, BlockVector());
    y_prev_.assign(N_, BlockVector());
    u_ = BlockVector();
    u_.Set(ckx, zs_.sn[0]);
    x_[zs_.ix].Set(zs_.sx.var_key, zs_.sn[1]);
    x_[N_ - 1].Set(zs_.zp.x_key, zs_.sn[2]);
    y_[zs_.ix].Set(ckx, zs_.sn[3]);
    y_[N_ - 1].Set(ckx, zs_.sn[4]);
    y_prev_[zs_.ix].Set(ckx, zs_.sn[5]);
    y_prev_[N_ - 1].Set(ckx, zs_.sn[6]);
    if (zs_.has_z) {
      u_.Set(ckz, zs_.sm[0]);
      x_[zs_.iz].Set(zs_.sz.var_key, zs_.sm[1]);
      x_[N_ - 1].Set(zs_.zp.z_key, zs_.sm[2]);
      y_[zs_.iz].Set(ckz, zs_.sm[3]);
      y_[N_ - 1].Set(ckz, zs_.sm[4]);
      y_prev_[zs_.iz].Set(ckz, zs_.sm[5]);
      y_prev_[N_ - 1].Set(ckz, zs_.sm[6]);
    }
    zfused_ = true;
    ZeroForwardFromState();
  }

  // w of the first sweep from the current state, with the generic operators: the sweep up to the
  // ZERO prox's input v (on copies: the state is not touched), then the forward substitution
  // r = (rhs - e v_z) - L(arg, x') v_x and the inverse apply.
  void ZeroForwardFromState() {
    ZeroFusedState& f = zs_;
    BlockVector u = u_;
    for (int i = 0; i < N_; ++i) u -= y_[i];
    for (int i = 0; i + 1 < N_; ++i) {
      u += y_[i];
      u -= A_ * prox_[i]->Apply(u);
    }
    u += y_[N_ - 1];
    if (f.zp.rhs_arg.n != 0) k::Copy(f.p, f.zp.rhs_arg);
    else k::Fill(f.p, 0.0);
    if (f.has_z) k::Axpby(f.p, -f.zp.e, u(f.zp.z_constraint_key), 1.0);
    f.zp.L_arg_x->Apply(-1.0, u(f.zp.x_constraint_key), 1.0, f.p);
    ZeroApplyInverse();
  }

  void ZeroApplyInverse() {
    ZeroFusedState& f = zs_;
    const DenseMatrixImpl& D = *f.zp.Dinv_arg;
    if (f.symv_packed.n > 0) k::SymvPacked(f.m, D.scale(), f.symv_packed, f.p, 0.0, f.w, &f.symv_work);
    else D.Apply(1.0, f.p, 0.0, f.w);
  }

  void ZeroSweep() {
    ZeroFusedState& f = zs_;
    k::LassoFusedPass(f.pass);
    if (f.has_z)
      k::ZeroFusedRows(f.rows);
    else
      k::ReducePartials(f.m, f.grid, f.tpart, f.pass.inst.pkappa, 0.0, f.p,
                        f.zp.rhs_arg.n != 0 ? &f.zp.rhs_arg : nullptr);
    ZeroApplyInverse();
  }

  void ResetGraph() {
    if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    graph_exec_ = nullptr;
    graph_ = nullptr;
    graph_len_ = 0;
    ResetGenericGraph();
  }

  void ResetGenericGraph() { gg_.Reset(); }

  std::vector<BlockVector*> StateHandles() {  // (the "previous" handles first: see SweepGraph::Capture)
    std::vector<BlockVector*> h;
    for (int i = 0; i < N_; ++i) h.push_back(&y_prev_[i]);
    h.push_back(&u_);
    for (int i = 0; i < N_; ++i) h.push_back(&x_[i]);
    for (int i = 0; i < N_; ++i) h.push_back(&y_[i]);
    return h;
  }

  bool GenericGraphWanted(int count) {
    if (fused_ || zfused_ || !capture_safe_ || eager_sweeps_ < SweepGraph::EagerSweepsFirst() ||
        static_cast<int>(y_prev_.size()) != N_)
      return false;
    return gg_.Wanted(count, StateHandles());
  }

  // The sweeps between two residual checks replayed from one hipGraph: a sharded sweep is 3
  // short dependent launches (~60 us of kernels at 8 ranks), so the host's per-launch cost and
  // jitter would otherwise sit on the critical path.  Iterates are bit-identical to the eager
  // launches (same kernels, same arguments; the exchange tags come from a device counter).
  void SweepBatch(int count) override {
    static const int mode = [] {  // EPSILON_HIP_GRAPH: 0 never, 1 always (fused), default: peer mode
      const char* e = std::getenv("EPSILON_HIP_GRAPH");
      return e ? std::atoi(e) : -1;
    }();
    Runtime& rt = Runtime::Get();
    if (GenericGraphWanted(count) && gg_.Run(count, StateHandles(), static_cast<size_t>(N_), [this] { Sweep(); })) return;
    const ShardSpec& sh = ShardSpec::Get();
    const bool rccl_in_sweep = fused_ && !fs_.use_peer && sh.active() && sh.IsSharded(fs_.ls.var_key);
    const bool fixed_buffers = (fs_.use_peer && fs_.peer_slab) || fs_.symv_work.n > 0 || fs_.whiten || fs_.wide;
    const bool want = fused_ && !rccl_in_sweep && fixed_buffers &&
                      (mode == 1 || (mode != 0 && fs_.use_peer));
    if (!want || count < 2 || rt.profiling()) {
      for (int i = 0; i < count; ++i) Sweep();
      if (!fused_) eager_sweeps_ += count;
      return;
    }
    if (graph_exec_ == nullptr || graph_len_ != count) {
      ResetGraph();
      hipStream_t s = rt.stream();
      EPS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      rt.set_capturing(true);
      try {
        for (int i = 0; i < count; ++i) FusedSweep();
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

  // The pass's arguments with the instance as the kernels read it, once per Init: EnableWhiten has
  // decided the matrix, kappa, p and rhs by now.  Only the peer exchange's epoch is set per sweep.
  void BuildPass() {
    FusedState& f = fs_;
    const DenseMatrixImpl& L = *f.ls.L_arg_var;
    k::LassoFusedArgs& a = f.pass;
    a.m = f.m;
    a.n = f.n;
    a.lda = f.whiten ? f.m : L.rows();
    a.A = f.whiten ? f.Ahat : L.data();
    k::LassoInstance& s = a.inst;
    s.w = f.w;
    s.tpart = f.tpart;
    s.u = f.u;
    s.x0 = f.x0;
    s.x1 = f.x1;
    s.y0 = f.y0;
    s.y1 = f.y1;
    s.y1prev = f.y1prev;
    s.alpha_vec = f.sz.alpha_vec;
    s.beta_vec = f.sz.beta_vec;
    // whitened route: the reduction writes w_hat itself, with X rhs folded in
    s.p = f.whiten ? f.w : f.p;
    s.rhs = f.whiten ? f.rhat : f.ls.rhs_arg;
    s.kappa = PassKappa();
    s.pkappa = -L.scale();
    s.Bs = f.sz.Bs;
    s.Cs = f.sz.Cs;
    s.a1 = f.a1;
    s.lam = f.sz.lam;
    s.alpha = f.sz.alpha;
    s.beta = f.sz.beta;
    s.M = f.sz.M;
    if (f.cols == 1) return;
    // a matrix variable: column c is member c, the slices of `inst` at its offsets; the table is
    // uploaded here, so that a sweep makes no upload and no host synchronisation
    f.members.assign(static_cast<size_t>(f.cols), s);
    f.rhs_aligned = true;
    for (int64_t c = 0; c < f.cols; ++c) {
      k::LassoInstance& mb = f.members[static_cast<size_t>(c)];
      auto col = [&](const DVec& v, int64_t len) { return v.n > 0 ? v.Slice(c * len, len) : v; };
      mb.w = col(s.w, f.m);
      mb.p = col(s.p, f.m);
      mb.rhs = col(s.rhs, f.m);
      if (!f.wide) mb.tpart = col(s.tpart, static_cast<int64_t>(f.grid) * f.m);
      else mb.tpart = mb.w;  // (not read on the wide route: its partials are panels of WideSweep)
      for (DVec k::LassoInstance::*v : {&k::LassoInstance::u, &k::LassoInstance::x0, &k::LassoInstance::x1,
                                       &k::LassoInstance::y0, &k::LassoInstance::y1, &k::LassoInstance::y1prev,
                                       &k::LassoInstance::alpha_vec, &k::LassoInstance::beta_vec})
        mb.*v = col(s.*v, f.n);
      if (mb.rhs.n > 0) f.rhs_aligned = f.rhs_aligned && reinterpret_cast<uintptr_t>(mb.rhs.data()) % 16 == 0;
    }
    std::vector<const k::LassoInstance*> v;
    for (const auto& mb : f.members) v.push_back(&mb);
    k::LassoBatchUpload(v, data_->dtype(), &f.table);
  }

  // A matrix variable's sweep: its columns through the batched or the wide kernels.
  void MatrixSweep() {
    FusedState& f = fs_;
    const int K = static_cast<int>(f.cols);
    const double* group_lam = f.group ? &f.sz.lam : nullptr;
    if (f.wide) {
      constexpr int PW = WideSweep::PW;
      for (int first = 0; first < K; first += PW) {
        const int nk = std::min(PW, K - first);
        const uint64_t live = nk == 64 ? ~uint64_t(0) : (uint64_t(1) << nk) - 1;
        const int64_t off = static_cast<int64_t>(first) * f.m;
        f.ws.Run(f.table, first, nk, live, f.w.Slice(off, f.ws.panel_len),
                 f.whiten ? DVec() : f.p.Slice(off, f.ws.panel_len), group_lam);
      }
      return;
    }
    const int width = k::LassoBatchWidth(f.m, f.n, data_->dtype());
    for (int first = 0; first < K; first += width)
      k::LassoBatchPass(f.m, f.n, f.pass.lda, f.pass.A, f.table, first, std::min(width, K - first), group_lam);
    k::ReducePartialsBatch(f.m, f.grid, f.table, K, data_->dtype(), f.rhs_aligned);
    if (!f.whiten) ApplyInverseFixed();
  }

  void FusedSweep() {
    FusedState& f = fs_;
    if (f.cols > 1) {
      MatrixSweep();
      return;
    }
    if (f.use_peer) {
      f.pass.epoch = Runtime::Get().peer()->view().epoch;
      k::LassoFusedPass(f.pass);
      FusedForwardPeer();
      return;
    }
    k::LassoFusedPass(f.pass);
    FusedForward(/*from_state=*/false);
  }

  void Sweep() override {  // :135-147
    if (fused_) {
      FusedSweep();
      return;
    }
    if (zfused_) {
      ZeroSweep();
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

  // ---- residual check of the fused structure: one launch, splittable for pipelining ------------
  // With A_ = [a0 I, a1 I] (a0 = 1), b_ empty and N = 2 the quantities of :178-217 are
  //   ||A x_i|| = ||y_i||,  r = ||y0 + y1||,  s = rho ||A_0^T (y1 - y1_prev)|| = rho ||y1 - y1_prev||,
  //   ||A^T u||^2 = (a0^2 + a1^2) ||u||^2.
  bool PipelinedChecks() const override {
    static const bool off = [] {
      const char* e = std::getenv("EPSILON_HIP_PIPELINE_CHECKS");
      return e && e[0] == '0';
    }();
    const ShardSpec& sh = ShardSpec::Get();
    return fused_ && !off && !(sh.active() && sh.consensus_terms());
  }
  void BeginResiduals() override {
    Runtime& rt = Runtime::Get();
    rt.ResetSlots();
    LaunchFusedNorms();
    rt.FetchSlotsAsync();
  }
  // the check's six scalars into the next six slots
  void LaunchFusedNorms() {
    Runtime& rt = Runtime::Get();
    FusedState& f = fs_;
    norm_slot_ = rt.NewSlot();
    for (int k = 1; k < 6; ++k) rt.NewSlot();
    const ShardSpec& sh = ShardSpec::Get();
    const bool sharded = sh.active() && sh.IsSharded(f.ls.var_key);
    k::LassoFusedNorms(f.u, f.y0, f.y1, f.y1prev,
                       sharded ? rt.ShardSlotPtr(norm_slot_) : rt.SlotPtr(norm_slot_), f.norm_work,
                       f.use_peer ? rt.peer()->device_error_word() : nullptr);
  }
  void EndResiduals() override {
    Runtime::Get().WaitSlots();
    FinishFusedCheck();
  }
  // the residuals and the state of the check from its fetched scalars
  void FinishFusedCheck() {
    Runtime& rt = Runtime::Get();
    // a timed-out exchange on ANY rank shows in the all-reduced sixth value: every rank raises at
    // the same check, none is left waiting in a collective the others never enter
    if (rt.SlotValue(norm_slot_ + 5) > 0) {
      rt.Sync();
      if (rt.peer()) rt.peer()->ClearError();
      EPS_FATAL("peer exchange: a poll timed out on at least one rank (a peer did not deliver its part)");
    }
    const double ny0 = rt.SlotValue(norm_slot_), ny1 = rt.SlotValue(norm_slot_ + 1),
                 nr = rt.SlotValue(norm_slot_ + 2), ns = rt.SlotValue(norm_slot_ + 3),
                 nu = rt.SlotValue(norm_slot_ + 4);
    const double rho = params_.rho;
    const double max_norm = std::fmax(std::sqrt(ny0), std::sqrt(ny1));
    FinishResiduals(std::sqrt(nr), rho * std::sqrt(ns),
                    params_.abs_tol * std::sqrt(static_cast<double>(m_)) + params_.rel_tol * max_norm,
                    params_.abs_tol * std::sqrt(static_cast<double>(n_)) +
                        params_.rel_tol * rho * std::sqrt((1.0 + fs_.a1 * fs_.a1) * nu));
  }
  void SaveSnapshot() override { k::Copy(fs_.snapshot, fs_.state_all); }
  void RestoreSnapshot() override {
    Runtime::Get().Sync();  // let the discarded sweeps drain
    if (Runtime::Get().peer()) Runtime::Get().peer()->CheckError();
    k::Copy(fs_.state_all, fs_.snapshot);
  }

  void ComputeResiduals() override {  // :178-217
    if (fused_) {
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
  struct FusedState {
    LeastSquaresDesc ls;
    ScaledZoneDesc sz;
    double a1 = 0;
    int64_t m = 0, n = 0;
    int grid = 0;
    int64_t slab = 0;  // rows of the cached inverse applied per rank (sharded runs)
    bool use_peer = false;   // exchanges ride in the sweep's kernels (peer window), not in RCCL
    bool peer_slab = false;  // ... and the inverse is applied by row slabs
    DVec u, x0, x1, y0, y1, y1prev, w, p, tpart, wpad, wslice;
    DVec symv_work;  // fixed workspace of the symmetric inverse apply (empty: not that form)
    DVec symv_packed;  // the cached inverse's lower tiles, each contiguous (empty: apply from the matrix)
    DVec state_all, snapshot;  // u, x0, x1, y0, y1, y1prev in one buffer; its copy at a check
    DVec norm_work;            // partials + ticket of the one-launch residual norms
    bool whiten = false;       // the pass streams Ahat = X A, w holds X p (EnableWhiten)
    double wscale = 1;         // c of Dinv_arg = c X^T X
    DVec X, Ahat, rhat;        // L^-1 of the inverse, X A (ld m), X rhs_arg (empty: no rhs)
    k::LassoFusedArgs pass;    // what the pass and a batch read of all this (BuildPass)
    // matrix variable (n x cols under I_cols (x) A): its columns are members of the batched kernels
    int64_t cols = 1;
    bool group = false;      // the threshold is the group shrinkage of the rows (weight sz.lam)
    int64_t group_rows = 0;
    bool wide = false;       // the wide route (f32): w and p are whole panels of 64 members
    bool rhs_aligned = true;
    std::vector<k::LassoInstance> members;
    DVec table;              // their descriptors on the device (LassoBatchUpload)
    WideSweep ws;
  };
  struct ZeroFusedState {
    ZeroProjectionDesc zp;
    ScaledZoneDesc sx, sz;  // the separable terms on x and on z
    bool has_z = false;
    int ix = -1, iz = -1;   // their positions among the objective terms
    double ax = 0, az = 0;  // constraint maps of x and z (their copies': 1)
    int64_t m = 0, n = 0;
    int grid = 0;
    // u, var, copy, y of the separable term, y of the ZERO term, the two previous y: slices of one
    // buffer per side (n: the x constraint's rows, m: the z constraint's)
    DVec state_n, state_m, sn[7], sm[7];
    DVec w, p, tpart, symv_work, symv_packed;
    k::LassoFusedArgs pass;
    k::ZeroRowsArgs rows;
  };
  bool fused_ = false;
  bool zfused_ = false;
  FusedState fs_;
  ZeroFusedState zs_;
  int norm_slot_ = 0;
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t graph_exec_ = nullptr;
  int graph_len_ = 0;
  SweepGraph gg_;  // the generic operator path's sweeps between two checks as one hipGraph
  bool capture_safe_ = false;  // every prox operator of the problem is (ProxOperator::CaptureSafe)
  int eager_sweeps_ = 0;       // operators build lazily on their first Apply: one eager sweep first
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
    TryEnableFused();
    gg_.Reset();
    gg_.ClearFailure();
    capture_safe_ = constr_prox_ != nullptr && constr_prox_->CaptureSafe();
    for (const auto& op : prox_) capture_safe_ = capture_safe_ && op->CaptureSafe();
    eager_sweeps_ = 0;
    Runtime::Get().Sync();
    init_seconds_ = Now() - t0;
  }

  BlockVector GetSolution() override { return x_; }

  // the sweeps between two residual checks: one hipGraph where the operators allow it (SweepGraph)
  void SweepBatch(int count) override {
    if (!fused_ && capture_safe_ && eager_sweeps_ >= SweepGraph::EagerSweepsFirst()) {
      const std::vector<BlockVector*> state = {&z_prev_, &x_, &z_, &u_};
      if (gg_.Wanted(count, state) && gg_.Run(count, state, 1, [this] { Sweep(); })) return;
    }
    for (int i = 0; i < count; ++i) Sweep();
    if (!fused_) eager_sweeps_ += count;
  }

 protected:
  // ---- fused sweep for "least squares + separable threshold" problems, two-block form -----------
  // [SUM_SQUARE with a dense argument map, scaled-zone prox], one constraint a0 x0 + a1 x1 = 0
  // without a constant: the x-updates are the same two operators as in the multi-block driver, the
  // z-update is the closed-form projection onto the constraint, so one pass over the data matrix
  // does a whole sweep (kernels_fused.hip, chain 1).  f32 and f64, single GPU.
  void TryEnableFused() {
    fused_ = false;
    const char* env = std::getenv("EPSILON_HIP_FUSED");
    if (env && env[0] == '0') return;
    if (N_ != 2 || problem_.constraint.size() != 1) return;
    if (ShardSpec::Get().active()) return;
    if (!constr_H_.b.data().empty()) return;
    FusedState f;
    if (!prox_[0]->DescribeLeastSquares(&f.ls) || !prox_[1]->DescribeScaledZone(&f.sz)) return;
    if (f.ls.cols != 1) return;  // matrix variables: the multi-block driver only
    if (f.ls.var_key == f.sz.var_key) return;
    const std::string ck = affine::constraint_key(0);
    const BlockMatrix& H = constr_H_.A;
    if (H.data().size() != 2 || !H.has_key(ck, f.ls.var_key) || !H.has_key(ck, f.sz.var_key)) return;
    const LinearMap& H0 = H(ck, f.ls.var_key);
    const LinearMap& H1 = H(ck, f.sz.var_key);
    if (H0.impl().type() != SCALAR_MATRIX || H1.impl().type() != SCALAR_MATRIX) return;
    f.a0 = GetScalar(H0);
    f.a1 = GetScalar(H1);
    if (f.a0 == 0 || f.a1 == 0) return;
    const DenseMatrixImpl& L = *f.ls.L_arg_var;
    if (L.trans()) return;
    f.m = L.rows();
    f.n = L.cols();
    if (H0.impl().n() != f.n || H1.impl().n() != f.n) return;
    if (!k::LassoFusedSupported(f.m, f.n, L.data(), L.rows())) return;
    if (f.ls.rhs_arg.n != 0 && f.ls.rhs_arg.n != f.m) return;
    const DenseMatrixImpl& D = *f.ls.Dinv_arg;
    if (D.trans() || D.rows() != f.m) return;
    const DType dt = data_->dtype();
    if ((f.sz.alpha_vec.n > 0 && f.sz.alpha_vec.dt != dt) || (f.sz.beta_vec.n > 0 && f.sz.beta_vec.dt != dt)) return;
    if (L.dtype() != dt || D.dtype() != dt) return;
    auto state = [&](const BlockVector& src, const std::string& key) {
      DVec v = DVec::Zeros(f.n, dt);
      if (src.has_key(key)) k::Copy(v, src(key));
      return v;
    };
    f.x0 = state(x_, f.ls.var_key);
    f.x1 = state(x_, f.sz.var_key);
    f.z0 = state(z_, f.ls.var_key);
    f.z1 = state(z_, f.sz.var_key);
    f.u0 = state(u_, f.ls.var_key);
    f.u1 = state(u_, f.sz.var_key);
    f.z0p = DVec::Zeros(f.n, dt);
    f.z1p = DVec::Zeros(f.n, dt);
    f.p = DVec::Zeros(f.m, dt);
    f.w = DVec::Zeros(f.m, dt);
    f.grid = k::LassoFusedGrid(f.m, f.n, dt);
    f.tpart = DVec::Empty(static_cast<int64_t>(f.grid) * f.m, dt);
    {
      // the pass's arguments, once per Init; chain 1 reads the state arrays as
      // u -> u0, y0 -> z0, y1 -> z1, y1prev -> z0_prev, e0 -> u1, e1 -> z1_prev
      k::LassoFusedArgs& a = f.pass;
      a.m = f.m;
      a.n = f.n;
      a.lda = L.rows();
      a.A = L.data();
      a.chain = 1;
      a.a0 = f.a0;
      a.e0 = f.u1;
      a.e1 = f.z1p;
      k::LassoInstance& s = a.inst;
      s.w = f.w;
      s.tpart = f.tpart;
      s.u = f.u0;
      s.x0 = f.x0;
      s.x1 = f.x1;
      s.y0 = f.z0;
      s.y1 = f.z1;
      s.y1prev = f.z0p;
      s.alpha_vec = f.sz.alpha_vec;
      s.beta_vec = f.sz.beta_vec;
      s.p = f.p;
      s.rhs = f.ls.rhs_arg;
      s.kappa = s.pkappa = -L.scale();
      s.Bs = f.sz.Bs;
      s.Cs = f.sz.Cs;
      s.a1 = f.a1;
      s.lam = f.sz.lam;
      s.alpha = f.sz.alpha;
      s.beta = f.sz.beta;
      s.M = f.sz.M;
    }
    fs_ = f;
    // the generic containers become views of the fused state
    auto two = [&](const DVec& a, const DVec& b) {
      BlockVector v;
      v.Set(fs_.ls.var_key, a);
      v.Set(fs_.sz.var_key, b);
      return v;
    };
    x_ = two(fs_.x0, fs_.x1);
    z_ = two(fs_.z0, fs_.z1);
    u_ = two(fs_.u0, fs_.u1);
    z_prev_ = two(fs_.z0p, fs_.z1p);
    fused_ = true;
    // p = rhs_arg - L(arg, var) (z0 - u0) of the current state, w = Dinv_arg p
    DVec v0 = fs_.z0.Clone();
    k::Axpby(v0, -1.0, fs_.u0, 1.0);
    L.Apply(-1.0, v0, 0.0, fs_.p);
    if (fs_.ls.rhs_arg.n != 0) k::Axpby(fs_.p, 1.0, fs_.ls.rhs_arg, 1.0);
    D.Apply(1.0, fs_.p, 0.0, fs_.w);
  }

  void FusedSweep() {
    FusedState& f = fs_;
    const DenseMatrixImpl& L = *f.ls.L_arg_var;
    k::LassoFusedPass(f.pass);
    k::ReducePartials(f.m, f.grid, f.tpart, -L.scale(), 0.0, f.p,
                      f.ls.rhs_arg.n != 0 ? &f.ls.rhs_arg : nullptr);
    f.ls.Dinv_arg->Apply(1.0, f.p, 0.0, f.w);
  }

  void Sweep() override {  // :97-112
    if (fused_) {
      FusedSweep();
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
  struct FusedState {
    LeastSquaresDesc ls;
    ScaledZoneDesc sz;
    double a0 = 1, a1 = -1;
    int64_t m = 0, n = 0;
    int grid = 0;
    DVec x0, x1, z0, z1, u0, u1, z0p, z1p, p, w, tpart;
    k::LassoFusedArgs pass;  // the pass's view of all this, built in TryEnableFused
  };
  bool fused_ = false;
  FusedState fs_;
  BlockVector x_, z_, u_, z_prev_;
  SweepGraph gg_;
  bool capture_safe_ = false;
  int eager_sweeps_ = 0;
};

// ---------------------------------------------------------------------------------------------------
// Batched solves: one group of fused instances sharing A and the cached inverse
// ---------------------------------------------------------------------------------------------------
namespace {

// Run()'s iteration schedule without the pipelining, for a group of batched members: sweeps up to
// the next multiple of the epoch, then one residual check of every active member with ONE fetch of
// their scalars.  A member that stops is frozen: it leaves `active`, and `stopped(gone)` is told
// which ones left (only when some did).  Members still active at the end get Run()'s
// max-iterations status.
template <class Sweep, class Stopped>
void RunGroupSchedule(const std::vector<ProxADMMSolver*>& g, std::vector<int>* active, Sweep sweep,
                      Stopped stopped) {
  Runtime& rt = Runtime::Get();
  const pb::SolverParams& params = g[0]->params();
  const int epoch = params.epoch_iterations > 0 ? params.epoch_iterations : 1;
  const int max_it = params.max_iterations;
  int iter = 0;
  while (!active->empty() && iter < max_it) {
    int batch = 1;
    while ((iter + batch - 1) % epoch != 0) ++batch;
    if (batch > max_it - iter) batch = max_it - iter;
    for (int s = 0; s < batch; ++s) sweep();
    iter += batch - 1;
    if (iter % epoch == 0) {
      rt.ResetSlots();
      for (int i : *active) g[i]->BatchLaunchNorms(iter);
      rt.FetchSlots();
      std::vector<int> still, gone;
      for (int i : *active) (g[i]->BatchFinishCheck() ? gone : still).push_back(i);
      active->swap(still);
      if (!gone.empty()) stopped(gone);
    }
    ++iter;
  }
  for (int i : *active) g[i]->BatchFinishMaxIterations(iter);
}

// The group's loop time, once the stream has drained.
void FinishGroup(const std::vector<ProxADMMSolver*>& g, double t0) {
  Runtime::Get().Sync();
  const double loop = Now() - t0;
  for (ProxADMMSolver* s : g) s->BatchSetLoopTime(loop);
}

void RunFusedGroup(const std::vector<ProxADMMSolver*>& g, const std::vector<k::LassoInstance>& mem) {
  const double t0 = Now();
  ProxADMMSolver& lead = *g[0];
  const DType dt = lead.data()->dtype();
  SetCurrentDType(dt);
  int64_t lda = 0;
  const DVec& A = lead.batch_matrix(&lda);
  const int64_t m = mem[0].p.n, n = mem[0].u.n;
  const int width = k::LassoBatchWidth(m, n, dt);
  const int grid = lead.batch_grid();
  const DVec& P = lead.batch_packed_inverse();
  const double dscale = lead.batch_inverse_scale();
  bool rhs_aligned = true;
  for (const auto& mb : mem)
    if (mb.rhs.n > 0) rhs_aligned = rhs_aligned && reinterpret_cast<uintptr_t>(mb.rhs.data()) % 16 == 0;
  const int K = static_cast<int>(g.size());
  DVec symv_work = P.n > 0 ? DVec::Empty(K * k::SymvWorkspace(m), dt) : DVec();

  std::vector<int> active(K);
  for (int i = 0; i < K; ++i) active[i] = i;
  DVec table;
  auto upload = [&] {
    std::vector<const k::LassoInstance*> v;
    for (int i : active) v.push_back(&mem[i]);
    k::LassoBatchUpload(v, dt, &table);
  };
  upload();
  auto sweep = [&] {
    const int na = static_cast<int>(active.size());
    for (int first = 0; first < na; first += width)
      k::LassoBatchPass(m, n, lda, A, table, first, std::min(width, na - first));
    k::ReducePartialsBatch(m, grid, table, na, dt, rhs_aligned);
    if (lead.batch_whitened()) {
      // the reduction wrote every member's w_hat: no inverse apply
    } else if (P.n > 0) {
      k::SymvPackedBatch(m, dscale, P, table, na, symv_work);
    } else {
      for (int i : active) g[i]->BatchApplyInverse();  // D.Apply / Symv: per instance
    }
  };
  // the stopped ones are frozen: drop their descriptors
  RunGroupSchedule(g, &active, sweep, [&](const std::vector<int>&) {
    if (!active.empty()) upload();
  });
  FinishGroup(g, t0);
}

// EPSILON_HIP_BATCH_WIDE (eps_set_option "batch_wide"), read per batch: "1" sends eligible groups
// to the wide route below.
bool BatchWideEnabled() {
  const char* e = std::getenv("EPSILON_HIP_BATCH_WIDE");
  if (e == nullptr || std::strcmp(e, "0") == 0) return false;
  EPS_CHECK_MSG(std::strcmp(e, "1") == 0, "batch_wide must be 0 or 1, got " << e);
  return true;
}

// Smallest group the wide route takes.  Measured crossovers against the batched pass on MI355X
// (DESIGN.md 3.8), rounded up to a multiple of 8.
constexpr int kWideMin = 8;
int BatchWideMin() {  // EPSILON_HIP_BATCH_WIDE_MIN: tuning knob (the crossover measurements)
  const char* e = std::getenv("EPSILON_HIP_BATCH_WIDE_MIN");
  return e && std::atoi(e) >= 2 ? std::atoi(e) : kWideMin;
}

// The wide route (kernels_fused_wide.hip): RunFusedGroup's schedule and residual checks, with the
// sweep of a panel of up to 64 members as back product + chain, forward product and reduction on
// the f32 matrix instruction.  The members' w (and p) live in instance-major panels for the
// duration; a member keeps its slot until the group ends and a stopped one is masked, so no
// summation order depends on who else is still iterating.  Not bit-identical to the single solve.
void RunWideGroup(const std::vector<ProxADMMSolver*>& g, const std::vector<k::LassoInstance>& mem_in) {
  const double t0 = Now();
  ProxADMMSolver& lead = *g[0];
  SetCurrentDType(F32);
  int64_t lda = 0;
  const DVec& A = lead.batch_matrix(&lda);
  const int64_t m = mem_in[0].p.n, n = mem_in[0].u.n;
  const bool whiten = lead.batch_whitened();
  const DenseMatrixImpl& D = lead.batch_inverse();
  const int K = static_cast<int>(g.size());
  constexpr int PW = WideSweep::PW;
  const int npanels = (K + PW - 1) / PW;
  WideSweep ws;
  ws.Init(m, n, A, lda, whiten, &D);
  const int64_t panel_len = ws.panel_len;

  std::vector<k::LassoInstance> mem = mem_in;
  DVec Wall = DVec::Zeros(npanels * panel_len, F32);
  DVec Pall = whiten ? DVec() : DVec::Zeros(npanels * panel_len, F32);
  for (int i = 0; i < K; ++i) {
    for (const DVec* v : {&mem[i].u, &mem[i].x0, &mem[i].x1, &mem[i].y0, &mem[i].y1, &mem[i].y1prev})
      EPS_CHECK_MSG(reinterpret_cast<uintptr_t>(v->data()) % 16 == 0, "wide batch: unaligned state vector");
    DVec slot = Wall.Slice(static_cast<int64_t>(i) * m, m);
    k::Copy(slot, mem_in[i].w);  // FusedForward's result at Init
    mem[i].w = slot;
    mem[i].p = whiten ? slot : Pall.Slice(static_cast<int64_t>(i) * m, m);
  }
  DVec table;
  {
    std::vector<const k::LassoInstance*> v;
    for (const auto& mb : mem) v.push_back(&mb);
    k::LassoBatchUpload(v, F32, &table);
  }
  std::vector<uint64_t> live(npanels, 0);
  std::vector<int> active(K);
  for (int i = 0; i < K; ++i) {
    active[i] = i;
    live[i / PW] |= uint64_t(1) << (i % PW);
  }
  auto sweep = [&] {
    for (int p = 0; p < npanels; ++p) {
      if (live[p] == 0) continue;
      const int first = p * PW, nk = std::min(PW, K - first);
      ws.Run(table, first, nk, live[p], Wall.Slice(p * panel_len, panel_len),
             whiten ? DVec() : Pall.Slice(p * panel_len, panel_len));
    }
  };
  // frozen: their slots are masked from here on
  RunGroupSchedule(g, &active, sweep, [&](const std::vector<int>& gone) {
    for (int i : gone) live[i / PW] &= ~(uint64_t(1) << (i % PW));
  });
  // every member's own w holds what its next sweep would read
  for (int i = 0; i < K; ++i) k::Copy(mem_in[i].w, mem[i].w);
  FinishGroup(g, t0);
}

}  // namespace

std::vector<bool> RunFusedBatches(const std::vector<Solver*>& solvers) {
  std::vector<bool> ran(solvers.size(), false);
  const bool wide = BatchWideEnabled();
  std::map<std::vector<uint64_t>, std::vector<size_t>> groups;
  std::vector<k::LassoInstance> mem(solvers.size());
  std::vector<std::vector<uint64_t>> order;  // groups in order of their first instance
  for (size_t i = 0; i < solvers.size(); ++i) {
    auto* s = dynamic_cast<ProxADMMSolver*>(solvers[i]);
    std::vector<uint64_t> key;
    if (s == nullptr || !s->BatchView(&mem[i], &key)) continue;
    auto& members = groups[key];
    if (members.empty()) order.push_back(key);
    members.push_back(i);
  }
  for (const auto& key : order) {
    const std::vector<size_t>& idx = groups[key];
    if (idx.size() < 2) continue;  // alone: the single path is the same solve, with pipelined checks
    std::vector<ProxADMMSolver*> g;
    std::vector<k::LassoInstance> gm;
    for (size_t i : idx) {
      g.push_back(static_cast<ProxADMMSolver*>(solvers[i]));
      gm.push_back(mem[i]);
    }
    int64_t lda = 0;
    const DVec& A = g[0]->batch_matrix(&lda);
    if (wide && static_cast<int>(g.size()) >= BatchWideMin() && g[0]->data()->dtype() == F32 &&
        k::LassoWideSupported(gm[0].p.n, gm[0].u.n, A, lda))
      RunWideGroup(g, gm);
    else
      RunFusedGroup(g, gm);
    for (size_t i : idx) ran[i] = true;
  }
  return ran;
}

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
