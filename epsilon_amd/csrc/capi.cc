// extern "C" boundary, the product ABI: see include/epsilon_hip.h for the contract of each function
// and the reference interface it replaces (python/epopt/solvemodule.cc).  The per-operator test
// entries are in capi_test.cc, the micro-benchmarks in capi_bench.cc, what they share in capi_util.h.
#include <cstdio>
#include <cstring>

#include "block.h"
#include "capi_util.h"
#include "comm.h"
#include "options.h"

using namespace eps;
using namespace eps::capi;

namespace {

thread_local std::string g_last_error;
int g_dtype_option = -1;  // -1: take EPSILON_HIP_DTYPE / default

void InsertBlobs(DataMap* dm, const eps_blob* data, size_t ndata, bool own_host) {
  bool device_blobs = false;
  for (size_t i = 0; i < ndata; ++i) {
    EPS_CHECK_MSG(data[i].key != nullptr, "data blob without a key");
    Blob b;
    b.ptr = data[i].ptr;
    b.len = data[i].len;
    b.kind = data[i].kind;
    EPS_CHECK_MSG(b.kind >= 0 && b.kind <= 2, "bad blob kind " << b.kind);
    if (b.kind != 0) device_blobs = true;
    if (own_host) dm->InsertOwned(data[i].key, b);
    else dm->Insert(data[i].key, b);
  }
  // Borrowed device memory is read on this library's own non-blocking stream, which has no
  // ordering with whatever stream produced it: wait for the device once, here.
  if (device_blobs) {
    Runtime::Get();
    EPS_HIP(hipDeviceSynchronize());
  }
}

void FillResult(Solver* solver, eps_result* r) {
  r->status = solver->status().Serialize();
  BlockVector x = solver->GetSolution();
  for (const auto& var : GetVariables(solver->problem())) {  // solvemodule.cc:166-176
    r->ids.push_back(var.first);
    r->values.push_back(x(var.first).ToHostArray());
  }
}

void LogToStdout(const std::string& msg) {  // reference util/logging.cc:10-13 -> PySys_WriteStdout
  std::fputs(msg.c_str(), stdout);
  std::fputc('\n', stdout);
  std::fflush(stdout);
}

// count contiguous signals of len samples; checked before anything touches the device
eps::k::Segs BatchSegs(size_t len, size_t count) {
  const size_t limit = (size_t(1) << 31) - 1;  // (by division: the product may not fit a size_t)
  EPS_CHECK_MSG(len == 0 || count <= (limit - 1) / len, "tv1d: len * count must be below 2^31");
  eps::k::Segs S;
  S.count = static_cast<int64_t>(count);
  S.len = static_cast<int64_t>(len);
  S.seg_stride = S.len;
  S.elem_stride = 1;
  return S;
}

// one signal of n samples (its size limit is k::Tv1dSeg's check, after the data is on the device)
eps::k::Segs OneSignal(size_t n) {
  eps::k::Segs S;
  S.len = S.seg_stride = static_cast<int64_t>(n);
  return S;
}

// The bodies of the eps_tv1d* entries behind their argument checks.  Host data goes through device
// buffers of the configured dtype; device data (of a checked `kind`) is borrowed, and the call
// waits for the device on both sides of the prox.
void Tv1dOnHostData(const double* v, double* x, const eps::k::Segs& S, double lam) {
  const int64_t n = S.len * S.count;
  const DType dt = ConfiguredDType();
  DVec vd = DVec::FromHost(v, n, dt);
  DVec xd = DVec::Empty(n, dt);
  eps::k::Tv1dSeg(xd, vd, lam, S);
  xd.ToHost(x);
}

void Tv1dOnDeviceData(const void* v_dev, void* x_dev, const eps::k::Segs& S, int kind, double lam, int* levels) {
  const int64_t n = S.len * S.count;
  const DType dt = kind == EPS_BLOB_DEVICE_F32 ? F32 : F64;
  DVec v = DVec::Borrow(const_cast<void*>(v_dev), n, dt);
  DVec x = DVec::Borrow(x_dev, n, dt);
  Runtime::Get();
  EPS_HIP(hipDeviceSynchronize());  // v may have been produced on any stream of the caller
  const int depth = eps::k::Tv1dSeg(x, v, lam, S);
  Runtime::Get().Sync();
  if (levels) *levels = depth;
}

}  // namespace

void eps::capi::ClearLastError() { g_last_error.clear(); }

void eps::capi::SetLastError(const char* what) { g_last_error = what; }

DType eps::capi::ConfiguredDType() {
  if (g_dtype_option >= 0) return static_cast<DType>(g_dtype_option);
  const char* e = opt::Raw(opt::kDtype);
  if (e && (std::strcmp(e, "f64") == 0 || std::strcmp(e, "float64") == 0)) return F64;
  return F32;
}

std::shared_ptr<DataMap> eps::capi::MakeDataMap(const eps_blob* data, size_t ndata, DType dt, bool own_host) {
  auto dm = std::make_shared<DataMap>(dt);
  InsertBlobs(dm.get(), data, ndata, own_host);
  return dm;
}

extern "C" {

const char* eps_last_error(void) { return g_last_error.c_str(); }

const char* eps_version(void) { return "epsilon_hip 0.1 gfx950"; }

int eps_set_option(const char* key, const char* value) {
  return Guard([&] {
    EPS_CHECK(key != nullptr && value != nullptr);
    if (std::strcmp(key, "dtype") == 0) {
      if (std::strcmp(value, "f32") == 0) g_dtype_option = F32;
      else if (std::strcmp(value, "f64") == 0) g_dtype_option = F64;
      else EPS_FATAL("dtype must be f32 or f64, got " << value);
    } else if (std::strcmp(key, "profile_filter") == 0) {
      Runtime::Get().set_prof_filter(value);
    } else {
      opt::Set(key, value);  // every key stored in the environment: the table of options.cc
    }
  });
}

int eps_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return count;
}

int eps_solve(const void* problem, size_t problem_len, const void* solver_params,
              size_t solver_params_len, const eps_blob* data, size_t ndata,
              const eps_param* params, size_t nparams, eps_result** out) {
  return Guard([&] {
    EPS_CHECK(out != nullptr);
    *out = nullptr;
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    pb::Problem p = pb::ParseProblem(problem, problem_len);
    pb::SolverParams sp = pb::ParseSolverParams(solver_params, solver_params_len);
    auto dm = MakeDataMap(data, ndata, dt);
    for (size_t i = 0; i < nparams; ++i)
      dm->SetParameter(params[i].id, pb::ParseConstant(params[i].constant_proto, params[i].len));
    std::unique_ptr<Solver> solver = CreateSolver(std::move(p), dm, sp);
    solver->set_log(LogToStdout);
    solver->Solve();
    std::unique_ptr<eps_result> r(new eps_result);
    FillResult(solver.get(), r.get());
    *out = r.release();
  });
}

int eps_solve_batch(const void* const* problems, const size_t* problem_lens, size_t count,
                    const void* solver_params, size_t solver_params_len, const eps_blob* data,
                    size_t ndata, const eps_param* const* params, const size_t* nparams,
                    eps_result** out) {
  if (out != nullptr && problems != nullptr)
    for (size_t k = 0; k < count; ++k) out[k] = nullptr;
  return Guard([&] {
    EPS_CHECK_MSG(count > 0, "eps_solve_batch: count is 0");
    EPS_CHECK_MSG(problems != nullptr && problem_lens != nullptr && out != nullptr,
                  "eps_solve_batch: null problems / problem_lens / out");
    EPS_CHECK_MSG(nparams == nullptr || params != nullptr, "eps_solve_batch: nparams without params");
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    pb::SolverParams sp = pb::ParseSolverParams(solver_params, solver_params_len);
    // every instance parsed before any work starts
    std::vector<pb::Problem> probs(count);
    std::vector<std::vector<std::pair<std::string, pb::Constant>>> binds(count);
    for (size_t k = 0; k < count; ++k) {
      try {
        EPS_CHECK_MSG(problems[k] != nullptr, "null problem");
        probs[k] = pb::ParseProblem(problems[k], problem_lens[k]);
        const size_t np = nparams ? nparams[k] : 0;
        EPS_CHECK_MSG(np == 0 || params[k] != nullptr, "nparams " << np << " with a null parameter array");
        for (size_t i = 0; i < np; ++i) {
          EPS_CHECK_MSG(params[k][i].id != nullptr, "parameter " << i << " without an id");
          binds[k].emplace_back(params[k][i].id,
                                pb::ParseConstant(params[k][i].constant_proto, params[k][i].len));
        }
      } catch (const std::exception& e) {
        EPS_FATAL("eps_solve_batch: instance " << k << ": " << e.what());
      }
    }
    // one data map (one upload of each constant) and one memo of Gram products / inverses for all
    auto dm = MakeDataMap(data, ndata, dt);
    OpCache shared;
    std::vector<std::unique_ptr<Solver>> solvers(count);
    std::vector<std::unique_ptr<eps_result>> results(count);
    std::vector<Solver*> pending;
    std::vector<size_t> pending_index;
    for (size_t k = 0; k < count; ++k) {
      try {
        dm->ClearParameters();
        for (const auto& b : binds[k]) dm->SetParameter(b.first, b.second);
        solvers[k] = CreateSolver(std::move(probs[k]), dm, sp);
        solvers[k]->set_log(LogToStdout);
        solvers[k]->set_shared_cache(&shared);
        solvers[k]->Init();
        pending.push_back(solvers[k].get());
        pending_index.push_back(k);
      } catch (const std::exception& e) {
        EPS_FATAL("eps_solve_batch: instance " << k << ": " << e.what());
      }
    }
    // fused instances that share A and the inverse run together; every other one alone, with
    // its own parameters bound again (its operators may read them on first use)
    const std::vector<bool> ran = RunFusedBatches(pending);
    for (size_t i = 0; i < pending.size(); ++i) {
      const size_t k = pending_index[i];
      try {
        if (!ran[i]) {
          dm->ClearParameters();
          for (const auto& b : binds[k]) dm->SetParameter(b.first, b.second);
          solvers[k]->Run(-1);
        }
        results[k].reset(new eps_result);
        FillResult(solvers[k].get(), results[k].get());
        solvers[k].reset();
      } catch (const std::exception& e) {
        EPS_FATAL("eps_solve_batch: instance " << k << ": " << e.what());
      }
    }
    for (size_t k = 0; k < count; ++k) out[k] = results[k].release();
  });
}

int eps_eval_prox(const void* f_expr, size_t f_expr_len, double lambda, const eps_blob* data,
                  size_t ndata, const eps_blob* v, size_t nv, eps_result** out) {
  return Guard([&] {
    EPS_CHECK(out != nullptr);
    *out = nullptr;
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    pb::Expression e = pb::ParseExpression(f_expr, f_expr_len);
    auto dm = MakeDataMap(data, ndata, dt);
    BlockVector vin;
    for (size_t i = 0; i < nv; ++i) {
      EPS_CHECK_MSG(v[i].kind == EPS_BLOB_HOST && v[i].len % sizeof(double) == 0,
                    "eval_prox: v must be host float64 bytes");
      vin.Set(v[i].key, DVec::FromHost(static_cast<const double*>(v[i].ptr),
                                       static_cast<int64_t>(v[i].len / sizeof(double)), dt));
    }
    BlockVector x = EvalProx(e, lambda, dm.get(), vin);
    std::unique_ptr<eps_result> r(new eps_result);
    for (const auto& kv : x.data()) {  // GetVariableMap, solvemodule.cc:45-56
      r->ids.push_back(kv.first);
      r->values.push_back(kv.second.ToHostArray());
    }
    *out = r.release();
  });
}

int eps_result_status(const eps_result* r, const void** bytes, size_t* len) {
  if (!r || !bytes || !len) return 1;
  *bytes = r->status.data();
  *len = r->status.size();
  return 0;
}

size_t eps_result_num_vars(const eps_result* r) { return r ? r->ids.size() : 0; }

int eps_result_var(const eps_result* r, size_t i, const char** id, const double** values,
                   size_t* count) {
  if (!r || i >= r->ids.size()) return 1;
  if (id) *id = r->ids[i].c_str();
  if (values) *values = r->values[i].data();
  if (count) *count = r->values[i].size();
  return 0;
}

int eps_result_copy_var(const eps_result* r, size_t i, void* dst, size_t bytes) {
  if (!r || i >= r->ids.size() || dst == nullptr || bytes != r->values[i].size() * sizeof(double)) return 1;
  ParallelHostCopy(dst, r->values[i].data(), bytes);
  return 0;
}

void eps_result_free(eps_result* r) { delete r; }

int eps_solver_create(const void* problem, size_t problem_len, const void* solver_params,
                      size_t solver_params_len, const eps_blob* data, size_t ndata,
                      eps_solver** out) {
  return Guard([&] {
    EPS_CHECK(out != nullptr);
    *out = nullptr;
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    std::unique_ptr<eps_solver> s(new eps_solver);
    s->dtype = dt;
    s->data = MakeDataMap(data, ndata, dt, /*own_host=*/true);
    s->solver = CreateSolver(pb::ParseProblem(problem, problem_len), s->data,
                             pb::ParseSolverParams(solver_params, solver_params_len));
    s->solver->set_log(LogToStdout);
    *out = s.release();
  });
}

int eps_solver_set_parameter(eps_solver* s, const char* id, const void* constant_proto,
                             size_t len, const eps_blob* data, size_t ndata) {
  return Guard([&] {
    EPS_CHECK(s != nullptr && id != nullptr);
    InsertBlobs(s->data.get(), data, ndata, /*own_host=*/true);
    s->data->SetParameter(id, pb::ParseConstant(constant_proto, len));
  });
}

int eps_solver_init(eps_solver* s) {
  return Guard([&] {
    EPS_CHECK(s != nullptr);
    SetCurrentDType(s->dtype);
    s->solver->Init();
  });
}

int eps_solver_run(eps_solver* s, int max_sweeps, int* sweeps_done) {
  return Guard([&] {
    EPS_CHECK(s != nullptr);
    SetCurrentDType(s->dtype);
    int done = s->solver->Run(max_sweeps);
    if (sweeps_done) *sweeps_done = done;
  });
}

int eps_solver_result(eps_solver* s, eps_result** out) {
  return Guard([&] {
    EPS_CHECK(s != nullptr && out != nullptr);
    *out = nullptr;
    SetCurrentDType(s->dtype);
    std::unique_ptr<eps_result> r(new eps_result);
    FillResult(s->solver.get(), r.get());
    *out = r.release();
  });
}

int eps_solver_timing(const eps_solver* s, double* init_seconds, double* loop_seconds) {
  if (!s) return 1;
  if (init_seconds) *init_seconds = s->solver->init_seconds();
  if (loop_seconds) *loop_seconds = s->solver->loop_seconds();
  return 0;
}

void eps_solver_destroy(eps_solver* s) {
  try {
    delete s;
  } catch (...) {
  }
}

int eps_comm_unique_id(void* out128) {
  return Guard([&] {
    EPS_CHECK(out128 != nullptr);
    GetRcclUniqueId(out128);
  });
}

int eps_comm_init_rccl(int rank, int world, const void* id128) {
  return Guard([&] {
    EPS_CHECK(id128 != nullptr && world >= 1 && rank >= 0 && rank < world);
    Runtime& rt = Runtime::Get();
    delete rt.peer();
    rt.set_peer(nullptr);
    delete rt.comm();
    rt.set_comm(nullptr);
    rt.set_comm(NewRcclComm(rank, world, id128));
  });
}

int eps_comm_init_callback(int rank, int world, eps_allreduce_fn fn, void* ctx) {
  return Guard([&] {
    EPS_CHECK(fn != nullptr && world >= 1 && rank >= 0 && rank < world);
    Runtime& rt = Runtime::Get();
    delete rt.peer();
    rt.set_peer(nullptr);
    delete rt.comm();
    rt.set_comm(nullptr);
    rt.set_comm(NewHostCallbackComm(rank, world, fn, ctx));
  });
}

int eps_comm_warmup(size_t count) {
  return Guard([&] {
    Runtime& rt = Runtime::Get();
    EPS_CHECK_MSG(rt.comm() != nullptr, "eps_comm_warmup: no communicator");
    // one all-reduce and one all-gather of `count` floats: RCCL sets up its rings / buffers on
    // the first collective of each kind, which should not land inside a timed solver Init
    const int64_t n = static_cast<int64_t>(count < 1 ? 1 : count);
    DVec a = DVec::Full(n, 1.0, F32);
    rt.comm()->AllReduceSum(a);
    DVec g = DVec::Zeros(n * rt.comm()->size(), F32);
    rt.comm()->AllGather(a.data(), g.data(), static_cast<size_t>(n), F32);
    rt.Sync();
    std::vector<double> h = a.Slice(0, 1).ToHost();
    EPS_CHECK_MSG(h[0] == static_cast<double>(rt.comm()->size()),
                  "eps_comm_warmup: all-reduce of ones gave " << h[0] << " on "
                                                              << rt.comm()->size() << " ranks");
  });
}

int eps_comm_enable_peer(size_t slot_floats, int rehearse_ranks, int* enabled) {
  return Guard([&] {
    Runtime& rt = Runtime::Get();
    EPS_CHECK_MSG(rt.comm() != nullptr, "eps_comm_enable_peer: no communicator");
    if (enabled) *enabled = 0;
    rt.Sync();
    delete rt.peer();
    rt.set_peer(nullptr);
    std::string why;
    PeerExchange* px = PeerExchange::Create(rt.comm(), static_cast<int64_t>(slot_floats ? slot_floats : 16384),
                                            rehearse_ranks, &why);
    if (px == nullptr) {
      g_last_error = "peer window not available: " + why;  // informational: the call succeeds
      return;
    }
    rt.set_peer(px);
    if (enabled) *enabled = 1;
  });
}

int eps_comm_disable_peer(void) {
  return Guard([&] {
    Runtime& rt = Runtime::Get();
    rt.Sync();
    delete rt.peer();
    rt.set_peer(nullptr);
  });
}

int eps_comm_shutdown(void) {
  return Guard([&] {
    Runtime& rt = Runtime::Get();
    rt.Sync();
    delete rt.peer();
    rt.set_peer(nullptr);
    delete rt.comm();
    rt.set_comm(nullptr);
    ShardSpec::Get().Clear();
  });
}

int eps_shard_keys(const char* const* keys, size_t nkeys) {
  return Guard([&] {
    ShardSpec::Get().Clear();
    for (size_t i = 0; i < nkeys; ++i) ShardSpec::Get().Add(keys[i]);
  });
}

int eps_shard_consensus_terms(int on) {
  return Guard([&] { ShardSpec::Get().set_consensus_terms(on != 0); });
}

int eps_block_solve_stats(double* max_condition, int* max_refine_steps, int reset) {
  return Guard([&] {
    BlockSolveStats& st = BlockSolveStats::Get();
    if (max_condition) *max_condition = st.max_condition;
    if (max_refine_steps) *max_refine_steps = st.max_refine_steps;
    if (reset) st.Reset();
  });
}

int eps_profile_enable(int on) {
  return Guard([&] { Runtime::Get().set_profiling(on != 0); });
}

int eps_profile_reset(void) {
  return Guard([&] { Runtime::Get().ProfReset(); });
}

int eps_profile_dump(char* buf, size_t cap) {
  return Guard([&] {
    EPS_CHECK(buf != nullptr && cap > 0);
    Runtime& rt = Runtime::Get();
    rt.ProfCollect();
    std::string out;
    for (const auto& kv : rt.prof_totals()) {
      char line[256];
      std::snprintf(line, sizeof(line), "%s %lld %.6f\n", kv.first.c_str(),
                    static_cast<long long>(kv.second.count), kv.second.ms);
      out += line;
    }
    std::strncpy(buf, out.c_str(), cap - 1);
    buf[cap - 1] = 0;
  });
}

int eps_tv1d(const double* v, size_t n, double lam, double* x) {
  return Guard([&] { Tv1dOnHostData(v, x, OneSignal(n), lam); });
}

int eps_tv1d_device(const void* v_dev, void* x_dev, size_t n, int kind, double lam, int* levels) {
  return Guard([&] {
    EPS_CHECK(v_dev != nullptr && x_dev != nullptr);
    EPS_CHECK_MSG(kind == EPS_BLOB_DEVICE_F32 || kind == EPS_BLOB_DEVICE_F64, "bad kind");
    Tv1dOnDeviceData(v_dev, x_dev, OneSignal(n), kind, lam, levels);
  });
}

int eps_tv1d_batch(const double* v, size_t len, size_t count, double lam, double* x) {
  return Guard([&] {
    const k::Segs S = BatchSegs(len, count);
    if (S.len * S.count == 0) return;
    EPS_CHECK(v != nullptr && x != nullptr);
    Tv1dOnHostData(v, x, S, lam);
  });
}

int eps_tv1d_batch_device(const void* v_dev, void* x_dev, size_t len, size_t count, int kind, double lam,
                          int* levels) {
  return Guard([&] {
    EPS_CHECK_MSG(kind == EPS_BLOB_DEVICE_F32 || kind == EPS_BLOB_DEVICE_F64, "bad kind");
    const k::Segs S = BatchSegs(len, count);
    EPS_CHECK(S.len * S.count == 0 || (v_dev != nullptr && x_dev != nullptr));
    Tv1dOnDeviceData(v_dev, x_dev, S, kind, lam, levels);
  });
}

}  // extern "C"
