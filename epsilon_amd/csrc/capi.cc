// extern "C" boundary: see include/epsilon_hip.h for the contract of each function and the
// reference interface it replaces (python/epopt/solvemodule.cc).
#include "../../include/epsilon_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "admm.h"
#include "block.h"
#include "comm.h"
#include "kernels.h"
#include "linear_map.h"
#include "options.h"
#include "wire.h"

using namespace eps;

struct eps_result {
  std::string status;
  std::vector<std::string> ids;
  std::vector<HostArray> values;  // not value-initialised, huge pages from 64 MB
};

struct eps_solver {
  std::shared_ptr<DataMap> data;
  std::unique_ptr<Solver> solver;
  DType dtype;
};

namespace {

thread_local std::string g_last_error;
int g_dtype_option = -1;  // -1: take EPSILON_HIP_DTYPE / default

DType ConfiguredDType() {
  if (g_dtype_option >= 0) return static_cast<DType>(g_dtype_option);
  const char* e = opt::Raw(opt::kDtype);
  if (e && (std::strcmp(e, "f64") == 0 || std::strcmp(e, "float64") == 0)) return F64;
  return F32;
}

template <class F> int Guard(F f) {
  try {
    g_last_error.clear();
    f();
    return 0;
  } catch (const std::exception& e) {
    g_last_error = e.what();
  } catch (...) {
    g_last_error = "unknown error";
  }
  // leave no half-finished GPU work behind
  (void)hipGetLastError();
  return 1;
}

// own_host: copy host blobs (solver handles outlive the call that passes them; the one-shot entry
// points read the caller's memory in place, it is theirs for the duration of the call).
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

std::shared_ptr<DataMap> MakeDataMap(const eps_blob* data, size_t ndata, DType dt,
                                     bool own_host = false) {
  auto dm = std::make_shared<DataMap>(dt);
  InsertBlobs(dm.get(), data, ndata, own_host);
  return dm;
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

LinearMap ParseMap(const void* bytes, size_t len, DataMap* dm) {
  pb::LinearMap p = pb::ParseLinearMap(bytes, len);
  return BuildLinearMap(p, dm);
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


// ---- eps_test_block_solve --------------------------------------------------------------------------

HostArray HostArrayOf(const std::vector<double>& v) {
  HostArray a;
  a.n = v.size();
  a.mem = AllocHostBuffer(std::max<size_t>(v.size(), 1) * sizeof(double));
  if (!v.empty()) std::memcpy(a.data(), v.data(), v.size() * sizeof(double));
  return a;
}

void PutValues(eps_result* r, const std::string& id, const std::vector<double>& v) {
  r->ids.push_back(id);
  r->values.push_back(HostArrayOf(v));
}

double FillValue(uint64_t bound) { return bound == kFillMax ? -1.0 : static_cast<double>(bound); }

// [ImplType, m, n, ImplType of the two factors of a Kronecker product (else -1, -1), values of the
// m x n map in column-major order]
void PutBlocks(eps_result* r, const char* name, const BlockMatrix& M) {
  for (const auto& col : M.data())
    for (const auto& row : col.second) {
      const LinearMapImpl& B = row.second.impl();
      std::vector<double> v = {static_cast<double>(B.type()), static_cast<double>(B.m()),
                               static_cast<double>(B.n()), -1.0, -1.0};
      if (B.type() == KRONECKER_PRODUCT) {
        const auto& K = static_cast<const KroneckerProductImpl&>(B);
        v[3] = static_cast<double>(K.A().impl().type());
        v[4] = static_cast<double>(K.B().impl().type());
      }
      const std::vector<double> dense = ToDense(B, MapDType(B, CurrentDType()))->data().ToHost();
      EPS_CHECK(static_cast<int64_t>(dense.size()) == B.m() * B.n());
      v.insert(v.end(), dense.begin(), dense.end());
      PutValues(r, std::string(name) + "\t" + row.first + "\t" + col.first, v);
    }
}

void PutVector(eps_result* r, const char* name, const BlockVector& x) {
  for (const auto& kv : x.data()) {
    r->ids.push_back(std::string(name) + "\t" + kv.first);
    r->values.push_back(kv.second.ToHostArray());
  }
}

// The argument checks of eps_test_block_solve: everything that can be decided from the payloads
// alone, so that no device work starts on arguments that do not fit together.
struct BlockSolveArgs {
  enum Mode { FILL, FACTOR, SOLVE, FORWARD, BACK } mode;
  std::vector<pb::LinearMap> maps;          // blocks[i], parsed
  std::map<std::string, int64_t> dim;       // size of every row / column key
  std::vector<std::string> keys;            // substitution order (FORWARD / BACK)
};

BlockSolveArgs CheckBlockSolveArgs(const char* mode, const eps_block* blocks, size_t nblocks,
                                   const eps_blob* rhs, size_t nrhs, const char* const* keys,
                                   size_t nkeys) {
  const char* const fn = "eps_test_block_solve: ";
  BlockSolveArgs a;
  EPS_CHECK_MSG(mode != nullptr, fn << "mode is null");
  const std::string m(mode);
  if (m == "fill") a.mode = BlockSolveArgs::FILL;
  else if (m == "factor") a.mode = BlockSolveArgs::FACTOR;
  else if (m == "solve") a.mode = BlockSolveArgs::SOLVE;
  else if (m == "forward") a.mode = BlockSolveArgs::FORWARD;
  else if (m == "back") a.mode = BlockSolveArgs::BACK;
  else EPS_FATAL(fn << "mode must be fill, factor, solve, forward or back, got " << m);
  const bool substitution = a.mode == BlockSolveArgs::FORWARD || a.mode == BlockSolveArgs::BACK;
  EPS_CHECK_MSG(blocks != nullptr && nblocks > 0, fn << "blocks is null or empty");
  EPS_CHECK_MSG(nrhs == 0 || rhs != nullptr, fn << "rhs is null with nrhs " << nrhs);
  EPS_CHECK_MSG(nkeys == 0 || keys != nullptr, fn << "keys is null with nkeys " << nkeys);
  std::set<std::pair<std::string, std::string>> seen;
  auto set_dim = [&](const std::string& key, int64_t d, size_t i) {
    auto ins = a.dim.insert(std::make_pair(key, d));
    EPS_CHECK_MSG(ins.first->second == d, fn << "block " << i << " gives key " << key << " the size " << d
                                             << ", an earlier block " << ins.first->second);
  };
  for (size_t i = 0; i < nblocks; ++i) {
    EPS_CHECK_MSG(blocks[i].row != nullptr && blocks[i].col != nullptr, fn << "block " << i << " has a null key");
    const std::string row(blocks[i].row), col(blocks[i].col);
    EPS_CHECK_MSG(seen.insert(std::make_pair(row, col)).second,
                  fn << "block (" << row << ", " << col << ") is given twice");
    EPS_CHECK_MSG(blocks[i].linear_map != nullptr && blocks[i].len > 0,
                  fn << "block (" << row << ", " << col << ") has an empty LinearMap payload");
    try {
      a.maps.push_back(pb::ParseLinearMap(blocks[i].linear_map, blocks[i].len));
    } catch (const std::exception& e) {
      EPS_FATAL(fn << "block (" << row << ", " << col << "): malformed LinearMap: " << e.what());
    }
    const pb::LinearMap& p = a.maps.back();
    EPS_CHECK_MSG(p.linear_map_type != pb::LinearMap::UNKNOWN && p.m > 0 && p.n > 0,
                  fn << "block (" << row << ", " << col << "): malformed LinearMap: type "
                     << p.linear_map_type << ", " << p.m << " x " << p.n);
    set_dim(row, p.m, i);
    set_dim(col, p.n, i);
  }
  if (substitution) {
    std::set<std::string> order;
    for (size_t i = 0; i < nkeys; ++i) {
      EPS_CHECK_MSG(keys[i] != nullptr, fn << "keys[" << i << "] is null");
      EPS_CHECK_MSG(order.insert(keys[i]).second, fn << "key " << keys[i] << " is given twice in keys");
      a.keys.push_back(keys[i]);
    }
    EPS_CHECK_MSG(!a.keys.empty(), fn << "mode " << m << " needs the key order in keys");
    for (const auto& kv : a.dim)
      EPS_CHECK_MSG(order.count(kv.first) != 0, fn << "block key " << kv.first << " is not in keys");
  } else {
    // symmetric in structure: both triangles given, every key a column
    for (const auto& rc : seen)
      EPS_CHECK_MSG(seen.count(std::make_pair(rc.second, rc.first)) != 0,
                    fn << "block (" << rc.first << ", " << rc.second << ") has no transpose ("
                       << rc.second << ", " << rc.first << ")");
  }
  std::set<std::string> rhs_seen;
  for (size_t i = 0; i < nrhs; ++i) {
    EPS_CHECK_MSG(rhs[i].key != nullptr, fn << "rhs " << i << " has a null key");
    const std::string key(rhs[i].key);
    EPS_CHECK_MSG(rhs_seen.insert(key).second, fn << "rhs key " << key << " is given twice");
    if (substitution && a.dim.count(key) == 0) {
      // a key of the order that no block touches: its block passes through unchanged
      EPS_CHECK_MSG(std::find(a.keys.begin(), a.keys.end(), key) != a.keys.end(),
                    fn << "rhs key " << key << " is not in keys");
    } else {
      EPS_CHECK_MSG(a.dim.count(key) != 0, fn << "rhs key " << key << " is not a key of the matrix");
    }
    EPS_CHECK_MSG(rhs[i].kind == EPS_BLOB_HOST && rhs[i].len % sizeof(double) == 0 &&
                      (rhs[i].len == 0 || rhs[i].ptr != nullptr),
                  fn << "rhs " << key << " must be host float64 bytes");
    auto d = a.dim.find(key);
    EPS_CHECK_MSG(d == a.dim.end() || static_cast<int64_t>(rhs[i].len / sizeof(double)) == d->second,
                  fn << "rhs " << key << " has " << rhs[i].len / sizeof(double) << " entries, the matrix "
                     << d->second);
  }
  return a;
}

// ---- eps_test_dense_op -----------------------------------------------------------------------------

// The argument checks of eps_test_dense_op, host only: the op, and that every operand the op reads
// is there with the length its dimensions need, so that no launcher is given a short buffer.
struct DenseOpArgs {
  enum Op { GEMV_N, GEMV_T, SYMV, SYMV_PACKED, REDUCE_PARTIALS, SUMSQ, SUMSQ_DIFF, DOT, AXPBY, DIAG_MUL } op;
  bool reduction = false;  // the result is a slot, not a vector
  bool use_a = false, use_x = false, use_y = false, use_add = false;
};

DenseOpArgs CheckDenseOpArgs(const eps_dense_op* g, const double* out, const double* out2) {
  const char* const fn = "eps_test_dense_op: ";
  DenseOpArgs a;
  EPS_CHECK_MSG(g != nullptr, fn << "args is null");
  EPS_CHECK_MSG(g->op != nullptr, fn << "op is null");
  const std::string op(g->op);
  if (op == "gemv_n") a.op = DenseOpArgs::GEMV_N;
  else if (op == "gemv_t") a.op = DenseOpArgs::GEMV_T;
  else if (op == "symv") a.op = DenseOpArgs::SYMV;
  else if (op == "symv_packed") a.op = DenseOpArgs::SYMV_PACKED;
  else if (op == "reduce_partials") a.op = DenseOpArgs::REDUCE_PARTIALS;
  else if (op == "sumsq") a.op = DenseOpArgs::SUMSQ;
  else if (op == "sumsq_diff") a.op = DenseOpArgs::SUMSQ_DIFF;
  else if (op == "dot") a.op = DenseOpArgs::DOT;
  else if (op == "axpby") a.op = DenseOpArgs::AXPBY;
  else if (op == "diag_mul") a.op = DenseOpArgs::DIAG_MUL;
  else
    EPS_FATAL(fn << "op must be gemv_n, gemv_t, symv, symv_packed, reduce_partials, sumsq, sumsq_diff, dot, "
                    "axpby or diag_mul, got " << op);
  EPS_CHECK_MSG(out != nullptr, fn << "out is null");
  EPS_CHECK_MSG(a.op != DenseOpArgs::SYMV_PACKED || out2 != nullptr, fn << "out2 is null");
  EPS_CHECK_MSG(g->rows >= 0, fn << "rows is negative: " << g->rows);
  const bool gemv = a.op == DenseOpArgs::GEMV_N || a.op == DenseOpArgs::GEMV_T;
  const bool symv = a.op == DenseOpArgs::SYMV || a.op == DenseOpArgs::SYMV_PACKED;
  if (gemv) EPS_CHECK_MSG(g->cols >= 0, fn << "cols is negative: " << g->cols);
  struct Operand { const char* name; const double* p; int64_t len, off; };
  const Operand A = {"a", g->a, g->a_len, g->a_off}, X = {"x", g->x, g->x_len, g->x_off},
                Y = {"y", g->y, g->y_len, g->y_off}, ADD = {"add", g->add, g->add_len, g->add_off};
  for (const Operand& o : {A, X, Y, ADD}) {
    EPS_CHECK_MSG(o.len >= 0, fn << o.name << "_len is negative: " << o.len);
    EPS_CHECK_MSG(o.off >= 0, fn << o.name << "_off is negative: " << o.off);
  }
  auto need = [&](const Operand& o, int64_t len) {
    EPS_CHECK_MSG(len == 0 || o.p != nullptr, fn << o.name << " is null");
    EPS_CHECK_MSG(o.len == len, fn << o.name << " has " << o.len << " entries, the dimensions need " << len);
  };
  const int64_t n = g->rows;
  int64_t a_need = 0, x_need = 0, y_need = n, add_need = 0;
  if (gemv || symv) {
    const int64_t cols = symv ? n : g->cols;
    EPS_CHECK_MSG(g->lda >= n, fn << "lda " << g->lda << " < rows " << n);
    EPS_CHECK_MSG(cols == 0 || g->lda <= (INT64_MAX - n) / cols, fn << "lda * cols overflows");
    a_need = cols == 0 ? 0 : (cols - 1) * g->lda + n;
    x_need = a.op == DenseOpArgs::GEMV_T ? n : cols;
    y_need = a.op == DenseOpArgs::GEMV_T ? cols : n;
    a.use_a = a.use_x = a.use_y = true;
  } else if (a.op == DenseOpArgs::REDUCE_PARTIALS) {
    EPS_CHECK_MSG(g->nparts >= 1, fn << "nparts must be at least 1, got " << g->nparts);
    EPS_CHECK_MSG(n == 0 || g->nparts <= INT64_MAX / n, fn << "nparts * rows overflows");
    a_need = static_cast<int64_t>(g->nparts) * n;
    add_need = g->with_add ? n : 0;
    a.use_a = a.use_y = true;
    a.use_add = g->with_add != 0;
  } else if (a.op == DenseOpArgs::SUMSQ) {
    a.reduction = a.use_x = true;
    x_need = n;
    y_need = 0;
  } else if (a.op == DenseOpArgs::SUMSQ_DIFF || a.op == DenseOpArgs::DOT) {
    a.reduction = a.use_x = a.use_y = true;
    x_need = n;
  } else if (a.op == DenseOpArgs::AXPBY) {
    a.use_x = !g->alias_xy;
    a.use_y = true;
    x_need = g->alias_xy ? 0 : n;
  } else {  // DIAG_MUL
    a.use_a = a.use_x = a.use_y = true;
    a_need = x_need = n;
  }
  if (a.use_a) need(A, a_need);
  if (a.use_x) need(X, x_need);
  if (a.use_y) need(Y, y_need);
  if (a.use_add) need(ADD, add_need);
  return a;
}

// `len` host doubles as the slice [off + guard, off + guard + len) of a device allocation of the
// configured dtype whose other elements hold EPS_DENSE_OP_SENTINEL; *whole receives the allocation.
DVec PlaceOperand(const double* p, int64_t len, int64_t off, int64_t guard, DType dt, DVec* whole) {
  std::vector<double> h(static_cast<size_t>(off + 2 * guard + len), EPS_DENSE_OP_SENTINEL);
  if (len > 0) std::memcpy(h.data() + off + guard, p, static_cast<size_t>(len) * sizeof(double));
  *whole = DVec::FromHost(h.data(), static_cast<int64_t>(h.size()), dt);
  return whole->Slice(off + guard, len);
}

// ---- eps_test_gemm_op ------------------------------------------------------------------------------

// The argument checks of eps_test_gemm_op, host only, and the operand lengths the dimensions need.
struct GemmOpArgs {
  enum Op { GEMM, GEMM_BATCHED, MAT_COPY, ADD_DIAG, SYMMETRIZE, COL_ABS_SUMS, KRON } op;
  bool use_a = false, use_b = false, use_c = false, use_d = false;
  int64_t out_len = 0;  // values between the guards of the result
};

GemmOpArgs CheckGemmOpArgs(const eps_gemm_op* g, const double* out, const char* route, size_t route_cap) {
  const char* const fn = "eps_test_gemm_op: ";
  GemmOpArgs a;
  EPS_CHECK_MSG(g != nullptr, fn << "args is null");
  EPS_CHECK_MSG(g->op != nullptr, fn << "op is null");
  const std::string op(g->op);
  if (op == "gemm") a.op = GemmOpArgs::GEMM;
  else if (op == "gemm_batched") a.op = GemmOpArgs::GEMM_BATCHED;
  else if (op == "mat_copy") a.op = GemmOpArgs::MAT_COPY;
  else if (op == "add_diag") a.op = GemmOpArgs::ADD_DIAG;
  else if (op == "symmetrize") a.op = GemmOpArgs::SYMMETRIZE;
  else if (op == "col_abs_sums") a.op = GemmOpArgs::COL_ABS_SUMS;
  else if (op == "kron") a.op = GemmOpArgs::KRON;
  else
    EPS_FATAL(fn << "op must be gemm, gemm_batched, mat_copy, add_diag, symmetrize, col_abs_sums or kron, got "
                 << op);
  EPS_CHECK_MSG(out != nullptr, fn << "out is null");
  EPS_CHECK_MSG(route != nullptr && route_cap >= 16, fn << "route needs room for 16 characters");
  const bool gemm = a.op == GemmOpArgs::GEMM || a.op == GemmOpArgs::GEMM_BATCHED;
  const bool batched = a.op == GemmOpArgs::GEMM_BATCHED;
  const int64_t M = g->M, N = g->N, K = g->K;
  EPS_CHECK_MSG(M >= 0, fn << "M is negative: " << M);
  EPS_CHECK_MSG(N >= 0, fn << "N is negative: " << N);
  EPS_CHECK_MSG(K >= 0, fn << "K is negative: " << K);
  struct Operand { const char* name; const double* p; int64_t len, off; };
  const Operand A = {"a", g->a, g->a_len, g->a_off}, B = {"b", g->b, g->b_len, g->b_off},
                C = {"c", g->c, g->c_len, g->c_off}, D = {"d", g->d, g->d_len, 0};
  for (const Operand& o : {A, B, C, D}) {
    EPS_CHECK_MSG(o.len >= 0, fn << o.name << "_len is negative: " << o.len);
    EPS_CHECK_MSG(o.off >= 0, fn << o.name << "_off is negative: " << o.off);
  }
  const int64_t big = int64_t(1) << 40;  // keeps every product of two sizes below inside int64
  EPS_CHECK_MSG(M < big && N < big && K < big, fn << "M, N and K must be below 2^40");
  auto need = [&](const Operand& o, int64_t len) {
    EPS_CHECK_MSG(len == 0 || o.p != nullptr, fn << o.name << " is null");
    EPS_CHECK_MSG(o.len == len, fn << o.name << " has " << o.len << " entries, the dimensions need " << len);
  };
  auto ld_holds = [&](const char* name, int64_t ld, int64_t rows) {
    EPS_CHECK_MSG(ld >= rows, fn << name << " " << ld << " < rows " << rows);
    EPS_CHECK_MSG(ld < big, fn << name << " must be below 2^40");
  };
  // a rows x cols matrix with leading dimension ld: (cols - 1) ld + rows entries
  auto span = [](int64_t rows, int64_t cols, int64_t ld) {
    return rows == 0 || cols == 0 ? int64_t(0) : (cols - 1) * ld + rows;
  };
  if (gemm) {
    int64_t n1 = 1, outer = 1, sA = 0, sB = 0, sC = 0, sA2 = 0, sB2 = 0;
    if (batched) {
      n1 = g->batch, outer = g->outer, sA = g->sA, sB = g->sB, sC = g->sC, sA2 = g->sA2, sB2 = g->sB2;
      EPS_CHECK_MSG(n1 >= 1 && n1 <= 255, fn << "batch must be 1..255, got " << n1);
      EPS_CHECK_MSG(outer >= 1 && outer <= 255, fn << "outer must be 1..255, got " << outer);
      const std::pair<const char*, int64_t> strides[] = {{"sA", sA}, {"sB", sB}, {"sC", sC}, {"sA2", sA2}, {"sB2", sB2}};
      for (const auto& s : strides)
        EPS_CHECK_MSG(s.second >= 0 && s.second < big, fn << s.first << " must be 0..2^40, got " << s.second);
    }
    EPS_CHECK_MSG(!g->lower_only || M == N, fn << "lower_only needs M == N, got " << M << " x " << N);
    const int64_t a_rows = g->trans_a ? K : M, a_cols = g->trans_a ? M : K;
    const int64_t b_rows = g->trans_b ? N : K, b_cols = g->trans_b ? K : N;
    ld_holds("lda", g->lda, a_rows);
    ld_holds("ldb", g->ldb, b_rows);
    ld_holds("ldc", g->ldc, M);
    const int64_t a_one = span(a_rows, a_cols, g->lda), b_one = span(b_rows, b_cols, g->ldb),
                  c_one = span(M, N, g->ldc);
    if (batched && c_one > 0)
      EPS_CHECK_MSG(n1 * outer == 1 || sC >= c_one, fn << "sC " << sC << " < the " << c_one
                                                       << " entries of one result: the results overlap");
    a.use_a = a.use_b = a.use_c = true;
    need(A, a_one == 0 ? 0 : (n1 - 1) * sA + (outer - 1) * sA2 + a_one);
    need(B, b_one == 0 ? 0 : (n1 - 1) * sB + (outer - 1) * sB2 + b_one);
    need(C, c_one == 0 ? 0 : (n1 * outer - 1) * sC + c_one);
    a.out_len = g->c_len;
  } else if (a.op == GemmOpArgs::MAT_COPY) {  // c (M x N, ld M) = alpha op(a)
    ld_holds("lda", g->lda, g->trans_a ? N : M);
    a.use_a = a.use_c = true;
    need(A, g->trans_a ? span(N, M, g->lda) : span(M, N, g->lda));
    need(C, M * N);
    a.out_len = g->c_len;
  } else if (a.op == GemmOpArgs::ADD_DIAG || a.op == GemmOpArgs::SYMMETRIZE) {  // c: M x M, ldc
    ld_holds("ldc", g->ldc, M);
    a.use_c = true;
    need(C, span(M, M, g->ldc));
    if (a.op == GemmOpArgs::ADD_DIAG && g->d != nullptr) {
      a.use_d = true;
      need(D, M);
    }
    a.out_len = g->c_len;
  } else if (a.op == GemmOpArgs::COL_ABS_SUMS) {  // a: M x N, lda; the result: N sums
    ld_holds("lda", g->lda, M);
    a.use_a = true;
    need(A, span(M, N, g->lda));
    a.out_len = N;
  } else {  // KRON: c = a (M x N) kron b (K x batch), all contiguous
    EPS_CHECK_MSG(g->batch >= 0 && g->batch < big, fn << "batch (the columns of b) must be 0..2^40, got " << g->batch);
    EPS_CHECK_MSG(M * N < big && K * g->batch < big && (M * N == 0 || K * g->batch < big / (M * N)),
                  fn << "the Kronecker product is too large");
    a.use_a = a.use_b = a.use_c = true;
    need(A, M * N);
    need(B, K * g->batch);
    need(C, M * N * K * g->batch);
    a.out_len = g->c_len;
  }
  return a;
}

// ---- eps_test_factor_op ----------------------------------------------------------------------------

// The argument checks of eps_test_factor_op, host only.
struct FactorOpArgs {
  enum Op { SPD_INVERSE, SPD_INVERSE_COLUMNS } op;
};

FactorOpArgs CheckFactorOpArgs(const eps_factor_op* g, const double* out) {
  const char* const fn = "eps_test_factor_op: ";
  FactorOpArgs a;
  EPS_CHECK_MSG(g != nullptr, fn << "args is null");
  EPS_CHECK_MSG(g->op != nullptr, fn << "op is null");
  const std::string op(g->op);
  if (op == "spd_inverse") a.op = FactorOpArgs::SPD_INVERSE;
  else if (op == "spd_inverse_columns") a.op = FactorOpArgs::SPD_INVERSE_COLUMNS;
  else EPS_FATAL(fn << "op must be spd_inverse or spd_inverse_columns, got " << op);
  EPS_CHECK_MSG(out != nullptr, fn << "out is null");
  const int64_t n = g->n;
  EPS_CHECK_MSG(n >= 0, fn << "n is negative: " << n);
  EPS_CHECK_MSG(n < (int64_t(1) << 20), fn << "n must be below 2^20");
  EPS_CHECK_MSG(g->a_len >= 0, fn << "a_len is negative: " << g->a_len);
  EPS_CHECK_MSG(g->a_off >= 0, fn << "a_off is negative: " << g->a_off);
  EPS_CHECK_MSG(n == 0 || g->a != nullptr, fn << "a is null");
  EPS_CHECK_MSG(g->a_len == n * n, fn << "a has " << g->a_len << " entries, the dimensions need " << n * n);
  EPS_CHECK_MSG(g->form >= -1 && g->form <= 1, fn << "form must be -1, 0 or 1, got " << g->form);
  if (a.op == FactorOpArgs::SPD_INVERSE) {
    // both ops have a second result today; what an op has no use for must not be given
    EPS_CHECK_MSG(g->lo == 0, fn << "lo is given (" << g->lo << "), spd_inverse has no column slab");
    EPS_CHECK_MSG(g->cnt == 0, fn << "cnt is given (" << g->cnt << "), spd_inverse has no column slab");
    EPS_CHECK_MSG(g->out_cols == 0, fn << "out_cols is given (" << g->out_cols << "), spd_inverse has no column slab");
  } else {
    EPS_CHECK_MSG(g->lo >= 0, fn << "lo is negative: " << g->lo);
    EPS_CHECK_MSG(g->cnt >= 0, fn << "cnt is negative: " << g->cnt);
    EPS_CHECK_MSG(g->lo <= n && g->cnt <= n - g->lo, fn << "lo + cnt > n: " << g->lo << " + " << g->cnt << " > " << n);
    EPS_CHECK_MSG(g->out_cols >= g->cnt, fn << "out_cols " << g->out_cols << " < cnt " << g->cnt);
    EPS_CHECK_MSG(g->out_cols < (int64_t(1) << 20), fn << "out_cols must be below 2^20");
  }
  return a;
}

}  // namespace

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

int eps_linear_map_apply(const void* linear_map, size_t len, const eps_blob* data, size_t ndata,
                         int transpose, const double* x, size_t nx, double* y, size_t ny) {
  return Guard([&] {
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    auto dm = MakeDataMap(data, ndata, dt);
    LinearMap A = ParseMap(linear_map, len, dm.get());
    if (transpose & 1) A = A.Transpose();
    if (transpose & 2) A = A.Inverse();  // apply the (cached, explicit) inverse map
    EPS_CHECK_MSG(static_cast<int64_t>(nx) == A.impl().n() && static_cast<int64_t>(ny) == A.impl().m(),
                  "map is " << A.impl().m() << " x " << A.impl().n() << ", got x of " << nx
                            << " and y of " << ny);
    DVec xd = DVec::FromHost(x, nx, dt);
    DVec yd = DVec::Empty(ny, dt);
    A.impl().Apply(1.0, xd, 0.0, yd);
    yd.ToHost(y);
  });
}

int eps_linear_map_binary(char op, const void* a, size_t a_len, int ta, const void* b,
                          size_t b_len, int tb, const eps_blob* data, size_t ndata,
                          int* result_type, int64_t* m, int64_t* n, double* dense,
                          size_t dense_capacity) {
  return Guard([&] {
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    auto dm = MakeDataMap(data, ndata, dt);
    LinearMap A = ParseMap(a, a_len, dm.get());
    LinearMap B = ParseMap(b, b_len, dm.get());
    if (ta) A = A.Transpose();
    if (tb) B = B.Transpose();
    LinearMap C;
    if (op == '+') C = A + B;
    else if (op == '*') C = A * B;
    else EPS_FATAL("op must be '+' or '*'");
    if (result_type) *result_type = static_cast<int>(C.impl().type());
    if (m) *m = C.impl().m();
    if (n) *n = C.impl().n();
    if (dense) {
      std::vector<double> D = C.impl().AsDenseHost();
      EPS_CHECK_MSG(D.size() <= dense_capacity, "dense output buffer too small");
      std::memcpy(dense, D.data(), D.size() * sizeof(double));
    }
  });
}

int eps_linear_map_inverse(const void* linear_map, size_t len, const eps_blob* data,
                           size_t ndata, double* dense, size_t dense_capacity) {
  return Guard([&] {
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    auto dm = MakeDataMap(data, ndata, dt);
    LinearMap A = ParseMap(linear_map, len, dm.get()).Inverse();
    std::vector<double> D = A.impl().AsDenseHost();
    EPS_CHECK_MSG(D.size() <= dense_capacity, "dense output buffer too small");
    std::memcpy(dense, D.data(), D.size() * sizeof(double));
  });
}

}  // extern "C"

namespace {
template <class F> double TimeLaunches(int iters, F f) {
  Runtime& rt = Runtime::Get();
  for (int i = 0; i < 2; ++i) f();
  hipEvent_t a, b;
  EPS_HIP(hipEventCreate(&a));
  EPS_HIP(hipEventCreate(&b));
  EPS_HIP(hipEventRecord(a, rt.stream()));
  for (int i = 0; i < iters; ++i) f();
  EPS_HIP(hipEventRecord(b, rt.stream()));
  EPS_HIP(hipEventSynchronize(b));
  float ms = 0;
  EPS_HIP(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return ms / iters;
}
// deterministic non-trivial fill: v[i] = ((i * 2654435761) mod 1024) / 1024 - 0.5
DVec Synthetic(int64_t n, DType dt, double scale) {
  std::vector<double> h(std::min<int64_t>(n, 1 << 20));
  for (size_t i = 0; i < h.size(); ++i)
    h[i] = scale * (static_cast<double>((i * 2654435761ull) & 1023) / 1024.0 - 0.5);
  DVec chunk = DVec::FromHost(h.data(), static_cast<int64_t>(h.size()), dt);
  if (n <= static_cast<int64_t>(h.size())) return chunk;
  DVec v = DVec::Empty(n, dt);
  for (int64_t off = 0; off < n; off += chunk.n) {
    int64_t len = std::min<int64_t>(chunk.n, n - off);
    k::Copy(v.Slice(off, len), chunk.Slice(0, len));
  }
  return v;
}
}  // namespace

extern "C" {

int eps_bench_gemv(int trans, int64_t rows, int64_t cols, int iters, double* ms_avg) {
  return Guard([&] {
    const DType dt = ConfiguredDType();
    DVec A = Synthetic(rows * cols, dt, 1.0);
    DVec x = Synthetic(trans ? rows : cols, dt, 1.0);
    DVec y = DVec::Zeros(trans ? cols : rows, dt);
    if (trans == 2) {  // symmetric apply (reads the lower tiles only)
      EPS_CHECK(rows == cols);
      *ms_avg = TimeLaunches(iters, [&] { k::Symv(rows, 1.0, A, rows, x, 0.0, y); });
      return;
    }
    *ms_avg = TimeLaunches(iters, [&] { k::Gemv(trans != 0, rows, cols, 1.0, A, rows, x, 0.0, y); });
  });
}

int eps_bench_stream(const void* device_ptr, size_t bytes, int mode, int grid, int iters,
                     double* ms_avg) {
  return Guard([&] {
    EPS_CHECK_MSG(bytes >= 16 && mode >= 0 && mode <= 2, "eps_bench_stream: bad arguments");
    Runtime& rt = Runtime::Get();
    DVec own;
    const void* src = device_ptr;
    if (src == nullptr) {
      own = Synthetic(static_cast<int64_t>(bytes / 4), F32, 1.0);
      src = own.data();
    }
    EPS_HIP(hipDeviceSynchronize());  // a borrowed pointer may still be written by another stream
    DVec dst;
    if (mode == 2) dst = DVec::Empty(static_cast<int64_t>(bytes / 4), F32);
    if (grid <= 0) grid = 2048;
    DVec scratch = DVec::Empty(grid, F32);
    *ms_avg = TimeLaunches(iters, [&] {
      k::StreamProbe(mode, src, mode == 2 ? dst.data() : nullptr, static_cast<int64_t>(bytes),
                     scratch.as<float>(), grid);
    });
    (void)rt;
  });
}

int eps_bench_stream_resident(const void* device_ptr, size_t bytes, size_t resident_bytes, int grid, int iters,
                              double* ms_avg) {
  return Guard([&] {
    const size_t column = 40000;  // k::StreamResidentProbe's
    EPS_CHECK_MSG(bytes >= column && resident_bytes <= bytes && iters >= 1 && ms_avg != nullptr,
                  "eps_bench_stream_resident: bad arguments");
    DVec own;
    const void* src = device_ptr;
    if (src == nullptr) {
      own = Synthetic(static_cast<int64_t>(bytes / 4), F32, 1.0);
      src = own.data();
    }
    EPS_HIP(hipDeviceSynchronize());  // a borrowed pointer may still be written by another stream
    if (grid <= 0) grid = 2048;
    DVec scratch = DVec::Empty(grid, F32);
    const int64_t per_column = static_cast<int64_t>(resident_bytes / (bytes / column)) / 16 * 16;
    // TimeLaunches' two untimed launches fill the cache: the average is of launches that find it filled
    *ms_avg = TimeLaunches(iters, [&] {
      k::StreamResidentProbe(src, static_cast<int64_t>(bytes), per_column, scratch.as<float>(), grid);
    });
  });
}

int eps_fused_residency(int64_t m, int64_t n, int f64, int64_t budget_bytes, int* qfull, int64_t* jcut,
                        int64_t* resident_bytes) {
  return Guard([&] {
    EPS_CHECK_MSG(m >= 1 && n >= 1 && qfull != nullptr && jcut != nullptr && resident_bytes != nullptr,
                  "eps_fused_residency: bad arguments");
    const k::FusedResidency r = k::LassoFusedResidency(m, n, f64 ? F64 : F32, budget_bytes);
    *qfull = r.qfull;
    *jcut = r.jcut;
    *resident_bytes = r.bytes;
  });
}

int eps_fused_residency_last(int* qfull, int64_t* jcut) {
  return Guard([&] {
    EPS_CHECK_MSG(qfull != nullptr && jcut != nullptr, "eps_fused_residency_last: bad arguments");
    const k::FusedResidency r = k::LastFusedResidency();
    *qfull = r.qfull;
    *jcut = r.jcut;
  });
}

int eps_bench_gemm(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, int lower_only,
                   int iters, double* ms_avg) {
  return Guard([&] {
    const DType dt = ConfiguredDType();
    // EPSILON_HIP_BENCH_RANDOM=1: operands with independent pseudo-random entries instead of the
    // repeating 1024-value pattern (the Gram product inside a solve multiplies random data and
    // runs 4.8 ms slower than this microbenchmark on the pattern: is it the data?)
    const bool rnd = opt::IsSet(opt::kBenchRandom);
    auto operand = [&](int64_t count, uint64_t seed) {
      if (!rnd) return Synthetic(count, dt, 1.0);
      DVec v = DVec::Empty(count, dt);
      k::FillHash(v, seed);
      return v;
    };
    DVec A = operand(M * K, 0xA11CEull);
    // lower_only == 2: SYRK proper, both operands are the same buffer (the Gram product)
    DVec B = lower_only == 2 ? A : operand(K * N, 0xB0Bull);
    DVec C = DVec::Zeros(M * N, dt);
    const int64_t lda = trans_a ? K : M, ldb = trans_b ? N : K;
    *ms_avg = TimeLaunches(iters, [&] {
      k::Gemm(trans_a != 0, trans_b != 0, M, N, K, 1.0, A, lda, B, ldb, 0.0, C, M, lower_only != 0);
    });
  });
}

int eps_bench_spd_inverse(int64_t n, int iters, double* ms_avg) {
  return Guard([&] {
    const DType dt = ConfiguredDType();
    DVec G = Synthetic(n * n, dt, 1.0);
    DVec W0 = DVec::Zeros(n * n, dt);
    k::Gemm(false, true, n, n, n, 1.0 / n, G, n, G, n, 0.0, W0, n, false);
    k::AddDiag(W0, n, n, 1.0, nullptr);
    DVec W = DVec::Empty(n * n, dt);
    Runtime& rt = Runtime::Get();
    double total = 0;
    for (int i = 0; i < iters + 1; ++i) {
      k::Copy(W, W0);
      rt.Sync();
      hipEvent_t a, b;
      EPS_HIP(hipEventCreate(&a));
      EPS_HIP(hipEventCreate(&b));
      EPS_HIP(hipEventRecord(a, rt.stream()));
      k::SpdInverseInPlace(W, n);
      EPS_HIP(hipEventRecord(b, rt.stream()));
      EPS_HIP(hipEventSynchronize(b));
      float e = 0;
      EPS_HIP(hipEventElapsedTime(&e, a, b));
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
      if (i > 0) total += e;
    }
    *ms_avg = total / iters;
  });
}

int eps_test_spd_inverse_repeat(int64_t n, int form_a, int form_b, double* diff_fro, double* norm_fro) {
  return Guard([&] {
    EPS_CHECK(n > 0 && diff_fro != nullptr && norm_fro != nullptr);
    const DType dt = ConfiguredDType();
    DVec G = Synthetic(n * n, dt, 1.0);
    DVec W0 = DVec::Zeros(n * n, dt);
    k::Gemm(false, true, n, n, n, 1.0 / n, G, n, G, n, 0.0, W0, n, false);
    k::AddDiag(W0, n, n, 1.0, nullptr);
    G = DVec();
    DVec Xa = W0.Clone(), Xb = W0.Clone();
    struct Restore { ~Restore() { k::SetPotrfForm(-1); } } restore;
    k::SetPotrfForm(form_a);
    k::SpdInverseInPlace(Xa, n);
    k::SetPotrfForm(form_b);
    k::SpdInverseInPlace(Xb, n);
    Runtime& rt = Runtime::Get();
    rt.ResetSlots();
    const int s0 = rt.NewSlot(), s1 = rt.NewSlot();
    k::SumSqDiff(Xa, Xb, rt.SlotPtr(s0), false);
    k::SumSq(Xa, rt.SlotPtr(s1), false);
    rt.FetchSlots();
    *diff_fro = std::sqrt(rt.SlotValue(s0));
    *norm_fro = std::sqrt(rt.SlotValue(s1));
  });
}

int eps_test_block_solve(const char* mode, const eps_block* blocks, size_t nblocks,
                         const eps_blob* data, size_t ndata, const eps_blob* rhs, size_t nrhs,
                         const char* const* keys, size_t nkeys, eps_result** out) {
  if (out != nullptr) *out = nullptr;
  return Guard([&] {
    EPS_CHECK_MSG(out != nullptr, "eps_test_block_solve: out is null");
    const BlockSolveArgs args = CheckBlockSolveArgs(mode, blocks, nblocks, rhs, nrhs, keys, nkeys);
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    auto dm = MakeDataMap(data, ndata, dt);
    BlockMatrix A;
    for (size_t i = 0; i < nblocks; ++i) {
      LinearMap B = BuildLinearMap(args.maps[i], dm.get());
      EPS_CHECK_MSG(B.impl().m() == args.maps[i].m && B.impl().n() == args.maps[i].n,
                    "eps_test_block_solve: block (" << blocks[i].row << ", " << blocks[i].col << ") is "
                        << B.impl().m() << " x " << B.impl().n() << ", its LinearMap says "
                        << args.maps[i].m << " x " << args.maps[i].n);
      A(blocks[i].row, blocks[i].col) = B;
    }
    BlockVector b;
    for (size_t i = 0; i < nrhs; ++i)
      b.Set(rhs[i].key, DVec::FromHost(static_cast<const double*>(rhs[i].ptr),
                                       static_cast<int64_t>(rhs[i].len / sizeof(double)), dt));
    std::unique_ptr<eps_result> r(new eps_result);
    switch (args.mode) {
      case BlockSolveArgs::FILL:
        for (const std::string& key : A.col_keys())
          PutValues(r.get(), "fill\t" + key, {FillValue(ComputeFill(A, key))});
        break;
      case BlockSolveArgs::FORWARD:
        PutVector(r.get(), "x", ForwardSub(A, args.keys, b));
        break;
      case BlockSolveArgs::BACK:
        PutVector(r.get(), "x", BackSub(A, args.keys, b));
        break;
      case BlockSolveArgs::FACTOR:
      case BlockSolveArgs::SOLVE: {
        BlockCholesky chol;
        std::vector<BlockCholesky::Step> trace;
        chol.set_trace(&trace);
        chol.Compute(A);
        for (size_t s = 0; s < trace.size(); ++s) {
          for (const auto& f : trace[s].fills)
            PutValues(r.get(), "trace\t" + std::to_string(s) + "\t" + f.first, {FillValue(f.second)});
          PutValues(r.get(), "pivot\t" + std::to_string(s) + "\t" + trace[s].pivot, {static_cast<double>(s)});
        }
        for (size_t i = 0; i < chol.order().size(); ++i)
          PutValues(r.get(), "order\t" + std::to_string(i) + "\t" + chol.order()[i], {static_cast<double>(i)});
        if (args.mode == BlockSolveArgs::FACTOR) {
          PutBlocks(r.get(), "L", chol.L());
          PutBlocks(r.get(), "D_inv", chol.D_inv());
        }
        PutValues(r.get(), "condition_estimate", {chol.condition_estimate()});
        PutValues(r.get(), "refine_steps", {static_cast<double>(chol.refine_steps())});
        if (nrhs > 0) {
          PutVector(r.get(), "x", chol.Solve(b));
          PutVector(r.get(), "x_again", chol.Solve(b));
        }
        break;
      }
    }
    *out = r.release();
  });
}

int eps_test_dense_op(const eps_dense_op* g, double* out, double* out2) {
  return Guard([&] {
    const DenseOpArgs args = CheckDenseOpArgs(g, out, out2);
    const DType dt = ConfiguredDType();
    constexpr int64_t G = EPS_DENSE_OP_GUARD;
    const int64_t n = g->rows;
    DVec a_all, x_all, y_all, add_all, a, x, y, add, work;
    if (args.use_a) a = PlaceOperand(g->a, g->a_len, g->a_off, 0, dt, &a_all);
    if (args.use_x) x = PlaceOperand(g->x, g->x_len, g->x_off, 0, dt, &x_all);
    if (args.use_add) add = PlaceOperand(g->add, g->add_len, g->add_off, 0, dt, &add_all);
    if (args.reduction) {
      if (args.use_y) y = PlaceOperand(g->y, g->y_len, g->y_off, 0, dt, &y_all);
      Runtime& rt = Runtime::Get();
      rt.ResetSlots();
      const int slot = rt.NewSlot();
      EPS_HIP(hipMemcpyAsync(rt.SlotPtr(slot), &g->preset, sizeof(double), hipMemcpyHostToDevice, rt.stream()));
      rt.Sync();
      const bool acc = g->accumulate != 0;
      if (args.op == DenseOpArgs::SUMSQ) k::SumSq(x, rt.SlotPtr(slot), acc);
      else if (args.op == DenseOpArgs::SUMSQ_DIFF) k::SumSqDiff(x, y, rt.SlotPtr(slot), acc);
      else k::Dot(x, y, rt.SlotPtr(slot), acc);
      EPS_HIP(hipGetLastError());
      rt.FetchSlots();
      out[0] = rt.SlotValue(slot);
      rt.ResetSlots();
      return;
    }
    // the output between its guards; (y_off + G) elements in is 16-byte aligned for y_off = 0
    static_assert(EPS_DENSE_OP_GUARD % 4 == 0, "the guard keeps offset 0 aligned");
    auto place_y = [&] { y = PlaceOperand(g->y, g->y_len, g->y_off, G, dt, &y_all); };
    auto fetch_y = [&](double* dst) { y_all.Slice(g->y_off, g->y_len + 2 * G).ToHost(dst); };
    place_y();
    const bool symv = args.op == DenseOpArgs::SYMV || args.op == DenseOpArgs::SYMV_PACKED;
    if (symv && g->use_work) work = DVec::Empty(k::SymvWorkspace(n), dt);
    const DVec* wp = (symv && g->use_work) ? &work : nullptr;
    switch (args.op) {
      case DenseOpArgs::GEMV_N:
      case DenseOpArgs::GEMV_T:
        k::Gemv(args.op == DenseOpArgs::GEMV_T, n, g->cols, g->alpha, a, g->lda, x, g->beta, y);
        break;
      case DenseOpArgs::SYMV:
        k::Symv(n, g->alpha, a, g->lda, x, g->beta, y, wp);
        break;
      case DenseOpArgs::SYMV_PACKED: {
        const DVec P = k::SymvPack(n, a, g->lda);
        k::SymvPacked(n, g->alpha, P, x, g->beta, y, wp);
        EPS_HIP(hipGetLastError());
        fetch_y(out);
        place_y();
        k::Symv(n, g->alpha, a, g->lda, x, g->beta, y, wp);
        EPS_HIP(hipGetLastError());
        fetch_y(out2);
        return;
      }
      case DenseOpArgs::REDUCE_PARTIALS:
        k::ReducePartials(n, g->nparts, a, g->alpha, g->beta, y, args.use_add ? &add : nullptr);
        break;
      case DenseOpArgs::AXPBY:
        k::Axpby(y, g->alpha, g->alias_xy ? y : x, g->beta);
        break;
      case DenseOpArgs::DIAG_MUL:
        k::DiagMul(y, g->alpha, a, x, g->beta);
        break;
      default:
        EPS_FATAL("eps_test_dense_op: unreachable");
    }
    EPS_HIP(hipGetLastError());
    fetch_y(out);
  });
}

int eps_test_gemm_op(const eps_gemm_op* g, double* out, char* route, size_t route_cap) {
  return Guard([&] {
    const GemmOpArgs args = CheckGemmOpArgs(g, out, route, route_cap);
    route[0] = '\0';
    const DType dt = ConfiguredDType();
    constexpr int64_t G = EPS_DENSE_OP_GUARD;
    const int64_t M = g->M, N = g->N, K = g->K;
    DVec a_all, b_all, c_all, d_all, a, b, c, d;
    if (args.use_a) a = PlaceOperand(g->a, g->a_len, g->a_off, G, dt, &a_all);
    if (args.use_b) b = PlaceOperand(g->b, g->b_len, g->b_off, G, dt, &b_all);
    if (args.use_c) c = PlaceOperand(g->c, g->c_len, g->c_off, G, dt, &c_all);
    if (args.use_d) d = PlaceOperand(g->d, g->d_len, 0, G, dt, &d_all);
    k::GemmClearRoute();
    switch (args.op) {
      case GemmOpArgs::GEMM:
        k::Gemm(g->trans_a != 0, g->trans_b != 0, M, N, K, g->alpha, a, g->lda, b, g->ldb, g->beta, c, g->ldc,
                g->lower_only != 0);
        break;
      case GemmOpArgs::GEMM_BATCHED:
        k::GemmBatched(g->trans_a != 0, g->trans_b != 0, M, N, K, g->alpha, a, g->lda, g->sA, b, g->ldb, g->sB,
                       g->beta, c, g->ldc, g->sC, g->batch, g->lower_only != 0, g->outer, g->sA2, g->sB2);
        break;
      case GemmOpArgs::MAT_COPY:
        k::MatCopy(g->trans_a != 0, M, N, g->alpha, a, g->lda, c);
        break;
      case GemmOpArgs::ADD_DIAG:
        k::AddDiag(c, M, g->ldc, g->alpha, args.use_d ? &d : nullptr);
        break;
      case GemmOpArgs::SYMMETRIZE:
        k::SymmetrizeFromLower(c, M, g->ldc);
        break;
      case GemmOpArgs::COL_ABS_SUMS: {
        // the sums are device doubles whatever the dtype
        std::vector<double> h(static_cast<size_t>(N + 2 * G), EPS_DENSE_OP_SENTINEL);
        c_all = DVec::FromHost(h.data(), N + 2 * G, F64);
        k::ColAbsSums(a, M, N, g->lda, c_all.as<double>() + G);
        EPS_HIP(hipGetLastError());
        c_all.ToHost(out);
        return;
      }
      case GemmOpArgs::KRON:
        k::KronDense(c, a, M, N, b, K, g->batch);
        break;
    }
    EPS_HIP(hipGetLastError());
    std::snprintf(route, route_cap, "%s", k::GemmLastRoute());
    c_all.Slice(g->c_off, g->c_len + 2 * G).ToHost(out);
  });
}

int eps_test_factor_op(const eps_factor_op* g, double* out, double* out2) {
  return Guard([&] {
    const FactorOpArgs args = CheckFactorOpArgs(g, out);
    const DType dt = ConfiguredDType();
    constexpr int64_t G = EPS_DENSE_OP_GUARD;
    const int64_t n = g->n;
    DVec w_all;
    DVec W = PlaceOperand(g->a, g->a_len, g->a_off, G, dt, &w_all);
    struct Restore { ~Restore() { k::SetPotrfForm(-1); } } restore;
    k::SetPotrfForm(g->form);
    if (args.op == FactorOpArgs::SPD_INVERSE) {
      DVec X;
      k::SpdInverseInPlace(W, n, out2 != nullptr ? &X : nullptr);
      EPS_HIP(hipGetLastError());
      w_all.Slice(g->a_off, n * n + 2 * G).ToHost(out);
      if (out2 != nullptr && n > 0) X.Slice(0, n * n).ToHost(out2);
      return;
    }
    // the slab as InverseDistributed pads it: n * out_cols, of which the launcher owns n * cnt; it
    // sits a_off elements in as well, so that an odd offset moves both operands off alignment
    const int64_t len = n * g->out_cols;
    std::vector<double> h(static_cast<size_t>(g->a_off + 2 * G + len), EPS_DENSE_OP_SENTINEL);
    DVec o_all = DVec::FromHost(h.data(), static_cast<int64_t>(h.size()), dt);
    k::SpdInverseColumns(W, n, g->lo, g->cnt, o_all.Slice(g->a_off + G, len));
    EPS_HIP(hipGetLastError());
    o_all.Slice(g->a_off, len + 2 * G).ToHost(out);
    if (out2 != nullptr && n > 0) W.ToHost(out2);
  });
}

int eps_bench_spd_inverse_columns(int64_t n, int64_t cnt, int iters, double* ms_avg) {
  return Guard([&] {
    const DType dt = ConfiguredDType();
    DVec G = Synthetic(n * n, dt, 1.0);
    DVec W0 = DVec::Zeros(n * n, dt);
    k::Gemm(false, true, n, n, n, 1.0 / n, G, n, G, n, 0.0, W0, n, false);
    k::AddDiag(W0, n, n, 1.0, nullptr);
    DVec W = DVec::Empty(n * n, dt);
    DVec Out = DVec::Empty(n * cnt, dt);
    Runtime& rt = Runtime::Get();
    double total = 0;
    for (int i = 0; i < iters + 1; ++i) {
      k::Copy(W, W0);
      rt.Sync();
      hipEvent_t a, b;
      EPS_HIP(hipEventCreate(&a));
      EPS_HIP(hipEventCreate(&b));
      EPS_HIP(hipEventRecord(a, rt.stream()));
      k::SpdInverseColumns(W, n, 0, cnt, Out);
      EPS_HIP(hipEventRecord(b, rt.stream()));
      EPS_HIP(hipEventSynchronize(b));
      float e = 0;
      EPS_HIP(hipEventElapsedTime(&e, a, b));
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
      if (i > 0) total += e;
    }
    *ms_avg = total / iters;
  });
}

int eps_bench_prox(int kind, int64_t n, int iters, double* ms_avg) {
  return Guard([&] {
    EPS_CHECK(n > 0 && iters > 0 && ms_avg != nullptr);
    const DType dt = ConfiguredDType();
    DVec v = Synthetic(n, dt, 4.0);
    DVec x = DVec::Empty(n, dt);
    k::ScaledZoneArgs a;
    a.lam = 0.7;
    DVec lamv;
    if (kind == 1) {  // per-element thresholds (weighted norm_1, quantile)
      lamv = Synthetic(n, dt, 1.0);
      k::Axpby(lamv, 0.0, lamv, 1.0);
      k::Fill(lamv, 0.7);
      a.lam_vec = &lamv;
    }
    *ms_avg = TimeLaunches(iters, [&] {
      if (kind == 2) k::MaxZero(x, v);
      else k::ScaledZone(x, v, a);
    });
  });
}

int eps_bench_svd(int64_t m, int64_t n, int rank, int max_sweeps, double perturb, double* ms_cold,
                  int* sweeps_cold, double* ms_warm, int* sweeps_warm, double* defects) {
  return Guard([&] {
    EPS_CHECK(m > 0 && n > 0 && ms_cold != nullptr);
    const DType dt = ConfiguredDType();
    Runtime& rt = Runtime::Get();
    // the reference's robust-PCA generator (python/epopt/problems/robust_pca.py:5-22):
    // rank-r part + 10 % sparse part of 10 * randn; a cheap host generator (sum of uniforms)
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto uni = [&] {
      st ^= st << 13;
      st ^= st >> 7;
      st ^= st << 17;
      return static_cast<double>(st >> 11) * (1.0 / 9007199254740992.0);
    };
    auto gauss = [&] { return (uni() + uni() + uni() + uni() - 2.0) * 1.7320508075688772; };
    std::vector<double> h(static_cast<size_t>(m) * std::max<int64_t>(rank, 1));
    for (auto& v : h) v = gauss();
    DVec A = DVec::FromHost(h.data(), m * std::max<int64_t>(rank, 1), dt);
    h.resize(static_cast<size_t>(n) * std::max<int64_t>(rank, 1));
    for (auto& v : h) v = gauss();
    DVec B = DVec::FromHost(h.data(), n * std::max<int64_t>(rank, 1), dt);
    DVec Y = DVec::Empty(m * n, dt);
    {
      std::vector<float> sp(static_cast<size_t>(m) * n);
      for (auto& v : sp) v = uni() < 0.1 ? static_cast<float>(10.0 * gauss()) : 0.0f;
      std::vector<double> col(m);
      // upload column by column through the fp64 staging the DVec helpers take
      std::vector<double> all(sp.begin(), sp.end());
      sp.clear();
      sp.shrink_to_fit();
      Y = DVec::FromHost(all.data(), m * n, dt);
    }
    if (rank > 0) k::Gemm(false, true, m, n, rank, 1.0, A, m, B, n, 1.0, Y, m);
    auto timed = [&](const DVec& W, const DVec& V, bool warm, double* ms, int* sweeps) {
      rt.Sync();
      hipEvent_t a, b;
      EPS_HIP(hipEventCreate(&a));
      EPS_HIP(hipEventCreate(&b));
      EPS_HIP(hipEventRecord(a, rt.stream()));
      const int sw = k::JacobiSvd(W, m, n, V, max_sweeps, warm, false);
      EPS_HIP(hipEventRecord(b, rt.stream()));
      EPS_HIP(hipEventSynchronize(b));
      float e = 0;
      EPS_HIP(hipEventElapsedTime(&e, a, b));
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
      *ms = e;
      if (sweeps) *sweeps = sw;
    };
    auto measure = [&](const DVec& Y0, const DVec& W, const DVec& V, double* out) {
      // out[0] = ||V^T V - I||_F / sqrt(n), out[1] = ||W V^T - Y||_F / ||Y||_F,
      // out[2] = ||offdiag(W^T W)||_F / ||diag(W^T W)||_F
      DVec T = DVec::Empty(n * n, dt);
      k::Gemm(true, false, n, n, n, 1.0, V, n, V, n, 0.0, T, n);
      k::AddDiag(T, n, n, -1.0, nullptr);
      rt.ResetSlots();
      const int s0 = rt.NewSlot(), s1 = rt.NewSlot(), s2 = rt.NewSlot(), s3 = rt.NewSlot(), s4 = rt.NewSlot();
      k::SumSq(T, rt.SlotPtr(s0), false);
      DVec R = Y0.Clone();
      k::Gemm(false, true, m, n, n, 1.0, W, m, V, n, -1.0, R, m);
      k::SumSq(R, rt.SlotPtr(s1), false);
      k::SumSq(Y0, rt.SlotPtr(s2), false);
      k::Gemm(true, false, n, n, m, 1.0, W, m, W, m, 0.0, T, n);
      k::SumSq(T, rt.SlotPtr(s3), false);
      DVec sig = DVec::Empty(n, dt);
      k::ColNorms(W, m, n, sig, false);
      DVec sq = DVec::Empty(n, dt);
      k::DiagMul(sq, 1.0, sig, sig, 0.0);
      k::SumSq(sq, rt.SlotPtr(s4), false);
      rt.FetchSlots();
      out[0] = std::sqrt(rt.SlotValue(s0) / static_cast<double>(n));
      out[1] = std::sqrt(rt.SlotValue(s1) / rt.SlotValue(s2));
      const double all = rt.SlotValue(s3), diag = rt.SlotValue(s4);
      out[2] = std::sqrt(std::max(0.0, all - diag) / diag);
    };
    DVec W = Y.Clone();
    DVec V = DVec::Empty(n * n, dt);
    timed(W, V, false, ms_cold, sweeps_cold);
    if (defects) measure(Y, W, V, defects);
    if (ms_warm != nullptr && perturb >= 0) {
      // a nearby matrix, as the next ADMM sweep would present: Y2 = Y + perturb * (scaled fill)
      DVec Y2 = Y.Clone();
      DVec N = Synthetic(m * n, dt, 1.0);
      k::Axpby(Y2, perturb, N, 1.0);
      DVec W2 = DVec::Empty(m * n, dt);
      k::Gemm(false, false, m, n, n, 1.0, Y2, m, V, n, 0.0, W2, m);
      timed(W2, V, true, ms_warm, sweeps_warm);
      if (defects) measure(Y2, W2, V, defects + 3);
    }
  });
}

int eps_bench_svd_device(const void* y_dev, int64_t m, int64_t n, int max_sweeps, double* ms, int* sweeps) {
  return Guard([&] {
    EPS_CHECK(y_dev != nullptr && m > 0 && n > 0 && ms != nullptr);
    Runtime& rt = Runtime::Get();
    EPS_HIP(hipDeviceSynchronize());  // the caller's stream may still be writing the matrix
    DVec Y = DVec::Borrow(const_cast<void*>(y_dev), m * n, F32);
    DVec W = Y.Clone();
    DVec V = DVec::Empty(n * n, F32);
    rt.Sync();
    hipEvent_t a, b;
    EPS_HIP(hipEventCreate(&a));
    EPS_HIP(hipEventCreate(&b));
    EPS_HIP(hipEventRecord(a, rt.stream()));
    const int sw = k::JacobiSvd(W, m, n, V, max_sweeps, false, false);
    EPS_HIP(hipEventRecord(b, rt.stream()));
    EPS_HIP(hipEventSynchronize(b));
    float e = 0;
    EPS_HIP(hipEventElapsedTime(&e, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *ms = e;
    if (sweeps) *sweeps = sw;
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
