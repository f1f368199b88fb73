// extern "C" boundary, the per-operator test entries: eps_linear_map_*, eps_test_*, eps_fused_residency*
// of include/epsilon_hip.h.  Each checks its arguments on the host before any device work starts
// (eps_test_csc_op, the host CSC algebra, starts none at all).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <set>

#include "block.h"
#include "capi_util.h"
#include "sparse.h"

using namespace eps;
using namespace eps::capi;

namespace {

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

// ---- the host operands of the dense, gemm and factor entries -----------------------------------------

// One operand as its entry was given it.  `fn` below is the entry's prefix in the messages.
struct Operand { const char* name; const double* p; int64_t len, off; };

void CheckOperandSigns(const char* fn, std::initializer_list<Operand> operands) {
  for (const Operand& o : operands) {
    EPS_CHECK_MSG(o.len >= 0, fn << o.name << "_len is negative: " << o.len);
    EPS_CHECK_MSG(o.off >= 0, fn << o.name << "_off is negative: " << o.off);
  }
}

// an operand that the op reads: there, with the length its dimensions need
void NeedOperand(const char* fn, const Operand& o, int64_t len) {
  EPS_CHECK_MSG(len == 0 || o.p != nullptr, fn << o.name << " is null");
  EPS_CHECK_MSG(o.len == len, fn << o.name << " has " << o.len << " entries, the dimensions need " << len);
}

// `len` host doubles as the slice [off + guard, off + guard + len) of a device allocation of the
// configured dtype whose other elements hold EPS_DENSE_OP_SENTINEL; *whole receives the allocation.
DVec PlaceOperand(const double* p, int64_t len, int64_t off, int64_t guard, DType dt, DVec* whole) {
  std::vector<double> h(static_cast<size_t>(off + 2 * guard + len), EPS_DENSE_OP_SENTINEL);
  if (len > 0) std::memcpy(h.data() + off + guard, p, static_cast<size_t>(len) * sizeof(double));
  *whole = DVec::FromHost(h.data(), static_cast<int64_t>(h.size()), dt);
  return whole->Slice(off + guard, len);
}

// puts the process back on the default Cholesky step when an entry that chose one returns
struct RestorePotrfForm { ~RestorePotrfForm() { k::SetPotrfForm(-1); } };

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
  const Operand A = {"a", g->a, g->a_len, g->a_off}, X = {"x", g->x, g->x_len, g->x_off},
                Y = {"y", g->y, g->y_len, g->y_off}, ADD = {"add", g->add, g->add_len, g->add_off};
  CheckOperandSigns(fn, {A, X, Y, ADD});
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
  if (a.use_a) NeedOperand(fn, A, a_need);
  if (a.use_x) NeedOperand(fn, X, x_need);
  if (a.use_y) NeedOperand(fn, Y, y_need);
  if (a.use_add) NeedOperand(fn, ADD, add_need);
  return a;
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
  const Operand A = {"a", g->a, g->a_len, g->a_off}, B = {"b", g->b, g->b_len, g->b_off},
                C = {"c", g->c, g->c_len, g->c_off}, D = {"d", g->d, g->d_len, 0};
  CheckOperandSigns(fn, {A, B, C, D});
  const int64_t big = int64_t(1) << 40;  // keeps every product of two sizes below inside int64
  EPS_CHECK_MSG(M < big && N < big && K < big, fn << "M, N and K must be below 2^40");
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
    NeedOperand(fn, A, a_one == 0 ? 0 : (n1 - 1) * sA + (outer - 1) * sA2 + a_one);
    NeedOperand(fn, B, b_one == 0 ? 0 : (n1 - 1) * sB + (outer - 1) * sB2 + b_one);
    NeedOperand(fn, C, c_one == 0 ? 0 : (n1 * outer - 1) * sC + c_one);
    a.out_len = g->c_len;
  } else if (a.op == GemmOpArgs::MAT_COPY) {  // c (M x N, ld M) = alpha op(a)
    ld_holds("lda", g->lda, g->trans_a ? N : M);
    a.use_a = a.use_c = true;
    NeedOperand(fn, A, g->trans_a ? span(N, M, g->lda) : span(M, N, g->lda));
    NeedOperand(fn, C, M * N);
    a.out_len = g->c_len;
  } else if (a.op == GemmOpArgs::ADD_DIAG || a.op == GemmOpArgs::SYMMETRIZE) {  // c: M x M, ldc
    ld_holds("ldc", g->ldc, M);
    a.use_c = true;
    NeedOperand(fn, C, span(M, M, g->ldc));
    if (a.op == GemmOpArgs::ADD_DIAG && g->d != nullptr) {
      a.use_d = true;
      NeedOperand(fn, D, M);
    }
    a.out_len = g->c_len;
  } else if (a.op == GemmOpArgs::COL_ABS_SUMS) {  // a: M x N, lda; the result: N sums
    ld_holds("lda", g->lda, M);
    a.use_a = true;
    NeedOperand(fn, A, span(M, N, g->lda));
    a.out_len = N;
  } else {  // KRON: c = a (M x N) kron b (K x batch), all contiguous
    EPS_CHECK_MSG(g->batch >= 0 && g->batch < big, fn << "batch (the columns of b) must be 0..2^40, got " << g->batch);
    EPS_CHECK_MSG(M * N < big && K * g->batch < big && (M * N == 0 || K * g->batch < big / (M * N)),
                  fn << "the Kronecker product is too large");
    a.use_a = a.use_b = a.use_c = true;
    NeedOperand(fn, A, M * N);
    NeedOperand(fn, B, K * g->batch);
    NeedOperand(fn, C, M * N * K * g->batch);
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
  const Operand A = {"a", g->a, g->a_len, g->a_off};
  CheckOperandSigns(fn, {A});
  NeedOperand(fn, A, n * n);
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

// ---- eps_test_sparse_op, eps_test_csc_op -------------------------------------------------------------

// A compressed structure as an entry was given it: `outer` compressed rows (CSR) or columns (CSC)
// whose indices lie in [0, inner).  ptr_name / idx_name are the argument names in the messages.
struct Compressed {
  const char *ptr_name, *idx_name, *outer_name, *inner_name;
  int64_t outer, inner, nnz;
  const int32_t* ptr; int64_t ptr_len;
  const int32_t* idx; int64_t idx_len;
  const double* val;  int64_t val_len;
};

// Everything that lets the structure be indexed safely: sizes, pointer array, index range; with
// `ascending` also the HostCsc invariant (indices strictly ascending within each outer slice).
void CheckCompressed(const char* fn, const Compressed& s, bool ascending) {
  const int64_t lim = int64_t(1) << 31;  // int32 structure
  EPS_CHECK_MSG(s.outer >= 0, fn << s.outer_name << " is negative: " << s.outer);
  EPS_CHECK_MSG(s.inner >= 0, fn << s.inner_name << " is negative: " << s.inner);
  EPS_CHECK_MSG(s.nnz >= 0, fn << "nnz is negative: " << s.nnz);
  EPS_CHECK_MSG(s.outer < lim - 1 && s.inner < lim && s.nnz < lim,
                fn << s.outer_name << ", " << s.inner_name << " and nnz must be below 2^31");
  EPS_CHECK_MSG(s.ptr != nullptr, fn << s.ptr_name << " is null");
  EPS_CHECK_MSG(s.nnz == 0 || s.idx != nullptr, fn << s.idx_name << " is null");
  EPS_CHECK_MSG(s.nnz == 0 || s.val != nullptr, fn << "val is null");
  EPS_CHECK_MSG(s.ptr_len == s.outer + 1, fn << s.ptr_name << " has " << s.ptr_len << " entries, " << s.outer_name
                                             << " + 1 is " << s.outer + 1);
  EPS_CHECK_MSG(s.idx_len == s.nnz, fn << s.idx_name << " has " << s.idx_len << " entries, nnz is " << s.nnz);
  EPS_CHECK_MSG(s.val_len == s.nnz, fn << "val has " << s.val_len << " entries, nnz is " << s.nnz);
  EPS_CHECK_MSG(s.ptr[0] == 0, fn << s.ptr_name << "[0] is " << s.ptr[0] << ", not 0");
  for (int64_t i = 0; i < s.outer; ++i)
    EPS_CHECK_MSG(s.ptr[i] <= s.ptr[i + 1], fn << s.ptr_name << " is not monotone at " << i << ": " << s.ptr[i]
                                               << " > " << s.ptr[i + 1]);
  EPS_CHECK_MSG(s.ptr[s.outer] == s.nnz, fn << s.ptr_name << " ends at " << s.ptr[s.outer] << ", nnz is " << s.nnz);
  for (int64_t i = 0; i < s.outer; ++i)
    for (int32_t p = s.ptr[i]; p < s.ptr[i + 1]; ++p) {
      EPS_CHECK_MSG(s.idx[p] >= 0 && s.idx[p] < s.inner, fn << s.idx_name << "[" << p << "] = " << s.idx[p]
                                                            << " is outside [0, " << s.inner << ")");
      EPS_CHECK_MSG(!ascending || p == s.ptr[i] || s.idx[p] > s.idx[p - 1],
                    fn << s.idx_name << " is not strictly ascending at " << p);
    }
}

// the structure as the host matrix whose columns are its outer slices
HostCsc HostCscOf(const Compressed& s) {
  HostCsc A;
  A.m = s.inner;
  A.n = s.outer;
  A.colptr.assign(s.ptr, s.ptr + s.ptr_len);
  if (s.nnz > 0) {
    A.rowidx.assign(s.idx, s.idx + s.nnz);
    A.val.assign(s.val, s.val + s.nnz);
  }
  return A;
}

// The argument checks of eps_test_sparse_op, host only: nothing malformed reaches a kernel.
struct SparseOpArgs {
  enum Op { SPMV, SPMM_CSR_DENSE, DENSE_SPMM_CSC, SCATTER_ADD_CSC } op;
  Compressed csr;
};

SparseOpArgs CheckSparseOpArgs(const eps_sparse_op* g, const double* out) {
  const char* const fn = "eps_test_sparse_op: ";
  SparseOpArgs a;
  EPS_CHECK_MSG(g != nullptr, fn << "args is null");
  EPS_CHECK_MSG(g->op != nullptr, fn << "op is null");
  const std::string op(g->op);
  if (op == "spmv") a.op = SparseOpArgs::SPMV;
  else if (op == "spmm_csr_dense") a.op = SparseOpArgs::SPMM_CSR_DENSE;
  else if (op == "dense_spmm_csc") a.op = SparseOpArgs::DENSE_SPMM_CSC;
  else if (op == "scatter_add_csc") a.op = SparseOpArgs::SCATTER_ADD_CSC;
  else EPS_FATAL(fn << "op must be spmv, spmm_csr_dense, dense_spmm_csc or scatter_add_csc, got " << op);
  EPS_CHECK_MSG(out != nullptr, fn << "out is null");
  a.csr = {"ptr", "idx", "rows", "cols", g->rows, g->cols, g->nnz, g->ptr, g->ptr_len,
           g->idx, g->idx_len, g->val, g->val_len};
  CheckCompressed(fn, a.csr, false);
  const int64_t rows = g->rows, cols = g->cols, n = g->n, ld = g->ld;
  const Operand D = {"d", g->d, g->d_len, 0}, Y = {"y", g->y, g->y_len, 0};
  CheckOperandSigns(fn, {D, Y});
  const bool product = a.op == SparseOpArgs::SPMM_CSR_DENSE || a.op == SparseOpArgs::DENSE_SPMM_CSC;
  if (a.op != SparseOpArgs::SPMV)
    EPS_CHECK_MSG(g->beta == 0.0, fn << "beta is given (" << g->beta << "), " << op << " has none");
  if (product) {
    EPS_CHECK_MSG(n >= 0, fn << "n is negative: " << n);
    EPS_CHECK_MSG(n < (int64_t(1) << 31), fn << "n must be below 2^31");
    // d: `held` rows per column, `count` columns
    const int64_t held = a.op == SparseOpArgs::SPMM_CSR_DENSE ? cols : n;
    const int64_t count = a.op == SparseOpArgs::SPMM_CSR_DENSE ? n : cols;
    EPS_CHECK_MSG(ld >= held, fn << "ld " << ld << " < rows " << held);
    EPS_CHECK_MSG(ld < (int64_t(1) << 31), fn << "ld must be below 2^31");
    // as the launchers ask: (count - 1) ld + held, whatever is empty
    NeedOperand(fn, D, std::max<int64_t>((count - 1) * ld + held, 0));
    NeedOperand(fn, Y, rows * n);
  } else {
    EPS_CHECK_MSG(n == 0, fn << "n is given (" << n << "), " << op << " has none");
    EPS_CHECK_MSG(ld == 0, fn << "ld is given (" << ld << "), " << op << " has none");
    if (a.op == SparseOpArgs::SPMV) {
      NeedOperand(fn, D, cols);
      NeedOperand(fn, Y, rows);
    } else {
      EPS_CHECK_MSG(g->d == nullptr && g->d_len == 0, fn << "d is given, " << op << " has none");
      NeedOperand(fn, Y, rows * cols);
    }
  }
  return a;
}

// The argument checks of eps_test_csc_op.
struct CscOpArgs {
  enum Op { TRANSPOSE, ADD, MULTIPLY, KRON, SCALE_ROWS, SCALE_COLS, FROM_DENSE, FROM_BLOB } op;
  bool use_a = false, use_b = false;
};

Compressed CompressedOf(const char* ptr_name, const char* idx_name, const char* m_name, const char* n_name,
                        const eps_csc& c) {
  return {ptr_name, idx_name, n_name, m_name, c.n, c.m, c.nnz, c.colptr, c.colptr_len,
          c.rowidx, c.rowidx_len, c.val, c.val_len};
}

CscOpArgs CheckCscOpArgs(const eps_csc_op* g, const int64_t* m, const int64_t* n, const int64_t* nnz) {
  const char* const fn = "eps_test_csc_op: ";
  CscOpArgs a;
  EPS_CHECK_MSG(g != nullptr, fn << "args is null");
  EPS_CHECK_MSG(g->op != nullptr, fn << "op is null");
  const std::string op(g->op);
  if (op == "transpose") a.op = CscOpArgs::TRANSPOSE;
  else if (op == "add") a.op = CscOpArgs::ADD;
  else if (op == "multiply") a.op = CscOpArgs::MULTIPLY;
  else if (op == "kron") a.op = CscOpArgs::KRON;
  else if (op == "scale_rows") a.op = CscOpArgs::SCALE_ROWS;
  else if (op == "scale_cols") a.op = CscOpArgs::SCALE_COLS;
  else if (op == "from_dense") a.op = CscOpArgs::FROM_DENSE;
  else if (op == "from_blob") a.op = CscOpArgs::FROM_BLOB;
  else
    EPS_FATAL(fn << "op must be transpose, add, multiply, kron, scale_rows, scale_cols, from_dense or from_blob, "
                    "got " << op);
  EPS_CHECK_MSG(m != nullptr && n != nullptr && nnz != nullptr, fn << "m, n or nnz is null");
  EPS_CHECK_MSG(g->colptr != nullptr, fn << "colptr is null");
  EPS_CHECK_MSG(g->colptr_cap >= 0, fn << "colptr_cap is negative: " << g->colptr_cap);
  EPS_CHECK_MSG(g->nnz_cap >= 0, fn << "nnz_cap is negative: " << g->nnz_cap);
  EPS_CHECK_MSG(g->nnz_cap == 0 || (g->rowidx != nullptr && g->val != nullptr), fn << "rowidx or val is null");
  EPS_CHECK_MSG(g->d_len >= 0, fn << "d_len is negative: " << g->d_len);
  const bool sized_only = a.op == CscOpArgs::FROM_DENSE || a.op == CscOpArgs::FROM_BLOB;
  a.use_a = !sized_only;
  a.use_b = a.op == CscOpArgs::ADD || a.op == CscOpArgs::MULTIPLY || a.op == CscOpArgs::KRON;
  if (a.use_a) CheckCompressed(fn, CompressedOf("a.colptr", "a.rowidx", "a.m", "a.n", g->a), true);
  if (a.use_b) CheckCompressed(fn, CompressedOf("b.colptr", "b.rowidx", "b.m", "b.n", g->b), true);
  const Operand D = {"d", g->d, g->d_len, 0};
  const int64_t lim = int64_t(1) << 31;
  switch (a.op) {
    case CscOpArgs::ADD:
      EPS_CHECK_MSG(g->a.m == g->b.m && g->a.n == g->b.n, fn << "add: a is " << g->a.m << " x " << g->a.n << ", b is "
                                                             << g->b.m << " x " << g->b.n);
      break;
    case CscOpArgs::MULTIPLY:
      EPS_CHECK_MSG(g->a.n == g->b.m, fn << "multiply: a has " << g->a.n << " columns, b has " << g->b.m << " rows");
      break;
    case CscOpArgs::SCALE_ROWS:
    case CscOpArgs::SCALE_COLS: {
      const int64_t need = a.op == CscOpArgs::SCALE_ROWS ? g->a.m : g->a.n;
      EPS_CHECK_MSG(g->d != nullptr, fn << "d is null");
      EPS_CHECK_MSG(g->d_len == 1 || g->d_len == need, fn << "d has " << g->d_len << " entries, " << op
                                                          << " needs 1 or " << need);
      break;
    }
    case CscOpArgs::FROM_DENSE:
    case CscOpArgs::FROM_BLOB:
      EPS_CHECK_MSG(g->a.m >= 0, fn << "a.m is negative: " << g->a.m);
      EPS_CHECK_MSG(g->a.n >= 0, fn << "a.n is negative: " << g->a.n);
      EPS_CHECK_MSG(g->a.m < lim && g->a.n < lim - 1, fn << "a.m and a.n must be below 2^31");
      if (a.op == CscOpArgs::FROM_DENSE) {
        EPS_CHECK_MSG(g->a.n == 0 || g->a.m <= (lim - 1) / g->a.n, fn << "a.m * a.n must be below 2^31");
        NeedOperand(fn, D, g->a.m * g->a.n);
      } else {
        EPS_CHECK_MSG(g->a.nnz >= 0, fn << "nnz is negative: " << g->a.nnz);
        EPS_CHECK_MSG(g->a.nnz < lim, fn << "nnz must be below 2^31");
        EPS_CHECK_MSG(g->blob != nullptr, fn << "blob is null");
      }
      break;
    default: break;
  }
  return a;
}

HostCsc HostCscOf(const char* ptr_name, const eps_csc& c) {
  return HostCscOf(CompressedOf(ptr_name, "", "", "", c));
}

}  // namespace

extern "C" {

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

int eps_test_spd_inverse_repeat(int64_t n, int form_a, int form_b, double* diff_fro, double* norm_fro) {
  return Guard([&] {
    EPS_CHECK(n > 0 && diff_fro != nullptr && norm_fro != nullptr);
    const DType dt = ConfiguredDType();
    DVec W0 = SpdTestMatrix(n, dt);
    DVec Xa = W0.Clone(), Xb = W0.Clone();
    RestorePotrfForm restore;
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
    RestorePotrfForm restore;
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

int eps_test_sparse_op(const eps_sparse_op* g, double* out) {
  return Guard([&] {
    const SparseOpArgs args = CheckSparseOpArgs(g, out);
    const DType dt = ConfiguredDType();
    constexpr int64_t G = EPS_DENSE_OP_GUARD;
    // the CSR arrays of S are the CSC arrays of S^T
    const std::shared_ptr<DeviceCsr> S = UploadAsCsrOfTranspose(HostCscOf(args.csr), dt);
    DVec d_all, y_all, d;
    if (args.op != SparseOpArgs::SCATTER_ADD_CSC) d = PlaceOperand(g->d, g->d_len, 0, 0, dt, &d_all);
    const DVec y = PlaceOperand(g->y, g->y_len, 0, G, dt, &y_all);
    switch (args.op) {
      case SparseOpArgs::SPMV: k::SpmvCsr(*S, g->alpha, d, g->beta, y); break;
      case SparseOpArgs::SPMM_CSR_DENSE: k::SpmmCsrDense(*S, g->alpha, d, g->ld, g->n, y); break;
      case SparseOpArgs::DENSE_SPMM_CSC: k::DenseSpmmCsc(*S, g->alpha, d, g->ld, g->n, y); break;
      case SparseOpArgs::SCATTER_ADD_CSC: k::ScatterAddCsc(*S, g->alpha, y); break;
    }
    EPS_HIP(hipGetLastError());
    y_all.ToHost(out);
  });
}

int eps_test_csc_op(const eps_csc_op* g, int64_t* m, int64_t* n, int64_t* nnz) {
  return Guard([&] {
    const char* const fn = "eps_test_csc_op: ";
    const CscOpArgs args = CheckCscOpArgs(g, m, n, nnz);
    HostCsc A, B, C;
    if (args.use_a) A = HostCscOf("a.colptr", g->a);
    if (args.use_b) B = HostCscOf("b.colptr", g->b);
    const std::vector<double> d(g->d, g->d + (g->d != nullptr ? g->d_len : 0));
    switch (args.op) {
      case CscOpArgs::TRANSPOSE: C = CscTranspose(A); break;
      case CscOpArgs::ADD: C = CscAdd(A, B); break;
      case CscOpArgs::MULTIPLY: C = CscMultiply(A, B); break;
      case CscOpArgs::KRON: C = CscKron(A, B); break;
      case CscOpArgs::SCALE_ROWS: C = CscScaleRows(A, d); break;
      case CscOpArgs::SCALE_COLS: C = CscScaleCols(A, d); break;
      case CscOpArgs::FROM_DENSE: C = CscFromDense(d, g->a.m, g->a.n); break;
      case CscOpArgs::FROM_BLOB: {
        pb::Constant c;
        c.constant_type = pb::Constant::SPARSE_MATRIX;
        c.m = static_cast<int32_t>(g->a.m);
        c.n = static_cast<int32_t>(g->a.n);
        c.nnz = static_cast<int32_t>(g->a.nnz);
        c.data_location = "blob";
        C = CscFromBlob(c, g->blob, g->blob_len);
        break;
      }
    }
    EPS_CHECK_MSG(static_cast<int64_t>(C.colptr.size()) == C.n + 1 && C.rowidx.size() == C.val.size(),
                  fn << "the result's arrays do not fit its size");
    EPS_CHECK_MSG(g->colptr_cap >= C.n + 1, fn << "colptr_cap " << g->colptr_cap << " < n + 1 = " << C.n + 1);
    EPS_CHECK_MSG(g->nnz_cap >= C.nnz(), fn << "nnz_cap " << g->nnz_cap << " < nnz = " << C.nnz());
    std::memcpy(g->colptr, C.colptr.data(), C.colptr.size() * sizeof(int32_t));
    if (C.nnz() > 0) {
      std::memcpy(g->rowidx, C.rowidx.data(), C.rowidx.size() * sizeof(int32_t));
      std::memcpy(g->val, C.val.data(), C.val.size() * sizeof(double));
    }
    *m = C.m;
    *n = C.n;
    *nnz = C.nnz();
  });
}

int eps_test_sparse_handle_op(const eps_sparse_handle_op* g, double* out, int64_t out_cap, double* out2) {
  return Guard([&] {
    const char* const fn = "eps_test_sparse_handle_op: ";
    EPS_CHECK_MSG(g != nullptr, fn << "args is null");
    EPS_CHECK_MSG(g->op != nullptr, fn << "op is null");
    const std::string op(g->op);
    enum { APPLY, ADJOINT, SD, DS, SPD, DPS } what;
    if (op == "apply") what = APPLY;
    else if (op == "adjoint") what = ADJOINT;
    else if (op == "sparse_dense") what = SD;
    else if (op == "dense_sparse") what = DS;
    else if (op == "sparse_plus_dense") what = SPD;
    else if (op == "dense_plus_sparse") what = DPS;
    else
      EPS_FATAL(fn << "op must be apply, adjoint, sparse_dense, dense_sparse, sparse_plus_dense or "
                      "dense_plus_sparse, got " << op);
    EPS_CHECK_MSG(g->sparse_map != nullptr && g->len > 0, fn << "sparse_map is null or empty");
    EPS_CHECK_MSG(g->ndata == 0 || g->data != nullptr, fn << "data is null with ndata " << g->ndata);
    EPS_CHECK_MSG(out != nullptr, fn << "out is null");
    EPS_CHECK_MSG(g->d != nullptr, fn << "d is null");
    EPS_CHECK_MSG(g->d_rows >= 0 && g->d_cols >= 0 && g->d_rows < (int64_t(1) << 31) && g->d_cols < (int64_t(1) << 31),
                  fn << "d_rows and d_cols must be 0..2^31, got " << g->d_rows << " x " << g->d_cols);
    EPS_CHECK_MSG(g->p == nullptr || out2 != nullptr, fn << "out2 is null with p given");
    pb::LinearMap proto;
    try {
      proto = pb::ParseLinearMap(g->sparse_map, g->len);
    } catch (const std::exception& e) {
      EPS_FATAL(fn << "malformed LinearMap: " << e.what());
    }
    EPS_CHECK_MSG(proto.linear_map_type == pb::LinearMap::SPARSE_MATRIX,
                  fn << "sparse_map is not a sparse matrix: type " << proto.linear_map_type);
    // the handle's size from the payload alone, so that the sizes are checked before any device work
    const int64_t hm = g->transpose ? proto.n : proto.m, hn = g->transpose ? proto.m : proto.n;
    int64_t need_rows = 0, need_cols = g->d_cols, rm = 0, rn = 0;
    switch (what) {
      case APPLY: need_rows = hn, need_cols = 1, rm = hm, rn = 1; break;
      case ADJOINT: need_rows = hm, need_cols = 1, rm = hn, rn = 1; break;
      case SD: need_rows = hn, rm = hm, rn = g->d_cols; break;
      case DS: need_rows = g->d_rows, need_cols = hm, rm = g->d_rows, rn = hn; break;
      case SPD:
      case DPS: need_rows = hm, need_cols = hn, rm = hm, rn = hn; break;
    }
    EPS_CHECK_MSG(g->d_rows == need_rows && g->d_cols == need_cols,
                  fn << "d is " << g->d_rows << " x " << g->d_cols << ", " << op << " with a " << hm << " x " << hn
                     << " handle needs " << need_rows << " x " << need_cols);
    EPS_CHECK_MSG(out_cap >= rm * rn, fn << "out_cap " << out_cap << " < the " << rm * rn << " entries of the result");
    EPS_CHECK_MSG(g->p == nullptr || g->p_len == proto.n, fn << "p has " << g->p_len << " entries, the map has "
                                                             << proto.n << " columns");
    const DType dt = ConfiguredDType();
    SetCurrentDType(dt);
    auto dm = MakeDataMap(g->data, g->ndata, dt);
    const LinearMap S = BuildLinearMap(proto, dm.get());
    EPS_CHECK_MSG(S.impl().m() == proto.m && S.impl().n() == proto.n, fn << "the constant is " << S.impl().m() << " x "
                                                                         << S.impl().n() << ", the LinearMap says "
                                                                         << proto.m << " x " << proto.n);
    if (g->p != nullptr) {
      DVec pd = DVec::FromHost(g->p, g->p_len, dt);
      DVec qd = DVec::Empty(proto.m, dt);
      S.impl().Apply(1.0, pd, 0.0, qd);
      qd.ToHost(out2);
    }
    LinearMap H = g->transpose ? S.Transpose() : S;
    if (g->scaled) H = LinearMap::Scalar(g->scale, H.impl().m()) * H;
    EPS_CHECK_MSG(H.impl().type() == SPARSE_MATRIX, fn << "the handle became " << H.impl().DebugString());
    DVec dd = DVec::FromHost(g->d, g->d_rows * g->d_cols, dt);
    if (what == APPLY || what == ADJOINT) {
      const LinearMap M = what == APPLY ? H : H.Transpose();
      DVec yd = DVec::Empty(rm, dt);
      M.impl().Apply(1.0, dd, 0.0, yd);
      yd.ToHost(out);
      return;
    }
    const LinearMap D = LinearMap::Dense(dd, g->d_rows, g->d_cols);
    const LinearMap C = what == SD ? H * D : what == DS ? D * H : what == SPD ? H + D : D + H;
    EPS_CHECK_MSG(C.impl().type() == DENSE_MATRIX && C.impl().m() == rm && C.impl().n() == rn,
                  fn << "the result is " << C.impl().DebugString());
    const std::vector<double> R = C.impl().AsDenseHost();
    std::memcpy(out, R.data(), R.size() * sizeof(double));
  });
}

}  // extern "C"
