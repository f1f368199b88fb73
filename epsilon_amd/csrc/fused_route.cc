// The fused routes (fused_route.h): the lasso structure with its sharded / peer, whitened,
// matrix-variable, wide and tall forms and the batched solves that run on it, the ZERO-term structure,
// and the lasso structure in two-block form.
#include "fused_route.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "admm.h"
#include "comm.h"
#include "kernels.h"
#include "options.h"

namespace eps {
namespace {

// ---------------------------------------------------------------------------------------------------
// What the routes share
// ---------------------------------------------------------------------------------------------------

// What stands in the threshold's place for a term of this kind.  Row groups keep the zone head: their
// threshold goes through the pass's group_lam.
k::Head HeadOf(SeparableDesc::Kind kind) {
  switch (kind) {
    case SeparableDesc::kZone:
    case SeparableDesc::kRowGroups: return k::kHeadZone;
    case SeparableDesc::kRidge: return k::kHeadRidge;
    case SeparableDesc::kLinear: return k::kHeadLinear;
    case SeparableDesc::kNonNegative: return k::kHeadNonNeg;
    case SeparableDesc::kSmooth: return k::kHeadSmooth;
  }
  return k::kHeadZone;
}

// The zone of a kernel record from the operator's description; a1: the scalar of the term's
// variable in its consensus constraint.  A ridge and a linear term take the record with Bs, Cs the
// two factors of their block solve; smooth terms and row groups read the scalar form alone (the
// zone's parameters are the defaults).
k::ZoneParams ZoneOf(const SeparableDesc& z, double a1) {
  k::ZoneParams s;
  s.alpha_vec = z.alpha_vec;
  s.beta_vec = z.beta_vec;
  s.Bs = z.Bs;
  s.Cs = z.Cs;
  s.a1 = a1;
  s.lam = z.lam;
  s.alpha = z.alpha;
  s.beta = z.beta;
  s.M = z.M;
  s.head = HeadOf(z.kind);
  return s;
}

// Empty, or `len` values of the compute type `dt`.
bool Fits(const DVec& v, int64_t len, DType dt) { return v.n == 0 || (v.n == len && v.dt == dt); }

// The prox input of the first sweep from an adopted state, into `v0`:
// v0 = ((u - y_zero) - y_term) + y_zero, in this order.
void FirstInput(const k::ConsensusState& s, const DVec& v0) {
  k::Copy(v0, s.u);
  k::Axpby(v0, -1.0, s.y_zero, 1.0);
  k::Axpby(v0, -1.0, s.y_term, 1.0);
  k::Axpby(v0, 1.0, s.y_zero, 1.0);
}

// The consensus tie a0 copy + a1 var = 0: row `ck` of A holds scalar maps of length `len` on
// `copy` and on `var`.  (That nothing else is in the row is the caller's count of A's columns.)
bool ConsensusTie(const BlockMatrix& A, const std::string& ck, const std::string& copy, const std::string& var,
                  int64_t len, double* a0, double* a1) {
  if (copy == var || !A.has_key(ck, copy) || !A.has_key(ck, var)) return false;
  const LinearMap& A0 = A(ck, copy);
  const LinearMap& A1 = A(ck, var);
  if (A0.impl().type() != SCALAR_MATRIX || A1.impl().type() != SCALAR_MATRIX) return false;
  if (A0.impl().n() != len || A1.impl().n() != len) return false;
  *a0 = GetScalar(A0);
  *a1 = GetScalar(A1);
  return true;
}

// w = Dinv p with every buffer at a fixed address (what a captured launch needs).  A symmetric
// m x m inverse from m = 1024 up is applied from its lower tiles with a fixed workspace, and from
// a tile-packed copy of them unless EPSILON_HIP_SYMV_PACKED=0 (the matrix as it lies): +m^2/2
// values of memory for a tenth of a millisecond at Init.
struct InverseApply {
  std::shared_ptr<const DenseMatrixImpl> D;
  int64_t m = 0;
  DVec p, w, work, packed;

  // p and w may hold `count` columns (column c at c * m): Column(c).  Instances that share the
  // inverse and the cache `shared` (a batch) share one packed copy.
  void Init(std::shared_ptr<const DenseMatrixImpl> D_, int64_t m_, const DVec& p_, const DVec& w_, OpCache* shared,
            int64_t count = 1) {
    D = std::move(D_);
    m = m_;
    p = p_;
    w = w_;
    if (!D->symmetric() || D->rows() != m || m < 1024 || D->trans()) return;
    work = DVec::Empty(count * k::SymvWorkspace(m), p.dt);
    static const bool pack = opt::SymvPacked() != opt::kSymvPackedOff;
    if (!pack) return;
    uint64_t key = 0;
    if (shared != nullptr) {
      key = HashCombine(HashCombine(reinterpret_cast<uintptr_t>(D->data().data()), 0x9ac4ed), m);
      if (auto hit = shared->Find(key)) {
        packed = hit->data();
        return;
      }
    }
    packed = k::SymvPack(m, D->data(), m);
    if (key) shared->Put(key, std::make_shared<DenseMatrixImpl>(packed, packed.n, 1, false, 1.0, key));
  }
  InverseApply Column(int64_t c) const {
    InverseApply a = *this;
    a.p = p.Slice(c * m, m);
    a.w = w.Slice(c * m, m);
    if (work.n > 0) a.work = work.Slice(c * k::SymvWorkspace(m), k::SymvWorkspace(m));
    return a;
  }
  void Apply() const {
    if (packed.n > 0) k::SymvPacked(m, D->scale(), packed, p, 0.0, w, &work);
    else if (work.n > 0) k::Symv(m, D->scale(), D->data(), m, p, 0.0, w, &work);
    else D->Apply(1.0, p, 0.0, w);
  }
};

// A slice of a route's state and the block of the driver's containers it stands for.
struct StateSlice {
  BlockVector* home;
  std::string key;
  DVec v;
  bool take = true;  // false: a "previous iterate", written by every sweep before it is read
};
// The slices take over what their blocks hold (warm start); then `homes`, the driver's
// containers, become views of the slices and of nothing else.
void AdoptState(const std::vector<StateSlice>& table, const std::vector<BlockVector*>& homes) {
  for (const StateSlice& s : table) {
    if (!s.take || !s.home->has_key(s.key)) continue;
    EPS_CHECK((*s.home)(s.key).n == s.v.n);
    k::Copy(s.v, (*s.home)(s.key));
  }
  for (BlockVector* h : homes) *h = BlockVector();
  for (const StateSlice& s : table) s.home->Set(s.key, s.v);
}
std::vector<BlockVector*> Homes(const MultiBlockParts& a) {
  std::vector<BlockVector*> h = {&a.u};
  for (auto* c : {&a.x, &a.y, &a.y_prev})
    for (BlockVector& v : *c) h.push_back(&v);
  return h;
}

int BatchWideMin();  // (with the batched solves below)

// The indices of the options' words (options.cc).  "fused" (off with a leading 0), "fused_zero",
// "fused_zero_check", "fused_zero_lp", "fused_zero_ridge", "fused_zero_tall", "fused_zero_tall_smooth", "fused_zero_xfree", "fused_tall", "fused_matrix" and
// "fused_resident" are read at every Init, "batch_wide" and "batch_zero_tall" per batch ("1" sends eligible groups to the wide
// route / lets the tall ZERO-term members of a batch form groups).
// "0", "1", "auto" of "fused_tall", "fused_zero_tall", "fused_zero_tall_smooth" and "fused_zero_ridge"
enum RouteMode { kRouteOff, kRouteOn, kRouteAuto };
enum MatrixRoute { kMatrixOff, kMatrixPass, kMatrixWide, kMatrixAuto };

// Whether such an option lets a problem of `size` onto its route: "0" no, "1" yes, "auto" from the
// route's measured floor up (a floor of 0: no measured cell got there, "auto" is "0").
bool Allowed(int mode, int64_t size, int64_t auto_floor) {
  if (mode == kRouteAuto) return auto_floor != 0 && size >= auto_floor;
  return mode == kRouteOn;
}

// What the Infinity Cache holds of lines loaded with the default policy before re-reads start to
// miss: the upper end of the plateau of the budget sweep on the pass ("A resident
// slab of the streamed matrix").
constexpr int64_t kResidentLimitBytes = int64_t(224) << 20;

// The share of the pass's m x n matrix that stays in the Infinity Cache (k::LassoFusedResidency)
// under the option, written into `pass` when one is given.  `touched`: the values the sweep itself
// moves with the default policy between two uses of a matrix line - "auto" leaves them their room.
// `auto_on`: false on the routes whose sweep has not been timed with a resident share
//  - there "auto" streams everything and only an explicit number of KiB gives a share.
k::FusedResidency ResidentShare(int64_t m, int64_t n, DType dt, int64_t touched, bool auto_on,
                                k::LassoFusedArgs* pass = nullptr) {
  int64_t budget = opt::FusedResident();
  if (budget < 0) budget = auto_on ? std::max<int64_t>(0, kResidentLimitBytes - touched * (dt == F32 ? 4 : 8)) : 0;
  const k::FusedResidency res = k::LassoFusedResidency(m, n, dt, budget);
  if (pass != nullptr) {
    pass->qfull = res.qfull;
    pass->jcut = res.jcut;
  }
  return res;
}

// Matrix variables X (n x k) under the data map I_k (x) A: the k columns run as k members of the
// batched kernels inside one solve (LassoRoute).  Below this many rows of A the solve keeps the
// generic operator path (a constant: no crossover was measured).
constexpr int64_t kMatrixFusedMinRows = 256;

// ZERO-term problems (basis pursuit, hinge / deadzone + l1 in graph form) on the fused sweep
// (ZeroRoute).  Below this many rows of the data matrix the solve keeps the
// generic operator path (a constant: no crossover was measured).
constexpr int64_t kZeroFusedMinRows = 256;

// Tall ZERO-term problems (more rows than columns: the order of the block LDL^T ends in x') on
// the fused sweep (ZeroRoute with `tall`, DESIGN.md 3.11 "Tall C").  Below this many columns of the
// data matrix the solve keeps the generic operator path whatever the option says.
constexpr int64_t kZeroTallMinCols = 256;
// The floor of "auto": the smallest n of the 4n x n ladder of bench_zero.py at which the fused
// sweep measured at least 1.05 x the generic one (5.5 x at n = 256, the first cell, and
// no cell above it below 2.9 x); 0 would mean that no cell got there and "auto" is "0".
constexpr int64_t kZeroTallAutoMinCols = 256;
// A smooth z term on the tall route (SUM_LOGISTIC; option "fused_zero_tall_smooth"): the sweep is five
// launches, with the sample kernel between the halves of the pass.  The floor of its "auto" by the
// same rule on the logreg_ladder cells of bench_zero.py, from n = 512 on (at n = 256 the default
// stays the generic path); 0 means that no cell got there, or that the cells were not run, and "auto"
// is "0".
// Measured: 3.5 x at n = 512, the first cell, and no cell above it below 2.4 x.
constexpr int64_t kZeroTallSmoothAutoMinCols = 512;

// A ridge term on x in place of the scaled zone (hinge_l2, svr_l2, logreg_l2; option "fused_zero_ridge",
// DESIGN.md 3.11 "A ridge term on x").  The floors of its "auto", one per route by the rule of
// kZeroTallAutoMinCols on the *_l2 cells of bench_zero.py: the smallest m of the fat ladder, the
// smallest n of the 4n x n ladder for the hinge / deadzone losses (one pass) and for the logistic loss
// (the pass in halves), from which every measured cell is ahead of the generic path by more than the
// spread of its runs; 0 means that no cell got there, or that the cells were not run, and "auto" is "0"
// on that route.
// Measured (profiles/r19_zero_ridge.jsonl): every cell is ahead, the spreads at most 0.13.
// Fat: 4.4 to 4.7 x at m = 256, the first cell, and no cell above it below 2.5 x.  Tall, hinge and
// deadzone: 5.6 and 4.5 x at n = 256, no cell above it below 2.7 x.  Tall, logistic: 3.7 x at n = 256,
// no cell above it below 2.2 x.  So each floor is the route's own and "auto" is "1" at present.
constexpr int64_t kZeroRidgeAutoMinRows = 256;
constexpr int64_t kZeroRidgeTallAutoMinCols = 256;
constexpr int64_t kZeroRidgeTallSmoothAutoMinCols = 256;

// Tall lasso (more rows than columns: the order of the least-squares prox's block LDL^T ends in the
// variable) on the fused sweep (LassoRoute with `tall`).  Below this many columns
// the solve keeps the generic operator path whatever the option says (a constant: no crossover was
// measured below it).
constexpr int64_t kLassoTallMinCols = 256;
// The floor of "auto" ("fused_tall"): the smallest n of the 4n x n ladder of bench_tall.py from
// which every cell measured at least 1.05 x the generic path of the same build (the rule of
// kZeroTallAutoMinCols; DESIGN.md 4: 5.0 x at n = 256, the first cell, and no cell above it below
// 4.7 x); 0 would mean that no cell got there and "auto" is "0".
constexpr int64_t kLassoTallAutoMinCols = 256;
// The first word of a tall lasso member's batch key (the others begin with the pass's k::Chain).
constexpr uint64_t kTallLassoKey = 0x7a111a550;

// The bits of a scalar, as a word of a batch key.
uint64_t Bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

// Every rhs that is given lies on a 16-byte boundary (k::ReducePartialsBatch's `rhs_aligned`).
bool RhsAligned(const std::vector<const k::LassoInstance*>& members) {
  bool aligned = true;
  for (const k::LassoInstance* s : members)
    if (s->rhs.n > 0) aligned = aligned && reinterpret_cast<uintptr_t>(s->rhs.data()) % 16 == 0;
  return aligned;
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

// ---------------------------------------------------------------------------------------------------
// What the routes on the batched pass share (the lasso route, the ZERO-term route)
// ---------------------------------------------------------------------------------------------------
// The shape, the forward vectors, the cached inverse and the pass's record of a route whose solves
// can run as members of a group (RunFusedBatches), and the launches of a sweep of such members.
struct BatchRoute : FusedRoute {
  DType dt = F32;
  int64_t m = 0, n = 0;  // the data matrix (the pass's own dimensions are pass.m, pass.n: a tall
                         // ZERO-term route streams the transposed copy, and its dense pivot has order n)
  int grid = 0;
  DVec w, p, tpart;
  InverseApply inv;          // (unused when whitened or wide)
  bool whiten = false;       // the lasso route alone: the pass streams Ahat = X A, w holds X p (EnableWhiten)
  k::LassoFusedArgs pass;    // the state vectors, and what the pass and a batch read of the rest
  k::FusedResidency res;     // the matrix's share that stays in the Infinity Cache
  bool tall_cols = false;    // the tall lasso route: no pass; w, p, inv are n-long / of order n, pass.inst
                             // is LassoTallCols' record, and a group runs on RunTallGroup

  // The key of the group a fresh solve on this route can join; false: it is solved by itself.
  // `tall_groups`: the option "batch_zero_tall" of this batch.
  virtual bool BatchKey(const pb::SolverParams& params, bool tall_groups, std::vector<uint64_t>* key) const = 0;
  // The record of the row kernel (a ZERO-term member with a z block; tall: its x side); null: the
  // partials go through the reduction.
  virtual const k::ZeroRowsArgs* Rows() const { return nullptr; }
  // The record of the sample kernel (a tall ZERO-term member with a smooth z term): the pass then
  // runs in two halves, `pass.chain` and k::kChainZeroTallAcc, around it.
  virtual const k::ZeroTallSamplesArgs* Samples() const { return nullptr; }
  // The resident share of a sweep of `count` members on this route's matrix.
  virtual k::FusedResidency Residency(int64_t count) const { return res; }

  // What every key begins with: the pass's chain (a lasso member and a ZERO-term member never
  // share a group), the data matrix, the shape, the dtype, the inverse with its packed copy, and
  // the schedule.
  std::vector<uint64_t> KeyHead(const DenseMatrixImpl& L, const DenseMatrixImpl& D,
                                const pb::SolverParams& params) const {
    return {static_cast<uint64_t>(pass.chain), reinterpret_cast<uintptr_t>(L.data().data()),
            static_cast<uint64_t>(L.rows()), static_cast<uint64_t>(m), static_cast<uint64_t>(n),
            static_cast<uint64_t>(dt), Bits(L.scale()), reinterpret_cast<uintptr_t>(D.data().data()),
            Bits(D.scale()), reinterpret_cast<uintptr_t>(inv.packed.data()), inv.work.n > 0 ? 1u : 0u,
            static_cast<uint64_t>(params.max_iterations), static_cast<uint64_t>(params.epoch_iterations)};
  }

  // One sweep of the `count` members of `table` (k::LassoBatchUpload) on this route's matrix, in
  // the pass's own dimensions pm x pn (pm: the register-held one, the order of the dense pivot): the
  // batched pass per `width` members - with a sample kernel (Samples()): the dot pass per its width
  // of members, one sample launch on `sample_table` (k::ZeroTallSamplesBatchUpload), the accumulate
  // pass per its own; the row kernel on `row_table` (k::ZeroRowsBatchUpload) for ZERO-term
  // members with a z block, else the batched reduction of the partials; then - unless whitened: the
  // reduction wrote every member's w_hat - one batched apply of the packed inverse (`work`:
  // count * k::SymvWorkspace(pm)), or `own_applies` without a packed copy (D.Apply / Symv: per
  // member).
  template <class Applies>
  void BatchSweep(const DVec& table, const DVec& row_table, const DVec& sample_table, int count,
                  const double* group_lam, const k::FusedResidency& share, bool rhs_aligned, const DVec& work,
                  Applies own_applies) const {
    const int64_t pm = pass.m, pn = pass.n;
    auto passes = [&](k::Chain chain) {
      const int width = k::LassoBatchWidth(pm, pn, dt, chain);
      for (int first = 0; first < count; first += width)
        k::LassoBatchPass(pm, pn, pass.lda, pass.A, table, first, std::min(width, count - first), group_lam, share,
                          chain);
    };
    passes(pass.chain);
    if (Samples() != nullptr) {
      k::ZeroTallSamplesBatch(pn, dt, sample_table, count);
      passes(k::kChainZeroTallAcc);
    }
    if (Rows() != nullptr)
      k::ZeroFusedRowsBatch(pm, grid, Rows()->side, Rows()->zone.head, dt, row_table, count);
    else k::ReducePartialsBatch(pm, grid, table, count, dt, rhs_aligned);
    if (whiten) return;
    if (inv.packed.n > 0) k::SymvPackedBatch(pm, inv.D->scale(), inv.packed, table, count, work);
    else own_applies();
  }
};

// ---------------------------------------------------------------------------------------------------
// The lasso route: "least squares + separable threshold" (kernels_fused.hip)
// ---------------------------------------------------------------------------------------------------
// Recognised structure (the compiled lasso): two terms [SUM_SQUARE with a dense
// argument map, scaled-zone prox with scalar maps], one consensus constraint a0 x' + a1 x = 0
// with a0 = 1 and no constant.  The sweep is then: one fused pass over A (back substitution of
// this sweep, elementwise chain, forward substitution of the next sweep), a partial-sum
// reduction (+ the all-reduce when sharded) and the apply of the cached inverse.
//
// Tall A (`tall`): the same terms and tie with the least-squares prox's block LDL^T
// in the order [constraint, arg, var].  The prox is then x0 = Dinv(var) (v0 - c) with the constant
// c = L(var, arg) rhs_arg, so a sweep never reads A: the tile launch of the packed inverse on
// r = v0 - c and the cols kernel (the tiles' sum, the chain from x0 on, the next r) from n = 1024,
// the dense apply and the cols kernel below.  One GPU, vector variables, f32 and f64.
struct LassoRoute final : BatchRoute {
  LeastSquaresDesc ls;
  SeparableDesc sz;  // the threshold: a zone, or - a matrix variable - the group shrinkage of the rows (weight sz.lam)
  double a1 = 0;
  int64_t slab = 0;  // rows of the cached inverse applied per rank (sharded runs)
  bool sharded = false;    // the least-squares variable is split over the ranks
  bool use_peer = false;   // exchanges ride in the sweep's kernels (peer window), not in RCCL
  bool peer_slab = false;  // ... and the inverse is applied by row slabs
  bool replicated_apply = false;  // EPSILON_HIP_SHARDED_APPLY=replicated (Enable)
  DVec wpad, wslice;
  DVec state_all, snapshot;  // x0, x1, y0, y1, u, y1prev in one buffer; its copy at a check
  DVec norm_work;            // partials + ticket of the one-launch residual norms
  int norm_slot = 0;
  double wscale = 1;         // c of Dinv_arg = c X^T X
  DVec X, Ahat, rhat;        // L^-1 of the inverse, X A (ld m), X rhs_arg (empty: no rhs)
  // matrix variable (n x cols under I_cols (x) A): its columns are members of the batched kernels
  int64_t cols = 1;
  bool wide = false;       // the wide route (f32): w and p are whole panels of 64 members
  bool rhs_aligned = true;
  std::vector<k::LassoInstance> members;
  DVec table;              // their descriptors on the device (LassoBatchUpload)
  WideSweep ws;
  bool tall = false;       // no pass, m > n
  DVec crhs;               // tall: c = L(var, arg) rhs_arg (empty: no rhs)

  // The matrix's resident share for a sweep of `count` members on it (`into`: the pass's record,
  // BuildPass): each has its partials (written and re-read: the same lines), six state vectors, p
  // and w; the explicit apply reads the inverse.  Sharded and peer sweeps and the wide kernels
  // stream everything; so does "auto" for more than one member (a batch, a matrix variable): the
  // batched pass has not been timed with a share.
  k::FusedResidency Residency(int64_t count, k::LassoFusedArgs* into) const {
    if (sharded || use_peer || wide || tall || ShardSpec::Get().active()) return k::FusedResidency();
    return ResidentShare(m, n, dt, count * (static_cast<int64_t>(grid) * m + 6 * n + 2 * m) + (whiten ? 0 : m * m),
                         /*auto_on=*/count == 1 && cols == 1, into);
  }
  k::FusedResidency Residency(int64_t count) const override { return Residency(count, nullptr); }

  // `tall_mode`: the option "fused_tall"; under "auto" the measured floor applies
  bool Enable(const MultiBlockParts& a, int tall_mode) {
    if (opt::Is0(opt::kFused) || a.prox.size() != 2 || a.num_constraints != 1 || !a.b.data().empty()) return false;
    const ShardSpec& sh = ShardSpec::Get();
    // consensus form: the threshold step averages over the ranks, which the fused pass does not
    if (sh.active() && sh.consensus_terms()) return false;
    if (!a.prox[0]->DescribeLeastSquares(&ls)) return false;
    cols = ls.cols;
    const int matrix_mode = cols > 1 ? opt::Word(opt::kFusedMatrix) : kMatrixAuto;
    if (cols > 1 && (matrix_mode == kMatrixOff || sh.active())) return false;
    // accepted: a zone without offset; or row groups, one per row of the n x cols variable (group lasso)
    if (!a.prox[1]->DescribeSeparable(&sz)) return false;
    if (!(sz.kind == SeparableDesc::kZone && sz.g.n == 0) &&
        !(sz.kind == SeparableDesc::kRowGroups && cols > 1 && sz.cols == cols))
      return false;
    dt = a.data->dtype();
    if ((sz.alpha_vec.n > 0 && sz.alpha_vec.dt != dt) || (sz.beta_vec.n > 0 && sz.beta_vec.dt != dt)) return false;
    const std::string ck = affine::constraint_key(0);
    if (ls.constraint_key != ck || sz.constraint_key != ck || a.A.data().size() != 2) return false;
    const DenseMatrixImpl& L = *ls.L_arg_var;  // (tall: L(var, arg), trans() set: its buffer is A, m x n)
    if (L.trans() != ls.tall) return false;
    m = L.rows();
    n = L.cols();
    const int64_t nx = n * cols;  // entries of the variable (a matrix variable: column c at c * n)
    double a0 = 0;
    if (!ConsensusTie(a.A, ck, ls.var_key, sz.var_key, nx, &a0, &a1) || a0 != 1.0) return false;
    if (ls.tall) return EnableTall(a, tall_mode, ck);
    if (!k::LassoFusedSupported(m, n, L.data(), L.rows())) return false;
    if (ls.rhs_arg.n != 0 && ls.rhs_arg.n != m * cols) return false;
    if (cols > 1 && !ChooseMatrixRoute(matrix_mode)) return false;
    const std::vector<StateSlice> views = StateViews(a, ck, nx);
    grid = k::LassoFusedGrid(m, n, dt);
    // a matrix variable: column c's p and w at c * m (the wide route's instance-major panels,
    // whole panels of 64), its partials at c * grid * m
    const int64_t wlen = wide ? (cols + WideSweep::PW - 1) / WideSweep::PW * WideSweep::PW * m : cols * m;
    p = DVec::Zeros(wlen, dt);
    if (!wide) tpart = DVec::Empty(static_cast<int64_t>(grid) * m * cols, dt);
    if (cols > 1) {
      w = DVec::Zeros(wlen, dt);
    } else {
      Comm* comm = Runtime::Get().comm();
      PeerExchange* px = Runtime::Get().peer();
      sharded = sh.active() && sh.IsSharded(ls.var_key);
      // one-shot peer-write exchange inside the sweep's own kernels (kernels_peer.hip) when the
      // ranks share a window and the m-float message fits its slots; RCCL collectives otherwise
      // (a granule carries 32 value bits: an f64 value takes two)
      use_peer = sharded && px != nullptr && m * (dt == F64 ? 2 : 1) <= px->slot() && ls.Dinv_arg != nullptr &&
                 !ls.Dinv_arg->trans() && ls.Dinv_arg->rows() == m;
      const int G = use_peer ? px->view().G : (comm ? comm->size() : 1);
      slab = ((m + G - 1) / G + 3) / 4 * 4;
      wpad = DVec::Zeros(slab * G, dt);
      wslice = DVec::Zeros(slab, dt);
      w = wpad.Slice(0, m);  // the gathered vector IS w (first m entries)
      // the inverse is applied by row slabs + all-gather from 3 ranks up; with 2 ranks the
      // symmetric apply of the whole matrix reads the same m^2/2 entries and needs no exchange
      // EPSILON_HIP_SHARDED_APPLY=replicated: every rank applies the whole inverse instead (no
      // all-gather; m^2 bytes per rank) - the cheaper form when the collective's latency exceeds
      // the apply, to be decided on the machine
      const char* e = opt::Raw(opt::kShardedApply);
      replicated_apply = e && e[0] == 'r';
      const bool want_slab = e ? !replicated_apply : G >= 3;
      peer_slab = use_peer && want_slab && k::PeerSlabApplySupported(px->view(), m, slab, ls.Dinv_arg->data(), m);
    }
    if (!use_peer && !sh.active() && EnableWhiten()) {
      // no inverse apply in the sweep: no workspace, no packed copy
    } else if (wide) {
      // the inverse times the panel is a product of its own (WideSweep::ApplyInverse)
    } else {
      inv.Init(ls.Dinv_arg, m, p, w, a.shared_cache, cols);
    }
    if (wide) ws.Init(m, n, whiten ? Ahat : L.data(), whiten ? m : L.rows(), whiten, ls.Dinv_arg.get());
    BuildPass();
    AdoptState(views, Homes(a));
    ForwardFromState();
    return true;
  }

  // The six state vectors (x0, x1, y0, y1, u, y1prev; `nx` entries each) as slices of ONE buffer, so
  // that a residual check can snapshot the iterates with a single copy (pipelined checks,
  // Solver::Run), in the pass's record and as the table AdoptState takes.
  std::vector<StateSlice> StateViews(const MultiBlockParts& a, const std::string& ck, int64_t nx) {
    const int64_t npad = (nx + 63) / 64 * 64;
    state_all = DVec::Zeros(6 * npad, dt);
    snapshot = DVec::Empty(6 * npad, dt);
    norm_work = DVec::Zeros(64 * 5 + 1, F64);
    a.y_prev.resize(2);
    std::vector<StateSlice> views = {{&a.x[0], ls.var_key}, {&a.x[1], sz.var_key}, {&a.y[0], ck},
                                     {&a.y[1], ck},         {&a.u, ck},            {&a.y_prev[1], ck}};
    views[5].take = false;
    for (size_t q = 0; q < views.size(); ++q) views[q].v = state_all.Slice(static_cast<int64_t>(q) * npad, nx);
    k::ConsensusState& s = pass.inst.state;
    s.copy = views[0].v, s.var = views[1].v, s.y_zero = views[2].v, s.y_term = views[3].v, s.u = views[4].v;
    s.y_term_prev = views[5].v;
    return views;
  }

  // The tall form, after the gates that both forms share (Enable).  Any m > n and any n from the
  // floor up, odd ones included: the sweep never streams A, so LassoFusedSupported does not apply.
  bool EnableTall(const MultiBlockParts& a, int mode, const std::string& ck) {
    const DenseMatrixImpl& L = *ls.L_arg_var;
    const DenseMatrixImpl& D = *ls.Dinv_arg;
    if (ShardSpec::Get().active() || n < kLassoTallMinCols || m <= n) return false;
    if (!Allowed(mode, n, kLassoTallAutoMinCols)) return false;
    if (L.dtype() != dt || D.dtype() != dt || D.rows() != n || D.cols() != n) return false;
    if (!Fits(ls.rhs_arg, m, dt) || !Fits(sz.alpha_vec, n, dt) || !Fits(sz.beta_vec, n, dt)) return false;
    tall = tall_cols = true;
    const std::vector<StateSlice> views = StateViews(a, ck, n);
    p = DVec::Zeros(n, dt);  // r, the apply's input
    w = DVec::Zeros(n, dt);  // the dense apply's output (below the packed floor)
    inv.Init(ls.Dinv_arg, n, p, w, a.shared_cache);
    // c at every Init: parameters re-bind the rhs (nothing here is keyed on A)
    if (ls.rhs_arg.n != 0) {
      crhs = DVec::Empty(n, dt);
      ProfScope prof("lasso_tall_rhs", m, n);
      L.Apply(1.0, ls.rhs_arg, 0.0, crhs);
    }
    k::LassoInstance& s = pass.inst;
    s.w = w;
    s.p = p;
    s.tpart = inv.work;  // the tile partials (empty below the packed floor)
    s.rhs = crhs;
    s.kappa = s.pkappa = D.scale();  // x0 = scale * (tiles' sum), SymvPacked's alpha
    s.zone = ZoneOf(sz, a1);
    AdoptState(views, Homes(a));
    // r of the first sweep from the adopted state: v0 - c
    FirstInput(s.state, p);
    if (crhs.n != 0) k::Axpby(p, -1.0, crhs, 1.0);
    return true;
  }

  // Route of a matrix-variable solve: the batched pass (f32 / f64) or the wide
  // kernels (f32).  The group threshold needs all columns in one launch (pass) or one panel (wide).
  bool ChooseMatrixRoute(int mode) {
    const DenseMatrixImpl& L = *ls.L_arg_var;
    const DenseMatrixImpl& D = *ls.Dinv_arg;
    const bool group = sz.kind == SeparableDesc::kRowGroups;
    if (m < kMatrixFusedMinRows || L.dtype() != dt || D.dtype() != dt) return false;
    if (group && sz.rows != n) return false;
    if (sz.alpha_vec.n > 0 && sz.alpha_vec.n != n * cols) return false;
    if (sz.beta_vec.n > 0 && sz.beta_vec.n != n * cols) return false;
    if (D.rows() != m || D.cols() != m) return false;
    const int width = k::LassoBatchWidth(m, n, dt);
    const bool pass_ok = width > 0 && (!group || cols <= width);
    const bool wide_ok = dt == F32 && k::LassoWideSupported(m, n, L.data(), L.rows()) &&
                         (!group || cols <= WideSweep::PW);
    if (mode == kMatrixPass) wide = false;
    else if (mode == kMatrixWide) wide = true;
    else wide = wide_ok && (cols >= BatchWideMin() || !pass_ok);
    return wide ? wide_ok : pass_ok;
  }

  // The whitened route.  With Dinv_arg = c X^T X, where X = L^-1 is the inverse Cholesky factor
  // kept by DenseMatrixImpl::Inverse, the forward product of a sweep is
  //   d = A^T Dinv p = c (X A)^T (X p),   X p = X rhs - s_L (X A) v,
  // so the pass streams A_hat = X A (same shape as A, formed once at Init) and its partials reduce
  // to w_hat = X p directly: no m x m matrix is read in the sweep.  f32, one GPU, m >= 2048, n >= 2m.
  bool EnableWhiten() {
    const DenseMatrixImpl& L = *ls.L_arg_var;
    const DenseMatrixImpl& D = *ls.Dinv_arg;
    OpCache* cache = CurrentOpCache();
    if (!FusedWhitenEnabled() || cache == nullptr || dt != F32 || L.dtype() != F32 || m < kWhitenMinRows)
      return false;
    // wide data only: A_hat is formed on the split-f16 matrix cores (about 4x the f32 rounding), and
    // a nearly square A amplifies that in the iterates (10244 x 10260: 4e-5 off the generic path
    // after 200 sweeps, twice the fused path's parity tolerance)
    if (n < 2 * m) return false;
    if (D.id() == 0 || D.trans() || D.rows() != m || D.cols() != m || L.rows() != m) return false;
    // X belongs to exactly this inverse: the cached entry under D's key holds D's own buffer
    const auto cached = cache->Find(D.id());
    const auto Xm = cache->Find(FactorInverseKey(D.id()));
    if (!cached || !Xm || cached->data().data() != D.data().data() || Xm->rows() != m || Xm->cols() != m)
      return false;
    // A_hat is shared like the packed inverse: a warm re-Init and the members of a batch find it
    const uint64_t key = HashCombine(HashCombine(HashCombine(HashCombine(Xm->id(), 0x3a7),
                                                             reinterpret_cast<uintptr_t>(L.data().data())),
                                                 L.id()),
                                     static_cast<uint64_t>(n));
    DVec Ah;
    if (auto hit = cache->Find(key)) {
      Ah = hit->data();
    } else {
      Ah = DVec::Empty(m * n, F32);
      // X is lower triangular: each tile of the product runs over its own k range
      if (!k::GemmSplitF16KRange(4, m, n, m, 1.0, Xm->data(), m, L.data(), m, Ah, m))
        k::Gemm(false, false, m, n, m, 1.0, Xm->data(), m, L.data(), m, 0.0, Ah, m);
      cache->Put(key, std::make_shared<DenseMatrixImpl>(Ah, m, n, false, 1.0, key));
    }
    if (!k::LassoFusedSupported(m, n, Ah, m)) return false;
    // X rhs on every Init: parameters re-bind the rhs
    if (ls.rhs_arg.n != 0 && cols > 1) {  // all columns in one product
      rhat = DVec::Empty(m * cols, F32);
      k::Gemm(false, false, m, cols, m, 1.0, Xm->data(), m, ls.rhs_arg, m, 0.0, rhat, m);
    } else if (ls.rhs_arg.n != 0) {
      rhat = DVec::Empty(m, F32);
      k::Gemv(false, m, m, 1.0, Xm->data(), m, ls.rhs_arg, 0.0, rhat);
    }
    X = Xm->data();
    Ahat = Ah;
    wscale = D.scale();
    whiten = true;
    return true;
  }

  // w of the first sweep from the current state: p = rhs_arg - L(arg,var) v0 with
  // v0 = ((u - y0) - y1) + y0, column by column for a matrix variable, then w = Dinv_arg p
  // (whitened: w_hat = X p).
  void ForwardFromState() {
    const DenseMatrixImpl& L = *ls.L_arg_var;
    const k::ConsensusState& s = pass.inst.state;
    DVec v0 = DVec::Empty(s.u.n, s.u.dt);
    FirstInput(s, v0);
    if (cols == 1 && !whiten) {
      L.Apply(-1.0, v0, 0.0, p);
      ForwardTail(/*reduced=*/false);
      return;
    }
    const int64_t mk = m * cols;
    DVec pp = whiten && cols > 1 ? DVec::Empty(mk, v0.dt) : p.Slice(0, mk);
    for (int64_t c = 0; c < cols; ++c) L.Apply(-1.0, v0.Slice(c * n, n), 0.0, pp.Slice(c * m, m));
    if (ls.rhs_arg.n != 0) k::Axpby(pp, 1.0, ls.rhs_arg, 1.0);
    for (int64_t c = 0; whiten && c < cols; ++c)
      k::Gemv(false, m, m, 1.0, X, m, pp.Slice(c * m, m), 0.0, w.Slice(c * m, m));
    if (!whiten) ApplyInverseFixed();
  }

  // The vector form's tail, one GPU or RCCL: p from the pass's partials (`reduced`) or as
  // ForwardFromState left it, all-reduced when sharded, + rhs_arg, then w = Dinv_arg p.
  void ForwardTail(bool reduced) {
    const DenseMatrixImpl& L = *ls.L_arg_var;
    if (whiten) {
      k::ReducePartials(m, grid, tpart, -L.scale(), 0.0, w, rhat.n != 0 ? &rhat : nullptr);
      return;
    }
    bool rhs_added = false;
    if (reduced) {
      // the constant part of the rhs rides in the reduction kernel (same rounding order as the
      // separate axpy: sum first, then + rhs); in a sharded run rank 0 alone contributes it to
      // the sum over ranks - one launch less in a sweep that is launch-latency-bound at N = 8
      const bool have_rhs = ls.rhs_arg.n != 0;
      const bool fold = have_rhs && (!sharded || Runtime::Get().comm()->rank() == 0);
      k::ReducePartials(m, grid, tpart, -L.scale(), 0.0, p, fold ? &ls.rhs_arg : nullptr);
      rhs_added = have_rhs;  // folded here, or by rank 0 into the all-reduced sum
    }
    if (sharded) Runtime::Get().comm()->AllReduceSum(p);
    if (ls.rhs_arg.n != 0 && !rhs_added) k::Axpby(p, 1.0, ls.rhs_arg, 1.0);
    const DenseMatrixImpl& D = *ls.Dinv_arg;
    Comm* comm = Runtime::Get().comm();
    if (sharded && comm->size() > 1 && !D.trans() && D.rows() == m && !replicated_apply) {
      // The cached inverse is replicated and symmetric: each rank applies only its slab of rows
      // (= columns, read contiguously) and the slices are all-gathered, so the m^2 bytes of the
      // apply are split over the ranks like the data matrix is.
      const int64_t per = slab;  // multiple of 4, G*per >= m
      const int64_t lo = std::min<int64_t>(m, comm->rank() * per);
      const int64_t cnt = std::min<int64_t>(m, lo + per) - lo;
      DVec mine = wslice;
      if (cnt < per) k::Fill(mine, 0.0);
      if (cnt > 0) {
        DVec rows = D.data().Slice(lo * m, cnt * m);
        k::Gemv(true, m, cnt, D.scale(), rows, m, p, 0.0, mine.Slice(0, cnt));
      }
      comm->AllGather(mine.data(), wpad.data(), static_cast<size_t>(per), wpad.dt);
    } else {
      ApplyInverseFixed();
    }
  }

  // The sharded sweep's tail on the peer window: 2 launches, no collective call.
  void ForwardTailPeer() {
    const DenseMatrixImpl& L = *ls.L_arg_var;
    const DenseMatrixImpl& D = *ls.Dinv_arg;
    const PeerView& pv = Runtime::Get().peer()->view();
    k::PeerReduceExchange(pv, m, grid, tpart, -L.scale(), ls.rhs_arg.n != 0 ? &ls.rhs_arg : nullptr, p);
    if (peer_slab) {
      const int64_t lo = std::min<int64_t>(m, static_cast<int64_t>(pv.rank) * slab);
      k::PeerSlabApplyExchange(pv, m, slab, lo, D.data(), m, D.scale(), p, wpad);
    } else {
      ApplyInverseFixed();
    }
  }

  // w = Dinv p, every column
  void ApplyInverseFixed() {
    if (wide) {
      for (int64_t q = 0; q * ws.panel_len < w.n; ++q)
        ws.ApplyInverse(p.Slice(q * ws.panel_len, ws.panel_len), w.Slice(q * ws.panel_len, ws.panel_len));
    } else if (cols == 1) {
      inv.Apply();
    } else if (inv.packed.n > 0) {
      k::SymvPackedBatch(m, inv.D->scale(), inv.packed, table, static_cast<int>(cols), inv.work);
    } else {
      for (int64_t c = 0; c < cols; ++c) inv.Column(c).Apply();
    }
  }

  // The pass's arguments with the instance as the kernels read it, once per Init: EnableWhiten has
  // decided the matrix, kappa, p and rhs by now.  Only the peer exchange's epoch is set per sweep.
  void BuildPass() {
    const DenseMatrixImpl& L = *ls.L_arg_var;
    pass.m = m;
    pass.n = n;
    pass.lda = whiten ? m : L.rows();
    pass.A = whiten ? Ahat : L.data();
    res = Residency(cols, &pass);
    k::LassoInstance& s = pass.inst;
    s.w = w;
    s.tpart = tpart;
    // whitened route: the reduction writes w_hat itself, with X rhs folded in
    s.p = whiten ? w : p;
    s.rhs = whiten ? rhat : ls.rhs_arg;
    // x0 = v0 + kappa A^T w (whitened: c A_hat^T w_hat)
    s.kappa = -L.scale() * (whiten ? wscale : 1.0);
    s.pkappa = -L.scale();
    s.zone = ZoneOf(sz, a1);
    if (cols == 1) return;
    // a matrix variable: column c is member c, the slices of `inst` at its offsets; the table is
    // uploaded here, so that a sweep makes no upload and no host synchronisation
    members.assign(static_cast<size_t>(cols), s);
    for (int64_t c = 0; c < cols; ++c) {
      k::LassoInstance& mb = members[static_cast<size_t>(c)];  // (a copy of `inst`: sliced in place)
      auto col = [&](const DVec& v, int64_t len) { return v.n > 0 ? v.Slice(c * len, len) : v; };
      mb.w = col(s.w, m);
      mb.p = col(s.p, m);
      mb.rhs = col(s.rhs, m);
      if (!wide) mb.tpart = col(s.tpart, static_cast<int64_t>(grid) * m);
      else mb.tpart = mb.w;  // (not read on the wide route: its partials are panels of WideSweep)
      k::ConsensusState& ms = mb.state;
      for (DVec* v : {&ms.u, &ms.var, &ms.copy, &ms.y_term, &ms.y_zero, &ms.y_term_prev, &mb.zone.alpha_vec,
                      &mb.zone.beta_vec})
        *v = col(*v, n);
    }
    std::vector<const k::LassoInstance*> v;
    for (const auto& mb : members) v.push_back(&mb);
    rhs_aligned = RhsAligned(v);
    k::LassoBatchUpload(v, dt, &table);
  }

  // A matrix variable's sweep: its columns through the batched or the wide kernels.
  void MatrixSweep() {
    const int K = static_cast<int>(cols);
    const double* group_lam = sz.kind == SeparableDesc::kRowGroups ? &sz.lam : nullptr;
    if (wide) {
      constexpr int PW = WideSweep::PW;
      for (int first = 0; first < K; first += PW) {
        const int nk = std::min(PW, K - first);
        const uint64_t live = nk == 64 ? ~uint64_t(0) : (uint64_t(1) << nk) - 1;
        const int64_t off = static_cast<int64_t>(first) * m;
        ws.Run(table, first, nk, live, w.Slice(off, ws.panel_len), whiten ? DVec() : p.Slice(off, ws.panel_len),
               group_lam);
      }
      return;
    }
    BatchSweep(table, DVec(), DVec(), K, group_lam, res, rhs_aligned, inv.work, [&] {
      for (int64_t c = 0; c < cols; ++c) inv.Column(c).Apply();
    });
  }

  void Sweep() override {
    if (tall) {
      const bool tiles = inv.packed.n > 0;  // two launches: the tiles, then their sum and the chain
      if (tiles) k::SymvPackedTiles(n, inv.packed, p, inv.work);
      else inv.Apply();
      k::LassoTallCols(n, pass.inst, tiles);
    } else if (cols > 1) {
      MatrixSweep();
    } else if (use_peer) {
      pass.epoch = Runtime::Get().peer()->view().epoch;
      k::LassoFusedPass(pass);
      ForwardTailPeer();
    } else {
      k::LassoFusedPass(pass);
      ForwardTail(/*reduced=*/true);
    }
  }

  // ---- residual check: one launch, splittable for pipelining -----------------------------------
  // With A = [a0 I, a1 I] (a0 = 1), b empty and N = 2 the quantities of prox_admm.cc:178-217 are
  //   ||A x_i|| = ||y_i||,  r = ||y0 + y1||,  s = rho ||A_0^T (y1 - y1_prev)|| = rho ||y1 - y1_prev||,
  //   ||A^T u||^2 = (a0^2 + a1^2) ||u||^2.
  bool HasCheck() const override { return true; }
  bool PipelineChecks() const override {
    static const bool off = opt::Is0(opt::kPipelineChecks);
    return !off;
  }
  // the check's six scalars into the next six slots
  void LaunchNorms() override {
    Runtime& rt = Runtime::Get();
    norm_slot = rt.NewSlot();
    for (int q = 1; q < 6; ++q) rt.NewSlot();
    const k::ConsensusState& s = pass.inst.state;
    k::LassoFusedNorms(s.u, s.y_zero, s.y_term, s.y_term_prev,
                       sharded ? rt.ShardSlotPtr(norm_slot) : rt.SlotPtr(norm_slot), norm_work,
                       use_peer ? rt.peer()->device_error_word() : nullptr,
                       tall ? "lasso_tall_norms" : "lasso_fused_norms");
  }
  Check FinishCheck() override {
    Runtime& rt = Runtime::Get();
    // a timed-out exchange on ANY rank shows in the all-reduced sixth value: every rank raises at
    // the same check, none is left waiting in a collective the others never enter
    if (rt.SlotValue(norm_slot + 5) > 0) {
      rt.Sync();
      if (rt.peer()) rt.peer()->ClearError();
      EPS_FATAL("peer exchange: a poll timed out on at least one rank (a peer did not deliver its part)");
    }
    const double ny0 = rt.SlotValue(norm_slot), ny1 = rt.SlotValue(norm_slot + 1), nr = rt.SlotValue(norm_slot + 2),
                 ns = rt.SlotValue(norm_slot + 3), nu = rt.SlotValue(norm_slot + 4);
    Check c;
    c.r = std::sqrt(nr);
    c.s = std::sqrt(ns);
    c.max_norm = std::fmax(std::sqrt(ny0), std::sqrt(ny1));
    c.atu = std::sqrt((1.0 + a1 * a1) * nu);
    return c;
  }
  void SaveSnapshot() override { k::Copy(snapshot, state_all); }
  void RestoreSnapshot() override {
    Runtime::Get().Sync();  // let the discarded sweeps drain
    if (Runtime::Get().peer()) Runtime::Get().peer()->CheckError();
    k::Copy(state_all, snapshot);
  }

  bool Capturable() const override {
    const bool fixed_buffers = (use_peer && peer_slab) || inv.work.n > 0 || whiten || wide;
    return fixed_buffers && !(sharded && !use_peer);  // (RCCL calls in the sweep are not captured)
  }
  bool CaptureByDefault() const override { return use_peer; }

  // ---- batched solves (RunFusedBatches) ---------------------------------------------------------
  // The key of the group a fresh solve on this route can join (same data matrix, inverse, dtype,
  // shape and schedule); false: its pass is none the batched one mirrors.
  // Tall: the same inverse with its packed copy (n >= 1024), n, the dtype and the schedule; lambda,
  // the zone's parameters and b are per member.
  bool BatchKey(const pb::SolverParams& params, bool, std::vector<uint64_t>* key) const override {
    if (use_peer || ShardSpec::Get().active()) return false;
    if (tall) {
      if (inv.packed.n == 0) return false;
      *key = {kTallLassoKey, reinterpret_cast<uintptr_t>(inv.D->data().data()), Bits(inv.D->scale()),
              reinterpret_cast<uintptr_t>(inv.packed.data()), static_cast<uint64_t>(n), static_cast<uint64_t>(dt),
              static_cast<uint64_t>(params.max_iterations), static_cast<uint64_t>(params.epoch_iterations)};
      return true;
    }
    if (cols > 1) return false;  // a matrix variable is a batch of its own: it runs alone
    const DenseMatrixImpl& L = *ls.L_arg_var;
    if (L.dtype() != dt || k::LassoBatchWidth(m, n, dt) == 0) return false;
    *key = KeyHead(L, *ls.Dinv_arg, params);
    key->insert(key->end(), {whiten ? 1u : 0u, reinterpret_cast<uintptr_t>(Ahat.data())});
    return true;
  }
};

// ---------------------------------------------------------------------------------------------------
// The ZERO-term route
// ---------------------------------------------------------------------------------------------------
// Recognised structure: the last term is a ZERO term over private copies (x', and z' unless the
// problem has no z: basis pursuit) whose block LDL^T is the projection ZeroProx describes; the
// other terms are one scaled-zone term on x and at most one on z (which may carry an offset, and
// may be SUM_LOGISTIC, a smooth separable term, instead of a scaled zone),
// each tied to its copy by a consensus constraint copy + a var = 0 without a constant.  The
// sweep is then: the pass over the data matrix (k::kChainZeroCols: back product, column chain, forward
// product), the row kernel (row chain, the partials' sum, r) - basis pursuit: the partials'
// reduction alone - and the apply of the cached inverse.  The residual check is the driver's
// generic one on views of the state, or - option "fused_zero_check" = "1" - one launch of the route's
// own, pipelined with the sweeps.  One GPU, every dtype the compute type.
//
// Tall C (`tall`, DESIGN.md 3.11 "Tall C"): the same terms and ties with the ZERO term's block
// LDL^T in the tall order: arg is a scalar pivot, x' the dense one.
// Everything between C x' of sweep k and C^T f_arg of sweep k+1 is element-wise in the sample, so
// the pass streams C^T (features x samples, one contiguous copy made at Init): per sample the
// product with x', the z-side chain and the forward product (k::kChainZeroTall); then the x-side kernel (the
// partials' sum, the chain on x, f_x) and the apply of Dinv(x').  A smooth z term (`samples_smooth`:
// SUM_LOGISTIC, under the option "fused_zero_tall_smooth") has its Newton in a kernel of its own over
// the samples, between the two halves of the pass: the dot products C x' (k::kChainZeroTallDot), the sample kernel
// with the carried head, the forward product (k::kChainZeroTallAcc).  Under the option "batch_zero_tall" the tall
// members of a batch that share C run as one group ("Tall members"); without it each is
// solved by itself.
//
// A ridge term on x (`sx` of kind kRidge, option "fused_zero_ridge"; DESIGN.md 3.11 "A ridge term on
// x"): the term on x may be SUM_SQUARE with a scalar argument map instead of a scaled zone; sx.Bs,
// sx.Cs are then the two factors of its block solve (SeparableDesc).  The side that owns x - the pass
// on fat C, the x-side kernel on tall C - then takes the block solve's two multiplies in the
// threshold's place; everything else is as above.
// Single solves on the multi-block driver alone: such a member of a batch is solved by itself.
//
// A linear term on x, the non-negative cone on z (`sx` of kind kLinear, `sz` of kind kNonNegative,
// option "fused_zero_lp" = "1"; DESIGN.md 3.11 "A linear term on x, a cone on z"): the two heads that
// problems.lp needs.  Each stands in its side's threshold's place - on fat C the linear step in the
// pass and the cone in the rows, on tall C the cone in the pass and the linear step in the x-side
// kernel - and the sides are independent, so either also runs with the other side's zone, ridge or
// smooth term.  The 256-thread shapes and single solves alone; never with free x.
//
// Free x (`zp.x_free`, option "fused_zero_xfree" = "1"; DESIGN.md 3.11 "x in the ZERO term alone"): no
// term on x, so x is no copy - it lives in the ZERO term alone and has no constraint row
// (least_abs_dev, quantile).  The tall form with one constraint and one separable term, a zone on z:
// the pass with k::kChainZeroTall as it is, an x side that is the partials' sum alone (k::kRowsXFree: x kept in
// `xcur`, f_x = pkappa sum, no state and no chain) and the apply of Dinv(x) = (C^T C / e^2)^-1, which
// exists for m > n alone - asked for here, since the factorisation has the same order for fat C.
// Under "batch_zero_tall" such members that share C form groups of their own.
struct ZeroRoute final : BatchRoute {
  using Side = k::ConsensusState;  // of the x constraint, of the z constraint

  ZeroProjectionDesc zp;
  // the separable terms on x (a zone, a ridge term or a linear term) and on z (a zone, smooth or the cone)
  SeparableDesc sx, sz;
  bool tall = false;
  bool has_z = false;
  // m, n: C is m x n.  w, p, tpart: the dense pivot's vectors (tall: x' of the coming sweep, f_x and
  // the pass's partials, n-long)
  DVec state_n, state_m;  // the slices of a side's state in one buffer (n: the x constraint's rows)
  DVec xcur;  // free x: the whole x side - x as the pass of the last sweep read it (no u, no y)
  DVec CT;    // tall: C^T, n x m, ld n: shared through the solve's cache
  DVec head;  // a smooth z term: the carried head (s, y_s, v of the coming sweep)
  k::ZeroRowsArgs rows;  // the side that is not in the pass: z (tall: x)
  // tall with a smooth z term: the sample kernel's record, its vectors d and f_arg, and the second
  // half of the pass (`pass` is the first)
  bool samples_smooth = false;
  k::ZeroTallSamplesArgs samples;
  DVec dfarg;
  k::LassoFusedArgs acc;
  // The residual check of the route's own (option "fused_zero_check" = "1"; DESIGN.md 3.11 "The
  // residual check"): everything a sweep hands to the next - w, either side's state, free x, the
  // carried head - then lies in ONE buffer, so that a snapshot is one copy.  Off: none of this exists.
  bool own_check = false;
  DVec carried, snapshot;
  int64_t carried_used = 0;
  double ax = 0, az = 0;  // the constraint maps of x and z (their copies': 1)
  Side check_x, check_z;  // the sides as the norms kernel reads them (absent: empty)
  DVec norm_work;         // partials + ticket of the one-launch residual norms
  int norm_slot = 0;

  // `len` zeroed values of what a sweep hands to the next: a buffer of their own, or - with a check
  // of the route's own - the next slice of `carried`, on a 64-value boundary.
  DVec Carried(int64_t len) {
    if (!own_check) return DVec::Zeros(len, dt);
    EPS_CHECK(carried_used + len <= carried.n);
    const DVec v = carried.Slice(carried_used, len);
    carried_used += (len + 63) / 64 * 64;
    return v;
  }

  // `tall_mode`, `tall_smooth_mode`, `ridge_mode`: the options "fused_zero_tall",
  // "fused_zero_tall_smooth" and "fused_zero_ridge"; under "auto" the measured floors apply.
  // `xfree_on`, `lp_on`, `check_on`: the options "fused_zero_xfree", "fused_zero_lp" and
  // "fused_zero_check" are "1"
  bool Enable(const MultiBlockParts& a, int tall_mode, int tall_smooth_mode, int ridge_mode, bool xfree_on,
              bool lp_on, bool check_on) {
    if (opt::Is0(opt::kFused) || ShardSpec::Get().active() || !a.b.data().empty()) return false;
    const int nc = a.num_constraints, N = static_cast<int>(a.prox.size());
    if (nc < 1 || nc > 2 || N != nc + 1) return false;
    if (!a.prox[N - 1]->DescribeZeroProjection(&zp)) return false;
    tall = zp.tall;
    has_z = !zp.z_key.empty();
    // free x: the tall form with one constraint, the z tie, and one separable term, the one on z
    const bool xfree = zp.x_free;
    if (xfree && (!xfree_on || !tall || !has_z || nc != 1)) return false;
    if (!xfree && has_z != (nc == 2)) return false;
    int ix = -1, iz = -1;  // positions of the separable terms among the objective terms
    for (int i = 0; i + 1 < N; ++i) {
      SeparableDesc d;
      if (!a.prox[i]->DescribeSeparable(&d)) return false;
      // accepted on x: a zone without offset, a ridge term, or - "fused_zero_lp" - a linear term; on z: a
      // zone (its offset with it), a smooth term (tall: SUM_LOGISTIC alone), or - "fused_zero_lp" - the
      // non-negative cone (its offset with it) - each once, on its own constraint row
      const bool zone = d.kind == SeparableDesc::kZone, smooth = d.kind == SeparableDesc::kSmooth;
      const bool linear = lp_on && d.kind == SeparableDesc::kLinear;
      const bool nonneg = lp_on && d.kind == SeparableDesc::kNonNegative;
      // free x: no term on x, and on z a zone alone (a smooth z term and the cone keep the generic path)
      const bool on_x = !xfree && ((zone && d.g.n == 0) || d.kind == SeparableDesc::kRidge || linear);
      const bool on_z = zone || ((smooth || nonneg) && !xfree && (!tall || !smooth || d.fn == k::SMOOTH_LOGISTIC));
      if (on_x && ix < 0 && d.constraint_key == zp.x_constraint_key) {
        sx = d;
        ix = i;
      } else if (on_z && has_z && iz < 0 && d.constraint_key == zp.z_constraint_key) {
        sz = d;
        iz = i;
      } else {
        return false;
      }
    }
    if ((!xfree && ix < 0) || (has_z && iz < 0)) return false;
    // the two sides' heads (a side without a term - free x, no z - has the default, the zone)
    const k::Head hx = HeadOf(sx.kind), hz = HeadOf(sz.kind);
    const bool x_ridge = hx == k::kHeadRidge;
    const bool lp_head = hx == k::kHeadLinear || hz == k::kHeadNonNeg;
    // (the smooth form belongs to the z side: tall, that is the sample kernel, not the rows)
    samples_smooth = tall && hz == k::kHeadSmooth;
    (tall ? samples.fn : rows.fn) = sz.fn;
    // the pass as FillTall / FillFat set it up: the z side over the transposed copy (in halves
    // around the sample kernel, which then has the head), or the x side
    const k::Chain chain = !tall ? k::kChainZeroCols : samples_smooth ? k::kChainZeroTallDot : k::kChainZeroTall;
    const k::Head pass_head = !tall ? hx : samples_smooth ? k::kHeadZone : hz;
    const DenseMatrixImpl& L = *zp.L;  // (tall: trans() set: its buffer is C, m x n)
    const DenseMatrixImpl& D = *zp.Dinv;
    dt = a.data->dtype();
    m = L.rows();
    n = L.cols();
    const int64_t nw = tall ? n : m;  // the order of the dense pivot
    if (L.dtype() != dt || D.dtype() != dt || D.rows() != nw || D.cols() != nw) return false;
    if (tall) {
      if (n < kZeroTallMinCols || m <= n || !Allowed(tall_mode, n, kZeroTallAutoMinCols)) return false;
      // the pass's shape conditions, on the copy's geometry, before the copy is made
      const int64_t chunk = dt == F32 ? 4 : 2;
      if (n % chunk != 0 || n > (dt == F32 ? 20 : 10) * 1024) return false;
      if (samples_smooth && !Allowed(tall_smooth_mode, n, kZeroTallSmoothAutoMinCols)) return false;
      const int64_t ridge_floor = samples_smooth ? kZeroRidgeTallSmoothAutoMinCols : kZeroRidgeTallAutoMinCols;
      if (x_ridge && !Allowed(ridge_mode, n, ridge_floor)) return false;
    } else {
      if (m < kZeroFusedMinRows || !k::LassoFusedSupported(m, n, L.data(), L.rows())) return false;
      if (x_ridge && !Allowed(ridge_mode, m, kZeroRidgeAutoMinRows)) return false;
    }
    // the pass's form exists in this thread shape (the halves, the linear and the non-negative head:
    // 256 threads alone); "fused_zero_lp" takes the 256-thread shapes alone on whichever side its head is
    const int block = tall ? k::LassoFusedBlock(n, m, dt) : k::LassoFusedBlock(m, n, dt);
    if (!k::FusedPassExists(chain, pass_head, block) || (lp_head && block != 256)) return false;
    // the consensus constraints: copy + a var = 0, nothing else in their rows or columns
    // (free x: the one tie is all there is, so no column of A is x's)
    if (static_cast<int>(a.A.data().size()) != 2 * nc || (xfree && a.A.data().count(zp.x_key) != 0)) return false;
    auto tie = [&](const std::string& ck, const std::string& copy, const std::string& var, int64_t len, double* av) {
      double a0 = 0;
      return ConsensusTie(a.A, ck, copy, var, len, &a0, av) && a0 == 1.0 && a.A.col(copy).size() == 1 &&
             a.A.col(var).size() == 1;
    };
    if (!xfree && !tie(zp.x_constraint_key, zp.x_key, sx.var_key, n, &ax)) return false;
    if (has_z && !tie(zp.z_constraint_key, zp.z_key, sz.var_key, m, &az)) return false;
    if (!Fits(zp.rhs_arg, m, dt) || !Fits(sx.alpha_vec, n, dt) || !Fits(sx.beta_vec, n, dt)) return false;
    if (!Fits(sz.alpha_vec, m, dt) || !Fits(sz.beta_vec, m, dt) || !Fits(sz.g, m, dt)) return false;
    if (hx == k::kHeadLinear ? (sx.g.n != n || sx.g.dt != dt) : sx.g.n != 0) return false;  // the linear term's vector, and no other
    if (tall && !TransposedCopy(a.shared_cache)) return false;
    own_check = check_on;
    if (own_check) {
      auto pad = [](int64_t len) { return (len + 63) / 64 * 64; };
      const bool smooth = hz == k::kHeadSmooth;
      const int64_t sides = (xfree ? pad(n) : 7 * pad(n)) + (has_z ? 7 * pad(m) : 0);
      carried = DVec::Zeros(pad(nw) + sides + (smooth ? pad(3 * m) : 0), dt);
      snapshot = DVec::Empty(carried.n, dt);
      norm_work = DVec::Zeros(k::kZeroNormsWork, F64);
    }

    // state: u, var, copy, y of the separable term, y of the ZERO term, their previous values -
    // per constraint row, taken over from the generic containers (warm start)
    a.y_prev.resize(N);
    std::vector<StateSlice> views;
    auto side = [&](int64_t len, const std::string& ck, int term, const std::string& var, const std::string& copy,
                    DVec* all) {
      const int64_t pad = (len + 63) / 64 * 64;
      *all = Carried(7 * pad);
      Side s;
      int64_t q = 0;  // the next slice of `all`
      auto slice = [&](DVec* v, BlockVector* home, const std::string& key, bool take = true) {
        *v = all->Slice(q++ * pad, len);
        views.push_back({home, key, *v, take});
      };
      slice(&s.u, &a.u, ck);
      slice(&s.var, &a.x[term], var);
      slice(&s.copy, &a.x[N - 1], copy);
      slice(&s.y_term, &a.y[term], ck);
      slice(&s.y_zero, &a.y[N - 1], ck);
      slice(&s.y_term_prev, &a.y_prev[term], ck, false);
      slice(&s.y_zero_prev, &a.y_prev[N - 1], ck, false);
      return s;
    };
    // (tall: the pass's register-held dimension is n, its streamed columns are the m samples)
    grid = tall ? k::LassoFusedGrid(n, m, dt) : k::LassoFusedGrid(m, n, dt);
    w = Carried(nw);
    p = DVec::Zeros(nw, dt);
    tpart = DVec::Empty(static_cast<int64_t>(grid) * nw, dt);
    inv.Init(zp.Dinv, nw, p, w, a.shared_cache);
    // (free x: x itself is the x side, a view of the ZERO term's own variable like a copy is)
    Side sn;
    if (xfree) {
      xcur = Carried(n);
      views.push_back({&a.x[N - 1], zp.x_key, xcur, true});
    } else {
      sn = side(n, zp.x_constraint_key, ix, sx.var_key, zp.x_key, &state_n);
    }
    const Side sm = has_z ? side(m, zp.z_constraint_key, iz, sz.var_key, zp.z_key, &state_m) : Side();
    check_x = sn;
    check_z = sm;
    if (tall) FillTall(sn, ax, sm, az);
    else FillFat(sn, ax, sm, az);
    // beside the matrix the sweep touches the partials (the rows kernel re-reads them), the seven
    // state vectors of either side (free x: x alone on its side), p, w, the inverse, and the sample
    // kernel's head, d and f_arg
    res = ResidentShare(pass.m, pass.n, dt,
                        static_cast<int64_t>(grid) * nw + (xfree ? 7 * m + n : 7 * (n + m)) + 2 * nw + nw * nw +
                            head.n + dfarg.n,
                        /*auto_on=*/false, &pass);
    if (samples_smooth) {  // the share holds for both halves: the matrix is read twice per sweep
      acc = pass;
      acc.chain = k::kChainZeroTallAcc;
    }
    EPS_CHECK(pass.chain == chain && pass.inst.zone.head == pass_head);
    AdoptState(views, Homes(a));
    if (rows.zone.head == k::kHeadSmooth) k::ZeroSmoothHead(rows);
    if (samples_smooth) k::ZeroTallSamplesHead(samples);
    ForwardFromState(a);
    return true;
  }

  // Tall: C^T as the pass streams it: one untransposed contiguous copy of the factor's operand
  // (unscaled: the scale stays in kappa), shared like the packed inverse
  bool TransposedCopy(OpCache* shared) {
    const DenseMatrixImpl& L = *zp.L;
    uint64_t key = 0;
    if (shared != nullptr) {
      key = HashCombine(HashCombine(HashCombine(reinterpret_cast<uintptr_t>(L.data().data()), 0x7a11c7), L.id()),
                        static_cast<uint64_t>(m * n));
      if (auto hit = shared->Find(key)) CT = hit->data();
    }
    if (CT.n == 0) {
      CT = DVec::Empty(m * n, dt);
      ProfScope prof("transpose_copy", n, m);  // (a setup step: the members of a batch share one copy)
      k::MatCopy(true, n, m, 1.0, L.data(), L.rows(), CT);
      if (key) shared->Put(key, std::make_shared<DenseMatrixImpl>(CT, n, m, false, 1.0, key));
    }
    return k::LassoFusedSupported(n, m, CT, n);
  }

  // The pass's instance from the side it runs (the two ZERO chains read the arrays alike, k::Chain),
  // the row kernel's record from the other side.
  void PassSide(k::Chain chain, const Side& s, const SeparableDesc& zone, double a1) {
    pass.chain = chain;
    k::LassoInstance& i = pass.inst;
    i.w = w;
    i.tpart = tpart;
    i.p = p;
    i.state = s;
    i.zone = ZoneOf(zone, a1);
    i.kappa = i.pkappa = -zp.L->scale();
  }
  void RowsSide(const Side& s, const SeparableDesc& zone, double a1) {
    rows.m = w.n;
    rows.nparts = grid;
    rows.w = w;
    rows.tpart = tpart;
    rows.r = p;
    rows.state = s;
    rows.zone = ZoneOf(zone, a1);
    rows.pkappa = -zp.L->scale();
  }

  // Fat: the x side into the pass (k::kChainZeroCols), the z side into the rows.
  void FillFat(const Side& sn, double ax, const Side& sm, double az) {
    pass.m = m;
    pass.n = n;
    pass.lda = zp.L->rows();
    pass.A = zp.L->data();
    PassSide(k::kChainZeroCols, sn, sx, ax);
    pass.inst.rhs = zp.rhs_arg;
    if (pass.inst.zone.head == k::kHeadLinear) pass.inst.zg = sx.g;  // one value per streamed column
    if (!has_z) return;
    RowsSide(sm, sz, az);
    rows.rhs = zp.rhs_arg;
    rows.g = sz.g;
    rows.e = zp.e;
    if (rows.zone.head == k::kHeadSmooth) {
      head = Carried(3 * m);
      rows.hs = head.Slice(0, m);
      rows.hys = head.Slice(m, m);
      rows.hv = head.Slice(2 * m, m);
    }
  }

  // Tall: the z side into the pass (k::kChainZeroTall) over the transposed copy, the x side into the rows.
  void FillTall(const Side& sn, double ax, const Side& sm, double az) {
    pass.m = n;
    pass.n = m;
    pass.lda = n;
    pass.A = CT;
    PassSide(k::kChainZeroTall, sm, sz, az);
    k::LassoInstance& i = pass.inst;
    i.zg = sz.g;
    i.zrhs = zp.rhs_arg;
    i.ke = -zp.e;
    i.dinv = zp.dinv_arg;
    RowsSide(sn, sx, ax);
    rows.side = k::kRowsX;
    if (rows.zone.head == k::kHeadLinear) rows.g = sx.g;
    if (zp.x_free) {  // no state and no term on this side: x alone (RowsSide's are empty defaults)
      rows.side = k::kRowsXFree;
      rows.xcur = xcur;
    }
    if (!samples_smooth) return;
    // the pass in two halves (the dot pass here, the accumulate pass in `acc`) around the sample kernel,
    // which takes the z side's state, zone with its head, offset, rhs and pivots from the pass's
    // record; the halves themselves run no head
    pass.chain = k::kChainZeroTallDot;
    head = Carried(3 * m);
    dfarg = DVec::Zeros(2 * m, dt);
    i.zd = dfarg.Slice(0, m);
    i.zfarg = dfarg.Slice(m, m);
    k::ZeroTallSamplesArgs& t = samples;
    t.m = m;
    t.d = i.zd;
    t.farg = i.zfarg;
    t.rhs = i.zrhs;
    t.g = i.zg;
    t.state = i.state;
    t.zone = i.zone;
    i.zone.head = k::kHeadZone;
    t.hs = head.Slice(0, m);
    t.hys = head.Slice(m, m);
    t.hv = head.Slice(2 * m, m);
    t.kappa = i.kappa;
    t.ke = i.ke;
    t.dinv = i.dinv;
  }

  // The dense pivot's vector of the first sweep from the current state, with the generic
  // operators: the sweep up to the ZERO prox's input v (on copies: the state is not touched), then
  // the forward substitution and the inverse apply.  Fat: r = (rhs - e v_z) - L(arg, x') v_x.
  // Tall: f_arg = rhs - e v_z, f_x = v_x - L(x', arg) f_arg; free x: f_x = -L(x, arg) f_arg, no v_x.
  void ForwardFromState(const MultiBlockParts& a) {
    const size_t N = a.prox.size();
    BlockVector v = a.u;
    for (size_t i = 0; i < N; ++i) v -= a.y[i];
    for (size_t i = 0; i + 1 < N; ++i) {
      v += a.y[i];
      v -= a.A * a.prox[i]->Apply(v);
    }
    v += a.y[N - 1];
    if (tall) {
      DVec farg = zp.rhs_arg.n != 0 ? zp.rhs_arg.Clone() : DVec::Zeros(m, dt);
      k::Axpby(farg, -zp.e, v(zp.z_constraint_key), 1.0);
      if (!zp.x_free) k::Copy(p, v(zp.x_constraint_key));
      zp.L->Apply(-1.0, farg, zp.x_free ? 0.0 : 1.0, p);
    } else {
      if (zp.rhs_arg.n != 0) k::Copy(p, zp.rhs_arg);
      else k::Fill(p, 0.0);
      if (has_z) k::Axpby(p, -zp.e, v(zp.z_constraint_key), 1.0);
      zp.L->Apply(-1.0, v(zp.x_constraint_key), 1.0, p);
    }
    inv.Apply();
  }

  void Sweep() override {
    k::LassoFusedPass(pass);
    if (samples_smooth) {
      k::ZeroTallSamples(samples);
      k::LassoFusedPass(acc);
    }
    if (has_z)
      k::ZeroFusedRows(rows);
    else
      k::ReducePartials(m, grid, tpart, pass.inst.pkappa, 0.0, p, zp.rhs_arg.n != 0 ? &zp.rhs_arg : nullptr);
    inv.Apply();
  }

  // ---- residual check (option "fused_zero_check"): one launch, splittable for pipelining ---------
  // With b empty, the ZERO term last and each row c tying its copy (coefficient 1) to one term's
  // variable (coefficient a_c), the quantities of prox_admm.cc:178-217 are, summed over the sides
  // that are present,
  //   ||A x_term,c|| = ||y_term,c||,  ||A x_ZERO||^2 = sum_c ||y_zero,c||^2,  r^2 = sum_c ||y_term,c + y_zero,c||^2,
  //   s^2 = sum_c a_c^2 ||y_zero,c - y_zero_prev,c||^2  (A_i^T of term i reads its own row alone, and
  //   on that row Ax_diff holds the ZERO term's difference and no other),
  //   ||A^T u||^2 = sum_c (1 + a_c^2) ||u_c||^2.
  bool HasCheck() const override { return own_check; }
  bool PipelineChecks() const override {
    static const bool off = opt::Is0(opt::kPipelineChecks);
    return own_check && !off;
  }
  // the check's ten scalars into the next ten slots
  void LaunchNorms() override {
    EPS_CHECK(own_check);
    Runtime& rt = Runtime::Get();
    norm_slot = rt.NewSlot();
    for (int q = 1; q < 10; ++q) rt.NewSlot();
    k::ZeroFusedNorms(check_x, check_z, rt.SlotPtr(norm_slot), norm_work,
                      tall ? "zero_tall_norms" : "zero_fused_norms");
  }
  Check FinishCheck() override {
    Runtime& rt = Runtime::Get();
    double x[5], z[5];
    for (int q = 0; q < 5; ++q) {
      x[q] = rt.SlotValue(norm_slot + q);
      z[q] = rt.SlotValue(norm_slot + 5 + q);
    }
    Check c;
    c.r = std::sqrt(x[2] + z[2]);
    c.s = std::sqrt(ax * ax * x[3] + az * az * z[3]);
    c.max_norm = std::fmax(std::fmax(std::sqrt(x[0]), std::sqrt(z[0])), std::sqrt(x[1] + z[1]));
    c.atu = std::sqrt((1.0 + ax * ax) * x[4] + (1.0 + az * az) * z[4]);
    return c;
  }
  // What a sweep hands to the next is `carried` and nothing else: the pass reads w and its side's
  // state, the row kernel (the sample kernel) the other side's and the head, the free-x kernel keeps
  // xcur; p, the partials, d and f_arg and the apply's workspace are written in every sweep before
  // they are read.
  void SaveSnapshot() override { k::Copy(snapshot, carried); }
  void RestoreSnapshot() override {
    Runtime::Get().Sync();  // let the discarded sweeps drain
    k::Copy(carried, snapshot);
  }

  // ---- batched solves (RunFusedBatches) ---------------------------------------------------------
  const k::ZeroRowsArgs* Rows() const override { return has_z ? &rows : nullptr; }
  const k::ZeroTallSamplesArgs* Samples() const override { return samples_smooth ? &samples : nullptr; }
  // The key of the group a fresh solve on this route can join: the same data matrix, the same
  // inverse (and packed copy), the same e and z block, the same form of the row kernel and the
  // same schedule.  Everything else - the zones' parameters and vectors, the offset g, the rhs -
  // is per member, so a hinge and a deadzone member on one matrix share a group.  false: the single
  // pass takes a form the batched one does not mirror (512-thread workgroups), or tall without
  // `tall_groups`.
  // Tall: the key also has the transposed copy (the members find one through the solve's cache),
  // the form (the pass whole, or in halves around the sample kernel: a logistic member never joins
  // a scaled-zone group), the scalar pivot, and whether x is free (such a member has another x-side
  // launch: it never joins a hinge or deadzone group).
  bool BatchKey(const pb::SolverParams& params, bool tall_groups, std::vector<uint64_t>* key) const override {
    // a head without a batched form (ridge, linear, the cone): such a member is solved by itself
    if (!k::BatchPassExists(pass.chain, pass.inst.zone.head)) return false;
    if (Rows() != nullptr && !k::BatchRowsExist(rows.side, rows.zone.head)) return false;
    if (tall && (!tall_groups || !has_z)) return false;
    if (k::LassoBatchWidth(pass.m, pass.n, dt, pass.chain) == 0) return false;
    if (samples_smooth && k::LassoBatchWidth(pass.m, pass.n, dt, acc.chain) == 0) return false;
    *key = KeyHead(*zp.L, *zp.Dinv, params);
    key->insert(key->end(), {Bits(zp.e), has_z ? 1u : 0u, rows.zone.head == k::kHeadSmooth ? 1u : 0u});
    if (tall)
      key->insert(key->end(), {reinterpret_cast<uintptr_t>(CT.data()), 1u, samples_smooth ? 1u : 0u,
                               Bits(zp.dinv_arg), zp.x_free ? 1u : 0u});
    return true;
  }
};

// ---------------------------------------------------------------------------------------------------
// The lasso structure in two-block form
// ---------------------------------------------------------------------------------------------------
// [SUM_SQUARE with a dense argument map, scaled-zone prox], one constraint a0 x0 + a1 x1 = 0
// without a constant: the x-updates are the same two operators as in the multi-block driver, the
// z-update is the closed-form projection onto the constraint, so one pass over the data matrix
// does a whole sweep (kernels_fused.hip, k::kChainTwoBlock).  f32 and f64, single GPU.  The residual check
// is the driver's generic one on views of the state.
struct TwoBlockRoute final : FusedRoute {
  LeastSquaresDesc ls;
  SeparableDesc sz;
  int64_t m = 0, n = 0;
  int grid = 0;
  DVec p, w, tpart;
  k::LassoFusedArgs pass;

  bool Enable(const TwoBlockParts& a) {
    if (opt::Is0(opt::kFused) || a.prox.size() != 2 || a.num_constraints != 1) return false;
    if (ShardSpec::Get().active() || !a.constr_H.b.data().empty()) return false;
    if (!a.prox[0]->DescribeLeastSquares(&ls) || !a.prox[1]->DescribeSeparable(&sz)) return false;
    if (sz.kind != SeparableDesc::kZone || sz.g.n != 0) return false;  // accepted: a zone without offset
    if (ls.cols != 1) return false;  // matrix variables: the multi-block driver only
    const DenseMatrixImpl& L = *ls.L_arg_var;
    if (L.trans()) return false;
    m = L.rows();
    n = L.cols();
    const BlockMatrix& H = a.constr_H.A;
    double a0 = 0, a1 = 0;
    if (H.data().size() != 2 || !ConsensusTie(H, affine::constraint_key(0), ls.var_key, sz.var_key, n, &a0, &a1))
      return false;
    if (a0 == 0 || a1 == 0) return false;
    if (!k::LassoFusedSupported(m, n, L.data(), L.rows())) return false;
    if (ls.rhs_arg.n != 0 && ls.rhs_arg.n != m) return false;
    const DenseMatrixImpl& D = *ls.Dinv_arg;
    if (D.trans() || D.rows() != m) return false;
    const DType dt = a.data->dtype();
    if ((sz.alpha_vec.n > 0 && sz.alpha_vec.dt != dt) || (sz.beta_vec.n > 0 && sz.beta_vec.dt != dt)) return false;
    if (L.dtype() != dt || D.dtype() != dt) return false;
    // x, z, u and the previous z of the two variables
    std::vector<StateSlice> views;
    for (BlockVector* home : {&a.x, &a.z, &a.u, &a.z_prev})
      for (const std::string& key : {ls.var_key, sz.var_key})
        views.push_back({home, key, DVec::Zeros(n, dt), home != &a.z_prev});
    const DVec &x0 = views[0].v, &x1 = views[1].v, &z0 = views[2].v, &z1 = views[3].v, &u0 = views[4].v,
               &u1 = views[5].v, &z0p = views[6].v, &z1p = views[7].v;
    p = DVec::Zeros(m, dt);
    w = DVec::Zeros(m, dt);
    grid = k::LassoFusedGrid(m, n, dt);
    tpart = DVec::Empty(static_cast<int64_t>(grid) * m, dt);
    // the pass's arguments, once per Init; what the chain reads in each state array: k::Chain
    pass.m = m;
    pass.n = n;
    pass.lda = L.rows();
    pass.A = L.data();
    pass.chain = k::kChainTwoBlock;
    pass.a0 = a0;
    // beside the matrix: the partials, eight state vectors, p, w, and the inverse
    ResidentShare(m, n, dt, static_cast<int64_t>(grid) * m + 8 * n + 2 * m + m * m, /*auto_on=*/false, &pass);
    pass.e1 = z1p;
    k::LassoInstance& s = pass.inst;
    s.w = w;
    s.tpart = tpart;
    s.state.u = u0;
    s.state.copy = x0;
    s.state.var = x1;
    s.state.y_zero = z0;
    s.state.y_term = z1;
    s.state.y_term_prev = z0p;
    s.state.y_zero_prev = u1;
    s.p = p;
    s.rhs = ls.rhs_arg;
    s.kappa = s.pkappa = -L.scale();
    s.zone = ZoneOf(sz, a1);
    AdoptState(views, {&a.x, &a.z, &a.u, &a.z_prev});
    // p = rhs_arg - L(arg, var) (z0 - u0) of the current state, w = Dinv_arg p
    DVec v0 = z0.Clone();
    k::Axpby(v0, -1.0, u0, 1.0);
    L.Apply(-1.0, v0, 0.0, p);
    if (ls.rhs_arg.n != 0) k::Axpby(p, 1.0, ls.rhs_arg, 1.0);
    D.Apply(1.0, p, 0.0, w);
    return true;
  }

  void Sweep() override {
    k::LassoFusedPass(pass);
    k::ReducePartials(m, grid, tpart, pass.inst.pkappa, 0.0, p, ls.rhs_arg.n != 0 ? &ls.rhs_arg : nullptr);
    ls.Dinv_arg->Apply(1.0, p, 0.0, w);
  }
};

template <class Route, class Parts, class... Options>
std::unique_ptr<FusedRoute> Recognise(const Parts& parts, Options... options) {
  std::unique_ptr<Route> r(new Route);
  if (!r->Enable(parts, options...)) return nullptr;
  return std::unique_ptr<FusedRoute>(std::move(r));
}

}  // namespace

std::unique_ptr<FusedRoute> RecogniseMultiBlockRoute(const MultiBlockParts& parts) {
  const bool zero = opt::Word(opt::kFusedZero) != 0;  // (read first: a bad value is an error whatever the problem)
  const int tall = opt::Word(opt::kFusedZeroTall);
  const int tall_smooth = opt::Word(opt::kFusedZeroTallSmooth);
  const int lasso_tall = opt::Word(opt::kFusedTall);
  const int ridge = opt::Word(opt::kFusedZeroRidge);
  const bool xfree = opt::Word(opt::kFusedZeroXfree) != 0;
  const bool lp = opt::Word(opt::kFusedZeroLp) != 0;
  const bool check = opt::Word(opt::kFusedZeroCheck) != 0;
  if (auto r = Recognise<LassoRoute>(parts, lasso_tall)) return r;  // fat, then tall
  if (!zero) return nullptr;
  return Recognise<ZeroRoute>(parts, tall, tall_smooth, ridge, xfree, lp, check);  // fat, then tall, then tall with free x
}

std::unique_ptr<FusedRoute> RecogniseTwoBlockRoute(const TwoBlockParts& parts) {
  return Recognise<TwoBlockRoute>(parts);
}

// ---------------------------------------------------------------------------------------------------
// Batched solves: groups of instances on the lasso route or on the ZERO-term route that share the
// data matrix and the cached inverse
// ---------------------------------------------------------------------------------------------------
namespace {

// A member of a group: its solver and its route.  Every member of a group has the lead's kind:
// the keys begin with the pass's chain.
struct BatchMember {
  Solver* solver;
  BatchRoute* route;
};
using Group = std::vector<BatchMember>;

// Run()'s iteration schedule without the pipelining, for a group of batched members: sweeps up to
// the next multiple of the epoch, then one residual check of every active member with ONE fetch of
// their scalars (a route without a check of its own: the driver's generic check, waited for, member
// by member).  A member that stops is frozen: it leaves `active`, and `stopped(gone)` is told
// which ones left (only when some did).  Members still active at the end get Run()'s
// max-iterations status.  Ends with the group's loop time since `t0`, once the stream has drained.
template <class Sweep, class Stopped>
void RunGroupSchedule(const Group& g, double t0, std::vector<int>* active, Sweep sweep, Stopped stopped) {
  Runtime& rt = Runtime::Get();
  const pb::SolverParams& params = g[0].solver->params();
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
      for (int i : *active) g[i].solver->BatchLaunchCheck(iter);
      rt.FetchSlots();
      std::vector<int> still, gone;
      for (int i : *active) (g[i].solver->BatchFinishCheck() ? gone : still).push_back(i);
      active->swap(still);
      if (!gone.empty()) stopped(gone);
    }
    ++iter;
  }
  for (int i : *active) g[i].solver->BatchFinishMaxIterations(iter);
  rt.Sync();
  const double loop = Now() - t0;
  for (const BatchMember& b : g) b.solver->BatchAddLoopTime(loop);
}

// A group on the batched pass: per sweep one batched pass per `width` active members, ONE launch
// for all of them that sums the partials - the row kernel for ZERO-term members (DESIGN.md 3.11;
// basis pursuit, which has no z block, and the lasso: one batched reduction of the partials with
// the rhs folded in) - and one batched apply of the packed inverse (below m = 1024: each member's
// own apply; whitened: none).  Each launch does per member what the member's own sweep does, so
// its iterates are the single solve's bit for bit; a ZERO-term member's residual check is the
// driver's generic one - under "fused_zero_check" its own one launch, with one fetch for the group -
// at the sweeps of the member's own Run().
// Tall ZERO-term members: every launch in the pass's own dimensions (pass.m = n, the order of the
// dense pivot), and for a smooth z term the pass in halves around one sample launch (BatchSweep).
void RunPassGroup(const Group& g) {
  const double t0 = Now();
  const BatchRoute& lead = *g[0].route;
  SetCurrentDType(lead.dt);
  const int K = static_cast<int>(g.size());
  std::vector<const k::LassoInstance*> all;
  for (const BatchMember& b : g) all.push_back(&b.route->pass.inst);
  const bool rhs_aligned = RhsAligned(all);
  // (the pass's own dimensions: a tall lead's pass.m is n, the order of its dense pivot)
  DVec symv_work = lead.inv.packed.n > 0 ? DVec::Empty(K * k::SymvWorkspace(lead.pass.m), lead.dt) : DVec();
  const k::FusedResidency res = lead.Residency(K);  // (a ZERO-term lead's own: none under "auto")

  std::vector<int> active(K);
  for (int i = 0; i < K; ++i) active[i] = i;
  DVec table, row_table, sample_table;
  auto upload = [&] {
    std::vector<const k::LassoInstance*> v;
    std::vector<const k::ZeroRowsArgs*> r;
    std::vector<const k::ZeroTallSamplesArgs*> t;
    for (int i : active) {
      const BatchRoute& mb = *g[i].route;
      EPS_CHECK(mb.pass.m == lead.pass.m && mb.pass.n == lead.pass.n && mb.pass.chain == lead.pass.chain);
      // present where the chain stores or loads through them (the upload checks what is there)
      EPS_CHECK(mb.pass.chain == k::kChainLasso || mb.pass.inst.state.y_zero_prev.n == lead.pass.n);
      if (mb.pass.chain == k::kChainZeroTallDot) EPS_CHECK(mb.pass.inst.zd.n == lead.pass.n && mb.pass.inst.zfarg.n == lead.pass.n);
      v.push_back(&mb.pass.inst);
      if (mb.Rows() != nullptr) r.push_back(mb.Rows());
      if (mb.Samples() != nullptr) t.push_back(mb.Samples());
    }
    k::LassoBatchUpload(v, lead.dt, &table);
    if (lead.Rows() != nullptr) k::ZeroRowsBatchUpload(r, &row_table);
    if (lead.Samples() != nullptr) k::ZeroTallSamplesBatchUpload(t, &sample_table);
  };
  upload();
  auto sweep = [&] {
    lead.BatchSweep(table, row_table, sample_table, static_cast<int>(active.size()), nullptr, res, rhs_aligned,
                    symv_work, [&] {
      for (int i : active) g[i].route->inv.Apply();
    });
  };
  // the stopped ones are frozen: drop their descriptors
  RunGroupSchedule(g, t0, &active, sweep, [&](const std::vector<int>&) {
    if (!active.empty()) upload();
  });
}

// A group on the tall lasso route: per sweep ONE tile launch of the packed inverse
// for all active members (the tile is read once) and ONE cols launch whose grid row b is member b's
// own launch on its own record, so its iterates are the single solve's bit for bit.
void RunTallGroup(const Group& g) {
  const double t0 = Now();
  const BatchRoute& lead = *g[0].route;
  SetCurrentDType(lead.dt);
  const int K = static_cast<int>(g.size());
  const int64_t n = lead.n;
  DVec work = DVec::Empty(K * k::SymvWorkspace(n), lead.dt);
  std::vector<int> active(K);
  for (int i = 0; i < K; ++i) active[i] = i;
  DVec table;
  auto upload = [&] {
    std::vector<const k::LassoInstance*> v;
    for (int i : active) {
      EPS_CHECK(g[i].route->tall_cols && g[i].route->n == n && g[i].route->inv.packed.data() == lead.inv.packed.data());
      v.push_back(&g[i].route->pass.inst);
    }
    k::LassoBatchUpload(v, lead.dt, &table);
  };
  upload();
  auto sweep = [&] {
    const int count = static_cast<int>(active.size());
    k::SymvPackedTilesBatch(n, lead.inv.packed, table, count, work);
    k::LassoTallColsBatch(n, lead.dt, table, count, work);
  };
  // the stopped ones are frozen: drop their descriptors
  RunGroupSchedule(g, t0, &active, sweep, [&](const std::vector<int>&) {
    if (!active.empty()) upload();
  });
}

// Smallest group the wide route takes.  Measured crossovers against the batched pass on MI355X
// (DESIGN.md 3.8), rounded up to a multiple of 8.
constexpr int kWideMin = 8;
int BatchWideMin() {  // EPSILON_HIP_BATCH_WIDE_MIN: tuning knob (the crossover measurements)
  const int v = opt::Int(opt::kBatchWideMin, 0);
  return v >= 2 ? v : kWideMin;
}

// The wide route (kernels_fused_wide.hip), lasso members alone: RunPassGroup's schedule and residual checks, with the
// sweep of a panel of up to 64 members as back product + chain, forward product and reduction on
// the f32 matrix instruction.  The members' w (and p) live in instance-major panels for the
// duration; a member keeps its slot until the group ends and a stopped one is masked, so no
// summation order depends on who else is still iterating.  Not bit-identical to the single solve.
void RunWideGroup(const Group& g) {
  const double t0 = Now();
  const BatchRoute& lead = *g[0].route;
  SetCurrentDType(F32);
  const int64_t m = lead.m, n = lead.n;
  const bool whiten = lead.whiten;
  const int K = static_cast<int>(g.size());
  constexpr int PW = WideSweep::PW;
  const int npanels = (K + PW - 1) / PW;
  WideSweep ws;
  ws.Init(m, n, lead.pass.A, lead.pass.lda, whiten, lead.inv.D.get());
  const int64_t panel_len = ws.panel_len;

  std::vector<k::LassoInstance> mem;
  DVec Wall = DVec::Zeros(npanels * panel_len, F32);
  DVec Pall = whiten ? DVec() : DVec::Zeros(npanels * panel_len, F32);
  for (int i = 0; i < K; ++i) {
    mem.push_back(g[i].route->pass.inst);
    const k::ConsensusState& s = mem[i].state;
    for (const DVec* v : {&s.u, &s.var, &s.copy, &s.y_term, &s.y_zero, &s.y_term_prev})
      EPS_CHECK_MSG(reinterpret_cast<uintptr_t>(v->data()) % 16 == 0, "wide batch: unaligned state vector");
    DVec slot = Wall.Slice(static_cast<int64_t>(i) * m, m);
    k::Copy(slot, mem[i].w);  // ForwardFromState's result at Init
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
    for (int q = 0; q < npanels; ++q) {
      if (live[q] == 0) continue;
      const int first = q * PW, nk = std::min(PW, K - first);
      ws.Run(table, first, nk, live[q], Wall.Slice(q * panel_len, panel_len),
             whiten ? DVec() : Pall.Slice(q * panel_len, panel_len));
    }
  };
  // frozen: their slots are masked from here on
  RunGroupSchedule(g, t0, &active, sweep, [&](const std::vector<int>& gone) {
    for (int i : gone) live[i / PW] &= ~(uint64_t(1) << (i % PW));
  });
  // every member's own w holds what its next sweep would read
  for (int i = 0; i < K; ++i) k::Copy(g[i].route->pass.inst.w, mem[i].w);
}

}  // namespace

std::vector<bool> RunFusedBatches(const std::vector<Solver*>& solvers) {
  std::vector<bool> ran(solvers.size(), false);
  const bool wide = opt::Word(opt::kBatchWide) != 0;
  const bool tall_groups = opt::Word(opt::kBatchZeroTall) != 0;  // (read first: a bad value is an error whatever the batch)
  std::map<std::vector<uint64_t>, std::vector<size_t>> groups;
  std::vector<BatchRoute*> routes(solvers.size(), nullptr);
  std::vector<std::vector<uint64_t>> order;  // groups in order of their first instance
  for (size_t i = 0; i < solvers.size(); ++i) {
    routes[i] = dynamic_cast<BatchRoute*>(solvers[i]->batch_route());
    std::vector<uint64_t> key;
    if (routes[i] == nullptr || !routes[i]->BatchKey(solvers[i]->params(), tall_groups, &key)) continue;
    auto& members = groups[key];
    if (members.empty()) order.push_back(key);
    members.push_back(i);
  }
  for (const auto& key : order) {
    const std::vector<size_t>& idx = groups[key];
    if (idx.size() < 2) continue;  // alone: the single path is the same solve, with pipelined checks
    Group g;
    for (size_t i : idx) g.push_back({solvers[i], routes[i]});
    const BatchRoute& lead = *g[0].route;
    // a tall lasso group has its own two launches; the wide kernels run the lasso chain alone
    if (lead.tall_cols)
      RunTallGroup(g);
    else if (wide && lead.pass.chain == k::kChainLasso && static_cast<int>(g.size()) >= BatchWideMin() && lead.dt == F32 &&
        k::LassoWideSupported(lead.m, lead.n, lead.pass.A, lead.pass.lda))
      RunWideGroup(g);
    else
      RunPassGroup(g);
    for (size_t i : idx) ran[i] = true;
  }
  return ran;
}

}  // namespace eps
