// Launchers for the hand-written gfx950 kernels.  All launch on Runtime::Get().stream().
// DVec arguments carry their dtype (f32 / f64); scalars are passed as double and narrowed in
// the kernel.  Reference call sites replaced are cited per group.
#pragma once

#include "device.h"

namespace eps {
struct PeerView;
namespace k {

// ---- K7: BlockVector += -= *=, scalar / diagonal Apply -------------------------------------
// (reference vector/block_vector.cc:9-48, linear/scalar_matrix_impl.h:24,
//  linear/diagonal_matrix_impl.h:23)
void Fill(const DVec& y, double v);
void Copy(const DVec& dst, const DVec& src);
// y[i] = deterministic pseudo-random value in (-1, 1) (hash of seed and index)
void FillHash(const DVec& y, uint64_t seed);
// y = a*x + b*y   (b == 0 never reads y)
void Axpby(const DVec& y, double a, const DVec& x, double b);
// y = a * d .* x + b*y
void DiagMul(const DVec& y, double a, const DVec& d, const DVec& x, double b);
// host f64 staging buffer (device memory, doubles) -> dst (dst.dt)
void ConvertFromF64(const DVec& dst, const double* src_dev);
// src (any dt) -> device doubles
void ConvertToF64(double* dst_dev, const DVec& src);
void ConvertFromF32(const DVec& dst, const float* src_dev);

// ---- K8: norms (reference vector/block_vector.cc:87-93) -----------------------------------
// *slot = (accumulate ? *slot : 0) + sum_i x_i^2, accumulated in double, deterministic.
void SumSq(const DVec& x, double* slot, bool accumulate);
// *slot (+)= sum_i (x_i - y_i)^2
void SumSqDiff(const DVec& x, const DVec& y, double* slot, bool accumulate);
void Dot(const DVec& x, const DVec& y, double* slot, bool accumulate);

// ---- K1/K2/K3: dense mat-vec (reference linear/dense_matrix_impl.cc:55-67 dgemv_) --------
// y = alpha * op(A) x + beta*y ; A is rows x cols column-major with leading dimension lda.
void Gemv(bool trans, int64_t rows, int64_t cols, double alpha, const DVec& A, int64_t lda,
          const DVec& x, double beta, const DVec& y);

// y = alpha * S x + beta * y for a symmetric S in full storage (n x n, leading dimension lds):
// reads only the lower-triangle tiles, half the bytes of Gemv.
// `work` (optional, SymvWorkspace(n) elements of S's dtype): per-tile partials at a fixed
// address instead of a pool allocation per call (launches captured in a hipGraph need that).
void Symv(int64_t n, double alpha, const DVec& S, int64_t lds, const DVec& x, double beta,
          const DVec& y, const DVec* work = nullptr);
int64_t SymvWorkspace(int64_t n);
// The same apply from a tile-packed copy of the lower tiles (every 128 x 128 tile contiguous,
// zero-padded at the edge): SymvPack builds it once (SymvPackedSize(n) values), SymvPacked applies it.
int64_t SymvPackedSize(int64_t n);
DVec SymvPack(int64_t n, const DVec& S, int64_t lds);
void SymvPacked(int64_t n, double alpha, const DVec& P, const DVec& x, double beta, const DVec& y,
                const DVec* work = nullptr);

// The tile launch of SymvPacked alone: the per-tile partials of P x into `work`
// (SymvWorkspace(n) values), for a caller whose own kernel sums them in SymvPacked's order
// (kernels_symv_reduce.h).  Profile tag "symv_packed_tiles".
void SymvPackedTiles(int64_t n, const DVec& P, const DVec& x, const DVec& work);

// y[r] = alpha * sum_{k < nparts} partial[k*rows + r] + beta*y[r], fixed summation order.
// `add` (optional) is added to the result afterwards: y = (alpha*sum + beta*y) + add.
void ReducePartials(int64_t rows, int nparts, const DVec& partial, double alpha, double beta,
                    const DVec& y, const DVec* add = nullptr);

// ---- fused lasso sweep: one pass over A per ADMM sweep (kernels_fused.hip) ------------------
// The state of one consensus constraint copy + a1 var = 0 (vectors of one length, updated in place):
// `var` is the separable term's variable, `copy` the other term's (least squares; ZERO) own.
struct ConsensusState {
  DVec u, var, copy;
  DVec y_term, y_zero;             // y of the separable term, y of the copy's term
  DVec y_term_prev, y_zero_prev;   // their previous values (the lasso chain keeps no y_zero_prev)
};
// The chain of a fused pass (LassoFusedArgs::chain, LassoBatchPass): what a streamed column j does
// between its dot product d_j = A[:,j] . w and its forward update t' += A[:,j] v_j.  The values are
// fixed: the batch keys begin with them.  Per chain: what the arrays of LassoInstance::state mean, what
// else of the instance is read, the profile tag (single; batched) and the thread shapes.  f32 and f64.
enum Chain {
  // The lasso sweep of the multi-block driver (ChainOneT): copy -> x0, var -> x1, y_zero -> y0, y_term
  // -> y1, y_term_prev -> y1prev; no y_zero_prev.  "lasso_fused"; "batch_fused_pass".  256 and 512
  // threads; batched: 256 alone, optionally with the group threshold (group_lam).
  kChainLasso = 0,
  // The two-block driver's sweep (prox_admm_two_block.cc:97-112; ChainTwoBlockT): copy -> x0, var -> x1,
  // u -> u0, y_zero -> z0, y_term -> z1, y_term_prev -> z0_prev, y_zero_prev -> u1, LassoFusedArgs::e1
  // -> z1_prev; a0, a1: the constraint a0 x0 + a1 x1 = 0 the z-update projects onto.  "lasso_fused"; no
  // batched form.  256 and 512 threads.
  kChainTwoBlock = 1,
  // The column side of a ZERO-term problem (ZeroChainT) on the x constraint: the term
  // on x first, the projection's copy x' = v_x + kappa A^T w last.  copy -> x', var -> x, y_zero -> the
  // ZERO term's y, y_term -> the x term's y, y_term_prev / y_zero_prev -> their previous values; a
  // linear head reads its vector g in zg.  "zero_fused"; "batch_zero_pass".  256 and 512 threads.
  kChainZeroCols = 2,
  // The sample side of a TALL ZERO-term problem (DESIGN.md 3.11 "Tall C"; ZeroTallChainT): A is C^T
  // (features x samples), w the copy x' of this sweep, the state is the z constraint's with
  // kChainZeroCols' meaning (copy -> z', var -> z); zg, zrhs: the z term's offset and the constant of
  // the arg row per sample (optional), ke = -L(arg, z'), dinv = Dinv(arg)'s scalar.  The partials are
  // C^T f_arg's of the next sweep.  "zero_tall"; "batch_zero_tall_pass".  256 and 512 threads.
  kChainZeroTall = 3,
  // kChainZeroTall in two launches around ZeroTallSamples, for a z term whose prox does not fit the
  // column step (a smooth term); they stream C^T as it does and run no head.  Dot: zd[j] = A[:,j] . w
  // per sample, nothing else is read or written.  "zero_tall_dot"; "batch_zero_tall_dot".  Acc: the
  // partials of sum_j A[:,j] zfarg[j]; w and the state are not read; no reduction, no barrier.
  // "zero_tall_acc"; "batch_zero_tall_acc".  256 threads alone.
  kChainZeroTallDot = 4,
  kChainZeroTallAcc = 5,
};
constexpr bool ChainIsTallHalf(Chain c) { return c == kChainZeroTallDot || c == kChainZeroTallAcc; }
// The chain keeps the previous y of the copy's term (ConsensusState::y_zero_prev).
constexpr bool ChainKeepsZeroPrev(Chain c) {
  return c == kChainTwoBlock || c == kChainZeroCols || c == kChainZeroTall;
}
// The profile tag of a launch, by chain: {single, batched}.
constexpr const char* kChainTags[6][2] = {
    {"lasso_fused", "batch_fused_pass"},      {"lasso_fused", "batch_fused_pass"},
    {"zero_fused", "batch_zero_pass"},        {"zero_tall", "batch_zero_tall_pass"},
    {"zero_tall_dot", "batch_zero_tall_dot"}, {"zero_tall_acc", "batch_zero_tall_acc"}};

// What stands in the threshold's place on a side, var = Cs f(Bs v); a1 scales `var`
// in the constraint.  One head per side.
enum Head {
  kHeadZone,    // the scaled zone, Cs (zone(Bs v + g) - g): every chain and side
  kHeadRidge,   // the x side of a ZERO-term sweep: a scalar least-squares prox, var = Cs (Bs v) with Bs
                // and Cs the two factors of its block solve (-L(var, constraint) and Dinv(var))
  kHeadLinear,  // the x side: a linear term, var = Cs (Bs v + g_j), Bs and Cs as for the ridge term, g
                // the vector the side carries (LassoInstance::zg in the pass, ZeroRowsArgs::g in the rows)
  kHeadNonNeg,  // the z side: the non-negative cone, var = Cs (max(Bs v + g, 0) - g), g optional
  kHeadSmooth,  // the z side: a smooth separable function (ZeroRowsArgs::fn), prox_{lam fn}(Bs v + g) by
                // the fp64 Newton of SmoothProx; Bs, Cs, a1, lam alone are read
};
struct ZoneParams {
  DVec alpha_vec, beta_vec;        // optional per-entry alpha / beta
  double Bs = 0, Cs = 0, a1 = 0, lam = 0, alpha = 1, beta = 1, M = 0;  // kHeadZone alone: lam ... M
  Head head = kHeadZone;
};
// Which side of a ZERO-term sweep the row kernel runs (ZeroRowsArgs::side).
enum RowsSide {
  kRowsZ,      // fat C: the z constraint's rows
  kRowsX,      // tall C: the entries of x
  kRowsXFree,  // tall C with x in the ZERO term alone: no state, no term, no head
};
// The forms that are instantiated; a launcher, an upload and a route's gate all read these.  `block`:
// LassoFusedBlock.  The halves of the tall pass run no head: their record says kHeadZone.
constexpr bool FusedPassExists(Chain c, Head h, int block) {
  if (h == kHeadZone) return !ChainIsTallHalf(c) || block == 256;
  if (c == kChainZeroCols) return h == kHeadRidge || (h == kHeadLinear && block == 256);
  return c == kChainZeroTall && h == kHeadNonNeg && block == 256;
}
constexpr bool ZeroRowsExist(RowsSide s, Head h) {
  if (h == kHeadZone) return true;
  if (s == kRowsZ) return h == kHeadNonNeg || h == kHeadSmooth;
  return s == kRowsX && (h == kHeadRidge || h == kHeadLinear);
}
constexpr bool BatchPassExists(Chain c, Head h) { return c != kChainTwoBlock && h == kHeadZone; }
constexpr bool BatchRowsExist(RowsSide s, Head h) { return h == kHeadZone || (s == kRowsZ && h == kHeadSmooth); }
// For the message of a check that one of these fails.
constexpr const char* kHeadNames[] = {"zone", "ridge", "linear", "non-negative", "smooth"};
constexpr const char* kRowsSideNames[] = {"z", "x", "free x"};
// One instance of the sweep as the kernels read it (host view: scalars as double, narrowed to
// the compute type in one place, kernels_fused_chain.h): the multi-block driver's fused state
// plus its forward vectors.  Built once per Init by the drivers; a batch uploads its members'.
struct LassoInstance {
  DVec w;        // m: the block-diagonal-scaled forward-substitution result of this sweep
  DVec tpart;    // LassoFusedGrid(m, n) * m: per-workgroup partials of A v0'
  ConsensusState state;             // n each; what they mean per chain: Chain
  ZoneParams zone;                  // (vectors: n entries)
  DVec p, rhs;   // m: the reduced partials (+ rhs), input of the inverse apply; its constant part
  double kappa = 0;                 // copy = v0 + kappa * (A^T w)
  double pkappa = 0;                // scale of the summed partials in p (see LassoBatchInst)
  // the tall ZERO chains alone (n entries each, n the streamed dimension: the samples)
  DVec zg, zrhs;                    // kChainZeroTall, optional; kChainZeroCols with kHeadLinear: zg = g
  DVec zd, zfarg;                   // kChainZeroTallDot writes zd, kChainZeroTallAcc reads zfarg
  double ke = 0, dinv = 0;          // kChainZeroTall
};
struct LassoFusedArgs {
  int64_t m = 0, n = 0, lda = 0;
  DVec A;        // m x n column-major
  LassoInstance inst;
  unsigned* epoch = nullptr;        // optional device counter, incremented once per launch
  Chain chain = kChainLasso;
  double a0 = 1;
  DVec e1;       // kChainTwoBlock alone
  // the matrix's share that is loaded to stay in the Infinity Cache (LassoFusedResidency); 0, 0:
  // every load non-temporal
  int qfull = 0;
  int64_t jcut = 0;
};

// The smooth separable functions of the Newton family (SmoothProx below; kernels_smooth_fn.h).
enum SmoothFn { SMOOTH_EXP, SMOOTH_LOGISTIC, SMOOTH_NEG_ENTR, SMOOTH_INV_POS, SMOOTH_NEG_LOG };

// The row side of the ZERO-term sweep (kernels_fused.hip), one launch, profile tag
// "zero_fused_rows".  Per row: finishes sweep k with w (z' = v_z - e w, y and u on the z
// constraint), runs the z term of sweep k + 1 (zone(Bs v + g) - g, scaled by Cs), forms the next
// v_z, sums the pass's partials in a fixed order and writes r = (rhs - e v_z) + pkappa sum(tpart).
// The head is zone.head (ZeroRowsExist says which a side takes).  kHeadSmooth: `fn` (SMOOTH_LOGISTIC
// alone); the z term of sweep k + 1 (s, y_s, v_z) is then carried to the next launch in hs, hys, hv
// instead of being recomputed there: ZeroSmoothHead fills them from the state before the first launch.
struct ZeroRowsArgs {
  int64_t m = 0;
  int nparts = 0;
  DVec w, tpart, r, rhs, g;            // rhs, g: optional (empty: zero)
  ConsensusState state;                // m each: the z constraint's (var -> z, copy -> z')
  ZoneParams zone;
  double e = 0, pkappa = 0;
  SmoothFn fn = SMOOTH_LOGISTIC;
  DVec hs, hys, hv;                    // kHeadSmooth: m each, private to the caller
  // kRowsX, the x side of a tall problem (profile tag "zero_tall_cols"): the m entries are those of x,
  // w is the copy x' as the inverse apply left it (q = w, no product on top), the term is the one on
  // x and r = v_x' + pkappa sum(tpart) is the next f_x; rhs and e are not read.  A linear head reads
  // its vector in `g`, m entries.
  // kRowsXFree (profile tag "zero_tall_free_cols"; DESIGN.md 3.11 "x in the ZERO term alone"): x has
  // no constraint row, so there is no state, no term and no chain.  Per entry j the launch sums the
  // partials in the same order, keeps xcur[j] = w[j] - x of the sweep the pass just used, the iterate
  // at this boundary - and writes r[j] = pkappa sum(tpart), the next f_x.  `state`, the zone, rhs, g
  // and e are not read; xcur: m entries.
  RowsSide side = kRowsZ;
  DVec xcur;
};
// The sample side of a tall ZERO-term sweep whose z term is smooth (SMOOTH_LOGISTIC alone), between
// the two halves of the pass (kChainZeroTallDot, kChainZeroTallAcc), one launch, a thread per sample,
// profile tag "zero_tall_samples".  Per sample: finishes sweep k from d = C[i,:] . x' (kChainZeroTall's
// arithmetic: f_arg, the scalar pivot, arg, z' = v + ke arg, y and u on the z constraint) with the z
// term of this sweep taken from the carried head hs, hys, hv; runs the z term of sweep k + 1 -
// prox_{lam fn}(Bs v + g) by the fp64 Newton of SmoothProx, once - leaves it in hs, hys, hv and
// writes farg = rhs + ke v_z of sweep k + 1.  ZeroTallSamplesHead (profile tag "zero_tall_head")
// fills hs, hys, hv from the state before the first launch.
struct ZeroTallSamplesArgs {
  int64_t m = 0;
  DVec d, farg;                           // m each: in, out
  DVec rhs, g;                            // optional (empty: zero)
  ConsensusState state;                   // m each: the z constraint's, as the pass's record has it
  ZoneParams zone;                        // Bs, Cs, a1, lam alone are read
  DVec hs, hys, hv;                       // m each, private to the caller
  double kappa = 0, ke = 0, dinv = 0;     // scale of d; -L(arg, z'); Dinv(arg)'s scalar
  SmoothFn fn = SMOOTH_LOGISTIC;
};
void ZeroTallSamples(const ZeroTallSamplesArgs& args);
void ZeroTallSamplesHead(const ZeroTallSamplesArgs& args);
void ZeroFusedRows(const ZeroRowsArgs& args);
void ZeroSmoothHead(const ZeroRowsArgs& args);  // profile tag "zero_fused_head"
// The row side of `count` members of a batch in ONE launch, profile tag "batch_zero_rows": member b
// (grid row b) runs ZeroFusedRows' own workgroups on its own record, so its result is that of its
// own launch bit for bit.  The members share m, nparts, the dtype, the side and the head
// (BatchRowsExist).  ZeroRowsBatchUpload writes their records in order into `table` (device; grown as
// needed): as with LassoBatchUpload, a member that stops is dropped by uploading the shorter list.
// kRowsX (profile tag "batch_zero_tall_cols"), kRowsXFree ("batch_zero_tall_free_cols"): grid row b is
// member b's own "zero_tall_cols" / "zero_tall_free_cols" launch.
void ZeroRowsBatchUpload(const std::vector<const ZeroRowsArgs*>& members, DVec* table);
void ZeroFusedRowsBatch(int64_t m, int nparts, RowsSide side, Head head, DType dt, const DVec& table, int count);
// The sample side of `count` tall members with a smooth z term in ONE launch, profile tag
// "batch_zero_tall_samples": grid row b is member b's own ZeroTallSamples launch, a thread per
// sample, on its own record with the carried head in its own hs, hys, hv; no wait, no barrier, no
// atomic.  The members share m and the dtype; the upload is ZeroRowsBatchUpload's.
void ZeroTallSamplesBatchUpload(const std::vector<const ZeroTallSamplesArgs*>& members, DVec* table);
void ZeroTallSamplesBatch(int64_t m, DType dt, const DVec& table, int count);
bool LassoFusedSupported(int64_t m, int64_t n, const DVec& A, int64_t lda);
int LassoFusedGrid(int64_t m, int64_t n, DType dt = F32);
int LassoFusedBlock(int64_t m, int64_t n, DType dt);  // threads per workgroup of the pass
// The share of the m x n matrix that the pass keeps resident in the Infinity Cache under a budget
// of `budget` bytes.  A row chunk is the rows one load instruction of the workgroup covers
// (LassoFusedBlock threads x 16 bytes of a column); chunk q of column j is resident iff
// q < qfull || (q == qfull && j < jcut) - every column carries its piece, so cache hits and HBM
// reads are in flight together.  `bytes` is the largest total of this form that is <= budget;
// a matrix that fits is resident as a whole, budget <= 0 gives qfull = jcut = 0.  A pure function
// of its arguments: no device is touched.
struct FusedResidency {
  int qfull = 0;
  int64_t jcut = 0;
  int64_t bytes = 0;
};
FusedResidency LassoFusedResidency(int64_t m, int64_t n, DType dt, int64_t budget);
// What the most recent launch of the pass (single or batched) in this process was given: lets a
// test see that an option reached the kernel, since no iterate depends on it.
FusedResidency LastFusedResidency();
void NoteFusedResidency(int qfull, int64_t jcut);
void LassoFusedPass(const LassoFusedArgs& args);
// out6 = {||y0||^2, ||y1||^2, ||y0 + y1||^2, ||y1 - y1prev||^2, ||u||^2, peer_err ? 1 : 0} (device
// doubles), one launch; `work`: 64 * 5 + 1 doubles, zero-initialised once (the last double is a
// ticket counter); `peer_err` (optional): the device-side error word of the peer exchange.
// `tag`: the launch's profile tag (the tall lasso route's is "lasso_tall_norms").
void LassoFusedNorms(const DVec& u, const DVec& y0, const DVec& y1, const DVec& y1prev, double* out6,
                     const DVec& work, const unsigned* peer_err = nullptr, const char* tag = "lasso_fused_norms");
// The residual check of a ZERO-term route ("The residual check"), one launch: per
// constraint side c, out10[5 c + ...] = {||y_term||^2, ||y_zero||^2, ||y_term + y_zero||^2,
// ||y_zero - y_zero_prev||^2, ||u||^2} (device doubles; c = 0: `x`, c = 1: `z`), accumulated in double
// from the state's own type.  A side whose u is empty is absent and its five values are 0; of a side
// present u, y_term, y_zero and y_zero_prev are read, all of one length and of the dtype both sides
// share.  At most 64 workgroups, split between the sides as ZeroFusedNormsGrid says; the summation
// order is a function of the two lengths alone.  `work`: kZeroNormsWork doubles, zero-initialised once
// and private to the caller (ten partials per workgroup; the last double is a ticket counter).
// `tag`: "zero_fused_norms" on the fat route, "zero_tall_norms" on the tall ones.
constexpr int64_t kZeroNormsWork = 64 * 10 + 1;
void ZeroFusedNorms(const ConsensusState& x, const ConsensusState& z, double* out10, const DVec& work,
                    const char* tag);
// The workgroups of each side for lengths nx, nz (0: absent, none): one per 1024 entries, and from
// 64 in all on in proportion to the lengths, a side that is present keeping at least one.
void ZeroFusedNormsGrid(int64_t nx, int64_t nz, int* gx, int* gz);

// ---- batched fused pass: instances sharing one data matrix (kernels_fused_batch.hip) ---------
// One instance of a batched sweep as the kernels read it (device array, compute type T): the
// multi-block driver's fused state plus its forward vectors.  Every instance's arithmetic is
// the single pass's (LassoFusedPass, ReducePartials, SymvPacked), so its iterates are
// bit-identical to its own solve.
template <class T> struct LassoBatchInst {
  const T* w;        // m: the inverse apply's output, read by the pass
  T* tpart;          // grid * m: per-workgroup partials of A v0'
  T* u; T* x0; T* x1; T* y0; T* y1; T* y1prev;  // n each, in place
  const T* alpha_v;  // per-column alpha / beta of the scaled zone (nullptr: uniform)
  const T* beta_v;
  T* p;              // m: the reduced partials (+ rhs), input of the inverse apply
  const T* rhs;      // m: constant part of the rhs (nullptr: none)
  T kappa, Bs, Cs, a1, lam, alpha, beta, M;
  T pkappa;          // scale of the summed partials in p (kappa, but for the whitened route)
  T* e0;             // n: the ZERO chain's second "previous y" (nullptr on the lasso chain)
  // the tall ZERO chains; nullptr / unused on kChainLasso and kChainZeroCols
  const T* zg;       // n: kChainZeroTall's offset of the z term (nullptr: none)
  const T* zrhs;     // n: kChainZeroTall's constant on the arg row (nullptr: none)
  T* zd;             // n: kChainZeroTallDot stores the dot products here
  const T* zfarg;    // n: kChainZeroTallAcc reads the forward weights here
  T ke, dinv;        // kChainZeroTall: -L(arg, z'), Dinv(arg)'s scalar
};
// Instances one launch of the batched pass carries for (m, dtype) - set by the register budget
// of its instantiation - or 0 where the single pass would take a form the batched one does not
// mirror (512-thread workgroups): such instances are solved one by one.  Every `chain` has widths of
// its own, (m, n) the pass's own dimensions (the tall chains: features x samples); the halves of the
// tall pass hold half of the per-member registers and are wider.
int LassoBatchWidth(int64_t m, int64_t n, DType dt, Chain chain = kChainLasso);
// The descriptors of `members` in order into `table` (device; grown as needed): the active set
// of a batch is this array, so an instance that stops is dropped by uploading the shorter list.
void LassoBatchUpload(const std::vector<const LassoInstance*>& members, DType dt, DVec* table);
// The fused pass of instances [first, first + count) of `table`, count <= LassoBatchWidth: each
// loaded column of A feeds every instance's dot product, chain and forward update.
// `group_lam` (optional): the instances are ALL the columns of one matrix variable and the
// threshold step is the group shrinkage of its rows with this weight (NORM_2 along axis 1)
// instead of each instance's scaled zone.
// `res`: the matrix's resident share, as in LassoFusedArgs.
// `chain` (BatchPassExists), every record holding what that chain reads and writes, count <=
// LassoBatchWidth(m, n, dt, chain).  group_lam: kChainLasso alone.
void LassoBatchPass(int64_t m, int64_t n, int64_t lda, const DVec& A, const DVec& table, int first,
                    int count, const double* group_lam = nullptr, const FusedResidency& res = FusedResidency(),
                    Chain chain = kChainLasso);
// p = pkappa * sum(tpart) (+ rhs) of `count` instances in one launch, each in the summation order
// of ReducePartials(m, nparts, tpart, pkappa, 0, p, rhs).  `rhs_aligned`: every rhs present is
// 16-byte aligned (picks the same kernel form as the single call).
void ReducePartialsBatch(int64_t m, int nparts, const DVec& table, int count, DType dt,
                         bool rhs_aligned);
// w = alpha * P p for `count` instances (P: SymvPack of a symmetric m x m matrix): every packed
// tile is read once for all of them; each result in SymvPacked's arithmetic order.  `work`:
// count * SymvWorkspace(m) values.
void SymvPackedBatch(int64_t m, double alpha, const DVec& P, const DVec& table, int count,
                     const DVec& work);
// The tile launch of SymvPackedBatch alone (profile tag "batch_symv_packed_tiles"): member b's
// partials of P p_b at work + b * SymvWorkspace(m).
void SymvPackedTilesBatch(int64_t m, const DVec& P, const DVec& table, int count, const DVec& work);

// ---- tall lasso sweep: no pass over A (kernels_fused_tall.hip) ------------------
// The element-wise side of a sweep of the lasso structure whose block LDL^T ends in the dense
// n x n pivot of the variable (more rows than columns): x0 = Dinv r is all of the least-squares
// prox that depends on the iterate.  One launch, profile tag "lasso_tall_cols", one workgroup of
// 256 threads per 128 entries; a thread touches its own entry alone.  Per entry j: x0_j - from
// `partials`, the tile partials of SymvPackedTiles(n, P, inst.p, inst.tpart) summed in SymvPacked's
// order and scaled by inst.kappa (bit for bit SymvPacked's output); else read from inst.w, the
// finished apply - then the lasso chain from x0 on (kernels_fused_chain.h), the six state stores and
// the next sweep's input inst.p[j] = v0'_j - inst.rhs[j] (rhs: c = L(var, arg) rhs_arg; empty: zero).
// inst.pkappa and the z fields are not read.
void LassoTallCols(int64_t n, const LassoInstance& inst, bool partials);
// `count` members (LassoBatchUpload) in ONE launch, profile tag "batch_lasso_tall_cols": grid row b
// is member b's own LassoTallCols launch on its own record with its partials at
// work + b * SymvWorkspace(n) (SymvPackedTilesBatch), so its result is that of its own solve bit for bit.
void LassoTallColsBatch(int64_t n, DType dt, const DVec& table, int count, const DVec& work);

// ---- wide batched sweep on the f32 matrix instruction (kernels_fused_wide.hip) -----------------
// A panel is up to kLassoWidePanel f32 instances of one `table` (LassoBatchUpload), slots
// [first, first + nk); bit s of `active` says that slot first + s is still iterating (a stopped
// slot is masked on every store).  Panels are instance-major: slot s of W (the pass's input w) at
// s * ldw, of V (the chain's return value, the forward product's input) at s * ldv, of T (the
// forward product's partials: LassoWideSlabs(m, n) panels of 16 * ceil(nk / 16) slots) at s * ldt;
// ld* are multiples of 4 and the padding of V (columns n .. ldv) is zero.  An instance's bits do
// not depend on its slot, on nk or on the other instances; they are not the single pass's bits.
constexpr int kLassoWidePanel = 64;
bool LassoWideSupported(int64_t m, int64_t n, const DVec& A, int64_t lda);
// Column slabs of the forward product: a function of (m, n) alone.
int LassoWideSlabs(int64_t m, int64_t n);
// D = A^T W and the chain of every live slot: updates its x0, x1, y0, y1, u, y1prev and writes V.
// `group_lam` (optional): the nk slots are all the columns of one matrix variable, all live, and
// the threshold step is the group shrinkage of its rows with this weight (as LassoBatchPass).
void LassoWideBack(int64_t m, int64_t n, int64_t lda, const DVec& A, const DVec& table, int first, int nk,
                   uint64_t active, const DVec& W, int64_t ldw, const DVec& V, int64_t ldv,
                   const double* group_lam = nullptr);
// T_s = A[:, slab s] V[slab s, :] for every slab s.
void LassoWideForward(int64_t m, int64_t n, int64_t lda, const DVec& A, int nk, const DVec& V, int64_t ldv,
                      const DVec& T, int64_t ldt);
// p = pkappa * (T_0 + T_1 + ...) + rhs of every live slot (its descriptor's p, rhs, pkappa).
void LassoWideReduce(int64_t m, int64_t n, const DVec& table, int first, int nk, uint64_t active, const DVec& T,
                     int64_t ldt);

// ---- one-shot peer-write exchange (kernels_peer.hip; PeerView in comm.h) ----------------------
void PeerBumpEpoch(const PeerView& pv);
// y = (sum over ranks, in rank order, of alpha * sum_k partial[k*rows + r]) + add
void PeerReduceExchange(const PeerView& pv, int64_t rows, int nparts, const DVec& partial,
                        double alpha, const DVec* add, const DVec& y);
bool PeerSlabApplySupported(const PeerView& pv, int64_t m, int64_t slab, const DVec& D, int64_t ldd);
// wpad[q*slab + j] = scale * D[:, q*slab + j] . p for every rank q (this rank computes q = rank,
// lo = rank*slab, pushes it to the peers and gathers theirs); columns >= m give 0.
void PeerSlabApplyExchange(const PeerView& pv, int64_t m, int64_t slab, int64_t lo, const DVec& D,
                           int64_t ldd, double scale, const DVec& p, const DVec& wpad);

// ---- K4: dense mat-mat (reference linear/linear_map_multiply.cc:14-37 dgemm_) -------------
// C (M x N, ldc) = alpha * op(A) (M x K) * op(B) (K x N) + beta * C ; column-major.
// lower_only: compute only tiles touching the lower triangle (SYRK-style); the caller
// mirrors with SymmetrizeFromLower.
void Gemm(bool transA, bool transB, int64_t M, int64_t N, int64_t K, double alpha,
          const DVec& A, int64_t lda, const DVec& B, int64_t ldb, double beta, const DVec& C,
          int64_t ldc, bool lower_only = false);
// The same for batch * outer problems (blockIdx.z = z): operands at element offsets
// (z % batch) * s + (z / batch) * s2, results at z * sC.
void GemmBatched(bool transA, bool transB, int64_t M, int64_t N, int64_t K, double alpha,
                 const DVec& A, int64_t lda, int64_t sA, const DVec& B, int64_t ldb, int64_t sB,
                 double beta, const DVec& C, int64_t ldc, int64_t sC, int64_t batch,
                 bool lower_only = false, int64_t outer = 1, int64_t sA2 = 0, int64_t sB2 = 0);
void SymmetrizeFromLower(const DVec& C, int64_t n, int64_t ldc);
// The branch the last Gemm / GemmBatched call of this thread took, a host-side record for the tests:
// "small", "generic", "mfma_f32", "mfma_f32_pipe", "mfma_f64", "mfma_f64_pipe", "split_k",
// "multi_gemv_n", "multi_gemv_t" or "f16split"; "" after GemmClearRoute or a call that launched nothing.
const char* GemmLastRoute();
void GemmClearRoute();
// Large f32 products on the f16 matrix cores with two-term split operands
// (kernels_gemm_f16split.hip): f32 accuracy at 3/16 of the f32 MFMA time.  Gemm routes there by
// itself (f32, M, N >= 1024, K >= 256, >= 8e9 multiply-adds); false = not eligible, nothing done.
bool GemmSplitF16(bool transA, bool transB, int64_t M, int64_t N, int64_t K, double alpha, const DVec& A,
                  int64_t lda, const DVec& B, int64_t ldb, double beta, const DVec& C, int64_t ldc,
                  bool lower_only);
// fp64 products on the software-pipelined f64 MFMA kernel (kernels_gemm_f64.hip), arguments as
// GemmBatched (n1 = inner batch count, batch = n1 * outer); false if the operands are not
// 16-byte aligned (nothing is done).
bool GemmF64Pipe(bool transA, bool transB, int64_t M, int64_t N, int64_t K, double alpha, const DVec& A,
                 int64_t lda, int64_t sA, const DVec& B, int64_t ldb, int64_t sB, double beta,
                 const DVec& C, int64_t ldc, int64_t sC, int64_t n1, int64_t batch, bool lower_only,
                 int64_t sA2, int64_t sB2);
// C = alpha A B (no transposes, beta = 0) with B (kmode 3) or A (kmode 4) lower triangular, on the
// split-f16 kernel with a k range per tile; false: not eligible, nothing done.
bool GemmSplitF16KRange(int kmode, int64_t M, int64_t N, int64_t K, double alpha, const DVec& A, int64_t lda,
                        const DVec& B, int64_t ldb, const DVec& C, int64_t ldc);
// Lower tiles of C = X^T X for a lower-triangular X (zeros stored above the diagonal) in one launch
// of the split-f16 kernel with a k range per tile; false: not eligible (f32, n >= 2048), nothing done.
bool SyrkSplitF16LowerTriangular(int64_t n, const DVec& X, int64_t ldx, const DVec& C, int64_t ldc);
// C (M x N, ldc == M, N <= 16) = alpha op(A) B + beta C as a mat-vec with N right-hand sides
// (kernels_gemv_multi.hip); false if the shape / alignment is not covered (nothing is done).
bool MultiGemv(bool transA, int64_t M, int64_t N, int64_t K, double alpha, const DVec& A, int64_t lda,
               const DVec& B, int64_t ldb, double beta, const DVec& C, int64_t ldc);
// HBM ceiling probes: mode 0 read (non-temporal), 1 read, 2 copy; scratch holds `grid` floats.
void StreamProbe(int mode, const void* src, void* dst, int64_t bytes, float* scratch, int grid);
// Residency probe: reads the buffer as 40000-byte columns, the first `resident_per_column` bytes
// (a multiple of 16) of each with the default policy, the rest non-temporal.
void StreamResidentProbe(const void* src, int64_t bytes, int64_t resident_per_column, float* scratch, int grid);

// dst (rows x cols, ld = rows) = alpha * op(src)
void MatCopy(bool trans, int64_t rows, int64_t cols, double alpha, const DVec& src,
             int64_t lds, const DVec& dst);
// W[i,i] += alpha (d undefined) or W[i,i] += alpha*d[i]
void AddDiag(const DVec& W, int64_t n, int64_t ld, double alpha, const DVec* d);
// colsum_dev[j] = sum_i |A(i, j)| as device doubles (max_j = the 1-norm of A): condition estimates
void ColAbsSums(const DVec& A, int64_t rows, int64_t cols, int64_t lda, double* colsum_dev);
// y = x / sqrt(*normsq_dev) (device scalar; 0 leaves x unscaled): power-iteration normalisation
void ScaleByInvNorm(const DVec& y, const DVec& x, const double* normsq_dev);
// dst (mA*mB x nA*nB) = kron(A, B), all column-major contiguous
void KronDense(const DVec& dst, const DVec& A, int64_t mA, int64_t nA, const DVec& B,
               int64_t mB, int64_t nB);
// y = A x for W = diag? helpers used by Kronecker apply are composed from Gemm.

// ---- K5: symmetric definite inverse (reference linear/dense_matrix_impl.cc:21-30) ---------
// W (n x n, ld = n, symmetric positive definite, full storage) -> W^{-1} in place.
// Blocked Cholesky + triangular inverse + X^T X, all on device.  Throws if a pivot is <= 0.
// `factor_inverse` (optional) receives X = L^-1 (n x n, ld n, zeros above the diagonal).
// Only the lower triangle of W (i >= j) is read: no result depends on what lies above the diagonal.
void SpdInverseInPlace(const DVec& W, int64_t n, DVec* factor_inverse = nullptr);
// Cholesky step form of the next factorisations: -1 by environment (default), 0 the fused f32 step,
// 1 the diagonal + panel launches (tests hold the two forms to each other)
void SetPotrfForm(int form);
// Columns [lo, lo + cnt) of W^-1 into Out (n x cnt, ld n); W is overwritten by its Cholesky
// factor.  Cholesky + two blocked triangular solves on the cnt unit columns.
// Only the lower triangle of W (i >= j) is read; its strict upper triangle is scratch afterwards.
void SpdInverseColumns(const DVec& W, int64_t n, int64_t lo, int64_t cnt, const DVec& Out);

// ---- K6 / K12: elementwise and group prox kernels ------------------------------------------
// reference prox/scaled_zone.cc:78-104 ; lam / alpha / beta are either uniform scalars or
// per-element device vectors (pass defined DVecs to use the vector form).
struct ScaledZoneArgs {
  double lam = 0, alpha = 1, beta = 1, M = 0, C = 0;
  const DVec* lam_vec = nullptr;
  const DVec* alpha_vec = nullptr;
  const DVec* beta_vec = nullptr;
  int64_t period = 0;  // >0: alpha/beta/lam vectors are indexed by (i % period)
};
void ScaledZone(const DVec& x, const DVec& v, const ScaledZoneArgs& args);
// reference prox/non_negative.cc:8
void MaxZero(const DVec& x, const DVec& v);
// reference prox/norm_2.cc:11-16 ; normsq is a device slot holding ||v||^2
void Norm2Shrink(const DVec& x, const DVec& v, double lam, const double* normsq);
// x = soft-threshold of singular values etc. is composed from ScaledZone.

// ---- epigraph projections (reference prox/sum_square.cc:42-57, prox/scaled_zone.cc:152-279) ----
// SUM_SQUARE epigraph: lam = max(0, largest real root of the cubic of newton.cc:293-323) from
// ||u||^2 (device slot) and s (1 element); x = u / (1 + 2 lam), t = s + lam.  No host sync.
void SumSquareEpigraph(const DVec& x, const DVec& t, const DVec& u, const DVec& s,
                       const double* normsq, double* lam_scratch);
// Scaled-zone epigraph, pass 1: keys k_i = (|y_i| - M) / w_i and weights w_i^2 for the samples
// that can move (w = alpha for y > 0, beta for y < 0), zero weight otherwise; *fval += f(y).
void ZoneEpigraphKeys(const DVec& v, double alpha, double beta, const DVec* alpha_vec,
                      const DVec* beta_vec, double M, double C, double* key, double* w2,
                      double* fval);
// pass 2: sums[0] += sum w2*k, sums[1] += sum w2, sums[2] += count over {k_i > lam, w2_i > 0}
void ZoneEpigraphSums(int64_t n, const double* key, const double* w2, double lam, double* sums);

// ---- K11: SVD for the orthogonally-invariant proxes (reference prox/ortho_invariant.cc) ------
// One-sided Jacobi on W (m x n, ld = m): on return W = U*Sigma (orthogonal columns) and the
// input equals W V^T; V (n x n) is overwritten.  Returns the number of sweeps used.
// warm: V holds an orthogonal matrix on entry and W has already been multiplied by it (the
// decomposition continues from there: Y = W V^T holds throughout).
// row_sharded: W holds this rank's block of rows (V replicated); the column inner products are
// all-reduced over the communicator (block form only).
int JacobiSvd(const DVec& W, int64_t m, int64_t n, const DVec& V, int max_sweeps = 40,
              bool warm = false, bool row_sharded = false);
// The same decomposition by the block algorithm (pairs of 32-column panels: batched Gram on the
// MFMA kernel, 64 x 64 eigenproblems on chip, batched GEMM updates); JacobiSvd switches to it
// from 1536 columns up (measured crossover on MI355X; EPSILON_HIP_SVD=block|scalar forces one).
int BlockJacobiSvd(const DVec& W, int64_t m, int64_t n, const DVec& V, int max_sweeps = 40,
                   bool warm = false, bool row_sharded = false);
// The same with the rotations applied to W only (no right factor is accumulated: a step moves
// 0.6 of the bytes); fp32 block form.  JacobiSvdCanSkipV says whether it applies.
bool JacobiSvdCanSkipV(int64_t m, int64_t n, DType dt);
int JacobiSvdNoV(const DVec& W, int64_t m, int64_t n, int max_sweeps = 40);
void ColNorms(const DVec& W, int64_t m, int64_t n, const DVec& sigma, bool row_sharded = false);
// W[:, j] *= xt[j] / sigma[j]   (0 where sigma[j] == 0, as ortho_invariant.cc:44-49)
void ColScaleByRatio(const DVec& W, int64_t m, int64_t n, const DVec& sigma, const DVec& xt);

// ---- batched ("segmented") and Newton-family operators (kernels_segprox.hip) ------------------
// A segment is one slice of the argument the reference's axis loop would visit
// (prox/vector_prox.cc:150-177): entry p of segment s lives at s*seg_stride + p*elem_stride.
struct Segs {
  int64_t count = 1, len = 0, seg_stride = 0, elem_stride = 1;
};
void SegNorm2Shrink(const DVec& x, const DVec& v, double lam, const Segs& S);
void SegMaxProx(const DVec& x, const DVec& v, double lam, const Segs& S);          // prox/max.cc:7-43
void SegMaxEpigraph(const DVec& x, const DVec& t, const DVec& v, const DVec& s, const Segs& S);
void SegSumLargestProx(const DVec& x, const DVec& v, double lam, int k, const Segs& S);
void SegSumLargestEpigraph(const DVec& x, const DVec& t, const DVec& v, const DVec& s, int k,
                           const Segs& S);
// scaled-zone epigraph per segment; alpha/beta vectors (if given) are indexed by the position
// within the segment (scaled_zone.cc:34-44 sizes them with the slice length)
void SegZoneEpigraph(const DVec& x, const DVec& t, const DVec& v, const DVec& s, double alpha,
                     double beta, const DVec* alpha_vec, const DVec* beta_vec, double M,
                     const Segs& S);
// one second-order cone per segment: (x_s, t_s) = proj{||x|| <= beta t} (second_order_cone.cc:58-79)
void SegSocProject(const DVec& x, const DVec& t, const DVec& v, const DVec& tin, double beta,
                   const Segs& S);
void SegLogSumExpProx(const DVec& x, const DVec& v, double lam, const Segs& S);
void SegLogSumExpEpigraph(const DVec& x, const DVec& t, const DVec& v, const DVec& s,
                          const Segs& S);
// elementwise argmin lam f(x) + 1/2 (x - v)^2 (prox/newton.cc:49-112, sum_neg_log.cc:9-24)
void SmoothProx(SmoothFn fn, const DVec& x, const DVec& v, double lam, const DVec* lam_vec);
void SegSmoothEpigraph(SmoothFn fn, const DVec& x, const DVec& t, const DVec& v, const DVec& s,
                       const Segs& S);
void KlDivProx(const DVec& x, const DVec& y, const DVec& u, const DVec& v, double lam,
               const DVec* lam_vec);
void SegKlDivEpigraph(const DVec& x, const DVec& y, const DVec& t, const DVec& u, const DVec& v,
                      const DVec& s, const Segs& S);
void ExpEpigraph(const DVec& x, const DVec& t, const DVec& v, const DVec& s);  // prox/exp.cc

// reference prox/total_variation_1d.cc:21 (glmgen tf_dp): exact 1-D TV prox of every slice of S
// on its own (no term couples two slices), one lam for all, in the passes of one call.  Slices
// are contiguous (elem_stride 1, seg_stride len) or the rows of a column-major matrix (seg_stride
// 1, elem_stride count).  Returns the depth of the level-set recursion, the maximum over the
// slices; 0 for the trivial cases (len <= 1 or lam == 0: x = v).  One signal is the single slice
// that covers v (count 1, len n).
int Tv1dSeg(const DVec& x, const DVec& v, double lam, const Segs& S);

}  // namespace k
}  // namespace eps
