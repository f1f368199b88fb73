// Fused sweep kernel for "least squares + separable threshold" problems (the compiled lasso,
// SURVEY.md 3.3): ONE pass over the data matrix per ADMM sweep instead of two.
//
// In the reference a sweep touches A twice - `A v` in the forward substitution and `A^T w` in
// the back substitution of the least-squares prox (reference vector/block_cholesky.cc:86-117 via
// linear/dense_matrix_impl.cc:63) - with the elementwise NORM_1 prox and the u/y bookkeeping of
// prox_admm.cc:135-147 in between.  Everything between `A^T w` of sweep k and `A v` of sweep k+1
// is elementwise in the column index j.  So for each column j, while it sits in registers:
//
//     d_j   = A[:,j] . w                         (back substitution of sweep k)
//     x0_j  = v0_j + kappa d_j ;  y0, u, prox-1 (two-sided threshold), y1, u  ... -> v0'_j
//     t'   += A[:,j] * v0'_j                     (forward substitution of sweep k+1)
//
// The elementwise chain repeats the reference's operations one by one, in order, one rounding
// each (this file is compiled with -ffp-contract=off), so given d_j the state is bit-identical
// to the unfused path.  HBM traffic per sweep drops from (2mn + m^2)s to (mn + m^2)s.
//
// Geometry: BS threads own all m rows (thread t: rows R(t + BS q), q < NR - 16 B loads of R = 4
// f32 or 2 f64 rows, coalesced); w and the partial t' stay in registers for the whole launch; the
// dot products are reduced with wave shuffles + LDS in a fixed order (deterministic);
// per-workgroup partial t' vectors are summed by ReducePartials.  LassoFusedStreamKernelT takes
// one column per step with the next column's NR loads already issued, so the memory pipe never
// drains.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "kernels.h"
#include "kernels_fused_chain.h"
#include "options.h"

namespace eps {
namespace k {

namespace {

constexpr int kBlock = 256;

// ONE column per step, the next column already in flight: the loads of column j+1 are issued
// before the dot product of column j is reduced, so every workgroup keeps NR 16-byte loads per
// lane outstanding at all times (6.0 TB/s on the 1e4 x 5e4 matrix, against 5.75 for a form that
// took columns in pairs with nothing in flight while it reduced).
// BS threads own the m rows: 256 (two workgroups per CU) up to m = 10240 in f32; 512 (one
// workgroup of 8 waves per CU) up to m = 20480 (6.37 TB/s on 2e4 x 5e4).  In f64 a 16-byte load
// holds two rows, so 512 threads x 10 chunks own up to 10240 rows.
// CHAIN: what a column does between its dot product and its forward update, and what the state
// arrays, e0, e1 and `zt` then hold (Chain, kernels.h; u, x0, x1, y0, y1, y1prev are the instance's u,
// copy, var, y_zero, y_term, y_term_prev, e0 its y_zero_prev).  kChainZeroTallDot stores d_j through
// `e0`, here the vector zd; kChainZeroTallAcc reads f_arg_j through `zt.rhs`, here zfarg.
// Head: the tag of what stands in the threshold's place (kernels_fused_chain.h; void: the zone), for
// the forms FusedPassExists lists; the same arrays, the same tag, and for LinearStep one broadcast
// load of g_j from `zt.g` per streamed column.
template <class T, int NR, int BS, int CHAIN, class Head = void>
__global__ __launch_bounds__(BS, 2) void LassoFusedStreamKernelT(
    int64_t m, int64_t n, const T* __restrict__ A, int64_t lda, const T* __restrict__ w,
    FusedScalarsT<T> c, T* u, T* x0, T* x1, T* y0, T* y1, T* y1prev, T* __restrict__ tpart,
    unsigned* epoch, T* e0, T* e1, int qfull, int64_t jcut, ZeroTallScalarsT<T> zt) {
  typedef typename Chunk<T>::V V;
  constexpr int R = Chunk<T>::R;
  constexpr bool kHalf = ChainIsTallHalf(static_cast<Chain>(CHAIN));  // no state, no head
  __shared__ T red[2][BS / 64];
  // sweep counter of the peer exchange (kernels_peer.hip): the two exchange kernels that follow
  // this pass in stream order tag their granules with it
  if (epoch != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *epoch += 1u;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (a constant, not a vector filled element by element: with the latter the compiler turns the
  // guarded loads below into selects and drops their non-temporal hint)
  const V zero = T(0);
  V wv[NR], tp[NR];
  int64_t row[NR];
#pragma unroll
  for (int q = 0; q < NR; ++q) {
    row[q] = (static_cast<int64_t>(q) * BS + tid) * R;
    if constexpr (CHAIN != kChainZeroTallAcc) wv[q] = row[q] < m ? *reinterpret_cast<const V*>(w + row[q]) : zero;
    if constexpr (CHAIN != kChainZeroTallDot) tp[q] = zero;
  }
  // this workgroup's columns: pairs (2 jp, 2 jp + 1), jp = blockIdx.x + k gridDim.x, one column
  // at a time
  const int64_t npairs = (n + 1) / 2;
  auto column = [&](int64_t step) -> int64_t {  // step -> column index, or -1 past the end
    const int64_t jp = blockIdx.x + (step >> 1) * gridDim.x;
    const int64_t j = 2 * jp + (step & 1);
    return (jp < npairs && j < n) ? j : -1;
  };
  // The matrix is read once per sweep.  Its resident share (LassoFusedResidency: row chunks below
  // qfull of every column, chunk qfull of the columns below jcut) is loaded with the default
  // policy and stays in the 256 MB Infinity Cache from sweep to sweep; the rest is non-temporal,
  // which neither displaces that share nor the cached inverse where the sweep applies one.
  auto load = [&](V (&a)[NR], int64_t j) {
    const T* cp = A + j * lda;
    const int nres = qfull + (j < jcut ? 1 : 0);  // uniform: the choice below is a scalar branch
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      if (row[q] < m) a[q] = LoadMatrixChunk<T>(cp + row[q], q < nres);
      else a[q] = zero;
    }
  };
  V cur[NR], nxt[NR];
  int64_t step = 0;
  int64_t j = column(0);
  if (j >= 0) load(cur, j);
  int par = 0;
  while (j >= 0) {
    // skip the odd slot of a trailing unpaired column without breaking the sequence
    int64_t jn = column(step + 1);
    if (jn < 0 && ((step + 1) & 1)) jn = column(step + 2);
    const int64_t step_n = (jn >= 0 && column(step + 1) < 0) ? step + 2 : step + 1;
    if (jn >= 0) load(nxt, jn);
    // per-column state (same address in every lane: broadcast loads)
    T uj = T(0), y0j = T(0), y1j = T(0);
    if constexpr (!kHalf) {
      uj = u[j];
      y0j = y0[j];
      y1j = y1[j];
    }
    T u1j = T(0);
    if constexpr (CHAIN == kChainTwoBlock) u1j = e0[j];
    T gj = T(0), rj = T(0);
    if constexpr (CHAIN == kChainZeroTall) {
      if (zt.g != nullptr) gj = zt.g[j];
      if (zt.rhs != nullptr) rj = zt.rhs[j];
    }
    if constexpr (std::is_same<Head, LinearStep>::value) gj = zt.g[j];
    T d = T(0);
    if constexpr (CHAIN != kChainZeroTallAcc) {
#pragma unroll
      for (int q = 0; q < NR; ++q)
#pragma unroll
        for (int r = 0; r < R; ++r) d += cur[q][r] * wv[q][r];
      d = WaveSumT<T>(d);
      if (lane == 0) red[par][wave] = d;
      __syncthreads();
      d = red[par][0];
#pragma unroll
      for (int w2 = 1; w2 < BS / 64; ++w2) d += red[par][w2];
      par ^= 1;
    }
    FusedScalarsT<T> cj = c;
    if (c.alpha_v != nullptr) cj.alpha = c.alpha_v[j];
    if (c.beta_v != nullptr) cj.beta = c.beta_v[j];
    T v0n = T(0);
    if constexpr (CHAIN == kChainZeroTallDot) {
      if (tid == 0) e0[j] = d;
    } else if constexpr (CHAIN == kChainZeroTallAcc) {
      v0n = zt.rhs[j];
    } else if constexpr (CHAIN == kChainLasso) {
      T nx0, nx1, ny0, ny1, nu;
      v0n = ChainOneT<T>(d, cj, uj, y0j, y1j, &nx0, &nx1, &ny0, &ny1, &nu);
      if (tid == 0) {
        y1prev[j] = y1j;
        x0[j] = nx0;
        x1[j] = nx1;
        y0[j] = ny0;
        y1[j] = ny1;
        u[j] = nu;
      }
    } else if constexpr (CHAIN == kChainZeroCols || CHAIN == kChainZeroTall) {
      T ns, nq, nys, nyq, nu;  // (gj: zero but for the linear head and kChainZeroTall's offset)
      if constexpr (CHAIN == kChainZeroCols)
        v0n = ZeroChainT<T, Head>(d, cj, gj, uj, y1j, y0j, &ns, &nq, &nys, &nyq, &nu);
      else
        v0n = ZeroTallChainT<T, Head>(d, cj, zt.ke, zt.dinv, gj, rj, uj, y1j, y0j, &ns, &nq, &nys, &nyq, &nu);
      if (tid == 0) {
        y1prev[j] = y1j;
        e0[j] = y0j;
        x1[j] = ns;
        x0[j] = nq;
        y1[j] = nys;
        y0[j] = nyq;
        u[j] = nu;
      }
    } else {
      T nx0, nx1, nz0, nz1, nu0, nu1;
      v0n = ChainTwoBlockT<T>(d, cj, y0j, y1j, uj, u1j, &nx0, &nx1, &nz0, &nz1, &nu0, &nu1);
      if (tid == 0) {
        y1prev[j] = y0j;  // z_prev
        e1[j] = y1j;
        x0[j] = nx0;
        x1[j] = nx1;
        y0[j] = nz0;
        y1[j] = nz1;
        u[j] = nu0;
        e0[j] = nu1;
      }
    }
    if constexpr (CHAIN != kChainZeroTallDot) {
#pragma unroll
      for (int q = 0; q < NR; ++q)
#pragma unroll
        for (int r = 0; r < R; ++r) tp[q][r] += cur[q][r] * v0n;
    }
#pragma unroll
    for (int q = 0; q < NR; ++q) cur[q] = nxt[q];
    j = jn;
    step = step_n;
  }
  if constexpr (CHAIN != kChainZeroTallDot) {
    T* out = tpart + static_cast<int64_t>(blockIdx.x) * m;
#pragma unroll
    for (int q = 0; q < NR; ++q)
      if (row[q] < m) *reinterpret_cast<V*>(out + row[q]) = tp[q];
  }
}

template <class T, int NR, int BS>
void LaunchFused(const LassoFusedArgs& a, int grid) {
  const LassoBatchInst<T> i = Narrow<T>(a.inst);
  const ZoneParams& z = a.inst.zone;
  T* e0 = a.chain == kChainZeroTallDot ? i.zd : i.e0;  // the dot half stores d through it
  T* e1 = a.chain == kChainTwoBlock ? a.e1.as<T>() : nullptr;
  ZeroTallScalarsT<T> zt = {nullptr, nullptr, T(0), T(0)};
  if (a.chain == kChainZeroTall) zt = {i.zg, i.zrhs, i.ke, i.dinv};
  if (a.chain == kChainZeroTallAcc) zt.rhs = i.zfarg;  // the accumulate half reads f_arg through it
  if (z.head == kHeadLinear) zt.g = i.zg;
  // the one instantiation of (chain, head) in this shape; LassoFusedPass has checked that it exists
  decltype(&LassoFusedStreamKernelT<T, NR, BS, kChainLasso>) kernel = nullptr;
  WithChain(a.chain, [&](auto chain) {
    WithHead(z.head, [&](auto head) {
      constexpr Chain kChain = decltype(chain)::value;
      typedef typename decltype(head)::type H;
      if constexpr (FusedPassExists(kChain, HeadOf<H>(), BS)) kernel = LassoFusedStreamKernelT<T, NR, BS, kChain, H>;
    });
  });
  EPS_CHECK(kernel != nullptr);
  hipLaunchKernelGGL(
      kernel,
      dim3(grid), dim3(BS), 0, Runtime::Get().stream(), a.m, a.n, a.A.as<T>(), a.lda, i.w,
      ScalarsOf<T>(z, a.inst.kappa, a.a0, 1.0 / (a.a0 * a.a0 + z.a1 * z.a1)), i.u, i.x0, i.x1, i.y0, i.y1,
      i.y1prev, i.tpart, a.epoch, e0, e1, a.qfull, a.jcut, zt);
}

// The instantiation for (type, threads, 16-byte row chunks a thread needs).  512 threads: the
// f32 pass also has the 2 and 5 chunk forms (EPSILON_HIP_FUSED_BLOCK=512 below 10240 rows; 5
// still fits two workgroups per CU), the f64 pass takes 512 threads only above 5120 rows.
template <class T>
void LaunchFusedT(const LassoFusedArgs& a, int grid, int block) {
  const int64_t need = (a.m + Chunk<T>::R * block - 1) / (Chunk<T>::R * block);
  if (block == 256) {
    if (need <= 1) LaunchFused<T, 1, 256>(a, grid);
    else if (need <= 2) LaunchFused<T, 2, 256>(a, grid);
    else if (need <= 4) LaunchFused<T, 4, 256>(a, grid);
    else if (need <= 8) LaunchFused<T, 8, 256>(a, grid);
    else LaunchFused<T, 10, 256>(a, grid);
    return;
  }
  if constexpr (std::is_same<T, float>::value) {
    if (need <= 2) return LaunchFused<T, 2, 512>(a, grid);
    if (need <= 5) return LaunchFused<T, 5, 512>(a, grid);
  }
  if (need <= 8) LaunchFused<T, 8, 512>(a, grid);
  else LaunchFused<T, 10, 512>(a, grid);
}

// ---- the sample side of a tall ZERO-term sweep with a smooth z term --------------------------------
// Between the two halves of the tall pass ("zero_tall_dot", "zero_tall_acc"): a thread per sample,
// so the fp64 Newton of the z term runs once per sample and sweep, on whole waves.  ZeroTallChainT
// from its second line on, with the head of this sweep (s, y_s, v) carried from the previous launch
// in hs, hys, hv as on the fat route's row kernel: finishes the sweep from d_i = C[i,:] . x', stores
// the boundary state as kChainZeroTall does, computes the next head once, leaves it in hs, hys, hv and
// writes the next f_arg_i for the accumulate pass.  A thread reads and writes its own sample alone.
//
// One member's sample side as the kernels read it (compute type T): the single launch takes it as
// its argument, the batched launch (tag "batch_zero_tall_samples") reads row blockIdx.y of a device
// table of them.  The arrays of one member do not overlap.
template <class T> struct ZeroTallSamplesInst {
  FusedScalarsT<T> c;
  double lam64;
  T ke, dinv;
  const T* g;    // nullptr: none
  const T* rhs;  // nullptr: none
  const T* d;
  T* u; T* z; T* zq; T* yz; T* yq; T* yzprev; T* yqprev;
  T* hs; T* hys; T* hv;
  T* farg;
};

// Sample i of one member: the body of the single and of the batched kernel.
template <class T, class Fn>
__device__ __forceinline__ void ZeroTallSamplesBody(int64_t m, const ZeroTallSamplesInst<T>& I, int64_t i) {
  if (i >= m) return;
  const FusedScalarsT<T>& c = I.c;
  const T ke = I.ke, dinv = I.dinv;
  const T gi = I.g != nullptr ? I.g[i] : T(0), ri = I.rhs != nullptr ? I.rhs[i] : T(0);
  const T s = I.hs[i], ys = I.hys[i], v = I.hv[i];
  const T fa = ZeroTallForwardT<T>(v, ri, ke);
  const T garg = dinv * fa;
  const T arg = c.kappa * I.d[i] + garg;
  const T q = ke * arg + v;
  const T un = v - q;  // y_q = q (its constraint map is I); u -= y_q
  I.yzprev[i] = I.yz[i];
  I.yqprev[i] = I.yq[i];
  I.z[i] = s;
  I.zq[i] = q;
  I.yz[i] = ys;
  I.yq[i] = q;
  I.u[i] = un;
  const ZeroHeadT<T> hn = ZeroHeadOfT<T, Fn>(c, gi, un, ys, q, I.lam64);
  I.hs[i] = hn.s;
  I.hys[i] = hn.ys;
  I.hv[i] = hn.v;
  I.farg[i] = ZeroTallForwardT<T>(hn.v, ri, ke);
}

template <class T, class Fn>
__global__ __launch_bounds__(kBlock) void ZeroTallSamplesKernel(int64_t m, ZeroTallSamplesInst<T> I) {
  ZeroTallSamplesBody<T, Fn>(m, I, static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x);
}

// The members of a batch: grid row b is member b's single launch, thread for thread.  A thread
// touches its own member's sample alone; nothing waits on another thread.
template <class T, class Fn>
__global__ __launch_bounds__(kBlock) void ZeroTallSamplesBatchKernel(
    int64_t m, const ZeroTallSamplesInst<T>* __restrict__ tab) {
  const ZeroTallSamplesInst<T> I = tab[blockIdx.y];
  ZeroTallSamplesBody<T, Fn>(m, I, static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x);
}

// ---- the row side of a ZERO-term sweep ------------------------------------------------------------
// A workgroup owns ROWS rows: thread (rl, pl) = (t % ROWS, t / ROWS) sums row rl's partials
// k = pl, pl + kZeroLanes, ... (independent loads), the lanes of a row are added in lane order
// through LDS - a fixed summation order, a function of (m, nparts) alone - and lane 0 runs the
// row's chain (d = w_i, kappa = -e) and writes r.  A workgroup reads and writes the state of its
// own rows only.
// Fn = void, 16 rows: the z term is a scaled zone (ZeroChainT; a threshold on 16 lanes).  Fn =
// NonNegStep: the same with the non-negative cone in the zone's place.
// Fn a smooth function, 64 rows: the lanes pl = 0 are one whole wave, so the fp64 Newton runs on
// every lane of the only wave that is still alive; consecutive lanes load consecutive rows of a
// partial vector.  The head of this sweep (s, y_s, v) comes from the previous launch in hs, hys,
// hv, and the next one is computed once and left there: one Newton solve per row and sweep.  A
// head is a function of the stored boundary state alone, so carrying it changes no bit.
constexpr int kZeroLanes = 16, kZeroRows = kBlock / kZeroLanes, kZeroSmoothRows = 64;

// One member's row side as the kernels read it (compute type T): the single launch takes it as
// its argument, the batched launch reads row blockIdx.y of a device table of them.
template <class T> struct ZeroRowsInst {
  const T* tpart;
  const T* w;
  const T* rhs;  // nullptr: none
  const T* g;    // nullptr: none
  T* u; T* z; T* zq; T* yz; T* yq; T* yzprev; T* yqprev;
  T* r;
  T* hs; T* hys; T* hv;  // smooth form alone
  FusedScalarsT<T> c;
  T pkappa;
  double lam64;
};

// Workgroup `block` of one member's row side: the body of the single and of the batched kernel.
// TALL (tag "zero_tall_cols"): the x side of a tall problem over the n entries of x.  The same
// summation of the partials; the chain takes q = x'_j as the inverse apply left it in w
// (ZeroTallColsChainT) and r_j = f_x = v_x' + pkappa sum: no rhs on this side.  Fn = void: the x term
// is a scaled zone; Fn = RidgeStep: a ridge term; Fn = LinearStep: a linear term, its per-entry
// constant in I.g.
// FREE (with TALL, Fn = void; tag "zero_tall_free_cols"): x lives in the ZERO term alone, so the side
// has no state, no term and no chain.  The same summation of the partials; then lane 0 keeps
// x_j = w_j of the sweep the pass just used in I.zq (the ZERO term's own variable of this side: here x
// itself) and writes r_j = f_x = pkappa sum.  Of the record it reads tpart, w, zq, r and pkappa alone.
template <class T, int ROWS, class Fn, bool TALL = false, bool FREE = false>
__device__ __forceinline__ void ZeroRowsBody(int64_t m, int nparts, const ZeroRowsInst<T>& I, unsigned block) {
  __shared__ T part[kZeroLanes][ROWS];
  const FusedScalarsT<T>& c = I.c;
  const int t = threadIdx.x, rl = t % ROWS, pl = t / ROWS;
  const int64_t i = static_cast<int64_t>(block) * ROWS + rl;
  T s = T(0);
  if (i < m) {
    const T* p = I.tpart + i;
    int k = pl;
    for (; k + 7 * kZeroLanes < nparts; k += 8 * kZeroLanes) {
      T v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = p[static_cast<int64_t>(k + q * kZeroLanes) * m];
#pragma unroll
      for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; k < nparts; k += kZeroLanes) s += p[static_cast<int64_t>(k) * m];
  }
  part[pl][rl] = s;
  __syncthreads();
  if (pl != 0 || i >= m) return;
  T sum = part[0][rl];
#pragma unroll
  for (int q = 1; q < kZeroLanes; ++q) sum += part[q][rl];
  if constexpr (FREE) {
    static_assert(TALL && std::is_void<Fn>::value, "free x: the tall form, no term on this side");
    I.zq[i] = I.w[i];         // the boundary iterate: x as the pass of this sweep read it
    I.r[i] = I.pkappa * sum;  // f_x = -L(x, arg) f_arg: no v_x (block.cc Substitute / the GEMV epilogue)
    return;
  }
  FusedScalarsT<T> ci = c;
  if (c.alpha_v != nullptr) ci.alpha = c.alpha_v[i];
  if (c.beta_v != nullptr) ci.beta = c.beta_v[i];
  const T gi = I.g != nullptr ? I.g[i] : T(0);
  const T yzi = I.yz[i], yqi = I.yq[i];
  T ns, nq, nys, nyq, nu, vn;
  if constexpr (TALL) {
    nq = nyq = I.w[i];
    vn = ZeroTallColsChainT<T, Fn>(nq, ci, gi, I.u[i], yzi, yqi, &ns, &nys, &nu);
  } else if constexpr (std::is_void<Fn>::value || std::is_same<Fn, NonNegStep>::value) {
    vn = ZeroChainT<T, Fn>(I.w[i], ci, gi, I.u[i], yzi, yqi, &ns, &nq, &nys, &nyq, &nu);
  } else {
    // ZeroChainT from the carried head on: q = kappa d + v, y_q = q, u -= y_q
    ns = I.hs[i];
    nys = I.hys[i];
    const T v = I.hv[i];
    nq = nyq = c.kappa * I.w[i] + v;
    nu = v - nq;
    const ZeroHeadT<T> hn = ZeroHeadOfT<T, Fn>(ci, gi, nu, nys, nq, I.lam64);
    I.hs[i] = hn.s;
    I.hys[i] = hn.ys;
    I.hv[i] = vn = hn.v;
  }
  I.yzprev[i] = yzi;
  I.yqprev[i] = yqi;
  I.z[i] = ns;
  I.zq[i] = nq;
  I.yz[i] = nys;
  I.yq[i] = nyq;
  I.u[i] = nu;
  if constexpr (TALL) {
    I.r[i] = I.pkappa * sum + vn;  // f_x = v_x - L(x', arg) f_arg
    return;
  }
  // forward substitution of the next sweep: (rhs - e v_z) first, then the product with x' on top
  const T base = c.kappa * vn + (I.rhs != nullptr ? I.rhs[i] : T(0));
  I.r[i] = I.pkappa * sum + base;
}

template <class T, int ROWS, class Fn, bool TALL = false>
__global__ __launch_bounds__(ROWS * kZeroLanes) void ZeroFusedRowsKernel(int64_t m, int nparts, ZeroRowsInst<T> I) {
  ZeroRowsBody<T, ROWS, Fn, TALL>(m, nparts, I, blockIdx.x);
}
// Free x (tag "zero_tall_free_cols"): the body's FREE form, 16 entries of x per workgroup.
template <class T>
__global__ __launch_bounds__(kZeroRows * kZeroLanes) void ZeroFreeColsKernel(int64_t m, int nparts, ZeroRowsInst<T> I) {
  ZeroRowsBody<T, kZeroRows, void, true, true>(m, nparts, I, blockIdx.x);
}

// The members of a batch: grid row b is member b's single launch, workgroup for workgroup.  A
// workgroup touches its own member's rows alone; nothing waits on another workgroup.
// TALL (tag "batch_zero_tall_cols"): grid row b is member b's "zero_tall_cols" launch.
template <class T, int ROWS, class Fn, bool TALL = false>
__global__ __launch_bounds__(ROWS * kZeroLanes) void ZeroFusedRowsBatchKernel(
    int64_t m, int nparts, const ZeroRowsInst<T>* __restrict__ tab) {
  const ZeroRowsInst<T> I = tab[blockIdx.y];
  ZeroRowsBody<T, ROWS, Fn, TALL>(m, nparts, I, blockIdx.x);
}
// Free x (tag "batch_zero_tall_free_cols"): grid row b is member b's "zero_tall_free_cols" launch.
template <class T>
__global__ __launch_bounds__(kZeroRows * kZeroLanes) void ZeroFreeColsBatchKernel(
    int64_t m, int nparts, const ZeroRowsInst<T>* __restrict__ tab) {
  const ZeroRowsInst<T> I = tab[blockIdx.y];
  ZeroRowsBody<T, kZeroRows, void, true, true>(m, nparts, I, blockIdx.x);
}

// The first head of a smooth z term from the adopted boundary state, a thread per row.
template <class T, class Fn>
__global__ __launch_bounds__(kBlock) void ZeroSmoothHeadKernel(
    int64_t m, FusedScalarsT<T> c, double lam64, const T* __restrict__ g, const T* __restrict__ u,
    const T* __restrict__ yz, const T* __restrict__ yq, T* __restrict__ hs, T* __restrict__ hys,
    T* __restrict__ hv) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= m) return;
  const ZeroHeadT<T> h = ZeroHeadOfT<T, Fn>(c, g != nullptr ? g[i] : T(0), u[i], yz[i], yq[i], lam64);
  hs[i] = h.s;
  hys[i] = h.ys;
  hv[i] = h.v;
}

template <class T> ZeroRowsInst<T> RowsInstOf(const ZeroRowsArgs& a) {
  if (a.side == kRowsXFree) {  // no state and no term: the partials, w, x (in the copy's place), r and pkappa
    ZeroRowsInst<T> f = {};
    f.tpart = a.tpart.as<T>();
    f.w = a.w.as<T>();
    f.zq = a.xcur.as<T>();
    f.r = a.r.as<T>();
    f.pkappa = static_cast<T>(a.pkappa);
    return f;
  }
  ZeroRowsInst<T> d;
  d.tpart = a.tpart.as<T>();
  d.w = a.w.as<T>();
  d.rhs = OptT<T>(a.rhs);
  d.g = OptT<T>(a.g);
  NarrowState<T>(a.state, &d.u, &d.z, &d.zq, &d.yz, &d.yq, &d.yzprev, &d.yqprev);
  d.r = a.r.as<T>();
  const bool smooth = a.zone.head == kHeadSmooth;
  d.hs = smooth ? a.hs.as<T>() : nullptr;
  d.hys = smooth ? a.hys.as<T>() : nullptr;
  d.hv = smooth ? a.hv.as<T>() : nullptr;
  d.c = ScalarsOf<T>(a.zone, -a.e, 1, 1);
  d.pkappa = static_cast<T>(a.pkappa);
  d.lam64 = a.zone.lam;
  return d;
}

// The single and the batched kernel of (side, head) - null where ZeroRowsExist, BatchRowsExist list
// none; the callers have checked - and the rows of their workgroups (the smooth head: a whole wave).
template <class T> struct RowsForm {
  void (*single)(int64_t, int, ZeroRowsInst<T>);
  void (*batch)(int64_t, int, const ZeroRowsInst<T>*);
  int rows;
};
template <class T> RowsForm<T> RowsFormOf(RowsSide side, Head h) {
  if (side == kRowsXFree) return {ZeroFreeColsKernel<T>, ZeroFreeColsBatchKernel<T>, kZeroRows};
  RowsForm<T> f = {nullptr, nullptr, h == kHeadSmooth ? kZeroSmoothRows : kZeroRows};
  WithHead(h, [&](auto head) {
    typedef typename decltype(head)::type Fn;
    auto pick = [&](auto tall) {
      constexpr bool kTall = decltype(tall)::value;
      constexpr RowsSide kSide = kTall ? kRowsX : kRowsZ;
      constexpr int kRows = HeadOf<Fn>() == kHeadSmooth ? kZeroSmoothRows : kZeroRows;
      if constexpr (ZeroRowsExist(kSide, HeadOf<Fn>())) f.single = ZeroFusedRowsKernel<T, kRows, Fn, kTall>;
      if constexpr (BatchRowsExist(kSide, HeadOf<Fn>())) f.batch = ZeroFusedRowsBatchKernel<T, kRows, Fn, kTall>;
    };
    if (side == kRowsX) pick(std::true_type());
    else pick(std::false_type());
  });
  return f;
}

template <class T> void LaunchZeroRows(const ZeroRowsArgs& a) {
  const RowsForm<T> f = RowsFormOf<T>(a.side, a.zone.head);
  EPS_CHECK(f.single != nullptr);
  hipLaunchKernelGGL(f.single, dim3(static_cast<unsigned>((a.m + f.rows - 1) / f.rows)), dim3(f.rows * kZeroLanes), 0,
                     Runtime::Get().stream(), a.m, a.nparts, RowsInstOf<T>(a));
}
template <class T>
void LaunchZeroRowsBatch(int64_t m, int nparts, RowsSide side, Head head, const DVec& table, int count) {
  const RowsForm<T> f = RowsFormOf<T>(side, head);
  EPS_CHECK(f.batch != nullptr);
  hipLaunchKernelGGL(f.batch, dim3(static_cast<unsigned>((m + f.rows - 1) / f.rows), static_cast<unsigned>(count)),
                     dim3(f.rows * kZeroLanes), 0, Runtime::Get().stream(), m, nparts,
                     reinterpret_cast<const ZeroRowsInst<T>*>(table.as<char>()));
}

template <class T>
void UploadRowsT(const std::vector<const ZeroRowsArgs*>& members, DVec* table) {
  std::vector<ZeroRowsInst<T>> host;
  host.reserve(members.size());
  for (const ZeroRowsArgs* a : members) host.push_back(RowsInstOf<T>(*a));
  UploadRecords(host, table);
}

template <class T>
void LaunchZeroSmoothHead(const ZeroRowsArgs& a) {
  const ZeroRowsInst<T> I = RowsInstOf<T>(a);
  hipLaunchKernelGGL((ZeroSmoothHeadKernel<T, FnLogistic>), dim3(static_cast<unsigned>((a.m + kBlock - 1) / kBlock)),
                     dim3(kBlock), 0, Runtime::Get().stream(), a.m, I.c, I.lam64, I.g, I.u, I.yz, I.yq, I.hs, I.hys,
                     I.hv);
}

// Every array of a constraint's state has n entries of type dt (`zero_prev`: y_zero_prev too).
void CheckState(const ConsensusState& s, int64_t n, DType dt, bool zero_prev = true) {
  for (const DVec* v : {&s.u, &s.var, &s.copy, &s.y_term, &s.y_zero, &s.y_term_prev})
    EPS_CHECK(v->n == n && v->dt == dt);
  if (zero_prev) EPS_CHECK(s.y_zero_prev.n == n && s.y_zero_prev.dt == dt);
}

// `exists`: ZeroRowsExist or BatchRowsExist (`what`: "" or "batched ") of (side, head).
void CheckRowsForm(bool exists, const char* what, RowsSide side, Head head) {
  EPS_CHECK_MSG(exists, "the " << what << "ZERO-term rows have no " << kHeadNames[head] << " head on the "
                               << kRowsSideNames[side] << " side");
}

void CheckZeroRows(const ZeroRowsArgs& a) {
  const DType dt = a.w.dt;
  EPS_CHECK(a.m >= 1 && a.nparts >= 1 && a.tpart.dt == dt && a.tpart.n >= static_cast<int64_t>(a.nparts) * a.m);
  EPS_CHECK(a.w.n == a.m && a.r.n == a.m && a.r.dt == dt);
  const Head head = a.zone.head;
  CheckRowsForm(ZeroRowsExist(a.side, head), "", a.side, head);
  if (a.side == kRowsXFree) {  // x alone in the state's place; no term, so nothing else of the record is read
    EPS_CHECK(a.xcur.n == a.m && a.xcur.dt == dt);
    return;
  }
  CheckState(a.state, a.m, dt);
  for (const DVec* v : {&a.rhs, &a.g, &a.zone.alpha_vec, &a.zone.beta_vec})
    if (v->n > 0) EPS_CHECK(v->n == a.m && v->dt == dt);
  EPS_CHECK_MSG(head != kHeadLinear || a.g.n == a.m, "a linear term carries its vector g, one value per entry of x");
  if (head != kHeadSmooth) return;
  EPS_CHECK_MSG(a.fn == SMOOTH_LOGISTIC, "the fused ZERO-term rows take SUM_LOGISTIC alone, got " << a.fn);
  for (const DVec* v : {&a.hs, &a.hys, &a.hv}) EPS_CHECK(v->n == a.m && v->dt == dt);
}

const char* RowsTag(RowsSide side, bool batched) {
  if (side == kRowsXFree) return batched ? "batch_zero_tall_free_cols" : "zero_tall_free_cols";
  if (side == kRowsX) return batched ? "batch_zero_tall_cols" : "zero_tall_cols";
  return batched ? "batch_zero_rows" : "zero_fused_rows";
}

}  // namespace

void ZeroFusedRows(const ZeroRowsArgs& a) {
  CheckZeroRows(a);
  ProfScope prof(RowsTag(a.side, false), a.m, a.nparts);
  if (a.w.dt == F32) LaunchZeroRows<float>(a);
  else LaunchZeroRows<double>(a);
  EPS_HIP(hipGetLastError());
}

namespace {

void CheckZeroTallSamples(const ZeroTallSamplesArgs& a) {
  const DType dt = a.d.dt;
  EPS_CHECK(a.m >= 1);
  for (const DVec* v : {&a.d, &a.farg, &a.hs, &a.hys, &a.hv}) EPS_CHECK(v->n == a.m && v->dt == dt);
  CheckState(a.state, a.m, dt);
  for (const DVec* v : {&a.rhs, &a.g})
    if (v->n > 0) EPS_CHECK(v->n == a.m && v->dt == dt);
  EPS_CHECK_MSG(a.fn == SMOOTH_LOGISTIC, "the tall ZERO-term sample side takes SUM_LOGISTIC alone, got " << a.fn);
}

template <class T> ZeroTallSamplesInst<T> SamplesInstOf(const ZeroTallSamplesArgs& a) {
  ZeroTallSamplesInst<T> d = {ScalarsOf<T>(a.zone, a.kappa, 1, 1), a.zone.lam, static_cast<T>(a.ke),
                              static_cast<T>(a.dinv), OptT<T>(a.g), OptT<T>(a.rhs), a.d.as<T>()};
  d.c.alpha = d.c.beta = T(1);  // the smooth term has no zone, whatever the description holds
  d.c.M = T(0);
  d.c.alpha_v = d.c.beta_v = nullptr;
  NarrowState<T>(a.state, &d.u, &d.z, &d.zq, &d.yz, &d.yq, &d.yzprev, &d.yqprev);
  d.hs = a.hs.as<T>();
  d.hys = a.hys.as<T>();
  d.hv = a.hv.as<T>();
  d.farg = a.farg.as<T>();
  return d;
}

template <class T>
void LaunchZeroTallSamples(const ZeroTallSamplesArgs& a, bool head_only) {
  const dim3 grid(static_cast<unsigned>((a.m + kBlock - 1) / kBlock));
  const ZeroTallSamplesInst<T> I = SamplesInstOf<T>(a);
  if (head_only)
    hipLaunchKernelGGL((ZeroSmoothHeadKernel<T, FnLogistic>), grid, dim3(kBlock), 0, Runtime::Get().stream(), a.m,
                       I.c, I.lam64, I.g, I.u, I.yz, I.yq, I.hs, I.hys, I.hv);
  else
    hipLaunchKernelGGL((ZeroTallSamplesKernel<T, FnLogistic>), grid, dim3(kBlock), 0, Runtime::Get().stream(), a.m, I);
}

template <class T>
void UploadSamplesT(const std::vector<const ZeroTallSamplesArgs*>& members, DVec* table) {
  std::vector<ZeroTallSamplesInst<T>> host;
  host.reserve(members.size());
  for (const ZeroTallSamplesArgs* a : members) host.push_back(SamplesInstOf<T>(*a));
  UploadRecords(host, table);
}

template <class T>
void LaunchZeroTallSamplesBatch(int64_t m, const DVec& table, int count) {
  hipLaunchKernelGGL((ZeroTallSamplesBatchKernel<T, FnLogistic>),
                     dim3(static_cast<unsigned>((m + kBlock - 1) / kBlock), static_cast<unsigned>(count)),
                     dim3(kBlock), 0, Runtime::Get().stream(), m,
                     reinterpret_cast<const ZeroTallSamplesInst<T>*>(table.as<char>()));
}

}  // namespace

void ZeroTallSamples(const ZeroTallSamplesArgs& a) {
  CheckZeroTallSamples(a);
  ProfScope prof("zero_tall_samples", a.m);
  if (a.d.dt == F32) LaunchZeroTallSamples<float>(a, false);
  else LaunchZeroTallSamples<double>(a, false);
  EPS_HIP(hipGetLastError());
}

void ZeroTallSamplesHead(const ZeroTallSamplesArgs& a) {
  CheckZeroTallSamples(a);
  ProfScope prof("zero_tall_head", a.m);
  if (a.d.dt == F32) LaunchZeroTallSamples<float>(a, true);
  else LaunchZeroTallSamples<double>(a, true);
  EPS_HIP(hipGetLastError());
}

void ZeroRowsBatchUpload(const std::vector<const ZeroRowsArgs*>& members, DVec* table) {
  EPS_CHECK(!members.empty());
  const ZeroRowsArgs& lead = *members[0];
  for (const ZeroRowsArgs* a : members) {
    CheckZeroRows(*a);
    EPS_CHECK(a->m == lead.m && a->nparts == lead.nparts && a->w.dt == lead.w.dt);
    EPS_CHECK(a->side == lead.side && a->zone.head == lead.zone.head);
    CheckRowsForm(BatchRowsExist(a->side, a->zone.head), "batched ", a->side, a->zone.head);
  }
  if (lead.w.dt == F32) UploadRowsT<float>(members, table);
  else UploadRowsT<double>(members, table);
}

void ZeroFusedRowsBatch(int64_t m, int nparts, RowsSide side, Head head, DType dt, const DVec& table, int count) {
  const int64_t record = dt == F32 ? sizeof(ZeroRowsInst<float>) : sizeof(ZeroRowsInst<double>);
  EPS_CHECK(m >= 1 && nparts >= 1 && count >= 1 && count <= 65535);
  EPS_CHECK(table.dt == F64 && table.n * 8 >= count * record);
  CheckRowsForm(BatchRowsExist(side, head), "batched ", side, head);
  ProfScope prof(RowsTag(side, true), m, count);
  if (dt == F32) LaunchZeroRowsBatch<float>(m, nparts, side, head, table, count);
  else LaunchZeroRowsBatch<double>(m, nparts, side, head, table, count);
  EPS_HIP(hipGetLastError());
}

void ZeroTallSamplesBatchUpload(const std::vector<const ZeroTallSamplesArgs*>& members, DVec* table) {
  EPS_CHECK(!members.empty());
  const ZeroTallSamplesArgs& lead = *members[0];
  for (const ZeroTallSamplesArgs* a : members) {
    CheckZeroTallSamples(*a);
    EPS_CHECK(a->m == lead.m && a->d.dt == lead.d.dt);
  }
  if (lead.d.dt == F32) UploadSamplesT<float>(members, table);
  else UploadSamplesT<double>(members, table);
}

void ZeroTallSamplesBatch(int64_t m, DType dt, const DVec& table, int count) {
  const int64_t record = dt == F32 ? sizeof(ZeroTallSamplesInst<float>) : sizeof(ZeroTallSamplesInst<double>);
  EPS_CHECK(m >= 1 && count >= 1 && count <= 65535);
  EPS_CHECK(table.dt == F64 && table.n * 8 >= count * record);
  ProfScope prof("batch_zero_tall_samples", m, count);
  if (dt == F32) LaunchZeroTallSamplesBatch<float>(m, table, count);
  else LaunchZeroTallSamplesBatch<double>(m, table, count);
  EPS_HIP(hipGetLastError());
}

void ZeroSmoothHead(const ZeroRowsArgs& a) {
  EPS_CHECK(a.zone.head == kHeadSmooth);
  CheckZeroRows(a);
  ProfScope prof("zero_fused_head", a.m);
  if (a.w.dt == F32) LaunchZeroSmoothHead<float>(a);
  else LaunchZeroSmoothHead<double>(a);
  EPS_HIP(hipGetLastError());
}

namespace {

// The five sums of squares of a residual check of the fused structure in ONE launch (the generic
// path takes ~10 launches and three temporaries for them): ||y0||^2, ||y1||^2, ||y0 + y1||^2,
// ||y1 - y1prev||^2, ||u||^2, accumulated in double.  Every workgroup reduces a contiguous part
// and publishes five partials; the workgroup whose ticket comes last adds the partials in
// workgroup order - deterministic, one launch.  (Hand-off: sc1 stores, every storing wave drained,
// one agent-scope ticket per workgroup; the last arriver reads with sc1 loads - MI355X_MICROARCH.md,
// Valid forms, first row.)
constexpr int kNormBlocks = 64;

template <class T>
__global__ __launch_bounds__(kBlock) void LassoFusedNormsKernel(
    int64_t n, const T* __restrict__ u, const T* __restrict__ y0, const T* __restrict__ y1,
    const T* __restrict__ y1prev, double* partial, unsigned* ticket, double* out,
    const unsigned* peer_err) {
  __shared__ double red[kBlock / 64][5];
  __shared__ bool last;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = blockIdx.x * per;
  int64_t hi = lo + per;
  if (hi > n) hi = n;
  double s[5] = {0, 0, 0, 0, 0};
  for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
    const double a = y0[i], b = y1[i], c = y1prev[i], d = u[i];
    s[0] += a * a;
    s[1] += b * b;
    s[2] += (a + b) * (a + b);
    s[3] += (b - c) * (b - c);
    s[4] += d * d;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double t = WaveSumT<double>(s[k]);
    if (lane == 0) red[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    const double t = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    __hip_atomic_store(partial + blockIdx.x * 5 + k, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    double t = 0;
    for (unsigned b = 0; b < gridDim.x; ++b)
      t += __hip_atomic_load(partial + b * 5 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    out[k] = t;
  }
  // sixth value: "an exchange kernel of this rank timed out" - it travels with the norms through
  // the all-reduce of the check, so every rank learns of a failure on ANY rank at the same check
  if (threadIdx.x == 5)
    out[5] = (peer_err != nullptr &&
              __hip_atomic_load(peer_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ? 1.0 : 0.0;
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

void LassoFusedNorms(const DVec& u, const DVec& y0, const DVec& y1, const DVec& y1prev, double* out6,
                     const DVec& work, const unsigned* peer_err, const char* tag) {
  const int64_t n = u.n;
  EPS_CHECK(y0.n == n && y1.n == n && y1prev.n == n && y0.dt == u.dt && y1.dt == u.dt && y1prev.dt == u.dt);
  EPS_CHECK(work.dt == F64 && work.n >= kNormBlocks * 5 + 1);
  int64_t grid = (n + 4 * kBlock - 1) / (4 * kBlock);
  if (grid > kNormBlocks) grid = kNormBlocks;
  if (grid < 1) grid = 1;
  double* partial = work.as<double>();
  unsigned* ticket = reinterpret_cast<unsigned*>(partial + kNormBlocks * 5);  // zero between launches
  ProfScope prof(tag, n);
  if (u.dt == F32)
    hipLaunchKernelGGL(LassoFusedNormsKernel<float>, dim3(static_cast<unsigned>(grid)), dim3(kBlock), 0,
                       Runtime::Get().stream(), n, u.as<float>(), y0.as<float>(), y1.as<float>(),
                       y1prev.as<float>(), partial, ticket, out6, peer_err);
  else
    hipLaunchKernelGGL(LassoFusedNormsKernel<double>, dim3(static_cast<unsigned>(grid)), dim3(kBlock), 0,
                       Runtime::Get().stream(), n, u.as<double>(), y0.as<double>(), y1.as<double>(),
                       y1prev.as<double>(), partial, ticket, out6, peer_err);
  EPS_HIP(hipGetLastError());
}

namespace {

// The residual check of a ZERO-term route in ONE launch: the five sums of squares ||y_term||^2,
// ||y_zero||^2, ||y_term + y_zero||^2, ||y_zero - y_zero_prev||^2, ||u||^2 of the x constraint's
// rows and of the z constraint's, accumulated in double from the state's own type.  Workgroups
// [0, gx) reduce contiguous parts of the x side, [gx, gridDim.x) of the z side (a side that is
// absent has none); each publishes ten partials, the five of the other side zero, and the
// workgroup whose ticket comes last adds them in workgroup order.  The hand-off is
// LassoFusedNormsKernel's as it stands.
static_assert(kZeroNormsWork == kNormBlocks * 10 + 1, "ten partials per workgroup and the ticket");
template <class T> struct ZeroNormsSideT {
  int64_t len;
  const T *u, *y_term, *y_zero, *y_zero_prev;
};

template <class T>
__global__ __launch_bounds__(kBlock) void ZeroFusedNormsKernel(ZeroNormsSideT<T> sx, ZeroNormsSideT<T> sz,
                                                               unsigned gx, double* partial, unsigned* ticket,
                                                               double* out) {
  __shared__ double red[kBlock / 64][5];
  __shared__ bool last;
  const bool on_x = blockIdx.x < gx;  // uniform over the workgroup
  const ZeroNormsSideT<T> side = on_x ? sx : sz;
  const int64_t parts = on_x ? gx : gridDim.x - gx, part = on_x ? blockIdx.x : blockIdx.x - gx;
  const int64_t per = (side.len + parts - 1) / parts;
  const int64_t lo = part * per;
  int64_t hi = lo + per;
  if (hi > side.len) hi = side.len;
  double s[5] = {0, 0, 0, 0, 0};
  for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
    const double a = side.y_term[i], b = side.y_zero[i], c = side.y_zero_prev[i], d = side.u[i];
    s[0] += a * a;
    s[1] += b * b;
    s[2] += (a + b) * (a + b);
    s[3] += (b - c) * (b - c);
    s[4] += d * d;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double t = WaveSumT<double>(s[k]);
    if (lane == 0) red[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const int k = threadIdx.x % 5;
    const bool mine = (threadIdx.x < 5) == on_x;  // slots 0-4: the x side's, 5-9: the z side's
    const double t = mine ? ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k] : 0.0;
    __hip_atomic_store(partial + blockIdx.x * 10 + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x < 10) {
    const int k = threadIdx.x;
    double t = 0;
    for (unsigned b = 0; b < gridDim.x; ++b)
      t += __hip_atomic_load(partial + b * 10 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    out[k] = t;
  }
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A side of the check from the route's state; absent (len 0) when the state is empty.
template <class T> ZeroNormsSideT<T> NormsSideOf(const ConsensusState& s) {
  return {s.u.n, OptT<T>(s.u), OptT<T>(s.y_term), OptT<T>(s.y_zero), OptT<T>(s.y_zero_prev)};
}

template <class T>
void LaunchZeroFusedNorms(const ConsensusState& x, const ConsensusState& z, unsigned gx, unsigned gz, double* partial,
                          unsigned* ticket, double* out10) {
  hipLaunchKernelGGL(ZeroFusedNormsKernel<T>, dim3(gx + gz), dim3(kBlock), 0, Runtime::Get().stream(),
                     NormsSideOf<T>(x), NormsSideOf<T>(z), gx, partial, ticket, out10);
}

}  // namespace

void ZeroFusedNormsGrid(int64_t nx, int64_t nz, int* gx, int* gz) {
  auto want = [](int64_t len) { return (len + 4 * kBlock - 1) / (4 * kBlock); };
  int64_t a = want(nx), b = want(nz);
  if (a + b > kNormBlocks) {
    // in proportion to the lengths, rounded to nearest, a side that is present keeping one
    a = (kNormBlocks * nx + (nx + nz) / 2) / (nx + nz);
    if (a < 1 && nx > 0) a = 1;
    if (a > kNormBlocks - 1 && nz > 0) a = kNormBlocks - 1;
    b = kNormBlocks - a;
  }
  *gx = static_cast<int>(a);
  *gz = static_cast<int>(b);
}

void ZeroFusedNorms(const ConsensusState& x, const ConsensusState& z, double* out10, const DVec& work,
                    const char* tag) {
  const int64_t nx = x.u.n, nz = z.u.n;
  EPS_CHECK_MSG(nx > 0 || nz > 0, "the ZERO-term check needs a side");
  const DType dt = nx > 0 ? x.u.dt : z.u.dt;
  for (const ConsensusState* s : {&x, &z})
    for (const DVec* v : {&s->u, &s->y_term, &s->y_zero, &s->y_zero_prev})
      EPS_CHECK(v->n == s->u.n && (v->n == 0 || v->dt == dt));
  EPS_CHECK(out10 != nullptr && work.dt == F64 && work.n >= kZeroNormsWork);
  int gx = 0, gz = 0;
  ZeroFusedNormsGrid(nx, nz, &gx, &gz);
  EPS_CHECK(gx + gz >= 1 && gx + gz <= kNormBlocks && (gx > 0) == (nx > 0) && (gz > 0) == (nz > 0));
  double* partial = work.as<double>();
  unsigned* ticket = reinterpret_cast<unsigned*>(partial + kNormBlocks * 10);  // zero between launches
  ProfScope prof(tag, nx, nz);
  if (dt == F32)
    LaunchZeroFusedNorms<float>(x, z, static_cast<unsigned>(gx), static_cast<unsigned>(gz), partial, ticket, out10);
  else
    LaunchZeroFusedNorms<double>(x, z, static_cast<unsigned>(gx), static_cast<unsigned>(gz), partial, ticket, out10);
  EPS_HIP(hipGetLastError());
}

bool LassoFusedSupported(int64_t m, int64_t n, const DVec& A, int64_t lda) {
  if (n < 1 || reinterpret_cast<uintptr_t>(A.data()) % 16 != 0) return false;
  if (A.dt == F32) return m >= 4 && m % 4 == 0 && lda % 4 == 0 && m <= 20 * 1024;
  return m >= 2 && m % 2 == 0 && lda % 2 == 0 && m <= 10 * 1024;  // f64: two rows per 16-byte load
}

// Threads per workgroup of the pass: 512 when the rows do not fit 256 threads (m > 10240).
// Measured on MI355X for m = 1e4 (EPSILON_HIP_FUSED_BLOCK=512 forces the wide form): one 512-thread
// workgroup per CU is SLOWER than two of 256 (61.9 vs 48.4 us on a 6272-column slab, 413 vs 310 us
// on 5e4 columns - one column in flight per CU instead of two), two per CU are equal; the halved
// number of partial vectors does not pay either, the reduce-exchange kernel behind the pass is
// latency-bound (11.5 us at 242 partials, 12.5 at 448).
int LassoFusedBlock(int64_t m, int64_t n, DType dt) {
  (void)n;
  if (dt == F64) return m > 5 * 1024 ? 512 : 256;
  if (m > 10 * 1024) return 512;
  static const int block = opt::Int(opt::kFusedBlock, 0);
  if (block == 512 && m >= 2048) return 512;
  return 256;
}

int LassoFusedGrid(int64_t m, int64_t n, DType dt) {
  int64_t npairs = (n + 1) / 2;
  // two 256-thread workgroups per CU; the 512-thread form with up to 5 row chunks per thread
  // (m <= 10240 in f32) also fits twice, above that once
  const int64_t rows_per_chunk = dt == F32 ? 4 : 2;
  const bool one_per_cu = LassoFusedBlock(m, n, dt) == 512 && m > 512 * 5 * rows_per_chunk;
  int64_t g = one_per_cu ? 256 : 512;
  static const int grid = opt::Int(opt::kFusedGrid, 0);  // tuning knob
  if (grid > 0) g = grid;
  if (g > npairs) g = npairs;
  if (g < 1) g = 1;
  // equal shares: with `per` column pairs per workgroup, ceil(npairs / per) workgroups leave no
  // workgroup a pair short (a 6272-column slab on 512 workgroups is 6 or 7 pairs each - the
  // launch then lasts as long as the 7s; on 448 workgroups every one has 7)
  const int64_t per = (npairs + g - 1) / g;
  g = (npairs + per - 1) / per;
  return static_cast<int>(g < 1 ? 1 : g);
}

FusedResidency LassoFusedResidency(int64_t m, int64_t n, DType dt, int64_t budget) {
  FusedResidency r;
  if (budget <= 0 || m < 1 || n < 1) return r;
  const int64_t elem = dt == F32 ? 4 : 8;
  const int64_t chunk_rows = static_cast<int64_t>(LassoFusedBlock(m, n, dt)) * (16 / elem);
  const int64_t nchunks = (m + chunk_rows - 1) / chunk_rows;
  // whole chunks of every column while they fit, then the next chunk of as many columns as fit
  // (the last chunk of a column may be partly filled: it costs its own bytes)
  for (int64_t q = 0; q < nchunks; ++q) {
    const int64_t piece = std::min(chunk_rows, m - q * chunk_rows) * elem;
    const int64_t left = budget - r.bytes;
    if (left / piece >= n) {
      r.bytes += piece * n;
      r.qfull = static_cast<int>(q + 1);
      continue;
    }
    r.jcut = left / piece;
    r.bytes += piece * r.jcut;
    break;
  }
  return r;
}

namespace {
FusedResidency g_last_residency;
}
FusedResidency LastFusedResidency() { return g_last_residency; }
void NoteFusedResidency(int qfull, int64_t jcut) {
  g_last_residency.qfull = qfull;
  g_last_residency.jcut = jcut;
}

void LassoFusedPass(const LassoFusedArgs& a) {
  EPS_CHECK(LassoFusedSupported(a.m, a.n, a.A, a.lda));
  EPS_CHECK(a.qfull >= 0 && a.jcut >= 0 && a.jcut <= a.n);
  const DType dt = a.A.dt;
  const LassoInstance& s = a.inst;
  EPS_CHECK(s.w.n == a.m && s.w.dt == dt);
  EPS_CHECK(a.chain >= kChainLasso && a.chain <= kChainZeroTallAcc);
  CheckState(s.state, a.n, dt, /*zero_prev=*/ChainKeepsZeroPrev(a.chain));
  for (const DVec* v : {&s.zone.alpha_vec, &s.zone.beta_vec})
    if (v->n > 0) EPS_CHECK(v->n == a.n && v->dt == dt);
  if (a.chain == kChainTwoBlock) EPS_CHECK(a.e1.n == a.n && a.e1.dt == dt);
  const Head head = s.zone.head;
  EPS_CHECK_MSG(head != kHeadLinear || (s.zg.n == a.n && s.zg.dt == dt),
                "a linear term carries its vector g, one value per column");
  if (a.chain == kChainZeroTallDot) EPS_CHECK(s.zd.n == a.n && s.zd.dt == dt);
  if (a.chain == kChainZeroTallAcc) EPS_CHECK(s.zfarg.n == a.n && s.zfarg.dt == dt);
  if (a.chain == kChainZeroTall)
    for (const DVec* v : {&s.zg, &s.zrhs})
      if (v->n > 0) EPS_CHECK(v->n == a.n && v->dt == dt);
  const int grid = LassoFusedGrid(a.m, a.n, dt);
  const int block = LassoFusedBlock(a.m, a.n, dt);
  EPS_CHECK(s.tpart.n >= static_cast<int64_t>(grid) * a.m && s.tpart.dt == dt);
  EPS_CHECK(reinterpret_cast<uintptr_t>(s.w.data()) % 16 == 0 &&
            reinterpret_cast<uintptr_t>(s.tpart.data()) % 16 == 0);
  const char* tag = kChainTags[a.chain][0];
  EPS_CHECK_MSG(FusedPassExists(a.chain, head, block),
                "the fused pass \"" << tag << "\" has no " << kHeadNames[head] << " head with " << block << " threads");
  ProfScope prof(tag, a.m, a.n);
  NoteFusedResidency(a.qfull, a.jcut);
  if (dt == F32) LaunchFusedT<float>(a, grid, block);
  else LaunchFusedT<double>(a, grid, block);
  EPS_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace eps
