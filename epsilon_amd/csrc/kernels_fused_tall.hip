// The tall lasso sweep: "least squares + separable threshold" with more rows than
// columns.  The block LDL^T of the least-squares prox then ends in the dense n x n pivot of the
// variable, and with v the prox input
//
//     Solve(b_ + v)[var] = Dinv(var) (v_c - c),   c = L(var, arg) rhs_arg,
//
// where c does not depend on the iterate (block.cc Substitute; the back substitution's products
// with L(var, arg)^T land on rows that Apply drops).  A sweep is the apply of the cached inverse to
// r = v0 - c and, per entry, the lasso chain from x0 on; no pass over the data matrix.
//
// This file holds the element-wise side.  From n = 1024 the apply's tile launch (SymvTileKernel<T,
// true>, kernels_gemv.hip) leaves per-tile partials and the kernel here sums its block's in
// SymvReduceBody's order (kernels_symv_reduce.h), so x0 is bit for bit what SymvPacked writes;
// below, it reads the finished vector.  The chain repeats the reference's operations one by one,
// one rounding each (compiled with -ffp-contract=off), in the expressions of kernels_fused_chain.h.
// A thread touches its own entry alone apart from the one __syncthreads of the half sums: no
// atomics, no waits on other workgroups, no scratch.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kernels_fused_chain.h"
#include "kernels_symv_reduce.h"

namespace eps {
namespace k {

namespace {

constexpr int kBlock = 256;
static_assert(kBlock == 2 * kSB, "SymvBlockSum's geometry: two half-workgroups per block of kSB entries");

// Block `I` (kSB entries) of one instance.  prow: the tile partials (FROM_PARTIALS), pcol behind
// them at ntiles * kSB.
template <class T, bool FROM_PARTIALS>
__device__ inline void LassoTallColsBody(int64_t n, int64_t nb, const LassoBatchInst<T>& s, const T* prow,
                                         int64_t I) {
  const int64_t j = I * kSB + (threadIdx.x & (kSB - 1));
  T x0j = T(0);
  bool mine;
  if constexpr (FROM_PARTIALS) {
    T tot;
    mine = SymvBlockSum<T>(nb, prow, prow + nb * (nb + 1) / 2 * kSB, I, &tot);
    if (mine) x0j = s.kappa * tot;  // SymvReduceBody with beta == 0: alpha * tot
  } else {
    mine = threadIdx.x < kSB;
    if (mine && j < n) x0j = s.w[j];
  }
  if (!mine || j >= n) return;
  FusedScalarsT<T> c;
  c.kappa = T(0);  // (x0 is given: ChainHeadFromT)
  c.Bs = s.Bs, c.Cs = s.Cs, c.a1 = s.a1, c.lam = s.lam, c.M = s.M;
  c.alpha = s.alpha_v != nullptr ? s.alpha_v[j] : s.alpha;
  c.beta = s.beta_v != nullptr ? s.beta_v[j] : s.beta;
  c.a0 = c.inv_aa = T(0);
  c.alpha_v = c.beta_v = nullptr;
  const T uj = s.u[j], y0j = s.y0[j], y1j = s.y1[j];
  const ChainHeadT<T> h = ChainHeadFromT<T>(ChainStartT<T>(uj, y0j, y1j), x0j, c, y1j);
  const T xz = ScaledZoneOneT<T>(h.vin, c.lam, c.alpha, c.beta, c.M);
  T nx0, nx1, ny0, ny1, nu;
  const T v0n = ChainTailT<T>(h, xz, c, &nx0, &nx1, &ny0, &ny1, &nu);
  s.y1prev[j] = y1j;
  s.x0[j] = nx0;
  s.x1[j] = nx1;
  s.y0[j] = ny0;
  s.y1[j] = ny1;
  s.u[j] = nu;
  // forward substitution of the next sweep: b_var = v_c - L(var, arg) b_arg
  s.p[j] = s.rhs != nullptr ? v0n - s.rhs[j] : v0n;
}

template <class T, bool FROM_PARTIALS>
__global__ __launch_bounds__(kBlock) void LassoTallColsKernel(int64_t n, int64_t nb, LassoBatchInst<T> s) {
  LassoTallColsBody<T, FROM_PARTIALS>(n, nb, s, s.tpart, blockIdx.x);
}

// grid row b: member b's own launch, its partials at work + b * ws
template <class T>
__global__ __launch_bounds__(kBlock) void LassoTallColsBatchKernel(int64_t n, int64_t nb,
                                                                   const LassoBatchInst<T>* __restrict__ tab,
                                                                   const T* __restrict__ work, int64_t ws) {
  LassoTallColsBody<T, true>(n, nb, tab[blockIdx.y], work + blockIdx.y * ws, blockIdx.x);
}

template <class T> void LaunchTallCols(int64_t n, const LassoInstance& inst, bool partials) {
  hipStream_t st = Runtime::Get().stream();
  const int64_t nb = (n + kSB - 1) / kSB;
  const LassoBatchInst<T> s = Narrow<T>(inst);
  if (partials)
    hipLaunchKernelGGL((LassoTallColsKernel<T, true>), dim3(static_cast<unsigned>(nb)), dim3(kBlock), 0, st, n, nb, s);
  else
    hipLaunchKernelGGL((LassoTallColsKernel<T, false>), dim3(static_cast<unsigned>(nb)), dim3(kBlock), 0, st, n, nb, s);
}

}  // namespace

void LassoTallCols(int64_t n, const LassoInstance& inst, bool partials) {
  if (n == 0) return;
  const ConsensusState& c = inst.state;
  const DType dt = c.u.dt;
  for (const DVec* v : {&c.u, &c.var, &c.copy, &c.y_term, &c.y_zero, &c.y_term_prev, &inst.p, &inst.w})
    EPS_CHECK(v->dt == dt && v->n == n);
  for (const DVec* v : {&inst.rhs, &inst.zone.alpha_vec, &inst.zone.beta_vec})
    EPS_CHECK(v->n == 0 || (v->dt == dt && v->n == n));
  EPS_CHECK(!partials || (inst.tpart.dt == dt && inst.tpart.n >= SymvWorkspace(n)));
  ProfScope prof("lasso_tall_cols", n);
  if (dt == F32) LaunchTallCols<float>(n, inst, partials);
  else LaunchTallCols<double>(n, inst, partials);
  EPS_HIP(hipGetLastError());
}

void LassoTallColsBatch(int64_t n, DType dt, const DVec& table, int count, const DVec& work) {
  if (n == 0 || count == 0) return;
  const int64_t ws = SymvWorkspace(n);
  EPS_CHECK(count <= 65535 && work.dt == dt && work.n >= count * ws);
  hipStream_t st = Runtime::Get().stream();
  const int64_t nb = (n + kSB - 1) / kSB;
  const dim3 grid(static_cast<unsigned>(nb), static_cast<unsigned>(count));
  ProfScope prof("batch_lasso_tall_cols", n, count);
  if (dt == F32)
    hipLaunchKernelGGL(LassoTallColsBatchKernel<float>, grid, dim3(kBlock), 0, st, n, nb,
                       reinterpret_cast<const LassoBatchInst<float>*>(table.as<char>()), work.as<float>(), ws);
  else
    hipLaunchKernelGGL(LassoTallColsBatchKernel<double>, grid, dim3(kBlock), 0, st, n, nb,
                       reinterpret_cast<const LassoBatchInst<double>*>(table.as<char>()), work.as<double>(), ws);
  EPS_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace eps
