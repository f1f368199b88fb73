// Batched fused sweep: K instances of the "least squares + separable threshold" structure that
// share the data matrix A (a regularisation path, cross-validation folds, several right-hand
// sides) in ONE pass over A per sweep instead of K.
//
// Same geometry as LassoFusedStreamKernelT (kernels_fused.hip) with 256 threads: thread t owns
// rows R(t + 256q), q < NR, of every column (R = 4 in f32, 2 in f64: one 16-byte load); the
// workgroups take the same columns in the same order (LassoFusedGrid), the next column's loads
// are in flight while the current one is reduced.  Each loaded column feeds KB instances: their
// dot products with their own w, one LDS round trip and ONE barrier for all KB block
// reductions, their elementwise chains and their forward updates into their own partial t'.
// w and t' of every instance stay in registers (2 NR 16-byte values per instance per thread),
// which is what bounds KB (LassoBatchWidth; DESIGN.md lists the registers of each form).
//
// Per instance the arithmetic is exactly the single pass's: the same chunk order in the dot
// product, the same shuffle tree and LDS sum, the same chain (kernels_fused_chain.h), the same
// order of forward updates, and this file is compiled with -ffp-contract=off as kernels_fused.hip
// is - so every instance's iterates are bit-identical to its own solve.
//
// CHAIN (Chain, kernels.h: the batched forms are those of BatchPassExists): a column runs the single
// pass's step of that chain, its stores among them, on every member's own record; everything around
// the chain is the same code.  kChainZeroTallDot holds no t' registers, kChainZeroTallAcc no w
// registers.  In kChainZeroTall and kChainZeroTallAcc the members' values of a sample (state, offset,
// rhs; zfarg) are fetched by one lane per member and read from its register.
#include <hip/hip_runtime.h>

#include <vector>

#include "kernels.h"
#include "kernels_fused_chain.h"

namespace eps {
namespace k {

namespace {

constexpr int kBlock = 256;

// Lane `l` (uniform) of v in every lane of the wave: a register read, no memory.
__device__ inline float LaneValue(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ inline double LaneValue(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}

// GROUP: the nk instances are the columns of ONE matrix variable and the threshold is the group
// shrinkage of its rows (NORM_2 along axis 1, weight glam): row j's nk threshold inputs are what
// the pass computes for column j of A, and after the barrier every thread holds all of them.
template <class T, int NR, int KB, bool GROUP, int CHAIN>
__global__ __launch_bounds__(kBlock) void LassoBatchStreamKernel(int64_t m, int64_t n, const T* __restrict__ A,
                                                                 int64_t lda,
                                                                 const LassoBatchInst<T>* __restrict__ tab,
                                                                 int nk, double glam, int qfull,
                                                                 int64_t jcut) {
  typedef typename Chunk<T>::V V;
  constexpr int R = Chunk<T>::R;
  __shared__ T red[2][KB][kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (a constant, as in the single pass: filled element by element, the guarded loads below
  // become selects and lose their non-temporal hint)
  const V zero = T(0);
  V wv[KB][NR], tp[KB][NR];
  int64_t row[NR];
#pragma unroll
  for (int q = 0; q < NR; ++q) row[q] = (static_cast<int64_t>(q) * kBlock + tid) * R;
#pragma unroll
  for (int i = 0; i < KB; ++i) {
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      if constexpr (CHAIN != kChainZeroTallAcc)
        wv[i][q] = (i < nk && row[q] < m) ? *reinterpret_cast<const V*>(tab[i].w + row[q]) : zero;
      if constexpr (CHAIN != kChainZeroTallDot) tp[i][q] = zero;
    }
  }
  // this workgroup's columns: exactly those of LassoFusedStreamKernelT, in its order
  const int64_t npairs = (n + 1) / 2;
  auto column = [&](int64_t step) -> int64_t {
    const int64_t jp = blockIdx.x + (step >> 1) * gridDim.x;
    const int64_t j = 2 * jp + (step & 1);
    return (jp < npairs && j < n) ? j : -1;
  };
  // the single pass's loads: its resident share with the default policy, the rest non-temporal
  auto load = [&](V (&a)[NR], int64_t j) {
    const T* cp = A + j * lda;
    const int nres = qfull + (j < jcut ? 1 : 0);
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      if (row[q] < m) a[q] = LoadMatrixChunk<T>(cp + row[q], q < nres);
      else a[q] = zero;
    }
  };
  // kChainZeroTall and kChainZeroTallAcc: lane i of every wave fetches member i's values of a sample - one vector load
  // per array for all members, in flight together - and the member's step reads them from that
  // lane's register (LaneValue).  Member by member through the table they are KB dependent scalar
  // loads, each waited for, which is what a sample then costs.  The values are the same.
  [[maybe_unused]] const T *pu = nullptr, *py0 = nullptr, *py1 = nullptr, *pg = nullptr, *pr = nullptr,
                           *pf = nullptr;
  if constexpr (CHAIN == kChainZeroTall || CHAIN == kChainZeroTallAcc) {
    static_assert(KB <= 64, "a lane per member");
    if (lane < nk) {
      const LassoBatchInst<T>& L = tab[lane];
      if constexpr (CHAIN == kChainZeroTall) {
        pu = L.u;
        py0 = L.y0;
        py1 = L.y1;
        pg = L.zg;
        pr = L.zrhs;
      } else {
        pf = L.zfarg;
      }
    }
  }
  V cur[NR], nxt[NR];
  int64_t step = 0;
  int64_t j = column(0);
  if (j >= 0) load(cur, j);
  int par = 0;
  while (j >= 0) {
    int64_t jn = column(step + 1);
    if (jn < 0 && ((step + 1) & 1)) jn = column(step + 2);
    const int64_t step_n = (jn >= 0 && column(step + 1) < 0) ? step + 2 : step + 1;
    if (jn >= 0) load(nxt, jn);
    // every instance's column state is read before the barrier: thread 0 overwrites it after
    [[maybe_unused]] T uj[KB], y0j[KB], y1j[KB];
    [[maybe_unused]] T gj[KB], rj[KB];  // kChainZeroTall: the member's offset and rhs of this sample
    [[maybe_unused]] T su = T(0), sy0 = T(0), sy1 = T(0), sg = T(0), sr = T(0), sf = T(0);  // lane i: member i's
    if constexpr (CHAIN == kChainZeroTall) {
      if (lane < nk) {
        su = pu[j];
        sy0 = py0[j];
        sy1 = py1[j];
        if (pg != nullptr) sg = pg[j];
        if (pr != nullptr) sr = pr[j];
      }
    }
    if constexpr (CHAIN == kChainZeroTallAcc) {
      if (lane < nk) sf = pf[j];
    }
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      if (i >= nk) continue;
      if constexpr (CHAIN == kChainLasso || CHAIN == kChainZeroCols) {
        uj[i] = tab[i].u[j];
        y0j[i] = tab[i].y0[j];
        y1j[i] = tab[i].y1[j];
      }
      if constexpr (CHAIN == kChainZeroTall) {
        uj[i] = LaneValue(su, i);
        y0j[i] = LaneValue(sy0, i);
        y1j[i] = LaneValue(sy1, i);
        gj[i] = LaneValue(sg, i);
        rj[i] = LaneValue(sr, i);
      }
      if constexpr (CHAIN != kChainZeroTallAcc) {
        T d = T(0);
#pragma unroll
        for (int q = 0; q < NR; ++q)
#pragma unroll
          for (int r = 0; r < R; ++r) d += cur[q][r] * wv[i][q][r];
        d = WaveSumT<T>(d);
        if (lane == 0) red[par][i][wave] = d;
      }
    }
    if constexpr (CHAIN != kChainZeroTallAcc) __syncthreads();
    if constexpr (CHAIN == kChainZeroTallDot) {
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if (i >= nk) continue;
        T d = red[par][i][0];
#pragma unroll
        for (int w2 = 1; w2 < kBlock / 64; ++w2) d += red[par][i][w2];
        if (tid == 0) tab[i].zd[j] = d;
      }
    } else if constexpr (CHAIN == kChainZeroTallAcc) {
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if (i >= nk) continue;
        const T v0n = LaneValue(sf, i);
#pragma unroll
        for (int q = 0; q < NR; ++q)
#pragma unroll
          for (int r = 0; r < R; ++r) tp[i][q][r] += cur[q][r] * v0n;
      }
    } else if constexpr (GROUP) {
      auto scalars = [&](int i) {
        const LassoBatchInst<T>& I = tab[i];
        FusedScalarsT<T> c;
        c.kappa = I.kappa;
        c.Bs = I.Bs;
        c.Cs = I.Cs;
        c.a1 = I.a1;
        c.lam = c.alpha = c.beta = c.M = T(0);  // (the scaled zone's: not read)
        return c;
      };
      ChainHeadT<T> h[KB];
      double ss = 0;
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if (i >= nk) continue;
        T d = red[par][i][0];
#pragma unroll
        for (int w2 = 1; w2 < kBlock / 64; ++w2) d += red[par][i][w2];
        h[i] = ChainHeadOfT<T>(d, scalars(i), uj[i], y0j[i], y1j[i]);
        const double v = static_cast<double>(h[i].vin);
        ss += v * v;
      }
      const double scale = GroupScale(ss, glam);
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if (i >= nk) continue;
        const LassoBatchInst<T>& I = tab[i];
        const T xz = static_cast<T>(scale * static_cast<double>(h[i].vin));
        T nx0, nx1, ny0, ny1, nu;
        const T v0n = ChainTailT<T>(h[i], xz, scalars(i), &nx0, &nx1, &ny0, &ny1, &nu);
        if (tid == 0) {
          I.y1prev[j] = y1j[i];
          I.x0[j] = nx0;
          I.x1[j] = nx1;
          I.y0[j] = ny0;
          I.y1[j] = ny1;
          I.u[j] = nu;
        }
#pragma unroll
        for (int q = 0; q < NR; ++q)
#pragma unroll
          for (int r = 0; r < R; ++r) tp[i][q][r] += cur[q][r] * v0n;
      }
    } else {
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if (i >= nk) continue;
        const LassoBatchInst<T>& I = tab[i];
        T d = red[par][i][0];
#pragma unroll
        for (int w2 = 1; w2 < kBlock / 64; ++w2) d += red[par][i][w2];
        FusedScalarsT<T> c;
        c.kappa = I.kappa;
        c.Bs = I.Bs;
        c.Cs = I.Cs;
        c.a1 = I.a1;
        c.lam = I.lam;
        c.alpha = I.alpha_v != nullptr ? I.alpha_v[j] : I.alpha;
        c.beta = I.beta_v != nullptr ? I.beta_v[j] : I.beta;
        c.M = I.M;
        T v0n;
        if constexpr (CHAIN == kChainZeroCols || CHAIN == kChainZeroTall) {
          T ns, nq, nys, nyq, nu;
          if constexpr (CHAIN == kChainZeroCols)
            v0n = ZeroChainT<T>(d, c, T(0), uj[i], y1j[i], y0j[i], &ns, &nq, &nys, &nyq, &nu);
          else
            v0n = ZeroTallChainT<T>(d, c, I.ke, I.dinv, gj[i], rj[i], uj[i], y1j[i], y0j[i], &ns, &nq, &nys, &nyq,
                                    &nu);
          if (tid == 0) {
            I.y1prev[j] = y1j[i];
            I.e0[j] = y0j[i];
            I.x1[j] = ns;
            I.x0[j] = nq;
            I.y1[j] = nys;
            I.y0[j] = nyq;
            I.u[j] = nu;
          }
        } else {
          T nx0, nx1, ny0, ny1, nu;
          v0n = ChainOneT<T>(d, c, uj[i], y0j[i], y1j[i], &nx0, &nx1, &ny0, &ny1, &nu);
          if (tid == 0) {
            I.y1prev[j] = y1j[i];
            I.x0[j] = nx0;
            I.x1[j] = nx1;
            I.y0[j] = ny0;
            I.y1[j] = ny1;
            I.u[j] = nu;
          }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q)
#pragma unroll
          for (int r = 0; r < R; ++r) tp[i][q][r] += cur[q][r] * v0n;
      }
    }
    par ^= 1;
#pragma unroll
    for (int q = 0; q < NR; ++q) cur[q] = nxt[q];
    j = jn;
    step = step_n;
  }
  if constexpr (CHAIN != kChainZeroTallDot) {
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      if (i >= nk) continue;
      T* out = tab[i].tpart + static_cast<int64_t>(blockIdx.x) * m;
#pragma unroll
      for (int q = 0; q < NR; ++q)
        if (row[q] < m) *reinterpret_cast<V*>(out + row[q]) = tp[i][q];
    }
  }
}

// 16-byte row chunks per thread of the single pass with 256 threads, rounded up to its ladder
int ChunksPerThread(int64_t m, DType dt) {
  const int64_t rows = dt == F32 ? 4 : 2;
  const int64_t need = (m + rows * kBlock - 1) / (rows * kBlock);
  return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 10;
}

// Instances per launch for NR chunks per thread: w and t' take 8 NR registers per instance in
// either type, the column and the next one in flight 8 NR more.  Chosen so that no
// instantiation spills to scratch (hipcc -Rpass-analysis=kernel-resource-usage).
constexpr int WidthFor(int nr) { return nr <= 2 ? 8 : nr <= 4 ? 6 : nr <= 8 ? 5 : 4; }
// Per chain.  The ZERO chains keep a few more values live per column step than the lasso's (DESIGN.md
// 3.11, "Registers"; kChainZeroTall also the sample's offset and rhs per member): a form of theirs
// that would spill at the lasso's width takes a smaller one without touching the lasso's.  The halves
// of the tall pass hold no t' or no w - 4 NR registers per member instead of 8 NR - so they carry
// more members per read of the matrix (DESIGN.md 3.6 has the registers of each form).
constexpr int WidthFor(int nr, Chain chain) {
  return ChainIsTallHalf(chain) ? (nr <= 2 ? 16 : nr <= 4 ? 12 : nr <= 8 ? 10 : 8) : WidthFor(nr);
}

// The one instantiation of the chain (BatchPassExists; LassoBatchPass has checked it), or the lasso
// chain's group form.
template <class T, int NR>
void LaunchBatch(int grid, int64_t m, int64_t n, const T* A, int64_t lda, const LassoBatchInst<T>* tab, int nk,
                 const double* glam, const FusedResidency& res, Chain chain) {
  decltype(&LassoBatchStreamKernel<T, NR, WidthFor(NR), false, kChainLasso>) kernel = nullptr;
  WithChain(chain, [&](auto c) {
    constexpr Chain kChain = decltype(c)::value;
    if constexpr (BatchPassExists(kChain, kHeadZone))
      kernel = LassoBatchStreamKernel<T, NR, WidthFor(NR, kChain), false, kChain>;
  });
  if (glam != nullptr) kernel = LassoBatchStreamKernel<T, NR, WidthFor(NR), true, kChainLasso>;
  EPS_CHECK(kernel != nullptr);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, Runtime::Get().stream(), m, n, A, lda, tab, nk,
                     glam != nullptr ? *glam : 0.0, res.qfull, res.jcut);
}

template <class T>
void LaunchBatchT(int nr, int grid, int64_t m, int64_t n, const T* A, int64_t lda, const LassoBatchInst<T>* tab,
                  int nk, const double* glam, const FusedResidency& res, Chain chain) {
  switch (nr) {
    case 1: LaunchBatch<T, 1>(grid, m, n, A, lda, tab, nk, glam, res, chain); break;
    case 2: LaunchBatch<T, 2>(grid, m, n, A, lda, tab, nk, glam, res, chain); break;
    case 4: LaunchBatch<T, 4>(grid, m, n, A, lda, tab, nk, glam, res, chain); break;
    case 8: LaunchBatch<T, 8>(grid, m, n, A, lda, tab, nk, glam, res, chain); break;
    default: LaunchBatch<T, 10>(grid, m, n, A, lda, tab, nk, glam, res, chain); break;
  }
}

template <class T>
void UploadT(const std::vector<const LassoInstance*>& members, DVec* table) {
  std::vector<LassoBatchInst<T>> host;
  host.reserve(members.size());
  for (const LassoInstance* s : members) host.push_back(Narrow<T>(*s));
  UploadRecords(host, table);
}

}  // namespace

int LassoBatchWidth(int64_t m, int64_t n, DType dt, Chain chain) {
  if (LassoFusedBlock(m, n, dt) != kBlock) return 0;
  return WidthFor(ChunksPerThread(m, dt), chain);
}

void LassoBatchUpload(const std::vector<const LassoInstance*>& members, DType dt, DVec* table) {
  for (const LassoInstance* s : members) {
    const ConsensusState& c = s->state;
    for (const DVec* v : {&s->w, &s->tpart, &c.u, &c.var, &c.copy, &c.y_term, &c.y_zero, &c.y_term_prev, &s->p})
      EPS_CHECK(v->dt == dt && v->n > 0);
    for (const DVec* v : {&c.y_zero_prev, &s->zg, &s->zrhs, &s->zd, &s->zfarg})
      EPS_CHECK(v->n == 0 || (v->dt == dt && v->n == c.u.n));
    EPS_CHECK_MSG(s->zone.head == kHeadZone, "the batched pass has no " << kHeadNames[s->zone.head] << " head");
  }
  if (dt == F32) UploadT<float>(members, table);
  else UploadT<double>(members, table);
}

void LassoBatchPass(int64_t m, int64_t n, int64_t lda, const DVec& A, const DVec& table, int first, int count,
                    const double* group_lam, const FusedResidency& res, Chain chain) {
  const DType dt = A.dt;
  EPS_CHECK_MSG(chain >= kChainLasso && chain <= kChainZeroTallAcc && BatchPassExists(chain, kHeadZone) &&
                    (chain == kChainLasso || group_lam == nullptr),
                "batched fused pass: chain " << chain);
  EPS_CHECK(LassoFusedSupported(m, n, A, lda));
  EPS_CHECK(res.qfull >= 0 && res.jcut >= 0 && res.jcut <= n);
  const int width = LassoBatchWidth(m, n, dt, chain);
  EPS_CHECK_MSG(width > 0 && count >= 1 && count <= width,
                "batched fused pass: " << count << " instances, width " << width);
  const int grid = LassoFusedGrid(m, n, dt);
  const int nr = ChunksPerThread(m, dt);
  ProfScope prof(kChainTags[chain][1], m, n);
  NoteFusedResidency(res.qfull, res.jcut);
  if (dt == F32)
    LaunchBatchT<float>(nr, grid, m, n, A.as<float>(), lda,
                        reinterpret_cast<const LassoBatchInst<float>*>(table.as<char>()) + first, count, group_lam, res,
                        chain);
  else
    LaunchBatchT<double>(nr, grid, m, n, A.as<double>(), lda,
                         reinterpret_cast<const LassoBatchInst<double>*>(table.as<char>()) + first, count, group_lam, res,
                         chain);
  EPS_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace eps
