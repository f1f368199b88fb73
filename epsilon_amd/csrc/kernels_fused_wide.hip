// Wide batched fused sweep: a panel of up to 64 f32 instances that share the data matrix A rides
// along with every byte of A on the exact-f32 matrix instruction (v_mfma_f32_16x16x4_f32: bit for
// bit an fmaf chain in the order of the contraction index).  Unlike the register-resident batched
// pass (kernels_fused_batch.hip) a sweep reads A twice:
//
//   WideBackKernel     D = A^T W (n x KW), then the elementwise chain per (column, instance)
//                      (ChainOneT, kernels_fused_chain.h), which writes the state and the panel V'
//   WideForwardKernel  partial T_s = A[:, slab s] V'[slab s, :] (m x KW) for S column slabs
//   WideReduceKernel   p = pkappa * (T_0 + ... + T_{S-1}) + rhs per instance, fixed order
//
// The single pass sums every product as a tree (per-thread pieces, wave shuffles, partials); a
// single MFMA chain over all of m or n would carry sqrt(length) times its rounding into the
// iterates and lift the floor of the residuals.  So every product here is summed in levels: MFMA
// chains of 16 terms, short runs of their sums, and compensated (Kahan) sums above that.
//
// Panels are instance-major: slot i's vector is contiguous at i * ld.  A lane's 16-byte load of A
// holds four consecutive values of the contraction index; the four MFMAs that consume its
// components take the other operand permuted the same way (the order of the contraction index is
// free as long as both operands agree), so A is read in 16-byte pieces in both kernels.
//
// Every output element is its own accumulation chain over a contraction order that depends on
// (m, n) only, and unused or stopped slots are masked on every store: an instance's bits depend
// neither on its slot nor on the other instances of the panel, and repeat from run to run.  They
// are NOT the bits of the single pass (another summation order); DESIGN.md 3.8.
//
// Compiled with -ffp-contract=off like the other fused-sweep files.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "kernels_fused_chain.h"

namespace eps {
namespace k {

namespace {

constexpr int kBlock = 256;  // four waves
typedef float F4 __attribute__((ext_vector_type(4)));

// ---- back product + chain ---------------------------------------------------------------------
constexpr int kBackRows = 128;              // rows of W staged per step of the pipeline
constexpr int kBackLd = kBackRows + 4;      // LDS floats per instance (16-byte aligned rows)
constexpr int kBackCols = 64;               // columns of A per workgroup, 16 per wave
constexpr int kBackChain = 2;               // MFMAs per chain (1, 2 or 4): 4 * kBackChain rows

// GROUP: the nk slots are ALL the columns of one matrix variable (every one live) and the
// threshold is the group shrinkage of its rows (NORM_2 along axis 1, weight glam).
template <int NB, bool GROUP>
__global__ __launch_bounds__(kBlock) void WideBackKernel(int64_t m, int64_t n, const float* __restrict__ A,
                                                         int64_t lda, const float* __restrict__ W, int64_t ldw,
                                                         const LassoBatchInst<float>* __restrict__ tab, int nk,
                                                         unsigned long long active, float* __restrict__ Vp,
                                                         int64_t ldv, double glam) {
  constexpr int KW = 16 * NB;
  constexpr int NW = KW / 8;  // 16-byte pieces of a W chunk per thread: KW * 32 / 256
  __shared__ __attribute__((aligned(16))) float lw[2][KW * kBackLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const F4 zero = {0.f, 0.f, 0.f, 0.f};
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kBackCols + wave * 16;
  const int64_t jcol = j0 + c16;
  const bool col_ok = jcol < n;
  const float* ap = A + (col_ok ? jcol : 0) * lda;
  const int64_t nchunks = (m + kBackRows - 1) / kBackRows;

  auto load_w = [&](F4 (&wr)[NW], int64_t r0) {
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      const int idx = tid + kBlock * q;
      const int inst = idx >> 5, rg = idx & 31;
      const int64_t r = r0 + 4 * rg;
      wr[q] = (inst < nk && r < m) ? *reinterpret_cast<const F4*>(W + inst * ldw + r) : zero;
    }
  };
  auto store_w = [&](const F4 (&wr)[NW], int buf) {
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      const int idx = tid + kBlock * q;
      const int inst = idx >> 5, rg = idx & 31;
      *reinterpret_cast<F4*>(&lw[buf][inst * kBackLd + 4 * rg]) = wr[q];
    }
  };
  auto load_a = [&](F4 (&a)[8], int64_t r0) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int64_t r = r0 + 16 * s + 4 * g;
      a[s] = (col_ok && r < m) ? __builtin_nontemporal_load(reinterpret_cast<const F4*>(ap + r)) : zero;
    }
  };

  F4 acc[NB], comp[NB];
#pragma unroll
  for (int ib = 0; ib < NB; ++ib) acc[ib] = comp[ib] = zero;
  F4 wr[NW], a_cur[8], a_nxt[8];
  load_w(wr, 0);
  load_a(a_cur, 0);
  store_w(wr, 0);
  __syncthreads();
  for (int64_t ch = 0; ch < nchunks; ++ch) {
    const int buf = static_cast<int>(ch & 1);
    const bool more = ch + 1 < nchunks;
    if (more) {
      load_w(wr, (ch + 1) * kBackRows);
      load_a(a_nxt, (ch + 1) * kBackRows);
    }
    // Summation in levels, so that the rounding does not grow with m as one chain over all rows
    // would: MFMA chains of kBackChain instructions (4 rows each), every chain's sum added to the
    // running sum with compensation (Kahan).
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      F4 b[NB];
#pragma unroll
      for (int ib = 0; ib < NB; ++ib)
        b[ib] = *reinterpret_cast<const F4*>(&lw[buf][(ib * 16 + c16) * kBackLd + 16 * s + 4 * g]);
#pragma unroll
      for (int c0 = 0; c0 < 4; c0 += kBackChain) {
        F4 part[NB];
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) part[ib] = zero;
#pragma unroll
        for (int c = c0; c < c0 + kBackChain; ++c)
#pragma unroll
          for (int ib = 0; ib < NB; ++ib)
            part[ib] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[s][c], b[ib][c], part[ib], 0, 0, 0);
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) {
          const F4 y = part[ib] - comp[ib];
          const F4 t = acc[ib] + y;
          comp[ib] = (t - acc[ib]) - y;
          acc[ib] = t;
          // the chain's sum is consumed here: left free, the compiler keeps the accumulators of
          // all unrolled steps alive at once
          asm volatile("" : "+v"(acc[ib]));
        }
      }
    }
    if (more) store_w(wr, buf ^ 1);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 8; ++s) a_cur[s] = a_nxt[s];
  }

  // C/D layout: acc[ib][i] = D[column j0 + 4 g + i][slot 16 ib + c16]
  const int64_t jb = j0 + 4 * g;
  if constexpr (GROUP) {
    // Row j's members sit in this lane's NB tiles and across the 16 lanes (c16) of its row group:
    // the squares are summed in-lane over the tiles, then across the lanes by a butterfly whose
    // two partners add the same two numbers, so all 16 lanes hold the same bits.  No lane leaves
    // before the exchange; slots >= nk and columns >= n contribute zero.
    ChainHeadT<float> h[NB][4];
    float y1o[NB][4];
    double ss[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) {
      const int slot = ib * 16 + c16;
      const bool live = slot < nk;
      const LassoBatchInst<float>& I = tab[live ? slot : 0];
      FusedScalarsT<float> c;
      c.kappa = I.kappa;
      c.Bs = I.Bs;
      c.Cs = I.Cs;
      c.a1 = I.a1;
      c.lam = c.alpha = c.beta = c.M = 0.f;  // (the scaled zone's: not read)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t j = jb + i;
        const bool ok = live && j < n;
        y1o[ib][i] = ok ? I.y1[j] : 0.f;
        h[ib][i] = ChainHeadOfT<float>(acc[ib][i], c, ok ? I.u[j] : 0.f, ok ? I.y0[j] : 0.f, y1o[ib][i]);
        const double v = ok ? static_cast<double>(h[ib][i].vin) : 0.0;
        ss[i] += v * v;
      }
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
#pragma unroll
      for (int i = 0; i < 4; ++i) ss[i] += __shfl_xor(ss[i], off, 64);
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) {
      const int slot = ib * 16 + c16;
      if (slot >= nk) continue;
      const LassoBatchInst<float>& I = tab[slot];
      FusedScalarsT<float> c;
      c.kappa = I.kappa;
      c.Bs = I.Bs;
      c.Cs = I.Cs;
      c.a1 = I.a1;
      c.lam = c.alpha = c.beta = c.M = 0.f;
      float* vp = Vp + slot * ldv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t j = jb + i;
        if (j >= n) continue;
        const float xz = static_cast<float>(GroupScale(ss[i], glam) * static_cast<double>(h[ib][i].vin));
        float x0, x1, z0, z1, uu;
        const float v = ChainTailT<float>(h[ib][i], xz, c, &x0, &x1, &z0, &z1, &uu);
        I.y1prev[j] = y1o[ib][i];
        I.x0[j] = x0;
        I.x1[j] = x1;
        I.y0[j] = z0;
        I.y1[j] = z1;
        I.u[j] = uu;
        vp[j] = v;
      }
    }
    return;
  }
  if (jb >= n) return;
#pragma unroll
  for (int ib = 0; ib < NB; ++ib) {
    const int slot = ib * 16 + c16;
    if (slot >= nk || !((active >> slot) & 1ull)) continue;
    const LassoBatchInst<float>& I = tab[slot];
    FusedScalarsT<float> c;
    c.kappa = I.kappa;
    c.Bs = I.Bs;
    c.Cs = I.Cs;
    c.a1 = I.a1;
    c.lam = I.lam;
    c.alpha = I.alpha;
    c.beta = I.beta;
    c.M = I.M;
    float* vp = Vp + slot * ldv;
    // (the columns of a matrix variable lie n apart: 16-byte pieces only where n allows)
    const bool aligned = ((reinterpret_cast<uintptr_t>(I.u) | reinterpret_cast<uintptr_t>(I.x0) |
                           reinterpret_cast<uintptr_t>(I.x1) | reinterpret_cast<uintptr_t>(I.y0) |
                           reinterpret_cast<uintptr_t>(I.y1) | reinterpret_cast<uintptr_t>(I.y1prev)) & 15) == 0;
    if (jb + 4 <= n && aligned) {
      const F4 u = *reinterpret_cast<const F4*>(I.u + jb);
      const F4 y0 = *reinterpret_cast<const F4*>(I.y0 + jb);
      const F4 y1 = *reinterpret_cast<const F4*>(I.y1 + jb);
      F4 nx0, nx1, ny0, ny1, nu, nv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (I.alpha_v != nullptr) c.alpha = I.alpha_v[jb + i];
        if (I.beta_v != nullptr) c.beta = I.beta_v[jb + i];
        float x0, x1, z0, z1, uu;
        nv[i] = ChainOneT<float>(acc[ib][i], c, u[i], y0[i], y1[i], &x0, &x1, &z0, &z1, &uu);
        nx0[i] = x0;
        nx1[i] = x1;
        ny0[i] = z0;
        ny1[i] = z1;
        nu[i] = uu;
      }
      *reinterpret_cast<F4*>(I.y1prev + jb) = y1;
      *reinterpret_cast<F4*>(I.x0 + jb) = nx0;
      *reinterpret_cast<F4*>(I.x1 + jb) = nx1;
      *reinterpret_cast<F4*>(I.y0 + jb) = ny0;
      *reinterpret_cast<F4*>(I.y1 + jb) = ny1;
      *reinterpret_cast<F4*>(I.u + jb) = nu;
      *reinterpret_cast<F4*>(vp + jb) = nv;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t j = jb + i;
        if (j >= n) continue;
        if (I.alpha_v != nullptr) c.alpha = I.alpha_v[j];
        if (I.beta_v != nullptr) c.beta = I.beta_v[j];
        const float y1 = I.y1[j];
        float x0, x1, z0, z1, uu;
        const float v = ChainOneT<float>(acc[ib][i], c, I.u[j], I.y0[j], y1, &x0, &x1, &z0, &z1, &uu);
        I.y1prev[j] = y1;
        I.x0[j] = x0;
        I.x1[j] = x1;
        I.y0[j] = z0;
        I.y1[j] = z1;
        I.u[j] = uu;
        vp[j] = v;
      }
    }
  }
}

// ---- forward product ---------------------------------------------------------------------------
constexpr int kFwdRows = 256;          // rows of A per workgroup, 64 per wave
constexpr int kFwdCols = 32;           // columns of V' staged per step of the pipeline
constexpr int kFwdLd = kFwdCols + 4;   // LDS floats per instance
constexpr int kFwdSlabMax = 512;       // columns per slab at most: bounds the length of a running sum

template <int NB>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void WideForwardKernel(int64_t m, int64_t n, const float* __restrict__ A,
                                                            int64_t lda, const float* __restrict__ Vp, int64_t ldv,
                                                            int nk, int64_t slab, float* __restrict__ Tp,
                                                            int64_t ldt) {
  constexpr int KW = 16 * NB;
  constexpr int NV = (KW * 8 + kBlock - 1) / kBlock;  // 16-byte pieces of a V' chunk per thread
  __shared__ __attribute__((aligned(16))) float lv[2][KW * kFwdLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mi = lane & 15, g = lane >> 4;
  const F4 zero = {0.f, 0.f, 0.f, 0.f};
  const int64_t rbase = static_cast<int64_t>(blockIdx.x) * kFwdRows + wave * 64;
  const int64_t row = rbase + 4 * mi;  // this lane's four rows of every loaded column
  const bool row_ok = row < m;
  const int64_t cs = static_cast<int64_t>(blockIdx.y) * slab;
  const int64_t ce = cs + slab < n ? cs + slab : n;
  const int64_t nchunks = (ce - cs + kFwdCols - 1) / kFwdCols;  // slab is a multiple of kFwdCols

  auto load_v = [&](F4 (&vr)[NV], int64_t jc) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int idx = tid + kBlock * q;
      const int inst = idx >> 3, cg = idx & 7;
      const int64_t j = jc + 4 * cg;
      // columns n .. ldv of V' are zero and never written
      vr[q] = (idx < KW * 8 && inst < nk && j + 4 <= ldv) ? *reinterpret_cast<const F4*>(Vp + inst * ldv + j) : zero;
    }
  };
  auto store_v = [&](const F4 (&vr)[NV], int buf) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int idx = tid + kBlock * q;
      const int inst = idx >> 3, cg = idx & 7;
      if (idx < KW * 8) *reinterpret_cast<F4*>(&lv[buf][inst * kFwdLd + 4 * cg]) = vr[q];
    }
  };
  auto load_a = [&](F4 (&a)[8], int64_t jc) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int64_t j = jc + 16 * (t >> 2) + 4 * g + (t & 3);
      a[t] = (row_ok && j < ce) ? __builtin_nontemporal_load(reinterpret_cast<const F4*>(A + j * lda + row)) : zero;
    }
  };

  F4 acc[4][NB];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) acc[c][ib] = zero;
  F4 vr[NV], a_cur[8], a_nxt[8];
  if (nchunks > 0) {
    load_v(vr, cs);
    load_a(a_cur, cs);
    store_v(vr, 0);
  }
  __syncthreads();
  for (int64_t ch = 0; ch < nchunks; ++ch) {
    const int buf = static_cast<int>(ch & 1);
    const bool more = ch + 1 < nchunks;
    if (more) {
      load_v(vr, cs + (ch + 1) * kFwdCols);
      load_a(a_nxt, cs + (ch + 1) * kFwdCols);
    }
    // summation in levels: two chains of 16 columns per tile and chunk, added to the running sum
    // of the slab (at most kFwdSlabMax / kFwdCols chunks)
    F4 b[2][NB];
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int ib = 0; ib < NB; ++ib)
        b[st][ib] = *reinterpret_cast<const F4*>(&lv[buf][(ib * 16 + mi) * kFwdLd + 16 * st + 4 * g]);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int ib = 0; ib < NB; ++ib) {
        F4 p0 = zero, p1 = zero;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[t][c], b[0][ib][t], p0, 0, 0, 0);
          p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[4 + t][c], b[1][ib][t], p1, 0, 0, 0);
        }
        acc[c][ib] += p0 + p1;
        // the tile's chains are consumed here: left free, the compiler keeps many tiles' alive
        asm volatile("" : "+v"(acc[c][ib]));
      }
    if (more) store_v(vr, buf ^ 1);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 8; ++t) a_cur[t] = a_nxt[t];
  }

  // acc[c][ib][i] = T[row rbase + 4 (4 g + i) + c][slot 16 ib + mi]
  float* tp = Tp + static_cast<int64_t>(blockIdx.y) * KW * ldt;
#pragma unroll
  for (int ib = 0; ib < NB; ++ib) {
    const int slot = ib * 16 + mi;
    if (slot >= nk) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = rbase + 16 * g + 4 * i;
      if (r >= m) continue;
      F4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = acc[c][ib][i];
      *reinterpret_cast<F4*>(tp + slot * ldt + r) = o;
    }
  }
}

// ---- reduction -----------------------------------------------------------------------------------
// p = pkappa * (T_0 + T_1 + ...) + rhs, the arithmetic of ReducePartials, for every live slot
__global__ __launch_bounds__(kBlock) void WideReduceKernel(int64_t m, int nslabs, int kw,
                                                           const LassoBatchInst<float>* __restrict__ tab,
                                                           unsigned long long active, const float* __restrict__ Tp,
                                                           int64_t ldt) {
  const int slot = blockIdx.y;
  if (!((active >> slot) & 1ull)) return;
  const int64_t r = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * 4;
  if (r >= m) return;
  const LassoBatchInst<float>& I = tab[slot];
  const float* tp = Tp + slot * ldt + r;
  // the slabs in order, with compensation (Kahan): the rounding does not grow with their number
  const F4 zero = {0.f, 0.f, 0.f, 0.f};
  F4 s = zero, comp = zero;
  for (int k2 = 0; k2 < nslabs; ++k2) {
    const F4 y = *reinterpret_cast<const F4*>(tp + static_cast<int64_t>(k2) * kw * ldt) - comp;
    const F4 t = s + y;
    comp = (t - s) - y;
    s = t;
  }
  F4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[i] = I.pkappa * s[i];
    if (I.rhs != nullptr) o[i] += I.rhs[r + i];
  }
  *reinterpret_cast<F4*>(I.p + r) = o;
}

int PanelBlocks(int nk) { return (nk + 15) / 16; }

}  // namespace

bool LassoWideSupported(int64_t m, int64_t n, const DVec& A, int64_t lda) {
  return A.dt == F32 && LassoFusedSupported(m, n, A, lda);
}

int64_t LassoWideSlabColumns(int64_t m, int64_t n) {
  // two workgroups per CU: 512 over the row tiles; between one staged chunk and kFwdSlabMax
  // columns per slab
  const int64_t row_tiles = (m + kFwdRows - 1) / kFwdRows;
  int64_t want = (512 + row_tiles - 1) / row_tiles;
  if (want < 1) want = 1;
  int64_t slab = ((n + want - 1) / want + kFwdCols - 1) / kFwdCols * kFwdCols;
  if (slab < kFwdCols) slab = kFwdCols;
  if (slab > kFwdSlabMax) slab = kFwdSlabMax;
  return slab;
}

int LassoWideSlabs(int64_t m, int64_t n) {
  const int64_t slab = LassoWideSlabColumns(m, n);
  return static_cast<int>((n + slab - 1) / slab);
}

void LassoWideBack(int64_t m, int64_t n, int64_t lda, const DVec& A, const DVec& table, int first, int nk,
                   uint64_t active, const DVec& W, int64_t ldw, const DVec& V, int64_t ldv, const double* group_lam) {
  EPS_CHECK(LassoWideSupported(m, n, A, lda));
  EPS_CHECK_MSG(nk >= 1 && nk <= kLassoWidePanel, "wide back product: " << nk << " instances in a panel");
  EPS_CHECK(W.dt == F32 && V.dt == F32 && ldw % 4 == 0 && ldw >= m && ldv % 4 == 0 && ldv >= n);
  EPS_CHECK(W.n >= static_cast<int64_t>(nk) * ldw && V.n >= static_cast<int64_t>(nk) * ldv);
  EPS_CHECK(reinterpret_cast<uintptr_t>(W.data()) % 16 == 0 && reinterpret_cast<uintptr_t>(V.data()) % 16 == 0);
  const auto* tab = reinterpret_cast<const LassoBatchInst<float>*>(table.as<char>()) + first;
  const dim3 grid(static_cast<unsigned>((n + kBackCols - 1) / kBackCols));
  hipStream_t s = Runtime::Get().stream();
  ProfScope prof("wide_back", m, n);
  const bool group = group_lam != nullptr;
  if (group) {
    const uint64_t all = nk == 64 ? ~uint64_t(0) : (uint64_t(1) << nk) - 1;
    EPS_CHECK_MSG((active & all) == all, "wide back product: a group's members are all live");
  }
#define EPS_WIDE_BACK(NB)                                                                                       \
  if (group)                                                                                                    \
    hipLaunchKernelGGL((WideBackKernel<NB, true>), grid, dim3(kBlock), 0, s, m, n, A.as<float>(), lda,          \
                       W.as<float>(), ldw, tab, nk, static_cast<unsigned long long>(active), V.as<float>(), ldv, \
                       *group_lam);                                                                             \
  else                                                                                                          \
    hipLaunchKernelGGL((WideBackKernel<NB, false>), grid, dim3(kBlock), 0, s, m, n, A.as<float>(), lda,         \
                       W.as<float>(), ldw, tab, nk, static_cast<unsigned long long>(active), V.as<float>(), ldv, 0.0)
  switch (PanelBlocks(nk)) {
    case 1: EPS_WIDE_BACK(1); break;
    case 2: EPS_WIDE_BACK(2); break;
    case 3: EPS_WIDE_BACK(3); break;
    default: EPS_WIDE_BACK(4); break;
  }
#undef EPS_WIDE_BACK
  EPS_HIP(hipGetLastError());
}

void LassoWideForward(int64_t m, int64_t n, int64_t lda, const DVec& A, int nk, const DVec& V, int64_t ldv,
                      const DVec& T, int64_t ldt) {
  EPS_CHECK(LassoWideSupported(m, n, A, lda));
  EPS_CHECK(nk >= 1 && nk <= kLassoWidePanel);
  const int nb = PanelBlocks(nk);
  const int64_t slab = LassoWideSlabColumns(m, n);
  const int nslabs = LassoWideSlabs(m, n);
  EPS_CHECK(V.dt == F32 && T.dt == F32 && ldv % 4 == 0 && ldv >= n && ldt % 4 == 0 && ldt >= m);
  EPS_CHECK(V.n >= static_cast<int64_t>(nk) * ldv && T.n >= static_cast<int64_t>(nslabs) * 16 * nb * ldt);
  EPS_CHECK(reinterpret_cast<uintptr_t>(V.data()) % 16 == 0 && reinterpret_cast<uintptr_t>(T.data()) % 16 == 0);
  const dim3 grid(static_cast<unsigned>((m + kFwdRows - 1) / kFwdRows), static_cast<unsigned>(nslabs));
  hipStream_t s = Runtime::Get().stream();
  ProfScope prof("wide_forward", m, n);
#define EPS_WIDE_FWD(NB)                                                                                          \
  hipLaunchKernelGGL(WideForwardKernel<NB>, grid, dim3(kBlock), 0, s, m, n, A.as<float>(), lda, V.as<float>(), \
                     ldv, nk, slab, T.as<float>(), ldt)
  switch (nb) {
    case 1: EPS_WIDE_FWD(1); break;
    case 2: EPS_WIDE_FWD(2); break;
    case 3: EPS_WIDE_FWD(3); break;
    default: EPS_WIDE_FWD(4); break;
  }
#undef EPS_WIDE_FWD
  EPS_HIP(hipGetLastError());
}

void LassoWideReduce(int64_t m, int64_t n, const DVec& table, int first, int nk, uint64_t active, const DVec& T,
                     int64_t ldt) {
  EPS_CHECK(nk >= 1 && nk <= kLassoWidePanel && m % 4 == 0 && ldt % 4 == 0 && ldt >= m);
  const int nslabs = LassoWideSlabs(m, n);
  const int kw = 16 * PanelBlocks(nk);
  EPS_CHECK(T.dt == F32 && T.n >= static_cast<int64_t>(nslabs) * kw * ldt);
  const auto* tab = reinterpret_cast<const LassoBatchInst<float>*>(table.as<char>()) + first;
  const dim3 grid(static_cast<unsigned>((m / 4 + kBlock - 1) / kBlock), static_cast<unsigned>(nk));
  ProfScope prof("wide_reduce", m, n);
  hipLaunchKernelGGL(WideReduceKernel, grid, dim3(kBlock), 0, Runtime::Get().stream(), m, nslabs, kw, tab,
                     static_cast<unsigned long long>(active), T.as<float>(), ldt);
  EPS_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace eps
