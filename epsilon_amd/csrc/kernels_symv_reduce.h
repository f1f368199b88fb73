// The fixed-order sum of the symmetric apply's tile partials (kernels_gemv.hip: SymvTileKernel
// writes them, SymvReduceKernel adds them), shared with the kernel that consumes the sum in
// registers instead of storing it (kernels_fused_tall.hip).  One statement of the order, so both
// give the same bits; the sum is additions alone and `alpha * tot` one product, which no
// contraction setting can change.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace eps {
namespace k {
namespace {

constexpr int kSB = 128;  // the tile's edge; a reducing workgroup has 2 * kSB threads

// tot = sum_{J <= I} prow[(I,J)][off] + sum_{I' > I} pcol[(I',I)][off] for the thread's entry
// `off` of block I.  One workgroup of 256 threads per block of 128 rows; the nb partial vectors of
// a block are dealt to two half-workgroups (even / odd position in the list), loaded eight at a
// time, and the two halves are added in a fixed order.  Every thread of the workgroup must call
// (one __syncthreads); true for the threads (the first half) that hold the total.
template <class T>
__device__ inline bool SymvBlockSum(int64_t nb, const T* __restrict__ prow, const T* __restrict__ pcol, int64_t I,
                                    T* tot) {
  __shared__ T half[kSB];
  const int off = threadIdx.x & (kSB - 1), grp = threadIdx.x >> 7;  // kSB == 128
  const int64_t base = I * (I + 1) / 2;
  auto part = [&](int64_t p) -> const T* {  // p-th partial vector of this block, p < nb
    return p <= I ? prow + (base + p) * kSB : pcol + (p * (p + 1) / 2 + I) * kSB;
  };
  T s = T(0);
  int64_t p = grp;
  for (; p + 14 < nb; p += 16) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part(p + 2 * u)[off];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; p < nb; p += 2) s += part(p)[off];
  if (grp == 1) half[off] = s;
  __syncthreads();
  if (grp != 0) return false;
  *tot = s + half[off];
  return true;
}

// y[r] = alpha * tot + beta * y[r] for the rows of block I.
template <class T>
__device__ inline void SymvReduceBody(int64_t n, int64_t nb, const T* __restrict__ prow,
                                      const T* __restrict__ pcol, T alpha, T beta, T* y, int64_t I) {
  T tot;
  const bool mine = SymvBlockSum<T>(nb, prow, pcol, I, &tot);
  const int64_t r = I * kSB + (threadIdx.x & (kSB - 1));
  if (mine && r < n) y[r] = (beta == T(0)) ? alpha * tot : alpha * tot + beta * y[r];
}

}  // namespace
}  // namespace k
}  // namespace eps
