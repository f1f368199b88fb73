// extern "C" boundary, the micro-benchmarks: the eps_bench_* entries of include/epsilon_hip.h.
// They return times, measured between two events on the library's stream.
#include <algorithm>
#include <cmath>

#include "capi_util.h"
#include "options.h"

using namespace eps;
using namespace eps::capi;

DVec eps::capi::Synthetic(int64_t n, DType dt, double scale) {
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

namespace {

// The milliseconds f() takes on the library's stream, between two events that are destroyed on
// every path out, a throw of f included.
template <class F> float TimedMs(F f) {
  struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } ev;
  hipStream_t stream = Runtime::Get().stream();
  EPS_HIP(hipEventCreate(&ev.a));
  EPS_HIP(hipEventCreate(&ev.b));
  EPS_HIP(hipEventRecord(ev.a, stream));
  f();
  EPS_HIP(hipEventRecord(ev.b, stream));
  EPS_HIP(hipEventSynchronize(ev.b));
  float ms = 0;
  EPS_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
  return ms;
}

// two untimed calls, then the average of iters calls timed together
template <class F> double TimeLaunches(int iters, F f) {
  for (int i = 0; i < 2; ++i) f();
  return TimedMs([&] {
    for (int i = 0; i < iters; ++i) f();
  }) / iters;
}

// For a call that consumes its input: iters + 1 rounds of reset(), a sync and one timed f(); the
// mean of all rounds but the first.
template <class R, class F> double TimeWithReset(int iters, R reset, F f) {
  Runtime& rt = Runtime::Get();
  double total = 0;
  for (int i = 0; i < iters + 1; ++i) {
    reset();
    rt.Sync();
    const float e = TimedMs(f);
    if (i > 0) total += e;
  }
  return total / iters;
}

// one cold or warm-started decomposition of the m x n matrix in W, timed from an idle stream
void TimedJacobiSvd(const DVec& W, int64_t m, int64_t n, const DVec& V, int max_sweeps, bool warm, double* ms,
                    int* sweeps) {
  Runtime::Get().Sync();
  int sw = 0;
  *ms = TimedMs([&] { sw = k::JacobiSvd(W, m, n, V, max_sweeps, warm, false); });
  if (sweeps) *sweeps = sw;
}

// a borrowed device buffer, or bytes of the synthetic fill held by *own
const void* StreamSource(const void* device_ptr, size_t bytes, DVec* own) {
  if (device_ptr == nullptr) {
    *own = Synthetic(static_cast<int64_t>(bytes / 4), F32, 1.0);
    device_ptr = own->data();
  }
  EPS_HIP(hipDeviceSynchronize());  // a borrowed pointer may still be written by another stream
  return device_ptr;
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
    Runtime::Get();
    DVec own;
    const void* src = StreamSource(device_ptr, bytes, &own);
    DVec dst;
    if (mode == 2) dst = DVec::Empty(static_cast<int64_t>(bytes / 4), F32);
    if (grid <= 0) grid = 2048;
    DVec scratch = DVec::Empty(grid, F32);
    *ms_avg = TimeLaunches(iters, [&] {
      k::StreamProbe(mode, src, mode == 2 ? dst.data() : nullptr, static_cast<int64_t>(bytes),
                     scratch.as<float>(), grid);
    });
  });
}

int eps_bench_stream_resident(const void* device_ptr, size_t bytes, size_t resident_bytes, int grid, int iters,
                              double* ms_avg) {
  return Guard([&] {
    const size_t column = 40000;  // k::StreamResidentProbe's
    EPS_CHECK_MSG(bytes >= column && resident_bytes <= bytes && iters >= 1 && ms_avg != nullptr,
                  "eps_bench_stream_resident: bad arguments");
    DVec own;
    const void* src = StreamSource(device_ptr, bytes, &own);
    if (grid <= 0) grid = 2048;
    DVec scratch = DVec::Empty(grid, F32);
    const int64_t per_column = static_cast<int64_t>(resident_bytes / (bytes / column)) / 16 * 16;
    // TimeLaunches' two untimed launches fill the cache: the average is of launches that find it filled
    *ms_avg = TimeLaunches(iters, [&] {
      k::StreamResidentProbe(src, static_cast<int64_t>(bytes), per_column, scratch.as<float>(), grid);
    });
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
    DVec W0 = SpdTestMatrix(n, dt);
    DVec W = DVec::Empty(n * n, dt);
    *ms_avg = TimeWithReset(iters, [&] { k::Copy(W, W0); }, [&] { k::SpdInverseInPlace(W, n); });
  });
}

int eps_bench_spd_inverse_columns(int64_t n, int64_t cnt, int iters, double* ms_avg) {
  return Guard([&] {
    const DType dt = ConfiguredDType();
    DVec W0 = SpdTestMatrix(n, dt);
    DVec W = DVec::Empty(n * n, dt);
    DVec Out = DVec::Empty(n * cnt, dt);
    *ms_avg = TimeWithReset(iters, [&] { k::Copy(W, W0); }, [&] { k::SpdInverseColumns(W, n, 0, cnt, Out); });
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
      lamv = DVec::Full(n, 0.7, dt);
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
    h.resize(static_cast<size_t>(m) * n);  // the sparse part, its values rounded to float
    for (auto& v : h) v = uni() < 0.1 ? static_cast<float>(10.0 * gauss()) : 0.0f;
    DVec Y = DVec::FromHost(h.data(), m * n, dt);
    if (rank > 0) k::Gemm(false, true, m, n, rank, 1.0, A, m, B, n, 1.0, Y, m);
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
    TimedJacobiSvd(W, m, n, V, max_sweeps, false, ms_cold, sweeps_cold);
    if (defects) measure(Y, W, V, defects);
    if (ms_warm != nullptr && perturb >= 0) {
      // a nearby matrix, as the next ADMM sweep would present: Y2 = Y + perturb * (scaled fill)
      DVec Y2 = Y.Clone();
      DVec N = Synthetic(m * n, dt, 1.0);
      k::Axpby(Y2, perturb, N, 1.0);
      DVec W2 = DVec::Empty(m * n, dt);
      k::Gemm(false, false, m, n, n, 1.0, Y2, m, V, n, 0.0, W2, m);
      TimedJacobiSvd(W2, m, n, V, max_sweeps, true, ms_warm, sweeps_warm);
      if (defects) measure(Y2, W2, V, defects + 3);
    }
  });
}

int eps_bench_svd_device(const void* y_dev, int64_t m, int64_t n, int max_sweeps, double* ms, int* sweeps) {
  return Guard([&] {
    EPS_CHECK(y_dev != nullptr && m > 0 && n > 0 && ms != nullptr);
    Runtime::Get();
    EPS_HIP(hipDeviceSynchronize());  // the caller's stream may still be writing the matrix
    DVec Y = DVec::Borrow(const_cast<void*>(y_dev), m * n, F32);
    DVec W = Y.Clone();
    DVec V = DVec::Empty(n * n, F32);
    TimedJacobiSvd(W, m, n, V, max_sweeps, false, ms, sweeps);
  });
}

}  // extern "C"
