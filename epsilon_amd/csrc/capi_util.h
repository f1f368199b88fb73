// What the units of the extern "C" boundary share: capi.cc (the product ABI), capi_test.cc (the
// per-operator test entries) and capi_bench.cc (the micro-benchmarks).
#pragma once

#include "../../include/epsilon_hip.h"

#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "admm.h"
#include "kernels.h"
#include "linear_map.h"
#include "wire.h"

struct eps_result {
  std::string status;
  std::vector<std::string> ids;
  std::vector<eps::HostArray> values;  // not value-initialised, huge pages from 64 MB
};

struct eps_solver {
  std::shared_ptr<eps::DataMap> data;
  std::unique_ptr<eps::Solver> solver;
  eps::DType dtype;
};

namespace eps {
namespace capi {

// capi.cc: the one thread-local string behind eps_last_error
void ClearLastError();
void SetLastError(const char* what);

template <class F> int Guard(F f) {
  try {
    ClearLastError();
    f();
    return 0;
  } catch (const std::exception& e) {
    SetLastError(e.what());
  } catch (...) {
    SetLastError("unknown error");
  }
  // leave no half-finished GPU work behind
  (void)hipGetLastError();
  return 1;
}

// capi.cc: the "dtype" option of eps_set_option, else EPSILON_HIP_DTYPE, else f32
DType ConfiguredDType();

// capi.cc.  own_host: copy host blobs (solver handles outlive the call that passes them; the
// one-shot entry points read the caller's memory in place, it is theirs for the duration of the call).
std::shared_ptr<DataMap> MakeDataMap(const eps_blob* data, size_t ndata, DType dt, bool own_host = false);

inline LinearMap ParseMap(const void* bytes, size_t len, DataMap* dm) {
  pb::LinearMap p = pb::ParseLinearMap(bytes, len);
  return BuildLinearMap(p, dm);
}

// capi_bench.cc.  Deterministic non-trivial fill: v[i] = scale * (((i * 2654435761) mod 1024) / 1024 - 0.5)
DVec Synthetic(int64_t n, DType dt, double scale);

// The symmetric positive definite n x n matrix of the factor benchmarks and tests: G G^T / n + I
// of the synthetic fill G.
inline DVec SpdTestMatrix(int64_t n, DType dt) {
  DVec G = Synthetic(n * n, dt, 1.0);
  DVec W0 = DVec::Zeros(n * n, dt);
  k::Gemm(false, true, n, n, n, 1.0 / n, G, n, G, n, 0.0, W0, n, false);
  k::AddDiag(W0, n, n, 1.0, nullptr);
  return W0;
}

}  // namespace capi
}  // namespace eps
