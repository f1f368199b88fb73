// The option table and its readers (options.h).  This unit alone touches the process environment.
#include "options.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "common.h"

namespace eps {
namespace opt {
namespace {

// One row per variable, in the order of `Id`: the eps_set_option key (null: none), and for the
// options with a choice of words the words in the order of their indices and the word that holds
// while the variable is unset.  What each knob does is told in README.md and epsilon_hip.h.
const struct Option {
  Id id;
  const char *env, *key, *words[5], *unset;
} kOptions[] = {
    {kBatchWide, "EPSILON_HIP_BATCH_WIDE", "batch_wide", {"0", "1"}, "0"},
    {kBatchWideMin, "EPSILON_HIP_BATCH_WIDE_MIN"},
    {kBatchZeroTall, "EPSILON_HIP_BATCH_ZERO_TALL", "batch_zero_tall", {"0", "1"}, "0"},
    {kBenchRandom, "EPSILON_HIP_BENCH_RANDOM"},
    {kDevice, "EPSILON_HIP_DEVICE", "device"},
    {kDistInverse, "EPSILON_HIP_DIST_INVERSE"},
    {kDtype, "EPSILON_HIP_DTYPE"},  // ("dtype" sets a process global, capi.cc)
    {kForceSharded, "EPSILON_HIP_FORCE_SHARDED"},
    {kFused, "EPSILON_HIP_FUSED", "fused"},
    {kFusedBlock, "EPSILON_HIP_FUSED_BLOCK"},
    {kFusedGrid, "EPSILON_HIP_FUSED_GRID"},
    {kFusedMatrix, "EPSILON_HIP_FUSED_MATRIX", "fused_matrix", {"0", "pass", "wide", "auto"}, "auto"},
    {kFusedResident, "EPSILON_HIP_FUSED_RESIDENT_KB", "fused_resident"},
    {kFusedTall, "EPSILON_HIP_FUSED_TALL", "fused_tall", {"0", "1", "auto"}, "auto"},
    {kFusedWhiten, "EPSILON_HIP_FUSED_WHITEN"},
    {kFusedZero, "EPSILON_HIP_FUSED_ZERO", "fused_zero", {"0", "auto"}, "auto"},
    {kFusedZeroCheck, "EPSILON_HIP_FUSED_ZERO_CHECK", "fused_zero_check", {"0", "1"}, "0"},
    {kFusedZeroLp, "EPSILON_HIP_FUSED_ZERO_LP", "fused_zero_lp", {"0", "1"}, "0"},
    {kFusedZeroRidge, "EPSILON_HIP_FUSED_ZERO_RIDGE", "fused_zero_ridge", {"0", "1", "auto"}, "auto"},
    {kFusedZeroTall, "EPSILON_HIP_FUSED_ZERO_TALL", "fused_zero_tall", {"0", "1", "auto"}, "auto"},
    {kFusedZeroTallSmooth, "EPSILON_HIP_FUSED_ZERO_TALL_SMOOTH", "fused_zero_tall_smooth", {"0", "1", "auto"}, "auto"},
    {kFusedZeroXfree, "EPSILON_HIP_FUSED_ZERO_XFREE", "fused_zero_xfree", {"0", "1"}, "0"},
    {kGemm, "EPSILON_HIP_GEMM", "gemm"},
    {kGemmOrder, "EPSILON_HIP_GEMM_ORDER"},
    {kGemmSmall, "EPSILON_HIP_GEMM_SMALL"},
    {kGemmStage, "EPSILON_HIP_GEMM_STAGE"},
    {kGramF16Split, "EPSILON_HIP_GRAM_F16SPLIT"},
    {kGraph, "EPSILON_HIP_GRAPH"},
    {kHostThreads, "EPSILON_HIP_HOST_THREADS"},
    {kInitTrace, "EPSILON_HIP_INIT_TRACE"},
    {kPeerWindowMemory, "EPSILON_HIP_PEER_WINDOW_MEMORY"},
    {kPinnedUpload, "EPSILON_HIP_PINNED_UPLOAD"},
    {kPipelineChecks, "EPSILON_HIP_PIPELINE_CHECKS"},
    {kPotrfTwoKernels, "EPSILON_HIP_POTRF_TWO_KERNELS"},
    {kRccl, "EPSILON_HIP_RCCL"},
    {kRefine, "EPSILON_HIP_REFINE", "refine"},
    {kSegGrid, "EPSILON_HIP_SEG_GRID"},
    {kShardedApply, "EPSILON_HIP_SHARDED_APPLY"},
    {kSvd, "EPSILON_HIP_SVD"},
    {kSvdConfirm, "EPSILON_HIP_SVD_CONFIRM"},
    {kSvdInner, "EPSILON_HIP_SVD_INNER"},
    {kSvdMfma, "EPSILON_HIP_SVD_MFMA"},
    {kSvdNoV, "EPSILON_HIP_SVD_NO_V"},
    {kSvdNsplit, "EPSILON_HIP_SVD_NSPLIT"},
    {kSvdPartial, "EPSILON_HIP_SVD_PARTIAL"},
    {kSvdPartialBackoff, "EPSILON_HIP_SVD_PARTIAL_BACKOFF"},
    {kSvdPolar, "EPSILON_HIP_SVD_POLAR"},
    {kSvdSmallFast, "EPSILON_HIP_SVD_SMALL_FAST"},
    {kSvdSort, "EPSILON_HIP_SVD_SORT"},
    {kSvdTrace, "EPSILON_HIP_SVD_TRACE"},
    {kSvdVerbose, "EPSILON_HIP_SVD_VERBOSE"},
    {kSvdWarm, "EPSILON_HIP_SVD_WARM"},
    {kSymvPacked, "EPSILON_HIP_SYMV_PACKED"},
    {kSyrk2d, "EPSILON_HIP_SYRK_2D"},
    {kSyrkTail, "EPSILON_HIP_SYRK_TAIL"},
};
static_assert(sizeof(kOptions) / sizeof(kOptions[0]) == kNumOptions, "one row per Id");

const Option& Row(Id id) {
  const Option& o = kOptions[id];
  EPS_CHECK(o.id == id);  // the rows stand in the order of the enum
  return o;
}

// The index of `value` among the row's words, or the error built from them: "0, 1 or auto".
int WordIndex(const Option& o, const char* value) {
  std::string list;
  for (int i = 0; o.words[i] != nullptr; ++i) {
    if (std::strcmp(o.words[i], value) == 0) return i;
    if (i > 0) list += o.words[i + 1] != nullptr ? ", " : " or ";
    list += o.words[i];
  }
  EPS_FATAL(o.key << " must be " << list << ", got " << value);
}

int64_t ParseFusedResident(const char* value) {
  if (std::strcmp(value, "auto") == 0) return -1;
  const int64_t cap = int64_t(1) << 40;  // KiB: far beyond any matrix, and kb * 1024 cannot overflow
  int64_t kb = 0;
  bool ok = value[0] != '\0';
  for (const char* c = value; ok && *c != '\0'; ++c) {
    ok = *c >= '0' && *c <= '9';
    if (ok) kb = std::min(cap, kb * 10 + (*c - '0'));
  }
  if (!ok) EPS_FATAL("fused_resident must be auto or a number of KiB, got " << value);
  return kb * 1024;
}

}  // namespace

const char* Raw(Id id) { return std::getenv(Row(id).env); }

bool IsSet(Id id) { return Raw(id) != nullptr; }

bool Is0(Id id) {
  const char* e = Raw(id);
  return e != nullptr && e[0] == '0';
}

bool Is1(Id id) {
  const char* e = Raw(id);
  return e != nullptr && e[0] == '1';
}

int Int(Id id, int fallback) {
  const char* e = Raw(id);
  return e != nullptr ? std::atoi(e) : fallback;
}

int Word(Id id) {
  const Option& o = Row(id);
  EPS_CHECK(o.words[0] != nullptr);
  const char* e = std::getenv(o.env);
  return WordIndex(o, e != nullptr ? e : o.unset);
}

void Set(const char* key, const char* value) {
  for (const Option& o : kOptions) {
    if (o.key == nullptr || std::strcmp(o.key, key) != 0) continue;
    if (o.words[0] != nullptr) (void)WordIndex(o, value);
    if (o.id == kFusedResident) (void)ParseFusedResident(value);
    if (o.id == kRefine && std::strcmp(value, "auto") == 0) unsetenv(o.env);
    else setenv(o.env, value, 1);
    return;
  }
  EPS_FATAL("unknown option " << key);
}

int64_t FusedResident() {
  const char* e = Raw(kFusedResident);
  return e == nullptr ? -1 : ParseFusedResident(e);
}

int InitTraceLevel() { return Int(kInitTrace, 0); }

SymvPackedMode SymvPacked() {
  const char* e = Raw(kSymvPacked);
  if (e != nullptr && e[0] == '0') return kSymvPackedOff;
  if (e != nullptr && e[0] == '2') return kSymvPackedFirst;
  return kSymvPackedDefault;
}

int DeviceOrdinal(int fallback) {
  const char* e = Raw(kDevice);
  if (e == nullptr) e = std::getenv("LOCAL_RANK");
  return e != nullptr ? std::atoi(e) : fallback;
}

}  // namespace opt
}  // namespace eps
