// The table does not own read time: every reader does one getenv and caches nothing.  A site that
// reads once per process keeps a `static` around its call; every other site reads where it stands.
//
// Every runtime knob of the library - its EPSILON_HIP_* variable, its eps_set_option key when it
// has one, and for the options with a choice of words those words - is one row of the table in
// options.cc, addressed by the enum below.  Options are stored in the process environment.
#pragma once

#include <cstdint>

namespace eps {
namespace opt {

enum Id {
  kBatchWide,
  kBatchWideMin,
  kBatchZeroTall,
  kBenchRandom,
  kDevice,
  kDistInverse,
  kDtype,
  kForceSharded,
  kFused,
  kFusedBlock,
  kFusedGrid,
  kFusedMatrix,
  kFusedResident,
  kFusedTall,
  kFusedWhiten,
  kFusedZero,
  kFusedZeroCheck,
  kFusedZeroLp,
  kFusedZeroRidge,
  kFusedZeroTall,
  kFusedZeroTallSmooth,
  kFusedZeroXfree,
  kGemm,
  kGemmOrder,
  kGemmSmall,
  kGemmStage,
  kGramF16Split,
  kGraph,
  kHostThreads,
  kInitTrace,
  kPeerWindowMemory,
  kPinnedUpload,
  kPipelineChecks,
  kPotrfTwoKernels,
  kRccl,
  kRefine,
  kSegGrid,
  kShardedApply,
  kSvd,
  kSvdConfirm,
  kSvdInner,
  kSvdMfma,
  kSvdNoV,
  kSvdNsplit,
  kSvdPartial,
  kSvdPartialBackoff,
  kSvdPolar,
  kSvdSmallFast,
  kSvdSort,
  kSvdTrace,
  kSvdVerbose,
  kSvdWarm,
  kSymvPacked,
  kSyrk2d,
  kSyrkTail,
  kNumOptions
};

const char* Raw(Id id);         // the variable's string, null when unset
bool IsSet(Id id);              // set at all
bool Is0(Id id);                // set and begins with '0'
bool Is1(Id id);                // set and begins with '1'
int Int(Id id, int fallback);   // atoi of the variable, `fallback` when unset
// The options with a choice of words: the index of the variable's value (unset: of the row's
// default word) among the row's words; any other value is the error "<key> must be <words>, got
// <value>".
int Word(Id id);

// What eps_set_option does for a key stored in the environment: a value that the row's words (or
// "fused_resident"'s rule) refuse is an error here and leaves the variable alone; "refine" = "auto"
// unsets its variable.  A key without a row is the error "unknown option <key>".
void Set(const char* key, const char* value);

// The knobs that several units read, one parse each.
// "fused_resident": -1 for "auto" (and unset), else the budget in bytes: a number of KiB (decimal
// digits alone) clamped to 2^50; anything else is an error that names the value.
int64_t FusedResident();
int InitTraceLevel();  // EPSILON_HIP_INIT_TRACE: 0 when unset, else its integer
enum SymvPackedMode { kSymvPackedOff, kSymvPackedFirst, kSymvPackedDefault };  // "0", "2", else
SymvPackedMode SymvPacked();
// EPSILON_HIP_DEVICE, else LOCAL_RANK, else `fallback`
int DeviceOrdinal(int fallback);

}  // namespace opt
}  // namespace eps
