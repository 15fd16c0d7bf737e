// Host-only: the calibration record of the guarded selection (include/adanerf_hip.h: adanerf_guard_calibration_file) -- the measured
// error bounds of the plain-fp16 sampling pass, kept beside the model (or under $ADANERF_GUARD_CACHE_DIR) so that a context need not
// measure them again.
#pragma once
#include <cstdint>
#include <string>

namespace adanerf {

// what a record belongs to: a record whose key line differs is somebody else's
struct GuardKey {
  uint64_t model_hash = 0;       // fnv1a64_file(model0.onnx)
  int fp = 0, fd = 0;            // posEncArgs[0]
  int transform = 0;             // kOracle*
  int engine_rev = 0;            // kGuardEngineRev (k_sampling16.hip.hpp)
  int num_samples = 0;
  float threshold = 0.f;
  std::string model_dir;
  int32_t flags = 0;             // adanerf_options::flags: ADANERF_FLAG_NO_GUARD_CACHE neither reads nor writes a record
};

struct GuardRecord {
  int poses = 0;
  uint32_t seed = 0;
  float max_diff = 0.f, max_pair = 0.f;
};

uint64_t fnv1a64_file(const std::string& path);      // FNV-1a 64 of a file's bytes, never 0; 0: unreadable
std::string hex64(uint64_t v);
std::string guard_record_path(const GuardKey& k);
bool read_guard_record(const GuardKey& k, GuardRecord* r);      // false: no record, not this key's, or malformed
// best effort: a read-only model directory simply keeps being calibrated at start-up (or use ADANERF_GUARD_CACHE_DIR)
void write_guard_record(const GuardKey& k, const GuardRecord& r);

}  // namespace adanerf
