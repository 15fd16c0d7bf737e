#include "guard_record.hpp"

#include <sys/stat.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/adanerf_hip.h"
#include "format.hpp"      // join_path

namespace adanerf {

uint64_t fnv1a64_file(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return 0;
  uint64_t h = 0xcbf29ce484222325ull;
  unsigned char buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0)
    for (size_t i = 0; i < n; ++i) h = (h ^ buf[i]) * 0x100000001b3ull;
  std::fclose(f);
  return h ? h : 1;
}

std::string hex64(uint64_t v) {
  char b[17];
  std::snprintf(b, sizeof(b), "%016llx", static_cast<unsigned long long>(v));
  return b;
}

static std::string guard_record_dir(const GuardKey& k) {
  const char* env = std::getenv("ADANERF_GUARD_CACHE_DIR");
  if (env && *env) return join_path(env, hex64(k.model_hash));
  return k.model_dir;
}

std::string guard_record_path(const GuardKey& k) {
  uint32_t tb;
  const float thr = k.threshold;
  std::memcpy(&tb, &thr, sizeof(tb));
  char name[64];
  std::snprintf(name, sizeof(name), "guard_band.n%d.t%08x.cal", k.num_samples, tb);
  return join_path(guard_record_dir(k), name);
}

// what a record must agree with to be this key's
static std::string guard_record_key(const GuardKey& k) {
  char b[160];
  std::snprintf(b, sizeof(b), "%s|enc %d-%d|transform %d|engine %d|n %d|thr %.9g", hex64(k.model_hash).c_str(), k.fp, k.fd, k.transform,
                k.engine_rev, k.num_samples, static_cast<double>(k.threshold));
  return b;
}

bool read_guard_record(const GuardKey& k, GuardRecord* r) {
  if (k.flags & ADANERF_FLAG_NO_GUARD_CACHE) return false;
  FILE* f = std::fopen(guard_record_path(k).c_str(), "r");
  if (!f) return false;
  char line[512];
  std::string key;
  bool have[4] = {false, false, false, false};
  while (std::fgets(line, sizeof(line), f)) {
    std::string l(line);
    const size_t eq = l.find('=');
    if (l.empty() || l[0] == '#' || eq == std::string::npos) continue;
    auto trim = [](std::string t) {
      const char* ws = " \t\r\n";
      const size_t a0 = t.find_first_not_of(ws), a1 = t.find_last_not_of(ws);
      return a0 == std::string::npos ? std::string() : t.substr(a0, a1 - a0 + 1);
    };
    const std::string name = trim(l.substr(0, eq)), v = trim(l.substr(eq + 1));
    if (name == "key") key = v;
    else if (name == "poses") { r->poses = std::atoi(v.c_str()); have[0] = true; }
    else if (name == "seed") { r->seed = static_cast<uint32_t>(std::strtoul(v.c_str(), nullptr, 10)); have[1] = true; }
    else if (name == "max_diff") { r->max_diff = std::strtof(v.c_str(), nullptr); have[2] = true; }
    else if (name == "max_pair_diff") { r->max_pair = std::strtof(v.c_str(), nullptr); have[3] = true; }
  }
  std::fclose(f);
  return key == guard_record_key(k) && have[0] && have[1] && have[2] && have[3] && r->poses >= 1 && r->max_diff > 0.f &&
         r->max_diff < INFINITY && r->max_pair >= 0.f && r->max_pair < INFINITY;
}

void write_guard_record(const GuardKey& k, const GuardRecord& r) {
  if (k.flags & ADANERF_FLAG_NO_GUARD_CACHE) return;
  const std::string dir = guard_record_dir(k), path = guard_record_path(k), tmp = path + ".tmp";
  if (std::getenv("ADANERF_GUARD_CACHE_DIR")) {
    (void)mkdir(std::getenv("ADANERF_GUARD_CACHE_DIR"), 0777);
    (void)mkdir(dir.c_str(), 0777);
  }
  FILE* f = std::fopen(tmp.c_str(), "w");
  if (!f) return;
  std::fprintf(f,
               "# libadanerf_hip: measured error bounds of the plain-fp16 sampling pass against the split-precision engine\n"
               "# (ADANERF_SAMPLING_GUARDED).  Delete this file to have them measured again.\n"
               "key = %s\nposes = %d\nseed = %u\nmax_diff = %.9g\nmax_pair_diff = %.9g\n",
               guard_record_key(k).c_str(), r.poses, r.seed, static_cast<double>(r.max_diff), static_cast<double>(r.max_pair));
  const bool ok = std::fclose(f) == 0;
  if (!ok || std::rename(tmp.c_str(), path.c_str()) != 0) (void)std::remove(tmp.c_str());
}

}  // namespace adanerf
