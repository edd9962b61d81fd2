// dfx_launch.cpp -- host side shared by the kernel translation units: the built-in profiler (HIP events around tracked launches),
// kernel names, the device's CU count and grid sizing.  No kernel lives here.
#include "dfx_launch.hpp"

#include <mutex>
#include <vector>

namespace dfx {

static const char* kKernelNames[KID_COUNT_] = {
    "predicate_mask", "compact", "project", "reduce_all", "hash_agg", "merge_rows", "rehash",
    "emit_mask", "finalize", "scan", "synth", "fill", "gather_utf8", "partial", "partition", "partition_agg", "csv", "sort",
    "distinct_insert", "distinct_count", "utf8_pred", "utf8_extrema", "csv_write", "parquet", "parquet_inflate", "parquet_write", "parquet_write_lz4"};
const char* kernel_name(int kid) { return (kid >= 0 && kid < KID_COUNT_) ? kKernelNames[kid] : "?"; }

namespace {
struct ProfEntry {
  int64_t launches = 0;
  double total_ms = 0.0;
  double algo_bytes = 0.0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};
std::mutex g_prof_mu;
bool g_prof_on = false;
ProfEntry g_prof[KID_COUNT_];
std::vector<hipEvent_t> g_event_pool;

hipEvent_t get_event() {
  if (!g_event_pool.empty()) {
    hipEvent_t e = g_event_pool.back();
    g_event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

void drain(ProfEntry& p) {
  for (auto& pr : p.pending) {
    float ms = 0.f;
    if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess)
      p.total_ms += (double)ms;
    g_event_pool.push_back(pr.first);
    g_event_pool.push_back(pr.second);
  }
  p.pending.clear();
}

int g_cu_count = 0;
}  // namespace

Scope::Scope(int kid_, hipStream_t s_, double bytes) : kid(kid_), s(s_) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof_on) return;
  a = get_event();
  b = get_event();
  g_prof[kid].launches += 1;
  g_prof[kid].algo_bytes += bytes;
  if (a) (void)hipEventRecord(a, s);
}
Scope::~Scope() {
  if (!a || !b) return;
  (void)hipEventRecord(b, s);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof[kid].pending.emplace_back(a, b);
}

int device_cu_count() {
  if (g_cu_count == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      g_cu_count = prop.multiProcessorCount;
    if (g_cu_count <= 0) g_cu_count = 256;
  }
  return g_cu_count;
}

void profile_enable(bool on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on;
}
void profile_reset() {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& p : g_prof) {
    drain(p);
    p.launches = 0;
    p.total_ms = 0;
    p.algo_bytes = 0;
  }
}
int profile_count() { return KID_COUNT_; }
bool profile_get(int index, const char** name, int64_t* launches, double* total_ms, double* algo_bytes) {
  if (index < 0 || index >= KID_COUNT_) return false;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  drain(g_prof[index]);
  *name = kKernelNames[index];
  *launches = g_prof[index].launches;
  *total_ms = g_prof[index].total_ms;
  *algo_bytes = g_prof[index].algo_bytes;
  return true;
}

// grid for a streaming kernel over `units` block-sized units: enough workgroups to fill 256 CUs
// several times over (>> 256 WGs; blocks land round-robin on the 8 XCDs), capped so the
// grid-stride loop amortises launch and tail effects.
int stream_grid(int64_t units, int per_cu) {
  int64_t cap = (int64_t)device_cu_count() * per_cu;
  if (units < 1) units = 1;
  return (int)(units < cap ? units : cap);
}

}  // namespace dfx
