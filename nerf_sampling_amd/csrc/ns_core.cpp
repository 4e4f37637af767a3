// Error string, version and device queries of libnerf_sampling_hip.so.
#include "ns_common.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

namespace ns {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// per-device caches (a process may drive several GPUs; round-1 code cached the first device's answer)
static std::mutex g_mu;
static std::map<int, int> g_cus;
static std::map<std::pair<const void*, int>, size_t> g_dyn_lds;

int cu_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_cus.find(dev);
  if (it != g_cus.end()) return it->second;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  g_cus[dev] = prop.multiProcessorCount;
  return prop.multiProcessorCount;
}

// hipFuncAttributeMaxDynamicSharedMemorySize for `kernel` on the CURRENT device, raised whenever a launch needs more
// than any earlier one did (the LDS size of the MLP kernels grows with the network depth through the bias image)
hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_mu);
  size_t& have = g_dyn_lds[std::make_pair(kernel, dev)];
  if (bytes <= have) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
  if (e == hipSuccess) have = bytes;
  return e;
}

int launch_plan(const char* who, const void* kernel, size_t lds, int64_t work, int* grid) {
  if (lds > 160 * 1024) {
    set_error("%s: %zu bytes of LDS needed (too deep a network for the resident bias image)", who, lds);
    return NS_E_UNSUPPORTED;
  }
  const hipError_t e = ensure_dynamic_lds(kernel, lds);
  if (e != hipSuccess) {
    set_error("%s: dynamic LDS limit of %zu bytes -> %s", who, lds, hipGetErrorString(e));
    return NS_E_HIP;
  }
  int cus = cu_count();
  if (cus <= 0) cus = 256;
  *grid = static_cast<int>(work < cus ? work : cus);
  return NS_OK;
}

// Diagnostic switches: read from the environment ONCE (first use), changed afterwards only through ns_debug_set -- no
// getenv on the launch path.
// the dead-suffix render kernel's initial switch: 2 (unit-ordered handles) -- a measured gain by DESIGN section 6's rule
// (profiles/r07_kblock_suffix.log); a handle packed in its trained order runs the render kernel as before
constexpr int kKblockSuffixDefault = 2;
static int kblock_suffix_initial() {
  const char* v = std::getenv("NS_KBLOCK_SUFFIX");
  return (v && v[0] >= '0' && v[0] <= '2') ? v[0] - '0' : kKblockSuffixDefault;
}
DebugFlags& debug_flags() {
  static DebugFlags f = [] {
    DebugFlags d{};
    const char* v = std::getenv("NS_OB16_GENERIC");
    d.generic_kernels = (v && v[0] == '1') ? 1 : 0;
    v = std::getenv("NS_OB16_TILES");
    d.prod_tiles = (v && (v[0] == '4' || v[0] == '5')) ? v[0] - '0' : 0;
    v = std::getenv("NS_KBLOCK_SKIP");
    d.kblock_skip = (v && v[0] == '1') ? 1 : 0;
    v = std::getenv("NS_KBLOCK_SUFFIX");
    d.kblock_suffix = kblock_suffix_initial();
    return d;
  }();
  return f;
}

// The render kernels' skip counters: a diagnostic (ns_debug_set("count_colour_skips", 1)), three uint32 per device -- [0] the waves that
// skipped their colour statements, [1] the chunk steps whose MFMAs the K-block-skipping kernel jumped over, [2] the chunk steps absent
// from the bodies the dead-suffix kernel's waves ran, summed over waves.  Allocated with
// hipMalloc by the first counted launch on a device and kept for the life of the process (four bytes, never freed); neither
// the allocation nor the host read-back in ns_colour_skip_count belongs in a stream capture -- do not set the switch while capturing.
static std::map<int, uint32_t*> g_skip_counters;
static uint32_t* skip_counter_of_device(bool create) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_skip_counters.find(dev);
  if (it != g_skip_counters.end()) return it->second;
  if (!create) return nullptr;
  uint32_t* p = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&p), 3 * sizeof(uint32_t)) != hipSuccess) return nullptr;
  g_skip_counters[dev] = p;
  return p;
}
int colour_skip_counter(uint32_t** counter, hipStream_t stream) {
  *counter = nullptr;
  if (!debug_flags().count_colour_skips) return NS_OK;
  uint32_t* p = skip_counter_of_device(true);
  if (!p) { set_error("colour_skip_counter: no device memory for the counter"); return NS_E_HIP; }
  NS_HIP(hipMemsetAsync(p, 0, 3 * sizeof(uint32_t), stream));
  *counter = p;
  return NS_OK;
}

int& prod_tiles_hint() {
  static thread_local int hint = 0;
  return hint;
}

}  // namespace ns

extern "C" {
const char* ns_last_error(void) { return ns::g_err; }
int ns_debug_set(const char* name, int value) {
  if (!name) { ns::set_error("ns_debug_set: null name"); return NS_E_INVALID; }
  ns::DebugFlags& f = ns::debug_flags();
  if (!std::strcmp(name, "generic_kernels")) { f.generic_kernels = value ? 1 : 0; return NS_OK; }
  if (!std::strcmp(name, "hier_chain")) { f.hier_chain = value ? 1 : 0; return NS_OK; }
  if (!std::strcmp(name, "no_colour_skip")) { f.no_colour_skip = value ? 1 : 0; return NS_OK; }
  if (!std::strcmp(name, "kblock_skip")) { f.kblock_skip = value ? 1 : 0; return NS_OK; }
  if (!std::strcmp(name, "kblock_suffix") && value >= -1 && value <= 2) {   // -1: back to the initial value
    f.kblock_suffix = value < 0 ? ns::kblock_suffix_initial() : value;
    return NS_OK;
  }
  if (!std::strcmp(name, "mesh_raster_big_box") && value >= 0) { f.mesh_raster_big_box = value; return NS_OK; }
  if (!std::strcmp(name, "count_colour_skips")) { f.count_colour_skips = value ? 1 : 0; return NS_OK; }
  if (!std::strcmp(name, "prod_tiles") && (value == 0 || value == 4 || value == 5)) { f.prod_tiles = value; return NS_OK; }
  ns::set_error("ns_debug_set: unknown switch or value (%s = %d)", name, value);
  return NS_E_INVALID;
}
static int read_skip_counter(int which, int64_t* out) {
  NS_REQUIRE(out, "null pointer");
  *out = 0;
  uint32_t* p = ns::skip_counter_of_device(false);
  if (!p) return NS_OK;   // no counted launch on this device yet
  uint32_t v = 0;
  NS_HIP(hipDeviceSynchronize());
  NS_HIP(hipMemcpy(&v, p + which, sizeof(v), hipMemcpyDeviceToHost));
  *out = v;
  return NS_OK;
}
int ns_colour_skip_count(int64_t* waves_out) { return read_skip_counter(0, waves_out); }
int ns_kblock_skip_count(int64_t* steps_out) { return read_skip_counter(1, steps_out); }
int ns_kblock_suffix_count(int64_t* steps_out) { return read_skip_counter(2, steps_out); }
int ns_version(void) { return 1; }
int ns_device_cu_count(void) { return ns::cu_count(); }
}
