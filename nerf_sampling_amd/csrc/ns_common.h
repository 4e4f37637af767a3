// Shared host-side helpers for libnerf_sampling_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/nerf_sampling_hip.h"

namespace ns {

void set_error(const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ceil-div on 64-bit sizes
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// what the evaluation entries ask of their sizes and pointers: a count a 32-bit index can hold, R * N in [1, 2^31) (the flat
// element index and its division by N are 32-bit in the kernels), a pointer on a multiple of `a` bytes (a power of two; NULL
// is), and a workspace size rounded up to whole 256-byte lines
inline bool below_2_31(int64_t n) { return n < (int64_t(1) << 31); }
inline bool flat_shape_ok(int64_t R, int N) { return R >= 1 && N >= 1 && R <= ((int64_t(1) << 31) - 1) / N; }
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int64_t round_256(int64_t bytes) { return (bytes + 255) / 256 * 256; }

// grid for grid-stride elementwise kernels: enough blocks to fill 256 CUs x 8, capped
inline int ew_grid(int64_t n, int block) {
  int64_t g = cdiv(n, block);
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return static_cast<int>(g);
}

// diagnostic switches (ns_debug_set; initial values from NS_OB16_GENERIC / NS_OB16_TILES, read once)
struct DebugFlags {
  int generic_kernels;   // 1: the production network runs the generic, compiler-scheduled kernels (tests compare the two)
  int prod_tiles;        // 4 / 5: tiles per wave of the 16-bit production kernel; 0 = chosen per launch
  int hier_chain;        // 1: ns_render_rays_hierarchical keeps raw [R,N,4] in HBM and composites with the stand-alone kernel
  int no_colour_skip;    // 1: launches the render kernel would take (ns_nerf_mlp_ob16.hip) run the production kernel instead
  int count_colour_skips;   // 1: the render kernels count the waves that skipped their colour statements (ns_colour_skip_count)
                            // and the chunk steps the K-block-skipping kernel jumped over (ns_kblock_skip_count)
  int kblock_skip;       // 1: launches of the render kernel run its K-block-skipping twin (off by default: measured no faster)
  int kblock_suffix;     // launches of the render kernel run its dead-suffix twin: 0 never, 1 always, 2 (the initial value) on unit-ordered handles
  int mesh_raster_big_box;  // > 0: ns_mesh_raster hands faces whose clamped bounding box has more pixels than this to its workgroup
                            // launch; 0 = NS_MESH_RASTER_BIG_BOX (the results are the same bits for every value)
};
DebugFlags& debug_flags();
// The render kernels' skip counters for a 16-bit field launch on `stream`: *counter = NULL unless count_colour_skips is set; then
// the current device's three counters (colour-skipping waves, skipped K-block steps, the dead-suffix kernel's absent steps), zeroed on `stream` ahead of the launch (ns_colour_skip_count reads the last launch's value).
int colour_skip_counter(uint32_t** counter, hipStream_t stream);
// Per-thread launch hint of the one-call renderers (ns_render.cpp): 4 = this call's per-sample outputs are about to be
// copied to the host while the NEXT call's MLP kernel runs -- the four-tile production kernel leaves 64+ registers of every
// SIMD free, so the blit kernels ROCm moves pinned device-to-host copies with can run beside it; the five-tile kernel
// (2.5 % faster alone) fills the register file and the copies would wait for the whole persistent grid.  0 = no preference.
int& prod_tiles_hint();

int cu_count();
hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes);

// The launch rule of the persistent MLP kernels.  launch_plan refuses more dynamic LDS than a CU's 160 KiB (NS_E_UNSUPPORTED),
// raises the kernel's limit to `lds` and sizes the grid: one workgroup per unit of `work` (groups, or runs of groups), at most
// one per CU (256 when the CU count is unknown).  `who` names the entry point in the error string.
int launch_plan(const char* who, const void* kernel, size_t lds, int64_t work, int* grid);
template <class Args>
int launch_persistent(const char* who, void (*kernel)(Args), const Args& a, int threads, size_t lds, int64_t work,
                      hipStream_t stream) {
  int grid = 0;
  const int rc = launch_plan(who, reinterpret_cast<const void*>(kernel), lds, work, &grid);
  if (rc != NS_OK) return rc;
  kernel<<<grid, threads, lds, stream>>>(a);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return NS_OK;
  set_error("%s: launch -> %s", who, hipGetErrorString(e));
  return NS_E_HIP;
}

}  // namespace ns

// internal (not part of the public header)
extern "C" int ns_coarse_z_scalar(float near_, float far_, int64_t R, int N, int lindisp, const float* t_rand_dev,
                                  float* z_dev, void* stream);

#define NS_REQUIRE(cond, msg)                    \
  do {                                           \
    if (!(cond)) {                               \
      ns::set_error("%s: %s", __func__, msg);    \
      return NS_E_INVALID;                       \
    }                                            \
  } while (0)

#define NS_HIP(call)                                                           \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) {                                                    \
      ns::set_error("%s: %s -> %s", __func__, #call, hipGetErrorString(e_));   \
      return NS_E_HIP;                                                         \
    }                                                                          \
  } while (0)

#define NS_LAUNCH_CHECK()                                                      \
  do {                                                                         \
    hipError_t e_ = hipGetLastError();                                         \
    if (e_ != hipSuccess) {                                                    \
      ns::set_error("%s: launch -> %s", __func__, hipGetErrorString(e_));      \
      return NS_E_HIP;                                                         \
    }                                                                          \
  } while (0)
