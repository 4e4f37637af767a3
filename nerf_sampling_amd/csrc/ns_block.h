// Workgroup primitives of the device evaluation kernels (ns_cloud, ns_mesh, ns_mesh_components, ns_mesh_normals, the scoring kernels of ns_rays,
// ns_map_max): device-side helpers only -- no kernel, no host state.  Each is called by ALL kBlock threads of a workgroup of kWaves
// 64-lane waves and fixes the order of everything it adds: a result is a function of the inputs alone, never of CU count or timing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns {

constexpr int kBlock = 256;                  // threads per workgroup
constexpr int kWaves = kBlock / 64;

// A share is the run of SHARE consecutive items one workgroup owns (the NS_*_SHARE macros of the public header): thread t takes
// items j * kBlock + t of it, j = 0 .. steps - 1, so consecutive lanes touch consecutive items and the order of the items of a
// share is (step, wave, lane).
template <int SHARE>
struct ShareOf {
  static_assert(SHARE > 0 && SHARE % kBlock == 0, "a whole number of items per thread");
  static constexpr int steps = SHARE / kBlock;
};

// The sum of v over the workgroup, returned to every thread.  THE ORDER IS PART OF THE CONTRACT for double: the lanes of a wave
// combine by the xor tree with offsets 32, 16, .. 1, lane 0 of each wave stores to slots[wave], one barrier, and the result is
// slots[0] + slots[1] + ... in wave order -- the tests of the sqerr, SSIM and depth sums restate exactly this order in numpy and
// compare bit for bit.  `slots`: kWaves values of LDS; a second call needs other slots, or a barrier after the first.
template <class T>
__device__ __forceinline__ void wave_sum_to(T v, T* slots) {        // the part before the barrier: slots[wave] = the wave's sum
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
}

template <class T>
__device__ __forceinline__ void wave_sum_to(T a, T* slots_a, T b, T* slots_b) {   // two values at once, their trees interleaved
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    slots_a[threadIdx.x >> 6] = a;
    slots_b[threadIdx.x >> 6] = b;
  }
}

template <class T>
__device__ __forceinline__ T slots_sum(const T* slots) {            // the part behind it: slots[0] + slots[1] + ... in order
  T s = slots[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s += slots[w];
  return s;
}

template <class T>
__device__ __forceinline__ T block_sum(T v, T* slots) {
  wave_sum_to(v, slots);
  __syncthreads();
  return slots_sum(slots);
}

// The exclusive scan of the per-share counts by ONE workgroup, in place: counts[g] <- carry0 + counts[0] + ... + counts[g - 1];
// returns carry0 + the sum of all, to every thread.  The workgroup walks tiles of kScanTile entries: thread t owns kScanPer
// consecutive ones, the lanes of a wave are scanned with shuffles, the waves through LDS (two buffers in turn, so one barrier per
// tile), the tiles by a running carry every thread keeps.  visit(g, in_range) is called beside the load of entry g by the thread
// that owns it, so a second total can ride along (the mesh's skipped cells) without a pass of its own; in_range is false for the
// last tile's slots beyond `groups`: a load written `in_range ? p[g] : 0` stays a select, so a tile's loads are in flight together.
constexpr int kScanPer = 8;
constexpr int kScanTile = kBlock * kScanPer;

template <class Visit>
__device__ __forceinline__ int64_t share_scan(int64_t* __restrict__ counts, int groups, int64_t carry0, Visit visit) {
  __shared__ int64_t wave_totals[2][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = carry0;
  int buf = 0;
  for (int tile0 = 0; tile0 < groups; tile0 += kScanTile, buf ^= 1) {
    const int first = tile0 + static_cast<int>(threadIdx.x) * kScanPer;
    int64_t v[kScanPer];
    int64_t mine = 0;
#pragma unroll
    for (int i = 0; i < kScanPer; ++i) {
      v[i] = first + i < groups ? counts[first + i] : 0;
      mine += v[i];
      visit(first + i, first + i < groups);
    }
    int64_t incl = mine;                                   // inclusive scan over the lanes of the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wave_totals[buf][wave] = incl;
    __syncthreads();
    int64_t before = carry, tile_total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w == wave) before += tile_total;
      tile_total += wave_totals[buf][w];
    }
    int64_t run = before + (incl - mine);
#pragma unroll
    for (int i = 0; i < kScanPer; ++i) {
      if (first + i < groups) counts[first + i] = run;
      run += v[i];
    }
    carry += tile_total;
  }
  return carry;
}

__device__ __forceinline__ int64_t share_scan(int64_t* __restrict__ counts, int groups, int64_t carry0) {
  return share_scan(counts, groups, carry0, [](int, bool) {});
}

// The wave's part of share_place: the sum of n over the lanes below this one, the wave's total left in *wave_total.  For a 0/1
// count a ballot and two popcounts; for any other an inclusive shuffle scan (the ballot form is the cheaper: keep it for flags).
__device__ __forceinline__ int wave_place(bool n, int* wave_total) {
  const int lane = threadIdx.x & 63;
  const unsigned long long mask = __ballot(n);
  if (lane == 0) *wave_total = __popcll(mask);
  return __popcll(mask & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ int wave_place(int n, int* wave_total) {
  const int lane = threadIdx.x & 63;
  int incl = n;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) *wave_total = incl;
  return incl - n;
}

// Placement inside a share: n_of(j) is the number of records this thread's item of step j emits -- a bool for 0 or 1 (the ballot
// form of wave_place), an int otherwise (the shuffle form) -- and emit(j, at) is called for j = 0 .. STEPS - 1 with `at` the
// number of records the share emits before them in the order (step, wave, lane): the earlier (step, wave) cells through
// cell_counts in LDS, the lanes below by wave_place.  n_of is called once per step, in order, before the one barrier.
template <int STEPS, class Count, class Emit>
__device__ __forceinline__ void share_place(Count n_of, int (*cell_counts)[kWaves], Emit emit) {
  const int wave = threadIdx.x >> 6;
  int below[STEPS];
#pragma unroll
  for (int j = 0; j < STEPS; ++j) below[j] = wave_place(n_of(j), &cell_counts[j][wave]);
  __syncthreads();
  int cells_before = 0;
#pragma unroll
  for (int j = 0; j < STEPS; ++j) {
    int mine = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w == wave) mine = cells_before;
      cells_before += cell_counts[j][w];
    }
    emit(j, mine + below[j]);
  }
}

}  // namespace ns
