// The scene's point cloud on the device (ns_cloud_append): an ordered stream compaction of the samples whose compositing weight
// passes a threshold.  fp32, HBM-bound.  Built with -ffp-contract=off like ns_rays.hip: a kept point is o + d * z with the
// multiply and the add rounded separately, the bits of ns_points_along_rays.
//
// The flat element e = r * N + k is kept iff w[r, k] >= min_weight (a NaN weight is dropped, -0.0 >= 0.0 keeps).  Workgroup g owns
// elements [g * kShare, (g + 1) * kShare); thread t takes g * kShare + j * kBlock + t, j = 0 .. kSteps - 1 (consecutive lanes
// read consecutive floats of a packed row), so within a share the order of e is (j, wave, lane).  Three launches on one stream:
//   count    workgroup g -> counts[g], the number of kept elements of its share;
//   scan     ONE workgroup turns counts[] into absolute record indices in place -- counts[g] = *count + the kept elements of
//            shares 0 .. g - 1 -- and adds the total to *count;
//   scatter  every workgroup evaluates the predicate again and places a kept element at counts[g] + the kept elements of the
//            earlier (j, wave) cells of its share (through LDS) + the kept lanes below it (__ballot, a 64-bit mask, and a popcount).
// No atomics and nothing that waits on another workgroup's memory: a launch boundary is the only ordering between workgroups, so
// the record order depends on the weights alone.
#include "ns_block.h"
#include "ns_common.h"

namespace {

using ns::kBlock;
using ns::kWaves;
constexpr int kShare = NS_CLOUD_SHARE;
constexpr int kSteps = ns::ShareOf<kShare>::steps;

// the predicate: utils.py:36-43 get_min_indices, weights >= min_weight
__device__ __forceinline__ bool cloud_keeps(float w, float min_weight) { return w >= min_weight; }

// the weights of this thread's kSteps elements and bit j of the result set iff element j is in range and kept
__device__ __forceinline__ uint32_t cloud_load(const float* __restrict__ w, int64_t stride, uint32_t total, uint32_t N,
                                               float min_weight, float wv[kSteps]) {
  const uint32_t base = blockIdx.x * static_cast<uint32_t>(kShare) + threadIdx.x;   // below 2^31 + kShare
  uint32_t kept = 0;
#pragma unroll
  for (int j = 0; j < kSteps; ++j) {
    const uint32_t e = base + j * kBlock;
    wv[j] = 0.0f;
    if (e < total) {
      const uint32_t r = e / N, k = e - r * N;
      wv[j] = w[static_cast<int64_t>(r) * stride + k];
      if (cloud_keeps(wv[j], min_weight)) kept |= 1u << j;
    }
  }
  return kept;
}

__global__ void __launch_bounds__(kBlock)
cloud_count_kernel(const float* __restrict__ w, int64_t stride, uint32_t total, uint32_t N, float min_weight,
                   int64_t* __restrict__ counts) {
  __shared__ int wave_counts[kWaves];
  float wv[kSteps];
  const int n = ns::block_sum<int>(__popc(cloud_load(w, stride, total, N, min_weight, wv)), wave_counts);
  if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// counts[g] <- *count + counts[0] + ... + counts[g - 1]; *count += the sum of all (ns::share_scan, one workgroup)
__global__ void __launch_bounds__(kBlock)
cloud_scan_kernel(int64_t* __restrict__ counts, int groups, int64_t* __restrict__ count) {
  const int64_t total = ns::share_scan(counts, groups, *count);
  __syncthreads();                                         // every thread has read *count
  if (threadIdx.x == 0) *count = total;
}

__global__ void __launch_bounds__(kBlock)
cloud_scatter_kernel(const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ z, int64_t z_stride,
                     const float* __restrict__ w, int64_t w_stride, const float* __restrict__ rgb, int64_t rgb_stride,
                     uint32_t total, uint32_t N, float min_weight, const int64_t* __restrict__ bases,
                     float* __restrict__ pts_out, float* __restrict__ w_out, float* __restrict__ rgb_out, int64_t capacity) {
  __shared__ int cell_counts[kSteps][kWaves];
  const int64_t base = bases[blockIdx.x];
  if (base >= capacity) return;                            // every record of this share lies at or beyond the capacity
  float wv[kSteps];
  const uint32_t kept = cloud_load(w, w_stride, total, N, min_weight, wv);
  const uint32_t e0 = blockIdx.x * static_cast<uint32_t>(kShare) + threadIdx.x;
  const auto keeps = [kept](int j) { return ((kept >> j) & 1u) != 0u; };
  ns::share_place<kSteps>(keeps, cell_counts, [&](int j, int at) {    // at: kept elements of the share before this one
    if (keeps(j)) {
      const int64_t i = base + at;
      if (i >= 0 && i < capacity) {                        // a counter that was negative places nothing below record 0
        const uint32_t e = e0 + j * kBlock;
        const uint32_t r = e / N, k = e - r * N;
        const float zv = z[static_cast<int64_t>(r) * z_stride + k];
        const float* orow = o + static_cast<int64_t>(r) * 3;
        const float* drow = d + static_cast<int64_t>(r) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) pts_out[i * 3 + c] = orow[c] + drow[c] * zv;    // points_kernel's expression
        w_out[i] = wv[j];
        if (rgb_out) {
          const float* p = rgb + static_cast<int64_t>(r) * rgb_stride;
#pragma unroll
          for (int c = 0; c < 3; ++c) rgb_out[i * 3 + c] = p[c];
        }
      }
    }
  });
}

int64_t cloud_groups(int64_t R, int N) { return ns::cdiv(R * N, kShare); }

}  // namespace

extern "C" {

int64_t ns_cloud_workspace_bytes(int64_t R, int N) {
  if (!ns::flat_shape_ok(R, N)) return 0;
  return ns::round_256(cloud_groups(R, N) * static_cast<int64_t>(sizeof(int64_t)));
}

int ns_cloud_append(const float* o_dev, const float* d_dev, const float* z_dev, int64_t z_row_stride, const float* w_dev,
                    int64_t w_row_stride, const float* rgb_dev, int64_t rgb_stride, int64_t R, int N, float min_weight,
                    float* pts_out, float* w_out, float* rgb_out, int64_t capacity, int64_t* count_dev, void* workspace_dev,
                    void* stream) {
  NS_REQUIRE(R >= 0 && N >= 1, "R must be at least 0 and N at least 1");
  NS_REQUIRE(R == 0 || ns::flat_shape_ok(R, N), "R * N must be below 2^31");
  NS_REQUIRE(z_row_stride == 0 || z_row_stride >= N, "z_row_stride is 0 (packed) or at least N floats");
  NS_REQUIRE(w_row_stride == 0 || w_row_stride >= N, "w_row_stride is 0 (packed) or at least N floats");
  NS_REQUIRE(rgb_stride == 0 || rgb_stride >= 3, "rgb_stride is 0 (packed) or at least 3 floats");
  NS_REQUIRE(capacity >= 0, "negative capacity");
  NS_REQUIRE(capacity == 0 || (pts_out && w_out), "pts_out and w_out are required when capacity > 0");
  NS_REQUIRE(!rgb_out || rgb_dev || R == 0, "rgb_out without rgb_dev");
  NS_REQUIRE(count_dev, "null counter");
  NS_REQUIRE(ns::aligned(count_dev, 8) && ns::aligned(workspace_dev, 8), "count_dev and workspace_dev are 8-byte aligned");
  if (R == 0) return NS_OK;
  NS_REQUIRE(o_dev && d_dev && z_dev && w_dev && workspace_dev, "null pointer");
  const int64_t total = R * N;
  const int groups = static_cast<int>(cloud_groups(R, N));       // at most 2^31 / NS_CLOUD_SHARE
  int64_t* counts = static_cast<int64_t*>(workspace_dev);
  hipStream_t s = ns::as_stream(stream);
  const int64_t ws = w_row_stride == 0 ? N : w_row_stride;
  cloud_count_kernel<<<groups, kBlock, 0, s>>>(w_dev, ws, static_cast<uint32_t>(total), static_cast<uint32_t>(N), min_weight,
                                               counts);
  NS_LAUNCH_CHECK();
  cloud_scan_kernel<<<1, kBlock, 0, s>>>(counts, groups, count_dev);
  NS_LAUNCH_CHECK();
  if (capacity == 0) return NS_OK;                               // a pure count: there is no record to place
  cloud_scatter_kernel<<<groups, kBlock, 0, s>>>(o_dev, d_dev, z_dev, z_row_stride == 0 ? N : z_row_stride, w_dev, ws, rgb_dev,
                                                 rgb_stride == 0 ? 3 : rgb_stride, static_cast<uint32_t>(total),
                                                 static_cast<uint32_t>(N), min_weight, counts, pts_out, w_out, rgb_out,
                                                 capacity);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
