// The PSNR guard's own kernels (ns_guard.h): the every-ray guard pass places the last sample of every ray and patches its sigma
// into raw; the selective guard gathers the rays the one-kernel renderer flagged and composites their last sample again.
#include "ns_guard.h"

#include "ns_common.h"
#include "ns_composite_ray.h"
#include "ns_place.h"

namespace {

constexpr int kBlock = 256;

// the LAST sample of every ray only (the guard pass of ns_render_rays_*: ns_render_args::nerf_guard)
__global__ void __launch_bounds__(kBlock)
place_last_kernel(const float* __restrict__ mean, int64_t R, int N, float std_, float* __restrict__ z_last) {
  const int steps = N - 1;
  const float step = steps > 1 ? (std_ - (-std_)) / static_cast<float>(steps - 1) : 0.0f;
  for (int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x; r < R; r += (int64_t)gridDim.x * kBlock)
    z_last[r] = nsplace::uniform_z(mean[r], std_, step, steps, N - 1);
}

// sigma of every ray's last sample <- the guard pass's (the chain renderer)
__global__ void __launch_bounds__(kBlock)
patch_sigma_last_kernel(float4* __restrict__ raw, const float4* __restrict__ raw_last, int64_t R, int N) {
  for (int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x; r < R; r += (int64_t)gridDim.x * kBlock)
    raw[r * N + (N - 1)].w = raw_last[r].w;
}

// inputs of the flagged rays' last samples, compacted for the fp32-grade network (N = 1 "rays")
__global__ void __launch_bounds__(kBlock)
fix_gather_kernel(const float* __restrict__ rec, int rec_floats, const uint32_t* __restrict__ count, int64_t cap,
                  const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ view, float* __restrict__ o_c,
                  float* __restrict__ d_c, float* __restrict__ view_c, float* __restrict__ z_c) {
  int64_t n = static_cast<int64_t>(*count);
  if (n > cap) n = cap;
  for (int64_t s = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; s < n; s += static_cast<int64_t>(gridDim.x) * kBlock) {
    const float* q = rec + s * rec_floats;
    const int64_t r = nsfix::fix_ray_of(q);
#pragma unroll
    for (int c = 0; c < 3; ++c) { o_c[s * 3 + c] = o[r * 3 + c]; d_c[s * 3 + c] = d[r * 3 + c]; view_c[s * 3 + c] = view[r * 3 + c]; }
    z_c[s] = q[nsfix::kZ];
  }
}

// the flagged pixels again.  A ray of one chunk: tree sums + the last sample's share with the re-evaluated sigma
// (nscomp::recomposite_last: the very additions composite_finish makes, so a ray whose sigma keeps its sign comes out bit-identical
// to the every-ray guard).  LONG, a ray of several chunks: the last chunk's additions again with the re-evaluated share, then the
// earlier chunks' totals (nscomp::recomposite_last_long).  The depth / acc maps, when asked for, are rewritten from the same totals
template <bool LONG>
__global__ void __launch_bounds__(kBlock)
fix_last_sample_kernel(const float* __restrict__ rec, const uint32_t* __restrict__ count, int64_t cap, const float4* __restrict__ raw_c,
                       int N, int white_bkgd, float* __restrict__ rgb, int64_t rgb_stride, float* __restrict__ disp_out,
                       int64_t disp_stride, float* __restrict__ weights, float* __restrict__ depth_out,
                       float* __restrict__ acc_out) {
  using namespace nsfix;
  int64_t n = static_cast<int64_t>(*count);
  if (n > cap) n = cap;
  for (int64_t s = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; s < n; s += static_cast<int64_t>(gridDim.x) * kBlock) {
    const float* q = rec + s * (LONG ? kLongFloats : kFloats);
    const int64_t r = fix_ray_of(q);
    nscomp::RayAccum A;
    A.r = q[kSum]; A.g = q[kSum + 1]; A.b = q[kSum + 2]; A.depth = q[kSum + 3]; A.acc = q[kSum + 4];
    float disp, w;
    if constexpr (LONG) {
      float op[kOps][kSums];
#pragma unroll
      for (int k = 0; k < kOps; ++k)
#pragma unroll
        for (int c = 0; c < kSums; ++c) op[k][c] = q[kLongOps + kSums * k + c];
      nscomp::recomposite_last_long(A, op, q[kT], q[kRaw], q[kRaw + 1], q[kRaw + 2], raw_c[s].w, q[kZ], q[kDist], white_bkgd, disp, w);
    } else {
      nscomp::recomposite_last(A, q[kT], q[kRaw], q[kRaw + 1], q[kRaw + 2], raw_c[s].w, q[kZ], q[kDist], white_bkgd, disp, w);
    }
    float* p = rgb + r * rgb_stride;
    p[0] = A.r; p[1] = A.g; p[2] = A.b;
    disp_out[r * disp_stride] = disp;
    if (depth_out) depth_out[r] = A.depth;
    if (acc_out) acc_out[r] = A.acc;
    if (weights) weights[r * N + (N - 1)] = w;
  }
}

}  // namespace

int ns_place_last_sample(const float* mean_dev, int64_t R, int N, float std_, float* z_last_dev, void* stream) {
  NS_REQUIRE(R >= 0 && N >= 2 && mean_dev && z_last_dev, "bad arguments");
  if (R == 0) return NS_OK;
  place_last_kernel<<<ns::ew_grid(R, kBlock), kBlock, 0, ns::as_stream(stream)>>>(mean_dev, R, N, std_, z_last_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_patch_sigma_last(float* raw_dev, const float* raw_last_dev, int64_t R, int N, void* stream) {
  NS_REQUIRE(R >= 0 && N >= 1 && raw_dev && raw_last_dev, "bad arguments");
  if (R == 0) return NS_OK;
  patch_sigma_last_kernel<<<ns::ew_grid(R, kBlock), kBlock, 0, ns::as_stream(stream)>>>(
      reinterpret_cast<float4*>(raw_dev), reinterpret_cast<const float4*>(raw_last_dev), R, N);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_fix_gather(const float* rec_dev, int rec_floats, const uint32_t* count_dev, int64_t cap, const float* o_dev,
                  const float* d_dev, const float* view_dev, float* o_c, float* d_c, float* view_c, float* z_c, void* stream) {
  NS_REQUIRE(rec_dev && (rec_floats == nsfix::kFloats || rec_floats == nsfix::kLongFloats) && count_dev && cap >= 0 && o_dev &&
             d_dev && view_dev && o_c && d_c && view_c && z_c, "bad arguments");
  if (cap == 0) return NS_OK;
  fix_gather_kernel<<<ns::ew_grid(cap, kBlock), kBlock, 0, ns::as_stream(stream)>>>(rec_dev, rec_floats, count_dev, cap, o_dev, d_dev,
                                                                                   view_dev, o_c, d_c, view_c, z_c);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_fix_last_sample(const float* rec_dev, int rec_floats, const uint32_t* count_dev, int64_t cap, const float* raw_c, int N,
                       int white_bkgd, float* rgb_dev, int64_t rgb_stride, float* disp_dev, int64_t disp_stride,
                       float* weights_dev, float* depth_dev, float* acc_dev, void* stream) {
  const bool long_rec = rec_floats == nsfix::kLongFloats;
  NS_REQUIRE(rec_dev && (long_rec || rec_floats == nsfix::kFloats) && count_dev && cap >= 0 && raw_c && rgb_dev && disp_dev,
             "bad arguments");
  NS_REQUIRE(long_rec ? N > 64 && N % 64 == 0 : N >= 2, "the record does not fit the sample count");
  if (cap == 0) return NS_OK;
  const auto kernel = long_rec ? fix_last_sample_kernel<true> : fix_last_sample_kernel<false>;
  kernel<<<ns::ew_grid(cap, kBlock), kBlock, 0, ns::as_stream(stream)>>>(
      rec_dev, count_dev, cap, reinterpret_cast<const float4*>(raw_c), N, white_bkgd, rgb_dev, rgb_stride, disp_dev, disp_stride,
      weights_dev, depth_dev, acc_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}
