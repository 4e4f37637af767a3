// The PSNR guard (ns_render_args::nerf_guard): the record the one-kernel renderer leaves for a flagged ray, and the entry points of
// the guard's own kernels (ns_guard.hip).  Host-safe: ns_render.cpp sizes the workspace from it, the kernels index through it.
//
// The selective guard (ns_render_args::guard_threshold > 0): a ray whose own sigma of the last sample lies within the threshold of
// zero -- where the step alpha = step(sigma) could flip under the 16-bit rounding -- leaves a record at slot atomicAdd(fix_count)
// of fix_rec (nsepi::composite_group writes it); fix_gather_kernel compacts the flagged rays' last samples for the fp32-grade
// network, and fix_last_sample_kernel repeats the forward's last additions with the re-evaluated sigma.
//
// A ray of ONE chunk (N <= 64), kFloats floats.  The last sample's share joins the sums last (nscomp::composite_finish), so the
// record keeps the tree sums of the samples before it and what the share is made of:
//   kSum + 0..4 tree sums {r, g, b, depth, acc} | kT the transmittance entering the last sample | kRaw + 0..2 its raw rgb |
//   kZ its depth | kDist its dist * |d| | kRayLo, kRayHi the ray index, two bit-cast halves
//
// A ray of SEVERAL chunks (ns_render_args::guard_long_selective), kLongFloats floats.  The last sample's share sits inside the
// last chunk's 64-lane sum, which reduce5<64> forms on lane 63 as
//   u6 + (u5 + (u4 + (u3 + (u2 + (x62 + x63)))))        x_i: lane i's share;  u_k: what lane 63 - 2^(k-1) holds after k - 1 steps
// (u2 = x60 + x61, u3 the sum of lanes 56 .. 59, u4 of 48 .. 55, u5 of 32 .. 47, u6 of 0 .. 31, each as the scan rounds it), and
// the ray's totals are (the earlier chunks' running totals) + that.  The record keeps, per sum, the earlier total and the six
// operands beside x63, so the fix-up repeats the seven additions with the re-evaluated share -- the forward's own arithmetic
// stays as it is:
//   kLongSum + 0..4 the earlier chunks' totals | kLongT .. kLongRayHi as in the single-chunk record (fix_gather_kernel and
//   fix_ray_of read either) | kLongOps + kSums k + 0..4, k = 0 .. kOps - 1: x62, u2, u3, u4, u5, u6 of {r, g, b, depth, acc}
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NS_GUARD_FN __host__ __device__ __forceinline__
#else
#define NS_GUARD_FN inline
#endif

enum { NS_FIX_LONG_FLOATS = 48 };

namespace nsfix {

constexpr int kSums = 5, kOps = 6;
constexpr int kSum = 0, kT = 5, kRaw = 6, kZ = 9, kDist = 10, kRayLo = 11, kRayHi = 12, kFloats = 16;
constexpr int kLongSum = 0, kLongT = 5, kLongRaw = 6, kLongZ = 9, kLongDist = 10, kLongRayLo = 11, kLongRayHi = 12, kLongOps = 16,
              kLongFloats = NS_FIX_LONG_FLOATS;

static_assert(kLongT == kT && kLongRaw == kRaw && kLongZ == kZ && kLongDist == kDist && kLongRayLo == kRayLo && kLongRayHi == kRayHi,
              "floats 5 .. 12 of the long record are the single-chunk record's: the gather and the fix-up read either");
static_assert(kRayHi < kFloats && kLongRayHi < kLongOps && kLongOps + kOps * kSums <= kLongFloats,
              "the fields end inside the record, the operand block behind them");
static_assert(kFloats % 4 == 0 && kLongFloats % 4 == 0, "records are float4-aligned: the producers store float4 groups");
// the float4 groups of those stores: {sums 0 .. 3} | {sum 4, T, raw r, raw g} | {raw b, z, dist, ray lo}; ray hi on its own
static_assert(kSum % 4 == 0 && kT == kSum + kSums && kRaw == kT + 1 && kZ == kRaw + 3 && kDist == kZ + 1 && kRayLo == kDist + 1 &&
              kRayHi == kRayLo + 1 && kRayHi % 4 == 0,
              "nsepi::composite_group stores the fields kSum .. kRayLo as three consecutive float4: they stay contiguous, in this order");

// the ray index of a record, and its two halves as the producers store them
NS_GUARD_FN int64_t fix_ray_of(const float* rec) {
  return static_cast<int64_t>(static_cast<uint64_t>(__builtin_bit_cast(uint32_t, rec[kRayLo])) |
                              (static_cast<uint64_t>(__builtin_bit_cast(uint32_t, rec[kRayHi])) << 32));
}
NS_GUARD_FN float fix_ray_lo(int64_t r) { return __builtin_bit_cast(float, static_cast<uint32_t>(r)); }
NS_GUARD_FN float fix_ray_hi(int64_t r) { return __builtin_bit_cast(float, static_cast<uint32_t>(static_cast<uint64_t>(r) >> 32)); }

}  // namespace nsfix

// The guard's launchers (ns_guard.hip), internal to the library.
// the every-ray guard pass: the depth of every ray's LAST sample;  raw [R,N,4]'s sigma of that sample <- the guard pass's
int ns_place_last_sample(const float* mean_dev, int64_t R, int N, float std_, float* z_last_dev, void* stream);
int ns_patch_sigma_last(float* raw_dev, const float* raw_last_dev, int64_t R, int N, void* stream);
// the selective guard (rec_floats: nsfix::kFloats or kLongFloats; the count stays on the device, the launches cover cap records):
// compact inputs of the flagged rays' last samples for the fp32-grade network; then the flagged pixels from the records and the
// re-evaluated sigma (raw_c [.,4], element 3)
int ns_fix_gather(const float* rec_dev, int rec_floats, const uint32_t* count_dev, int64_t cap, const float* o_dev,
                  const float* d_dev, const float* view_dev, float* o_c, float* d_c, float* view_c, float* z_c, void* stream);
int ns_fix_last_sample(const float* rec_dev, int rec_floats, const uint32_t* count_dev, int64_t cap, const float* raw_c, int N,
                       int white_bkgd, float* rgb_dev, int64_t rgb_stride, float* disp_dev, int64_t disp_stride,
                       float* weights_dev, float* depth_dev, float* acc_dev, void* stream);
