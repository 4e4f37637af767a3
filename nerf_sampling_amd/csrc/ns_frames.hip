// A rendered frame as 8-bit pixels on the device (ns_frame_to8b): run_nerf_helpers.to8b,
// (255 * np.clip(x, 0, 1)).astype(np.uint8) on fp32 input, so that a quarter of the frame's bytes cross to the host.
// Elementwise, fp32 in, bytes out; its time is a launch's.
//
// Thread t owns the kGroup = 4 pixels 4 t .. 4 t + 3: 4 * C output bytes are 3 (C = 3) or 4 (C = 4) whole dwords, and they lie
// on a dword boundary whenever out_dev does.  A whole group on an aligned base is packed in registers and stored as dwords;
// the last group when n_pixels is no multiple of 4, and every group of a base that is not 4-byte aligned (a row band whose
// row0 * W * C is no multiple of 4), store bytes.  Either way a thread writes only the bytes of its own pixels p < n_pixels:
// nothing outside out_dev[0 .. n_pixels * C).
// Loads: rgb_dev is only known to be 4-byte aligned (a band of packed-3 data), so the default is one dword per value; when the
// base happens to be 16-byte aligned (whole frames are) a group of packed-3 pixels is three float4 loads, and a pixel of the
// interleaved [R,4] layout one -- except the last pixel of the buffer, whose fourth float nobody promised exists.
//
// Below it, the disparity sequence of the turntable (Trainer.py:371-376 to8b(disps / np.max(disps))): ns_map_max keeps the
// maximum of the frames' maps on the device, ns_map_to8b divides by it where it lies and quantises with the same to8b.
#include <cmath>

#include "ns_block.h"
#include "ns_common.h"

namespace {

using ns::kBlock;
using ns::kWaves;
constexpr int kGroup = 4;

// run_nerf_helpers.py:11.  The comparisons (not fmaxf / fminf) state what happens to the values numpy leaves to the platform:
// NaN fails `x > 0` and becomes 0, as -0.0 and everything below 0 do; +inf becomes 1.  Then ONE fp32 multiply and a truncation.
__device__ __forceinline__ uint32_t to8b(float x) {
  const float lo = x > 0.0f ? x : 0.0f;
  const float c = lo < 1.0f ? lo : 1.0f;
  return static_cast<uint32_t>(255.0f * c);                  // in [0, 255]: v_cvt_u32_f32 truncates
}

template <int C>
__global__ void __launch_bounds__(kBlock)
frame_to8b_kernel(const float* __restrict__ rgb, int stride, const float* __restrict__ alpha, int n, uint8_t* __restrict__ out,
                  int wide_loads, int dword_stores) {
  const int p0 = (blockIdx.x * kBlock + threadIdx.x) * kGroup;     // below n + kBlock * kGroup, and 4 n is below 2^31
  if (p0 >= n) return;
  const int m = n - p0 < kGroup ? n - p0 : kGroup;                 // pixels of this group that exist
  float v[kGroup][3];
  if (m == kGroup && wide_loads && stride == 3) {
    const float4* q = reinterpret_cast<const float4*>(rgb + static_cast<int64_t>(p0) * 3);      // 48 p0 bytes: 16-byte aligned
    const float4 a = q[0], b = q[1], c = q[2];
    v[0][0] = a.x, v[0][1] = a.y, v[0][2] = a.z;
    v[1][0] = a.w, v[1][1] = b.x, v[1][2] = b.y;
    v[2][0] = b.z, v[2][1] = b.w, v[2][2] = c.x;
    v[3][0] = c.y, v[3][1] = c.z, v[3][2] = c.w;
  } else {
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
      if (i < m) {
        const float* q = rgb + static_cast<int64_t>(p0 + i) * stride;
        if (wide_loads && stride == 4 && p0 + i + 1 < n) {         // the fourth float is the next pixel's neighbour: it exists
          const float4 a = *reinterpret_cast<const float4*>(q);
          v[i][0] = a.x, v[i][1] = a.y, v[i][2] = a.z;
        } else {
          v[i][0] = q[0], v[i][1] = q[1], v[i][2] = q[2];
        }
      } else {
        v[i][0] = v[i][1] = v[i][2] = 0.0f;
      }
    }
  }
  uint32_t b[kGroup * C];                                           // one byte value per output byte, in output order
#pragma unroll
  for (int i = 0; i < kGroup; ++i) {
#pragma unroll
    for (int c = 0; c < 3; ++c) b[i * C + c] = to8b(v[i][c]);
    if (C == 4) b[i * C + 3] = (alpha != nullptr && i < m) ? to8b(alpha[p0 + i]) : 255u;
  }
  uint8_t* o = out + static_cast<int64_t>(p0) * C;
  if (m == kGroup && dword_stores) {
    uint32_t* w = reinterpret_cast<uint32_t*>(o);                   // out is 4-byte aligned and 4 C p0 / 4 is whole
#pragma unroll
    for (int j = 0; j < C; ++j) w[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
      if (i < m) {
#pragma unroll
        for (int c = 0; c < C; ++c) o[i * C + c] = static_cast<uint8_t>(b[i * C + c]);
      }
    }
  }
}

// ---- a per-ray map as 8-bit pixels, divided by a number in device memory (ns_map_to8b) -------------------------------------
// Trainer.py:371-376: to8b(disps / np.max(disps)).  numpy divides float32 by float32 with ONE correctly rounded division, so
// the quotient here is the `/` operator (hipcc's default for HIP: v_div_scale / v_rcp / the fma refinement / v_div_fmas /
// v_div_fixup, 0.5 ulp), never x * (1 / d); then to8b above.  0 / 0, inf / inf and a NaN divisor give NaN, and NaN gives 0.
// Thread t owns the kGroup pixels 4 t .. 4 t + 3 and their four output bytes: ONE dword where out_dev is 4-byte aligned and
// the group is whole, bytes otherwise; a thread writes only the bytes of its own pixels p < n.
// Loads: a packed map whose base is 16-byte aligned gives a whole group as one float4; any other packed base and the [:, 3]
// column of an [R,4] shard -- 12 bytes into the shard, so never 16-byte aligned -- are read one dword per value.
__global__ void __launch_bounds__(kBlock)
map_to8b_kernel(const float* __restrict__ map, int stride, int64_t n, const float* __restrict__ denom, uint8_t* __restrict__ out,
                int wide_loads, int dword_stores) {
  const int64_t p0 = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) * kGroup;
  if (p0 >= n) return;
  const int m = n - p0 < kGroup ? static_cast<int>(n - p0) : kGroup;     // pixels of this group that exist
  float v[kGroup];
  if (m == kGroup && wide_loads) {                                        // stride == 1 and 4 p0 floats = 16 p0 bytes on
    const float4 a = *reinterpret_cast<const float4*>(map + p0);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
  } else {
#pragma unroll
    for (int i = 0; i < kGroup; ++i) v[i] = i < m ? map[(p0 + i) * stride] : 0.0f;
  }
  uint32_t b[kGroup];
  if (denom != nullptr) {
    const float d = *denom;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) b[i] = to8b(v[i] / d);
  } else {
#pragma unroll
    for (int i = 0; i < kGroup; ++i) b[i] = to8b(v[i]);
  }
  uint8_t* o = out + p0;
  if (m == kGroup && dword_stores) {
    *reinterpret_cast<uint32_t*>(o) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);    // out is 4-byte aligned, p0 = 4 t
  } else {
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
      if (i < m) o[i] = static_cast<uint8_t>(b[i]);
    }
  }
}

// ---- the running maximum of per-ray maps (ns_map_max) ---------------------------------------------------------------------
// np.max(disps) over all frames, kept on the device as state = (max over the values that are not NaN, 1.0f if a NaN was
// seen).  Shaped as ns_image_sqerr: workgroup g owns the kMaxShare values from g * kMaxShare on and leaves (max, flag) in
// partial[g]; a second launch of ONE workgroup folds the partials, and under `accumulate` the state already there, into the
// state.  A maximum does not depend on the order of its comparisons: no atomics.  (-0.0 against +0.0 is whichever came first.)
// block_fold is ns::block_sum with fold for +; it stays here: a combine parameter on block_sum would cost more lines than this.
constexpr int kMaxPerThread = 8;
constexpr int kMaxShare = kBlock * kMaxPerThread;

struct MaxState {
  float max, nan;
};

__device__ __forceinline__ void fold(MaxState& s, float x) {
  if (x == x) s.max = x > s.max ? x : s.max;
  else s.nan = 1.0f;
}

__device__ __forceinline__ void fold(MaxState& s, const MaxState& o) {
  s.max = o.max > s.max ? o.max : s.max;                     // o.max is never NaN
  s.nan = o.nan != 0.0f ? 1.0f : s.nan;
}

__device__ __forceinline__ MaxState block_fold(MaxState s, MaxState* wave_states) {   // valid in thread 0
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    MaxState o;
    o.max = __shfl_xor(s.max, off, 64);
    o.nan = __shfl_xor(s.nan, off, 64);
    fold(s, o);
  }
  if ((threadIdx.x & 63) == 0) wave_states[threadIdx.x >> 6] = s;
  __syncthreads();
  MaxState r = wave_states[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) fold(r, wave_states[w]);
  return r;
}

__global__ void __launch_bounds__(kBlock)
map_max_kernel(const float* __restrict__ map, int stride, int64_t n, MaxState* __restrict__ partial, int wide_loads) {
  __shared__ MaxState wave_states[kWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kMaxShare;
  MaxState s = {-INFINITY, 0.0f};
  if (wide_loads) {                                          // packed, 16-byte aligned base: kMaxShare / 4 float4s per share
#pragma unroll
    for (int k = 0; k < kMaxPerThread / 4; ++k) {
      const int64_t e = base + (static_cast<int64_t>(k) * kBlock + threadIdx.x) * 4;
      if (e + 3 < n) {
        const float4 a = *reinterpret_cast<const float4*>(map + e);
        fold(s, a.x), fold(s, a.y), fold(s, a.z), fold(s, a.w);
      } else {
        for (int64_t j = e; j < n; ++j) fold(s, map[j]);     // the map's last, partial group of four
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kMaxPerThread; ++k) {
      const int64_t e = base + k * kBlock + threadIdx.x;
      if (e < n) fold(s, map[e * stride]);
    }
  }
  const MaxState r = block_fold(s, wave_states);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ void __launch_bounds__(kBlock)
map_max_combine_kernel(const MaxState* __restrict__ partial, int n_partial, int accumulate, MaxState* state) {
  __shared__ MaxState wave_states[kWaves];
  MaxState s = {-INFINITY, 0.0f};
  for (int i = threadIdx.x; i < n_partial; i += kBlock) fold(s, partial[i]);
  MaxState r = block_fold(s, wave_states);
  if (threadIdx.x == 0) {
    if (accumulate) {
      const MaxState old = *state;
      fold(r, old.max);                                      // a NaN in the old maximum (never written here) is a NaN seen
      r.nan = old.nan != 0.0f ? 1.0f : r.nan;
    }
    *state = r;
  }
}

int64_t map_max_groups(int64_t n) { return ns::cdiv(n, kMaxShare); }

// what both map entries ask of (stride, n); `who` is the entry's name
int check_map(const char* who, int64_t stride, int64_t n) {
  if (n < 0) {
    ns::set_error("%s: negative n", who);
    return NS_E_INVALID;
  }
  if (!ns::below_2_31(n)) {
    ns::set_error("%s: n must be below 2^31", who);
    return NS_E_INVALID;
  }
  if (stride != 1 && stride != 4) {
    ns::set_error("%s: stride is 1 (a packed map) or 4 floats (a column of the [R,4] shard)", who);
    return NS_E_INVALID;
  }
  return NS_OK;
}

}  // namespace

extern "C" {

int ns_frame_to8b(const float* rgb_dev, int64_t rgb_stride, const float* alpha_dev, int64_t n_pixels, uint8_t* out_dev,
                  int out_channels, void* stream) {
  NS_REQUIRE(n_pixels >= 0, "negative n_pixels");
  NS_REQUIRE(n_pixels < (int64_t(1) << 29), "n_pixels * 4 must be below 2^31");
  NS_REQUIRE(rgb_stride == 0 || rgb_stride == 3 || rgb_stride == 4, "rgb_stride is 0 (packed), 3 or 4 floats");
  NS_REQUIRE(out_channels == 3 || out_channels == 4, "out_channels is 3 or 4");
  if (n_pixels == 0) return NS_OK;
  NS_REQUIRE(rgb_dev && out_dev, "null pointer");
  const int n = static_cast<int>(n_pixels);
  const int stride = rgb_stride == 0 ? 3 : static_cast<int>(rgb_stride);
  const int groups = (n + kGroup - 1) / kGroup;
  const int grid = (groups + kBlock - 1) / kBlock;                  // at most 2^19 workgroups
  const int wide_loads = ns::aligned(rgb_dev, 16);
  const int dword_stores = ns::aligned(out_dev, 4);
  hipStream_t s = ns::as_stream(stream);
  if (out_channels == 3)
    frame_to8b_kernel<3><<<grid, kBlock, 0, s>>>(rgb_dev, stride, alpha_dev, n, out_dev, wide_loads, dword_stores);
  else
    frame_to8b_kernel<4><<<grid, kBlock, 0, s>>>(rgb_dev, stride, alpha_dev, n, out_dev, wide_loads, dword_stores);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int64_t ns_map_max_workspace_bytes(int64_t n) {
  if (n <= 0 || !ns::below_2_31(n)) return 0;
  return ns::round_256(map_max_groups(n) * static_cast<int64_t>(sizeof(MaxState)));
}

int ns_map_max(const float* map_dev, int64_t stride, int64_t n, int accumulate, float* state_dev, void* workspace_dev,
               void* stream) {
  const int rc = check_map(__func__, stride, n);
  if (rc != NS_OK) return rc;
  NS_REQUIRE(state_dev, "null pointer");
  NS_REQUIRE(ns::aligned(state_dev, 4), "state_dev must be 4-byte aligned");
  NS_REQUIRE(n == 0 || (map_dev && workspace_dev), "null pointer");
  NS_REQUIRE(ns::aligned(workspace_dev, 8), "workspace_dev must be 8-byte aligned");
  if (n == 0 && accumulate) return NS_OK;                    // nothing to fold: the state stays
  const int groups = static_cast<int>(map_max_groups(n));    // at most 2^20
  MaxState* partial = static_cast<MaxState*>(workspace_dev);
  hipStream_t s = ns::as_stream(stream);
  if (n > 0) {
    const int wide_loads = stride == 1 && ns::aligned(map_dev, 16);
    map_max_kernel<<<groups, kBlock, 0, s>>>(map_dev, static_cast<int>(stride), n, partial, wide_loads);
    NS_LAUNCH_CHECK();
  }
  map_max_combine_kernel<<<1, kBlock, 0, s>>>(partial, groups, accumulate != 0, reinterpret_cast<MaxState*>(state_dev));
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_map_to8b(const float* map_dev, int64_t stride, int64_t n, const float* denom_dev, uint8_t* out_dev, void* stream) {
  const int rc = check_map(__func__, stride, n);
  if (rc != NS_OK) return rc;
  NS_REQUIRE(ns::aligned(denom_dev, 4), "denom_dev must be 4-byte aligned");
  if (n == 0) return NS_OK;
  NS_REQUIRE(map_dev && out_dev, "null pointer");
  const int64_t groups = (n + kGroup - 1) / kGroup;
  const int grid = static_cast<int>((groups + kBlock - 1) / kBlock);          // at most 2^21 workgroups
  const int wide_loads = stride == 1 && ns::aligned(map_dev, 16);
  const int dword_stores = ns::aligned(out_dev, 4);
  map_to8b_kernel<<<grid, kBlock, 0, ns::as_stream(stream)>>>(map_dev, static_cast<int>(stride), n, denom_dev, out_dev,
                                                              wide_loads, dword_stores);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
