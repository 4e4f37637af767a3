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
#include "ns_common.h"

namespace {

constexpr int kBlock = 256;
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
  const int wide_loads = (reinterpret_cast<uintptr_t>(rgb_dev) & 15) == 0;
  const int dword_stores = (reinterpret_cast<uintptr_t>(out_dev) & 3) == 0;
  hipStream_t s = ns::as_stream(stream);
  if (out_channels == 3)
    frame_to8b_kernel<3><<<grid, kBlock, 0, s>>>(rgb_dev, stride, alpha_dev, n, out_dev, wide_loads, dword_stores);
  else
    frame_to8b_kernel<4><<<grid, kBlock, 0, s>>>(rgb_dev, stride, alpha_dev, n, out_dev, wide_loads, dword_stores);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
