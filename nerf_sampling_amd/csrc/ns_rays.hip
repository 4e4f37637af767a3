// Ray-side element-wise kernels: camera rays, ray-sphere intersection, positional encoding,
// sample placement, coarse depths.  All HBM-bound, fp32, one thread per output element or per
// ray, grid-stride.  Built with -ffp-contract=off so that mul/add stay separate roundings like
// the reference's eager PyTorch arithmetic.
#include "ns_block.h"
#include "ns_common.h"
#include "ns_place.h"

namespace {

using ns::kBlock;
using ns::kWaves;

using nsplace::linspace_at;

struct Cam {
  float fx, fy, cx, cy;
  float r[9];  // c2w[:3,:3] row-major
  float t[3];  // c2w[:3,3]
};

// a1: run_nerf_helpers.py:187-202 + nerf_utils.py:156-188.  The direction of pixel (column i, row j) and its norm: the ONE
// statement of the ray arithmetic, shared by get_rays_kernel and the ray-batch kernels below (same bits from all of them).
__device__ __forceinline__ void pixel_ray(const Cam& cam, int i, int j, float d[3], float& nrm) {
  const float dx = (static_cast<float>(i) - cam.cx) / cam.fx;
  const float dy = -((static_cast<float>(j) - cam.cy) / cam.fy);
  const float dz = -1.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    d[c] = (dx * cam.r[3 * c + 0] + dy * cam.r[3 * c + 1]) + dz * cam.r[3 * c + 2];
  // torch.norm on the CPU accumulates squares as an fma chain (verified bit-for-bit on the golden rays)
  nrm = sqrtf(__builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0])));
}

__global__ void __launch_bounds__(kBlock)
get_rays_kernel(Cam cam, int W, int row0, int64_t R, float near_, float far_,
                float* __restrict__ rays_o, float* __restrict__ rays_d,
                float* __restrict__ viewdirs, float* __restrict__ ray_batch) {
  for (int64_t idx = blockIdx.x * (int64_t)kBlock + threadIdx.x; idx < R;
       idx += (int64_t)gridDim.x * kBlock) {
    const int j = row0 + static_cast<int>(idx / W);
    const int i = static_cast<int>(idx % W);
    float d[3], nrm;
    pixel_ray(cam, i, j, d, nrm);
    if (rays_o) {
      rays_o[idx * 3 + 0] = cam.t[0]; rays_o[idx * 3 + 1] = cam.t[1]; rays_o[idx * 3 + 2] = cam.t[2];
    }
    if (rays_d) {
      rays_d[idx * 3 + 0] = d[0]; rays_d[idx * 3 + 1] = d[1]; rays_d[idx * 3 + 2] = d[2];
    }
    if (viewdirs) {
      viewdirs[idx * 3 + 0] = d[0] / nrm; viewdirs[idx * 3 + 1] = d[1] / nrm; viewdirs[idx * 3 + 2] = d[2] / nrm;
    }
    if (ray_batch) {
      float* b = ray_batch + idx * 11;
      b[0] = cam.t[0]; b[1] = cam.t[1]; b[2] = cam.t[2];
      b[3] = d[0]; b[4] = d[1]; b[5] = d[2];
      b[6] = near_; b[7] = far_;
      b[8] = d[0] / nrm; b[9] = d[1] / nrm; b[10] = d[2] / nrm;
    }
  }
}

// ---- training ray batches from a device-resident dataset (ns_ray_batch_gather / ns_ray_batch_draw) ----------------------
struct BatchOut {
  float* rays_o;
  float* rays_d;
  float* viewdirs;
  float* target;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The target colour of pixel `pix` of image `img` (both in range): the ONE statement of it, shared by the ray-batch kernels and
// image_sqerr_kernel (same bits from all of them).
__device__ __forceinline__ void dataset_target(const ns_ray_dataset& ds, int img, int pix, float rgb[3]) {
  const float* px = ds.images_dev + (static_cast<int64_t>(img) * (ds.H * ds.W) + pix) * ds.C;
  rgb[0] = px[0]; rgb[1] = px[1]; rgb[2] = px[2];
  if (ds.C == 4 && ds.white_bkgd) {            // BlenderTrainer.load_data: rgb * a + (1 - a), three separate roundings
    const float a = px[3];
    const float inv = 1.0f - a;
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] * a + inv;
  }
}

// Ray b of a batch: pixel `pix` (flat row * W + col) of image `img`, both clamped into range (no index reads out of bounds).
__device__ __forceinline__ void emit_batch_ray(const ns_ray_dataset& ds, int img, int pix, int64_t b, const BatchOut& out) {
  img = clampi(img, 0, ds.n_images - 1);
  pix = clampi(pix, 0, ds.H * ds.W - 1);
  if (out.rays_o || out.rays_d || out.viewdirs) {
    const float* pose = ds.poses_dev + static_cast<int64_t>(img) * ds.pose_stride;
    Cam cam;
    cam.fx = ds.fx; cam.fy = ds.fy; cam.cx = ds.cx; cam.cy = ds.cy;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) cam.r[3 * r + c] = pose[4 * r + c];
      cam.t[r] = pose[4 * r + 3];
    }
    float d[3], nrm;
    pixel_ray(cam, pix % ds.W, pix / ds.W, d, nrm);
    if (out.rays_o) {
      out.rays_o[b * 3 + 0] = cam.t[0]; out.rays_o[b * 3 + 1] = cam.t[1]; out.rays_o[b * 3 + 2] = cam.t[2];
    }
    if (out.rays_d) {
      out.rays_d[b * 3 + 0] = d[0]; out.rays_d[b * 3 + 1] = d[1]; out.rays_d[b * 3 + 2] = d[2];
    }
    if (out.viewdirs) {
      out.viewdirs[b * 3 + 0] = d[0] / nrm; out.viewdirs[b * 3 + 1] = d[1] / nrm; out.viewdirs[b * 3 + 2] = d[2] / nrm;
    }
  }
  if (out.target) {
    float rgb[3];
    dataset_target(ds, img, pix, rgb);
    out.target[b * 3 + 0] = rgb[0]; out.target[b * 3 + 1] = rgb[1]; out.target[b * 3 + 2] = rgb[2];
  }
}

__global__ void __launch_bounds__(kBlock)
ray_batch_gather_kernel(ns_ray_dataset ds, const int* __restrict__ image_idx, int image_scalar,
                        const int* __restrict__ pixel, int64_t B, BatchOut out) {
  for (int64_t b = blockIdx.x * (int64_t)kBlock + threadIdx.x; b < B; b += (int64_t)gridDim.x * kBlock)
    emit_batch_ray(ds, image_idx ? image_idx[b] : image_scalar, pixel[b], b, out);
}

// The keyed permutation of ns_ray_batch_draw (ray_batches.permute_index repeats it in integers).
__device__ __forceinline__ uint64_t mix64(uint64_t z) {        // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kImageSalt = 0xD1B54A32D192ED03ull;
constexpr int kRounds = NS_RAY_DRAW_ROUNDS;

__device__ __forceinline__ uint64_t draw_key(uint64_t seed, uint64_t counter) { return mix64(seed ^ mix64(counter + kGolden)); }

__device__ __forceinline__ uint32_t mix32(uint32_t h) {        // murmur3's finaliser
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

// P_{seed,counter}(i) on [0, n), 1 <= n < 2^31, 0 <= i < n: a balanced Feistel network over the smallest even bit width that
// covers n, walked along its cycle until the value is below n again (it is a bijection of the wider range and starts below n).
__device__ __forceinline__ uint32_t permute_index(uint32_t n, uint64_t key, uint32_t i) {
  int half = 1;
  while ((1ull << (2 * half)) < n) ++half;
  const uint32_t mask = (1u << half) - 1u;
  uint32_t rk[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) rk[r] = static_cast<uint32_t>(mix64(key + static_cast<uint64_t>(r + 1) * kGolden));
  uint32_t v = i;
  do {
    uint32_t l = v >> half, r = v & mask;
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
      const uint32_t t = l ^ (mix32(r + rk[k]) & mask);
      l = r;
      r = t;
    }
    v = (l << half) | r;
  } while (v >= n);
  return v;
}

__global__ void __launch_bounds__(kBlock)
ray_batch_draw_kernel(ns_ray_dataset ds, const int* __restrict__ train_idx, int n_train, int scope,
                      const int* __restrict__ params_dev, ns_ray_draw_params host, uint64_t seed, int64_t B,
                      int* __restrict__ image_idx_out, int* __restrict__ pixel_out, BatchOut out) {
  ns_ray_draw_params p = host;
  if (params_dev) {
    p.step = params_dev[0]; p.row0 = params_dev[1]; p.row1 = params_dev[2]; p.col0 = params_dev[3]; p.col1 = params_dev[4];
  }
  const int HW = ds.H * ds.W;
  for (int64_t b = blockIdx.x * (int64_t)kBlock + threadIdx.x; b < B; b += (int64_t)gridDim.x * kBlock) {
    int slot, pix;
    if (scope == NS_RAY_SCOPE_ALL_IMAGES) {
      const uint64_t N = static_cast<uint64_t>(n_train) * static_cast<uint64_t>(HW);
      const uint64_t pos = static_cast<uint64_t>(static_cast<uint32_t>(p.step)) * static_cast<uint64_t>(B) + static_cast<uint64_t>(b);
      const uint32_t g = permute_index(static_cast<uint32_t>(N), draw_key(seed, pos / N), static_cast<uint32_t>(pos % N));
      slot = static_cast<int>(g / static_cast<uint32_t>(HW));
      pix = static_cast<int>(g % static_cast<uint32_t>(HW));
    } else {
      // a window read from device memory is clamped to a non-empty part of the frame, and a ray index beyond it wraps
      const int r0 = clampi(p.row0, 0, ds.H - 1), r1 = clampi(p.row1, r0 + 1, ds.H);
      const int c0 = clampi(p.col0, 0, ds.W - 1), c1 = clampi(p.col1, c0 + 1, ds.W);
      const int cols = c1 - c0;
      const uint32_t n = static_cast<uint32_t>((r1 - r0) * cols);
      const uint64_t key = draw_key(seed, static_cast<uint64_t>(static_cast<uint32_t>(p.step)));
      slot = static_cast<int>(mix64(key ^ kImageSalt) % static_cast<uint64_t>(n_train));
      const uint32_t w = permute_index(n, key, static_cast<uint32_t>(static_cast<uint64_t>(b) % n));
      pix = (r0 + static_cast<int>(w) / cols) * ds.W + c0 + static_cast<int>(w) % cols;
    }
    const int img = clampi(train_idx[slot], 0, ds.n_images - 1);
    if (image_idx_out) image_idx_out[b] = img;
    if (pixel_out) pixel_out[b] = pix;
    emit_batch_ray(ds, img, pix, b, out);
  }
}

// ---- frame PSNR on the device (ns_image_sqerr) ----------------------------------------------------------------------
// sum over the pixels of a row band and the three channels of (double)(fl32(rgb - target))^2.  Workgroup g owns pixels
// [g * kSqerrShare, (g + 1) * kSqerrShare); thread t adds its pixels g * kSqerrShare + k * kBlock + t in the order of k, the
// workgroup's sum in the fixed order of ns::block_sum -> partial[g].  A second launch of ONE workgroup adds the partials the
// same way (thread t: partials t, t + kBlock, ... in order).  Every addition is fixed by the pixel count alone -- no atomics,
// nothing that depends on the CU count; a NaN term makes the sum NaN.
constexpr int kSqerrPerThread = 8;
constexpr int kSqerrShare = kBlock * kSqerrPerThread;

__global__ void __launch_bounds__(kBlock)
image_sqerr_kernel(ns_ray_dataset ds, int img, int pix0, int n, const float* __restrict__ rgb, int stride,
                   double* __restrict__ partial) {
  __shared__ double wave_sums[kWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kSqerrShare + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kSqerrPerThread; ++k) {
    const int64_t r = base + k * kBlock;
    if (r < n) {
      float t[3];
      dataset_target(ds, img, pix0 + static_cast<int>(r), t);
      const float* p = rgb + r * stride;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double d = static_cast<double>(p[c] - t[c]);   // one fp32 subtraction, as numpy's rgbs - gt
        acc += d * d;                                        // the square of an fp32 value is exact in double
      }
    }
  }
  const double s = ns::block_sum(acc, wave_sums);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kBlock)
image_sqerr_combine_kernel(const double* __restrict__ partial, int n_partial, double* __restrict__ sum) {
  __shared__ double wave_sums[kWaves];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[i];
  const double s = ns::block_sum(acc, wave_sums);
  if (threadIdx.x == 0) *sum = s;
}

// ---- placed samples against the field's depth (ns_depth_sqerr) ------------------------------------------------------
// sum over rays r and samples k of (double)(fl32(z[r, k] - ref[r]))^2, the flat element e = r * N + k.  Workgroup g owns
// elements [g * kDepthShare, (g + 1) * kDepthShare); thread t adds its elements g * kDepthShare + j * kBlock + t in the order of
// j (consecutive lanes read consecutive floats of a packed z); lanes, waves and workgroups are combined as ns_image_sqerr's are
// (ns::block_sum, partial[g], the same second launch), so every addition is fixed by (R, N) alone.
constexpr int kDepthShare = NS_DEPTH_SQERR_SHARE;
constexpr int kDepthSteps = ns::ShareOf<kDepthShare>::steps;

__global__ void __launch_bounds__(kBlock)
depth_sqerr_kernel(const float* __restrict__ z, int64_t stride, const float* __restrict__ ref, uint32_t total, uint32_t N,
                   double* __restrict__ partial) {
  __shared__ double wave_sums[kWaves];
  const uint32_t base = blockIdx.x * static_cast<uint32_t>(kDepthShare) + threadIdx.x;   // below 2^31 + kDepthShare
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kDepthSteps; ++j) {
    const uint32_t e = base + j * kBlock;
    if (e < total) {
      const uint32_t r = e / N, k = e - r * N;
      const double d = static_cast<double>(z[static_cast<int64_t>(r) * stride + k] - ref[r]);   // one fp32 subtraction, as mse_loss
      acc += d * d;                                                                            // exact in double
    }
  }
  const double s = ns::block_sum(acc, wave_sums);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---- frame SSIM on the device (ns_image_ssim) -----------------------------------------------------------------------
// Wang et al. 2004 over every 11 x 11 window that lies wholly inside the frame, per colour channel, weights g(i) g(j).
// Workgroup b owns the kSsimTileH x kSsimTileW tile of window origins at (b / tiles_x, b % tiles_x) * tile, thread t the
// window (t / kSsimTileW, t % kSsimTileW) of it.  The frame and target patch (tile + 10 in each direction, zero beyond the
// frame) is staged once as floats; per channel the five 11-tap row sums of every patch row go to LDS as doubles (taps in
// the order k = 0..10), one barrier, then every thread adds the 11 row sums of its window (rows in order) and forms S.
// Everything after the fp32 loads is double: with fp32 moments E[x^2] - mu^2 on a flat background is rounding noise of
// 1e-7 against C2 = 9e-4.  A window beyond (H - 10, W - 10) is predicated out, never multiplied by 0.  A thread adds its
// S of channel 0, 1, 2 in that order; lanes, waves and workgroups are combined as ns_image_sqerr's are (the same second
// launch), so every addition is fixed by (H, W) alone -- no atomics; a NaN pixel makes the sum NaN.
constexpr int kSsimWin = NS_SSIM_WINDOW;
constexpr int kSsimTileH = NS_SSIM_TILE_H, kSsimTileW = NS_SSIM_TILE_W;
constexpr int kSsimPatchH = kSsimTileH + kSsimWin - 1, kSsimPatchW = kSsimTileW + kSsimWin - 1;
static_assert(kSsimTileH * kSsimTileW == kBlock, "one thread per window of the tile");
static_assert(kSsimWin == 11, "the tap table below is the 11-tap one");

// g(k) = exp(-(k - 5)^2 / 4.5) / sum, sigma = 1.5
__device__ constexpr double kSsimTap[kSsimWin] = {
    0.00102838008447911,  0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
    0.2130055377112537,   0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
    0.03600077212843083,  0.007598758135239185, 0.00102838008447911};

__global__ void __launch_bounds__(kBlock)
image_ssim_kernel(ns_ray_dataset ds, int img, int tiles_x, const float* __restrict__ rgb, int stride,
                  double* __restrict__ partial) {
  __shared__ float xs[3][kSsimPatchH][kSsimPatchW];      // the rendered frame's patch
  __shared__ float ys[3][kSsimPatchH][kSsimPatchW];      // the target's
  __shared__ double rows[5][kSsimPatchH][kSsimTileW];    // row sums of x, y, x^2, y^2, xy
  __shared__ double wave_sums[kWaves];
  const int H = ds.H, W = ds.W;
  const int oy = (static_cast<int>(blockIdx.x) / tiles_x) * kSsimTileH;
  const int ox = (static_cast<int>(blockIdx.x) % tiles_x) * kSsimTileW;
  for (int i = threadIdx.x; i < kSsimPatchH * kSsimPatchW; i += kBlock) {
    const int py = i / kSsimPatchW, px = i % kSsimPatchW;
    const int r = oy + py, c = ox + px;
    float x[3] = {0.0f, 0.0f, 0.0f}, y[3] = {0.0f, 0.0f, 0.0f};
    if (r < H && c < W) {
      const int pix = r * W + c;
      dataset_target(ds, img, pix, y);
      const float* p = rgb + static_cast<int64_t>(pix) * stride;
      x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { xs[ch][py][px] = x[ch]; ys[ch][py][px] = y[ch]; }
  }
  __syncthreads();
  const int ty = threadIdx.x / kSsimTileW, tx = threadIdx.x % kSsimTileW;
  const bool valid = (oy + ty < H - (kSsimWin - 1)) && (ox + tx < W - (kSsimWin - 1));
  constexpr double C1 = 1e-4, C2 = 9e-4;
  double acc = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    for (int i = threadIdx.x; i < kSsimPatchH * kSsimTileW; i += kBlock) {
      const int py = i / kSsimTileW, px = i % kSsimTileW;
      double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < kSsimWin; ++k) {
        const double g = kSsimTap[k];
        const double x = static_cast<double>(xs[ch][py][px + k]), y = static_cast<double>(ys[ch][py][px + k]);
        s[0] += g * x; s[1] += g * y; s[2] += g * (x * x); s[3] += g * (y * y); s[4] += g * (x * y);
      }
#pragma unroll
      for (int m = 0; m < 5; ++m) rows[m][py][px] = s[m];
    }
    __syncthreads();
    if (valid) {
      double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < kSsimWin; ++k) {
        const double g = kSsimTap[k];
#pragma unroll
        for (int m = 0; m < 5; ++m) s[m] += g * rows[m][ty + k][tx];
      }
      const double mx = s[0], my = s[1];
      const double vx = s[2] - mx * mx, vy = s[3] - my * my, cxy = s[4] - mx * my;
      acc += ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2));
    }
    __syncthreads();                                      // rows is rewritten by the next channel
  }
  const double s = ns::block_sum(acc, wave_sums);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// a2: utils.py:159-217.  t[.,0] is the minus-sqrt root.
__global__ void __launch_bounds__(kBlock)
sphere_kernel(const float* __restrict__ o, const float* __restrict__ d, int64_t R, float radius,
              float* __restrict__ t_out, float* __restrict__ p_out) {
  for (int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x; r < R;
       r += (int64_t)gridDim.x * kBlock) {
    const float ox = o[r * 3], oy = o[r * 3 + 1], oz = o[r * 3 + 2];
    const float dx = d[r * 3], dy = d[r * 3 + 1], dz = d[r * 3 + 2];
    const float b = 2.0f * ((dx * ox + dy * oy) + dz * oz);
    const float on = sqrtf(__builtin_fmaf(oz, oz, __builtin_fmaf(oy, oy, ox * ox)));  // torch.norm(o)**2: sqrt, then square
    const float c = on * on - radius * radius;
    const float a = (dx * dx + dy * dy) + dz * dz;
    const float sq = sqrtf(b * b - 4.0f * a * c);           // NaN when the line misses
    const float t0 = (-b - sq) / (2.0f * a);
    const float t1 = (-b + sq) / (2.0f * a);
    if (t_out) { t_out[r * 2] = t0; t_out[r * 2 + 1] = t1; }
    if (p_out) {
      float* p = p_out + r * 6;
      p[0] = ox + t0 * dx; p[1] = oy + t0 * dy; p[2] = oz + t0 * dz;
      p[3] = ox + t1 * dx; p[4] = oy + t1 * dy; p[5] = oz + t1 * dz;
    }
  }
}

__global__ void __launch_bounds__(kBlock)
quadratic_kernel(const float* __restrict__ a, const float* __restrict__ b,
                 const float* __restrict__ c, int64_t n, float* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const float sq = sqrtf(b[i] * b[i] - 4.0f * a[i] * c[i]);
    out[i] = (-b[i] - sq) / (2.0f * a[i]);
    out[n + i] = (-b[i] + sq) / (2.0f * a[i]);
  }
}

// a3: run_nerf_helpers.py:15-63.  One thread per output element so stores are coalesced.
__global__ void __launch_bounds__(kBlock)
posenc_kernel(const float* __restrict__ x, int64_t M, int d, int L, float* __restrict__ out) {
  const int width = d * (1 + 2 * L);
  const int64_t total = M * width;
  for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kBlock) {
    const int64_t m = e / width;
    const int c = static_cast<int>(e % width);
    const int blk = c / d, comp = c % d;
    const float v = x[m * d + comp];
    float r;
    if (blk == 0) {
      r = v;
    } else {
      const int f = blk - 1;
      const float arg = v * exp2f(static_cast<float>(f >> 1));  // freq bands are exact powers of two
      r = (f & 1) ? cosf(arg) : sinf(arg);
    }
    out[e] = r;
  }
}

// a5: utils.py:220-244, values before any sort.  UNIFORM is emitted already sorted + clipped
// (the grid is increasing, so the mean is merged at its rank instead of sorting: nsplace::uniform_z).
__global__ void __launch_bounds__(kBlock)
place_z_kernel(int mode, const float* __restrict__ mean, const float* __restrict__ noise,
               int64_t R, int N, float std_, float* __restrict__ z) {
  const int64_t total = R * N;
  const float step = N > 2 ? (std_ - (-std_)) / static_cast<float>(N - 2) : 0.0f;   // linspace(-std, std, N - 1)
  for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kBlock) {
    const int64_t r = e / N;
    const int j = static_cast<int>(e % N);
    const float m = mean[r];
    float v;
    if (mode == NS_MODE_DEPTH_ONLY) {
      v = m;
    } else if (mode == NS_MODE_GAUSSIAN) {
      v = (j < N - 1) ? m + std_ * noise[r * (N - 1) + j] : m;
    } else {
      v = nsplace::uniform_z(m, std_, step, N - 1, j);   // already sorted + clipped (ns_place.h)
    }
    z[e] = v;
  }
}

// UNIFORM mode, N % 4 == 0: one thread per four consecutive samples of a ray, the store is a float4 (the generic kernel
// above is ~6x off the HBM rate at N = 64).
__global__ void __launch_bounds__(kBlock)
place_z_uniform4_kernel(const float* __restrict__ mean, int64_t R, int N, float std_, float4* __restrict__ z4) {
  const int q = N >> 2, steps = N - 1;
  const float step = steps > 1 ? (std_ - (-std_)) / static_cast<float>(steps - 1) : 0.0f;
  const int64_t total = R * q;
  for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t r = e / q;
    const int j0 = 4 * static_cast<int>(e - r * q);
    const float m = mean[r];
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = nsplace::uniform_z(m, std_, step, steps, j0 + k);
    z4[e] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

__global__ void __launch_bounds__(kBlock)
points_kernel(const float* __restrict__ o, const float* __restrict__ d,
              const float* __restrict__ z, int64_t R, int N, float* __restrict__ pts) {
  const int64_t total = R * N * 3;
  for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kBlock) {
    const int64_t s = e / 3;
    const int c = static_cast<int>(e % 3);
    const int64_t r = s / N;
    pts[e] = o[r * 3 + c] + d[r * 3 + c] * z[s];
  }
}

// a11: Trainer.py:603-626
__global__ void __launch_bounds__(kBlock)
coarse_z_kernel(const float* __restrict__ near_, const float* __restrict__ far_, float near_s, float far_s,
                int64_t R, int N, int lindisp, const float* __restrict__ t_rand, float* __restrict__ z) {
  const int64_t total = R * N;
  for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kBlock) {
    const int64_t r = e / N;
    const int i = static_cast<int>(e % N);
    const float nr = near_ ? near_[r] : near_s, fr = far_ ? far_[r] : far_s;
    auto zval = [&](int k) {
      const float t = linspace_at(0.0f, 1.0f, N, k);
      return lindisp ? 1.0f / (1.0f / nr * (1.0f - t) + 1.0f / fr * t) : nr * (1.0f - t) + fr * t;
    };
    float v = zval(i);
    if (t_rand) {
      const float upper = (i < N - 1) ? 0.5f * (zval(i + 1) + v) : v;
      const float lower = (i > 0) ? 0.5f * (v + zval(i - 1)) : v;
      v = lower + (upper - lower) * t_rand[e];
    }
    z[e] = v;
  }
}

// torch.sort(x, -1).values per row, one wave per row, bitonic in LDS; NaN sorts last.
__device__ __forceinline__ bool sort_less(float a, float b) {
  return !(a != a) && ((b != b) || a < b);
}

template <int P>
__global__ void __launch_bounds__(64)
sort_rows_kernel(const float* x, int64_t R, int N, float* out) {  // x may alias out
  __shared__ float buf[P];
  const int lane = threadIdx.x;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    for (int i = lane; i < P; i += 64) buf[i] = (i < N) ? x[r * N + i] : __builtin_nanf("");
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = lane; t < P / 2; t += 64) {
          const int lo = ((t / j) * 2 * j) + (t % j);
          const int hi = lo + j;
          const bool up = ((lo & k) == 0);
          const float a = buf[lo], b = buf[hi];
          const bool swap = up ? sort_less(b, a) : sort_less(a, b);
          if (swap) { buf[lo] = b; buf[hi] = a; }
        }
        __syncthreads();
      }
    }
    for (int i = lane; i < N; i += 64) out[r * N + i] = buf[i];
    __syncthreads();
  }
}

}  // namespace

extern "C" {

int ns_get_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w_host,
                int row0, int row1, float near_, float far_, float* rays_o_dev, float* rays_d_dev,
                float* viewdirs_dev, float* ray_batch_dev, void* stream) {
  NS_REQUIRE(H > 0 && W > 0 && c2w_host, "bad camera");
  NS_REQUIRE(row0 >= 0 && row1 <= H && row0 <= row1, "bad row range");
  const int64_t R = static_cast<int64_t>(row1 - row0) * W;
  if (R == 0) return NS_OK;
  Cam cam{fx, fy, cx, cy, {}, {}};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) cam.r[3 * r + c] = c2w_host[4 * r + c];
    cam.t[r] = c2w_host[4 * r + 3];
  }
  get_rays_kernel<<<ns::ew_grid(R, kBlock), kBlock, 0, ns::as_stream(stream)>>>(
      cam, W, row0, R, near_, far_, rays_o_dev, rays_d_dev, viewdirs_dev, ray_batch_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

// what both ray-batch entries ask of the dataset descriptor and the batch size
static int check_ray_dataset(const ns_ray_dataset* ds, int64_t B, bool rays, bool target, const char* who) {
  auto bad = [&](const char* msg) { ns::set_error("%s: %s", who, msg); return NS_E_INVALID; };
  if (!ds) return bad("null dataset");
  if (B < 0 || B >= (int64_t(1) << 31)) return bad("batch size outside [0, 2^31)");
  if (ds->n_images <= 0 || ds->H <= 0 || ds->W <= 0) return bad("empty dataset");
  if (static_cast<int64_t>(ds->n_images) * ds->H * ds->W >= (int64_t(1) << 31)) return bad("n_images * H * W must be below 2^31");
  if (ds->C != 3 && ds->C != 4) return bad("images have 3 or 4 channels");
  if (ds->pose_stride != 12 && ds->pose_stride != 16) return bad("pose_stride is 12 or 16 floats");
  if (rays && !ds->poses_dev) return bad("rays requested without poses");
  if (target && !ds->images_dev) return bad("target requested without images");
  return NS_OK;
}

int ns_ray_batch_gather(const ns_ray_dataset* ds, const int* image_idx_dev, int image_idx, const int* pixel_dev, int64_t B,
                        float* rays_o_dev, float* rays_d_dev, float* viewdirs_dev, float* target_dev, void* stream) {
  const int rc = check_ray_dataset(ds, B, rays_o_dev || rays_d_dev || viewdirs_dev, target_dev != nullptr, __func__);
  if (rc != NS_OK) return rc;
  NS_REQUIRE(image_idx_dev || (image_idx >= 0 && image_idx < ds->n_images), "image index out of range");
  if (B == 0) return NS_OK;
  NS_REQUIRE(pixel_dev, "null pixel indices");
  ray_batch_gather_kernel<<<ns::ew_grid(B, kBlock), kBlock, 0, ns::as_stream(stream)>>>(
      *ds, image_idx_dev, image_idx, pixel_dev, B, BatchOut{rays_o_dev, rays_d_dev, viewdirs_dev, target_dev});
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_ray_batch_draw(const ns_ray_dataset* ds, const int* train_idx_dev, int n_train, int scope, const int* params_dev,
                      const ns_ray_draw_params* params_host, uint64_t seed, int64_t B, int* image_idx_out_dev,
                      int* pixel_out_dev, float* rays_o_dev, float* rays_d_dev, float* viewdirs_dev, float* target_dev,
                      void* stream) {
  const int rc = check_ray_dataset(ds, B, rays_o_dev || rays_d_dev || viewdirs_dev, target_dev != nullptr, __func__);
  if (rc != NS_OK) return rc;
  NS_REQUIRE(scope == NS_RAY_SCOPE_PER_IMAGE || scope == NS_RAY_SCOPE_ALL_IMAGES, "unknown scope");
  NS_REQUIRE(train_idx_dev && n_train > 0, "no training images");
  NS_REQUIRE(static_cast<int64_t>(n_train) * ds->H * ds->W < (int64_t(1) << 31), "n_train * H * W must be below 2^31");
  NS_REQUIRE((params_dev != nullptr) != (params_host != nullptr), "params come from the device or from the host");
  ns_ray_draw_params host{0, 0, ds->H, 0, ds->W};
  if (params_host) {
    host = *params_host;
    NS_REQUIRE(host.step >= 0, "negative step");
    if (scope == NS_RAY_SCOPE_PER_IMAGE) {
      NS_REQUIRE(host.row0 >= 0 && host.row1 <= ds->H && host.col0 >= 0 && host.col1 <= ds->W, "window outside the frame");
      NS_REQUIRE(host.row0 < host.row1 && host.col0 < host.col1, "empty window");
      NS_REQUIRE(B <= static_cast<int64_t>(host.row1 - host.row0) * (host.col1 - host.col0),
                 "a per-image batch is drawn without replacement: B exceeds the window");
    }
  }
  if (B == 0) return NS_OK;
  ray_batch_draw_kernel<<<ns::ew_grid(B, kBlock), kBlock, 0, ns::as_stream(stream)>>>(
      *ds, train_idx_dev, n_train, scope, params_dev, host, seed, B, image_idx_out_dev, pixel_out_dev,
      BatchOut{rays_o_dev, rays_d_dev, viewdirs_dev, target_dev});
  NS_LAUNCH_CHECK();
  return NS_OK;
}

static int64_t image_sqerr_groups(int64_t n_pixels) { return ns::cdiv(n_pixels, kSqerrShare); }

int64_t ns_image_sqerr_workspace_bytes(int64_t n_pixels) {
  if (n_pixels <= 0) return 0;
  return ns::round_256(image_sqerr_groups(n_pixels) * static_cast<int64_t>(sizeof(double)));
}

int ns_image_sqerr(const ns_ray_dataset* ds, int image_idx, int row0, int row1, const float* rgb_dev, int64_t rgb_stride,
                   double* sum_dev, void* workspace_dev, void* stream) {
  const int rc = check_ray_dataset(ds, 0, false, true, __func__);
  if (rc != NS_OK) return rc;
  NS_REQUIRE(image_idx >= 0 && image_idx < ds->n_images, "image index out of range");
  NS_REQUIRE(row0 >= 0 && row1 <= ds->H, "row band outside the frame");
  NS_REQUIRE(row0 < row1, "empty row band");
  NS_REQUIRE(rgb_stride == 0 || rgb_stride == 3 || rgb_stride == 4, "rgb_stride is 0 (packed), 3 or 4 floats");
  NS_REQUIRE(rgb_dev && sum_dev && workspace_dev, "null pointer");
  const int n = (row1 - row0) * ds->W;                       // below 2^31: check_ray_dataset bounds n_images * H * W
  const int groups = static_cast<int>(image_sqerr_groups(n));
  double* partial = static_cast<double*>(workspace_dev);
  hipStream_t s = ns::as_stream(stream);
  image_sqerr_kernel<<<groups, kBlock, 0, s>>>(*ds, image_idx, row0 * ds->W, n, rgb_dev,
                                               rgb_stride == 0 ? 3 : static_cast<int>(rgb_stride), partial);
  NS_LAUNCH_CHECK();
  image_sqerr_combine_kernel<<<1, kBlock, 0, s>>>(partial, groups, sum_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int64_t ns_depth_sqerr_workspace_bytes(int64_t R, int N) {
  if (!ns::flat_shape_ok(R, N)) return 0;
  return ns::round_256(ns::cdiv(R * N, kDepthShare) * static_cast<int64_t>(sizeof(double)));
}

int ns_depth_sqerr(const float* z_dev, int64_t z_row_stride, const float* ref_dev, int64_t R, int N, double* sum_dev,
                   void* workspace_dev, void* stream) {
  NS_REQUIRE(z_dev && ref_dev && sum_dev && workspace_dev, "null pointer");
  NS_REQUIRE(R >= 1 && N >= 1, "R and N must be at least 1");
  NS_REQUIRE(ns::flat_shape_ok(R, N), "R * N must be below 2^31");
  NS_REQUIRE(z_row_stride == 0 || z_row_stride >= N, "z_row_stride is 0 (packed) or at least N floats");
  const int64_t total = R * N;
  const int groups = static_cast<int>(ns::cdiv(total, kDepthShare));
  double* partial = static_cast<double*>(workspace_dev);
  hipStream_t s = ns::as_stream(stream);
  depth_sqerr_kernel<<<groups, kBlock, 0, s>>>(z_dev, z_row_stride == 0 ? N : z_row_stride, ref_dev,
                                               static_cast<uint32_t>(total), static_cast<uint32_t>(N), partial);
  NS_LAUNCH_CHECK();
  image_sqerr_combine_kernel<<<1, kBlock, 0, s>>>(partial, groups, sum_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

// tiles of window origins along the rows / the columns of an H x W frame (H, W >= 11)
static int64_t image_ssim_tiles_y(int H) { return (H - (kSsimWin - 1) + kSsimTileH - 1) / kSsimTileH; }
static int64_t image_ssim_tiles_x(int W) { return (W - (kSsimWin - 1) + kSsimTileW - 1) / kSsimTileW; }

void ns_image_ssim_tile(int* tile_h, int* tile_w) {
  if (tile_h) *tile_h = kSsimTileH;
  if (tile_w) *tile_w = kSsimTileW;
}

int64_t ns_image_ssim_workspace_bytes(int H, int W) {
  if (H < kSsimWin || W < kSsimWin) return 0;
  return ns::round_256(image_ssim_tiles_y(H) * image_ssim_tiles_x(W) * static_cast<int64_t>(sizeof(double)));
}

int ns_image_ssim(const ns_ray_dataset* ds, int image_idx, const float* rgb_dev, int64_t rgb_stride, double* sum_dev,
                  void* workspace_dev, void* stream) {
  const int rc = check_ray_dataset(ds, 0, false, true, __func__);
  if (rc != NS_OK) return rc;
  NS_REQUIRE(ds->H >= kSsimWin && ds->W >= kSsimWin, "the frame is smaller than the 11 x 11 window");
  NS_REQUIRE(image_idx >= 0 && image_idx < ds->n_images, "image index out of range");
  NS_REQUIRE(rgb_stride == 0 || rgb_stride == 3 || rgb_stride == 4, "rgb_stride is 0 (packed), 3 or 4 floats");
  NS_REQUIRE(rgb_dev && sum_dev && workspace_dev, "null pointer");
  const int tiles_x = static_cast<int>(image_ssim_tiles_x(ds->W));
  const int groups = static_cast<int>(image_ssim_tiles_y(ds->H)) * tiles_x;    // below 2^31 / 256: H * W is below 2^31
  double* partial = static_cast<double*>(workspace_dev);
  hipStream_t s = ns::as_stream(stream);
  image_ssim_kernel<<<groups, kBlock, 0, s>>>(*ds, image_idx, tiles_x, rgb_dev, rgb_stride == 0 ? 3 : static_cast<int>(rgb_stride),
                                              partial);
  NS_LAUNCH_CHECK();
  image_sqerr_combine_kernel<<<1, kBlock, 0, s>>>(partial, groups, sum_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_sphere_intersect(const float* o_dev, const float* d_dev, int64_t R, float radius,
                        float* t_dev, float* pts_dev, void* stream) {
  NS_REQUIRE(R >= 0, "negative ray count");
  if (R == 0) return NS_OK;
  NS_REQUIRE(o_dev && d_dev, "null rays");
  sphere_kernel<<<ns::ew_grid(R, kBlock), kBlock, 0, ns::as_stream(stream)>>>(o_dev, d_dev, R, radius,
                                                                             t_dev, pts_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_solve_quadratic(const float* a_dev, const float* b_dev, const float* c_dev, int64_t n,
                       float* out_dev, void* stream) {
  NS_REQUIRE(n >= 0, "negative size");
  if (n == 0) return NS_OK;
  NS_REQUIRE(a_dev && b_dev && c_dev && out_dev, "null pointer");
  quadratic_kernel<<<ns::ew_grid(n, kBlock), kBlock, 0, ns::as_stream(stream)>>>(a_dev, b_dev, c_dev, n,
                                                                                out_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_posenc(const float* x_dev, int64_t M, int d, int n_freqs, float* out_dev, void* stream) {
  NS_REQUIRE(M >= 0 && d > 0 && n_freqs >= 0, "bad shape");
  if (M == 0) return NS_OK;
  NS_REQUIRE(x_dev && out_dev, "null pointer");
  posenc_kernel<<<ns::ew_grid(M * d * (1 + 2 * n_freqs), kBlock), kBlock, 0, ns::as_stream(stream)>>>(
      x_dev, M, d, n_freqs, out_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_sort_rows(const float* x_dev, int64_t R, int N, float* out_dev, void* stream) {
  NS_REQUIRE(R >= 0 && N >= 0, "bad shape");
  if (R == 0 || N == 0) return NS_OK;
  NS_REQUIRE(x_dev && out_dev, "null pointer");
  NS_REQUIRE(N <= 2048, "rows longer than 2048 are not supported");
  const int grid = static_cast<int>(R < 256 * 32 ? R : 256 * 32);
  hipStream_t s = ns::as_stream(stream);
  if (N <= 64) sort_rows_kernel<64><<<grid, 64, 0, s>>>(x_dev, R, N, out_dev);
  else if (N <= 128) sort_rows_kernel<128><<<grid, 64, 0, s>>>(x_dev, R, N, out_dev);
  else if (N <= 256) sort_rows_kernel<256><<<grid, 64, 0, s>>>(x_dev, R, N, out_dev);
  else if (N <= 512) sort_rows_kernel<512><<<grid, 64, 0, s>>>(x_dev, R, N, out_dev);
  else if (N <= 1024) sort_rows_kernel<1024><<<grid, 64, 0, s>>>(x_dev, R, N, out_dev);
  else sort_rows_kernel<2048><<<grid, 64, 0, s>>>(x_dev, R, N, out_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_points_along_rays(const float* o_dev, const float* d_dev, const float* z_dev, int64_t R,
                         int N, float* pts_dev, void* stream) {
  NS_REQUIRE(R >= 0 && N >= 0, "bad shape");
  if (R == 0 || N == 0) return NS_OK;
  NS_REQUIRE(o_dev && d_dev && z_dev && pts_dev, "null pointer");
  points_kernel<<<ns::ew_grid(R * N * 3, kBlock), kBlock, 0, ns::as_stream(stream)>>>(o_dev, d_dev, z_dev,
                                                                                      R, N, pts_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

int ns_place_samples(int mode, const float* o_dev, const float* d_dev, const float* mean_dev,
                     const float* noise_dev, int64_t R, int N, float std_, float* pts_dev,
                     float* z_dev, void* stream) {
  NS_REQUIRE(mode == NS_MODE_DEPTH_ONLY || mode == NS_MODE_UNIFORM || mode == NS_MODE_GAUSSIAN,
             "unknown mode");
  if (mode == NS_MODE_DEPTH_ONLY) N = 1;
  NS_REQUIRE(R >= 0 && N >= 1, "bad shape");
  if (R == 0) return NS_OK;
  NS_REQUIRE(mean_dev && z_dev, "mean and z are required");
  NS_REQUIRE(mode != NS_MODE_GAUSSIAN || N == 1 || noise_dev, "gaussian mode needs the noise draws");
  NS_REQUIRE(mode != NS_MODE_UNIFORM || N >= 2, "uniform mode needs n_samples >= 2");
  if (mode == NS_MODE_UNIFORM && (N & 3) == 0 && (reinterpret_cast<uintptr_t>(z_dev) & 15) == 0)
    place_z_uniform4_kernel<<<ns::ew_grid(R * (N >> 2), kBlock), kBlock, 0, ns::as_stream(stream)>>>(
        mean_dev, R, N, std_, reinterpret_cast<float4*>(z_dev));
  else
    place_z_kernel<<<ns::ew_grid(R * N, kBlock), kBlock, 0, ns::as_stream(stream)>>>(mode, mean_dev, noise_dev,
                                                                                    R, N, std_, z_dev);
  NS_LAUNCH_CHECK();
  if (mode == NS_MODE_GAUSSIAN && N > 1) {
    int rc = ns_sort_rows(z_dev, R, N, z_dev, stream);
    if (rc != NS_OK) return rc;
  }
  if (pts_dev) {
    NS_REQUIRE(o_dev && d_dev, "pts requested without rays");
    return ns_points_along_rays(o_dev, d_dev, z_dev, R, N, pts_dev, stream);
  }
  return NS_OK;
}

int ns_coarse_z(const float* near_dev, const float* far_dev, int64_t R, int N, int lindisp,
                const float* t_rand_dev, float* z_dev, void* stream) {
  NS_REQUIRE(R >= 0 && N >= 1, "bad shape");
  if (R == 0) return NS_OK;
  NS_REQUIRE(near_dev && far_dev && z_dev, "null pointer");
  coarse_z_kernel<<<ns::ew_grid(R * N, kBlock), kBlock, 0, ns::as_stream(stream)>>>(near_dev, far_dev, 0.f, 0.f, R, N,
                                                                                   lindisp, t_rand_dev, z_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

// same with one near / far for every ray (used by ns_render_rays_hierarchical)
int ns_coarse_z_scalar(float near_, float far_, int64_t R, int N, int lindisp, const float* t_rand_dev,
                       float* z_dev, void* stream) {
  NS_REQUIRE(R >= 0 && N >= 1, "bad shape");
  if (R == 0) return NS_OK;
  NS_REQUIRE(z_dev, "null pointer");
  coarse_z_kernel<<<ns::ew_grid(R * N, kBlock), kBlock, 0, ns::as_stream(stream)>>>(nullptr, nullptr, near_, far_, R, N,
                                                                                   lindisp, t_rand_dev, z_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
