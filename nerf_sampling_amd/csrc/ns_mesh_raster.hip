// The device mesh rasterised from a pinhole camera (ns_mesh_raster): a z-buffer of 64-bit words (depth bits, face index) merged by
// an unsigned atomic minimum, coverage in exact integer arithmetic on vertices snapped to 1/256 pixel, depth and colour in fp64.
// Built with -ffp-contract=off: every fp32 and fp64 operation is rounded on its own and the divisions are the correctly rounded
// ones, so numpy restates the bits; the minimum and the integer counts do not depend on the order of the atomics, so a frame is
// a function of the inputs alone.  The header's comment block is the contract; this file only adds how the work is laid out.
//
// Five launches on one stream (two where F == 0), nothing read back in between, no workgroup waits for another:
//   clear    one thread per pixel: the z-buffer word <- all ones; the four counters and the length of the big list <- 0;
//   project  one thread per vertex: (X, Y, z, usable) into the workspace, 16 bytes per vertex;
//   faces    workgroup g owns faces [g * kShare, (g + 1) * kShare), thread t takes g * kShare + s * kBlock + t: the face is
//            checked, counted, culled, and -- its clamped bounding box having at most big_box pixels -- rasterised by that one
//            thread; a larger one is appended to the big list (an integer atomicAdd on its length: the ORDER of the list
//            varies from run to run, the set does not, and the z-buffer does not depend on the order);
//   big      a fixed grid that strides over the big list, whose length it reads from device memory: entry e is cut into tiles
//            of 16 x 16 pixels, tile t goes to workgroup (t + e) mod grid, one pixel per thread -- so one frame-covering
//            triangle is spread over the whole grid instead of being a 640 000-iteration loop in one lane;
//   resolve  one thread per pixel: the word taken apart, the colour interpolated, the covered pixels counted.
// Which of the two paths a face takes is not observable: both call the same coverage, depth and merge functions.
#include <cmath>

#include "ns_block.h"
#include "ns_common.h"
#include "ns_mesh_raster_cover.h"

namespace {

using ns::kBlock;
using ns::kWaves;
using ns_raster::covered;
using ns_raster::edge_values;
using ns_raster::kBand;
using ns_raster::Proj;
using ns_raster::setup;
using ns_raster::Tri;
constexpr int kShare = NS_MESH_RASTER_SHARE;
constexpr int kSteps = ns::ShareOf<kShare>::steps;
constexpr int kBigGrid = 1024;               // workgroups of the big launch: four per CU, whatever the list holds
constexpr int kTile = 16;                    // a workgroup's tile of a big face: kTile x kTile = kBlock pixels
static_assert(kTile * kTile == kBlock, "one pixel of a tile per thread");
constexpr unsigned long long kEmpty = ~0ull;

struct Cam {
  float fx, fy, cx, cy;
  float r[9];  // c2w[:3,:3] row-major
  float t[3];  // c2w[:3,3]
  float near_;
};

__device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the inverse of pixel_ray (ns_rays.hip): q = R^T (p - t), z = -q_2, x = cx + fx (q_0 / z), y = cy - fy (q_1 / z)
__device__ __forceinline__ Proj project(const Cam& cam, const float* __restrict__ p) {
  const float e0 = p[0] - cam.t[0], e1 = p[1] - cam.t[1], e2 = p[2] - cam.t[2];
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = (e0 * cam.r[k] + e1 * cam.r[3 + k]) + e2 * cam.r[6 + k];
  const float z = -q[2];
  const float x = cam.cx + cam.fx * (q[0] / z);
  const float y = cam.cy - cam.fy * (q[1] / z);
  Proj out;
  out.usable = finite(x) && finite(y) && finite(z) && !(z < cam.near_) && !(fabsf(x) > kBand) && !(fabsf(y) > kBand);
  out.X = out.usable ? static_cast<int32_t>(static_cast<int64_t>(rintf(x * 256.0f))) : 0;
  out.Y = out.usable ? static_cast<int32_t>(static_cast<int64_t>(rintf(y * 256.0f))) : 0;
  out.z = z;
  return out;
}

// s = sum of w_k / z_k, added left to right in fp64: area2 / s is the perspective-correct depth (1 / z is affine on the screen)
__device__ __forceinline__ double inverse_depth_sum(const Tri& t, const int64_t (&w)[3], double (&q)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = static_cast<double>(w[k]) / t.z[k];
  return (q[0] + q[1]) + q[2];
}

// One pixel of one face: covered -> its fragment merged into the z-buffer word.
__device__ __forceinline__ void shade(const Tri& t, uint32_t face, int i, int j, int W, unsigned long long* zbuf) {
  int64_t w[3];
  edge_values(t, i, j, w);
  if (!covered(t, w)) return;
  double q[3];
  const double s = inverse_depth_sum(t, w, q);
  const float zpix = static_cast<float>(static_cast<double>(t.area2) / s);
  const unsigned long long frag = (static_cast<unsigned long long>(__float_as_uint(zpix)) << 32) | face;
  unsigned long long* word = zbuf + (static_cast<int64_t>(j) * W + i);
  // A plain load ahead of the atomic: the word only ever decreases during these launches, so a stale value read here is
  // never below the current one -- a fragment that does not beat it cannot win, and one that beats a stale value only costs
  // an atomic whose minimum changes nothing.
  if (frag < *word) atomicMin(word, frag);
}

__global__ void __launch_bounds__(kBlock)
raster_clear_kernel(unsigned long long* __restrict__ zbuf, int64_t pixels, unsigned long long* __restrict__ count,
                    uint32_t* __restrict__ big_len) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (p < pixels) zbuf[p] = kEmpty;
  if (p < 4) count[p] = 0;
  if (p == 0) *big_len = 0;
}

__global__ void __launch_bounds__(kBlock)
raster_project_kernel(Cam cam, const float* __restrict__ vertices, int64_t V, Proj* __restrict__ proj) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (v < V) proj[v] = project(cam, vertices + v * 3);
}

// -> 0 ready, 1 clipped, 2 degenerate, 3 invalid, 4 culled or off the frame.  No index is used before it is known to be valid.
__device__ __forceinline__ int load_face(const int64_t* __restrict__ faces, int64_t f, int64_t V, const Proj* __restrict__ proj,
                                         int H, int W, int cull, Tri& t) {
  const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) return 3;
  const Proj v[3] = {proj[a], proj[b], proj[c]};
  if (!(v[0].usable && v[1].usable && v[2].usable)) return 1;
  setup(v, H, W, t);
  if (t.area2 == 0) return 2;
  // seen from outside, ns_mesh_extract's outward winding has area2 < 0 (x to the right, y DOWN): that is the front
  if ((cull == 1 && t.area2 > 0) || (cull == 2 && t.area2 < 0)) return 4;
  if (t.i0 > t.i1 || t.j0 > t.j1) return 4;
  return 0;
}

__global__ void __launch_bounds__(kBlock)
raster_faces_kernel(const int64_t* __restrict__ faces, int64_t F, int64_t V, const Proj* __restrict__ proj, int H, int W,
                    int cull, int big_box, unsigned long long* zbuf, int32_t* __restrict__ big_list, uint32_t* big_len,
                    unsigned long long* count) {
  __shared__ int wave_counts[3][kWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int counts[3] = {0, 0, 0};                               // clipped, degenerate, invalid
  for (int s = 0; s < kSteps; ++s) {
    const int64_t f = base + s * kBlock;
    if (f >= F) continue;
    Tri t;
    const int what = load_face(faces, f, V, proj, H, W, cull, t);
    if (what >= 1 && what <= 3) ++counts[what - 1];
    if (what != 0) continue;
    const int wide = t.i1 - t.i0 + 1, tall = t.j1 - t.j0 + 1;             // at most 2^14 each
    if (wide * tall > big_box) {
      big_list[atomicAdd(big_len, 1u)] = static_cast<int32_t>(f);         // at most F entries: every face is appended once
      continue;
    }
    for (int j = t.j0; j <= t.j1; ++j)                                    // at most big_box pixels
      for (int i = t.i0; i <= t.i1; ++i) shade(t, static_cast<uint32_t>(f), i, j, W, zbuf);
  }
  ns::wave_sum_to(counts[0], wave_counts[0], counts[1], wave_counts[1]);
  ns::wave_sum_to(counts[2], wave_counts[2]);
  __syncthreads();
  if (threadIdx.x < 3) {
    const int n = ns::slots_sum(wave_counts[threadIdx.x]);
    if (n > 0) atomicAdd(count + threadIdx.x, static_cast<unsigned long long>(n));       // integers: any order, one total
  }
}

__global__ void __launch_bounds__(kBlock)
raster_big_kernel(const int64_t* __restrict__ faces, int64_t V, const Proj* __restrict__ proj, int H, int W, int cull,
                  unsigned long long* zbuf, const int32_t* __restrict__ big_list, const uint32_t* __restrict__ big_len) {
  const uint32_t n = *big_len;
  const int li = threadIdx.x % kTile, lj = threadIdx.x / kTile;
  for (uint32_t e = 0; e < n; ++e) {
    const int64_t f = big_list[e];
    Tri t;
    if (load_face(faces, f, V, proj, H, W, cull, t) != 0) continue;       // never: the faces launch appended it as ready
    const int tiles_x = (t.i1 - t.i0 + kTile) / kTile, tiles_y = (t.j1 - t.j0 + kTile) / kTile;
    const int tiles = tiles_x * tiles_y;                                  // at most 2^20
    const int first = static_cast<int>((blockIdx.x + kBigGrid - e % kBigGrid) % kBigGrid);
    for (int tile = first; tile < tiles; tile += kBigGrid) {
      const int i = t.i0 + (tile % tiles_x) * kTile + li, j = t.j0 + (tile / tiles_x) * kTile + lj;
      if (i <= t.i1 && j <= t.j1) shade(t, static_cast<uint32_t>(f), i, j, W, zbuf);
    }
  }
}

// zbuf == NULL: a frame without faces -- every pixel empty, and the four counters written here
__global__ void __launch_bounds__(kBlock)
raster_resolve_kernel(const unsigned long long* __restrict__ zbuf, int64_t pixels, int W, int H, const int64_t* __restrict__ faces,
                      const Proj* __restrict__ proj, const float* __restrict__ attr, float background,
                      float* __restrict__ depth_out, int32_t* __restrict__ tri_out, float* __restrict__ rgb_out,
                      unsigned long long* count) {
  __shared__ int wave_counts[kWaves];
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  int hit = 0;
  if (p < pixels) {
    const unsigned long long word = zbuf ? zbuf[p] : kEmpty;
    if (word == kEmpty) {
      if (depth_out) depth_out[p] = 0.0f;
      if (tri_out) tri_out[p] = -1;
      if (rgb_out) rgb_out[p * 3] = rgb_out[p * 3 + 1] = rgb_out[p * 3 + 2] = background;
    } else {
      hit = 1;
      const int64_t f = static_cast<int64_t>(word & 0xffffffffull);
      if (depth_out) depth_out[p] = __uint_as_float(static_cast<uint32_t>(word >> 32));
      if (tri_out) tri_out[p] = static_cast<int32_t>(f);
      if (rgb_out) {
        const int64_t idx[3] = {faces[f * 3], faces[f * 3 + 1], faces[f * 3 + 2]};       // valid: the face left a fragment
        const Proj v[3] = {proj[idx[0]], proj[idx[1]], proj[idx[2]]};
        Tri t;
        setup(v, H, W, t);
        int64_t w[3];
        edge_values(t, static_cast<int>(p % W), static_cast<int>(p / W), w);
        double q[3];
        const double s = inverse_depth_sum(t, w, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double num = (q[0] * static_cast<double>(attr[idx[0] * 3 + c]) + q[1] * static_cast<double>(attr[idx[1] * 3 + c])) +
                             q[2] * static_cast<double>(attr[idx[2] * 3 + c]);
          rgb_out[p * 3 + c] = static_cast<float>(num / s);
        }
      }
    }
  }
  const int n = ns::block_sum(hit, wave_counts);
  if (zbuf == nullptr) {
    if (blockIdx.x == 0 && threadIdx.x < 4) count[threadIdx.x] = 0;
  } else if (threadIdx.x == 0 && n > 0) {
    atomicAdd(count + 3, static_cast<unsigned long long>(n));
  }
}

bool frame_ok(int H, int W) { return H >= 1 && W >= 1 && H <= 16384 && W <= 16384; }
bool count_ok(int64_t n) { return n >= 0 && ns::below_2_31(n); }

struct Layout {  // the workspace: z-buffer words, projected vertices, the big list, its length
  int64_t proj, big_list, big_len, bytes;
};
Layout layout(int64_t V, int64_t F, int H, int W) {
  Layout l;
  l.proj = ns::round_256(static_cast<int64_t>(H) * W * 8);
  l.big_list = l.proj + ns::round_256(V * static_cast<int64_t>(sizeof(Proj)));
  l.big_len = l.big_list + ns::round_256(F * 4);
  l.bytes = l.big_len + 256;
  return l;
}

}  // namespace

extern "C" {

int64_t ns_mesh_raster_workspace_bytes(int64_t V, int64_t F, int H, int W) {
  if (!frame_ok(H, W) || !count_ok(V) || !count_ok(F) || F == 0) return 0;
  return layout(V, F, H, W).bytes;
}

int ns_mesh_raster(const float* vertices_dev, int64_t V, const int64_t* faces_dev, int64_t F, const float* attr_dev,
                   const float* c2w_host, float fx, float fy, float cx, float cy, int H, int W, float near_, int cull,
                   float background, float* depth_out, int32_t* tri_out, float* rgb_out, int64_t* count_dev,
                   void* workspace_dev, void* stream) {
  NS_REQUIRE(frame_ok(H, W), "H and W must lie in [1, 16384]");
  NS_REQUIRE(count_ok(V) && count_ok(F), "V and F must lie in [0, 2^31)");
  NS_REQUIRE(c2w_host, "c2w_host is required");
  for (int k = 0; k < 12; ++k) NS_REQUIRE(std::isfinite(c2w_host[k]), "c2w must be finite");
  NS_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy), "fx, fy, cx, cy must be finite");
  NS_REQUIRE(fx != 0.0f && fy != 0.0f, "fx and fy must not be 0");
  NS_REQUIRE(std::isfinite(near_) && near_ > 0.0f, "near_ must be finite and positive");
  NS_REQUIRE(std::isfinite(background), "background must be finite");
  NS_REQUIRE(cull >= 0 && cull <= 2, "cull is 0 (none), 1 (back faces) or 2 (front faces)");
  NS_REQUIRE(count_dev, "count_dev is required");
  NS_REQUIRE(F == 0 || (vertices_dev && faces_dev && workspace_dev),
             "vertices_dev, faces_dev and workspace_dev are required when F > 0");
  NS_REQUIRE(!rgb_out || attr_dev, "rgb_out needs attr_dev");
  NS_REQUIRE(ns::aligned(faces_dev, 8) && ns::aligned(count_dev, 8) && ns::aligned(workspace_dev, 8),
             "faces_dev, count_dev and workspace_dev are 8-byte aligned");
  Cam cam{fx, fy, cx, cy, {}, {}, near_};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) cam.r[3 * r + c] = c2w_host[4 * r + c];
    cam.t[r] = c2w_host[4 * r + 3];
  }
  const int64_t pixels = static_cast<int64_t>(H) * W;                    // at most 2^28
  const int pixel_groups = static_cast<int>(ns::cdiv(pixels, kBlock));
  unsigned long long* count = reinterpret_cast<unsigned long long*>(count_dev);
  hipStream_t s = ns::as_stream(stream);
  if (F == 0) {
    raster_resolve_kernel<<<pixel_groups, kBlock, 0, s>>>(nullptr, pixels, W, H, nullptr, nullptr, nullptr, background, depth_out,
                                                          tri_out, rgb_out, count);
    NS_LAUNCH_CHECK();
    return NS_OK;
  }
  const Layout l = layout(V, F, H, W);
  char* ws = static_cast<char*>(workspace_dev);
  unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(ws);
  Proj* proj = reinterpret_cast<Proj*>(ws + l.proj);
  int32_t* big_list = reinterpret_cast<int32_t*>(ws + l.big_list);
  uint32_t* big_len = reinterpret_cast<uint32_t*>(ws + l.big_len);
  const int big_box = ns::debug_flags().mesh_raster_big_box > 0 ? ns::debug_flags().mesh_raster_big_box : NS_MESH_RASTER_BIG_BOX;
  raster_clear_kernel<<<pixel_groups, kBlock, 0, s>>>(zbuf, pixels, count, big_len);
  NS_LAUNCH_CHECK();
  if (V > 0) {
    raster_project_kernel<<<static_cast<int>(ns::cdiv(V, kBlock)), kBlock, 0, s>>>(cam, vertices_dev, V, proj);
    NS_LAUNCH_CHECK();
  }
  raster_faces_kernel<<<static_cast<int>(ns::cdiv(F, kShare)), kBlock, 0, s>>>(faces_dev, F, V, proj, H, W, cull, big_box, zbuf,
                                                                               big_list, big_len, count);
  NS_LAUNCH_CHECK();
  raster_big_kernel<<<kBigGrid, kBlock, 0, s>>>(faces_dev, V, proj, H, W, cull, zbuf, big_list, big_len);
  NS_LAUNCH_CHECK();
  raster_resolve_kernel<<<pixel_groups, kBlock, 0, s>>>(zbuf, pixels, W, H, faces_dev, proj, attr_dev, background, depth_out,
                                                        tri_out, rgb_out, count);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
