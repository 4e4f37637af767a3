// The integer half of ns_mesh_raster: a projected vertex, a face set up for rasterising, its edge values at a pixel centre and the
// coverage test with the tie rule -- one statement for the kernels and for the CPU alike (tools/mesh_raster_hostcheck.cpp runs it
// under a host sanitizer and compares it with the header's rule written with plain loops).  Integers only: no rounding anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns_raster {

constexpr int kSub = 256;                    // sub-pixel steps per pixel: eight bits
// A usable vertex has |x|, |y| <= 2^20 pixels, so its snapped |X|, |Y| <= 2^28; a pixel centre has 0 <= 256 i < 2^22 (i < 2^14).
// Every difference in an edge function is therefore below 2^29 in magnitude, a product below 2^58, and an edge value -- the
// difference of two products -- below 2^59: an int64 with four bits to spare.  The snapped coordinates themselves fit an int32.
constexpr float kBand = 1048576.0f;          // 2^20 pixels: a vertex projected beyond it is unusable (ns_mesh_raster.hip)

struct alignas(8) Proj {  // 16 bytes; the workspace is 8-byte aligned
  int32_t X, Y;
  float z;
  int32_t usable;
};

__host__ __device__ inline int32_t min2(int32_t a, int32_t b) { return a < b ? a : b; }
__host__ __device__ inline int32_t max2(int32_t a, int32_t b) { return a > b ? a : b; }
__host__ __device__ inline int32_t min3(int32_t a, int32_t b, int32_t c) { return min2(a, min2(b, c)); }
__host__ __device__ inline int32_t max3(int32_t a, int32_t b, int32_t c) { return max2(a, max2(b, c)); }

// A face ready to be rasterised.  w_k, the edge value opposite vertex k, at pixel (i, j) is c[k] + j * sj[k] - i * si[k]:
// w_0 = E_12, w_1 = E_20, w_2 = E_01, which sum to area2 at every point.
struct Tri {
  int64_t c[3], si[3], sj[3];
  int64_t area2;
  int32_t bias[3];         // 0: a pixel centre exactly on this edge is covered; 1: it is not
  int32_t sign;            // of area2
  double z[3];
  int32_t i0, i1, j0, j1;  // the bounding box clamped to the frame (empty: i0 > i1 or j0 > j1)
};

__host__ __device__ inline int32_t floor_div_sub(int32_t v) { return v >> 8; }            // floor(v / 256), arithmetic shift
__host__ __device__ inline int32_t ceil_div_sub(int32_t v) { return (v + (kSub - 1)) >> 8; }

__host__ __device__ inline void setup(const Proj (&v)[3], int H, int W, Tri& t) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const Proj &a = v[(k + 1) % 3], &b = v[(k + 2) % 3];
    const int64_t dx = static_cast<int64_t>(b.X) - a.X, dy = static_cast<int64_t>(b.Y) - a.Y;
    t.c[k] = dy * a.X - dx * a.Y;
    t.si[k] = dy * kSub;
    t.sj[k] = dx * kSub;
    t.z[k] = static_cast<double>(v[k].z);
  }
  // E_01(V_2)
  t.area2 = (static_cast<int64_t>(v[1].X) - v[0].X) * (static_cast<int64_t>(v[2].Y) - v[0].Y) -
            (static_cast<int64_t>(v[1].Y) - v[0].Y) * (static_cast<int64_t>(v[2].X) - v[0].X);
  t.sign = t.area2 > 0 ? 1 : -1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    // The tie rule, top-left: the edge walked in the orientation that makes area2 positive has the direction
    // d = sign * (B - A) and the triangle on the side where its edge value is positive.  A centre on the edge is covered iff
    // d_y < 0 (the triangle lies at larger x: a left edge) or d_y == 0 and d_x > 0 (it lies at larger y, rows growing
    // downwards: a top edge) -- of the two triangles on either side of an edge exactly one.
    const int64_t dx = t.sj[k] * t.sign, dy = t.si[k] * t.sign;
    t.bias[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
  }
  const int32_t x_lo = min3(v[0].X, v[1].X, v[2].X), x_hi = max3(v[0].X, v[1].X, v[2].X);
  const int32_t y_lo = min3(v[0].Y, v[1].Y, v[2].Y), y_hi = max3(v[0].Y, v[1].Y, v[2].Y);
  t.i0 = max2(ceil_div_sub(x_lo), 0), t.i1 = min2(floor_div_sub(x_hi), W - 1);
  t.j0 = max2(ceil_div_sub(y_lo), 0), t.j1 = min2(floor_div_sub(y_hi), H - 1);
}

__host__ __device__ inline void edge_values(const Tri& t, int i, int j, int64_t (&w)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = t.c[k] + static_cast<int64_t>(j) * t.sj[k] - static_cast<int64_t>(i) * t.si[k];
}

__host__ __device__ inline bool covered(const Tri& t, const int64_t (&w)[3]) {
  return w[0] * t.sign >= t.bias[0] && w[1] * t.sign >= t.bias[1] && w[2] * t.sign >= t.bias[2];
}

}  // namespace ns_raster
