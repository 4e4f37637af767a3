// The cluster lattice of ns_mesh_simplify: a vertex's fixed-point coordinate and cell, and a member's squared distance from its
// cluster's centroid -- one statement for the kernels and for the CPU alike (ns_mesh_cluster_coord / ns_mesh_cluster_distance
// hand it to the CPU tests, tools/mesh_simplify_hostcheck.cpp runs it under a host sanitizer).  Built with -ffp-contract=off
// wherever it is included: every fp64 operation below is rounded on its own, and numpy float64 restates the bits.
//
// LATTICE: lo[3] and cell[3] fp32, finite, cell > 0; dimensions C[3], each in [1, kMaxDim]; C[0] * C[1] * C[2] <= kMaxCells.
// COORDINATE per axis, 16 fractional bits:  t = (((double) v - (double) lo) / (double) cell) * 65536.0  -- a subtraction (exact:
// both are fp32), one correctly rounded division, one multiplication (exact: a power of two) --, u = llrint(t) (round half to
// even) clamped to [0, C * 65536 - 1].  For finite v the quotient is finite (|v - lo| < 2^129, cell >= 2^-149), so t is; the clamp
// is applied to t, before the conversion, which gives the same u (both bounds are integers and rounding is monotone) and never
// converts a double outside the target's range.  u < 2^31.  The CELL index per axis is u >> 16.
// A vertex with a NaN or infinite coordinate has no coordinate and belongs to no cell.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace ns_cluster {

constexpr int kFracBits = 16;
constexpr int kMaxDim = 1 << 15;
constexpr int64_t kMaxCells = int64_t(1) << 24;     // 256^3: a dense table of 40 bytes per cell, 640 MiB at the limit

struct Lattice {
  float lo[3], cell[3];
  int32_t C[3];
};

__host__ __device__ inline bool finite(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }          // false for NaN

// what the entry checks before any launch
__host__ __device__ inline bool lattice_ok(const Lattice& L) {
  int64_t cells = 1;
  for (int x = 0; x < 3; ++x) {
    if (!finite(L.lo[x]) || !finite(L.cell[x]) || !(L.cell[x] > 0.0f)) return false;
    if (L.C[x] < 1 || L.C[x] > kMaxDim) return false;
    cells *= L.C[x];                                 // at most 2^45
  }
  return cells <= kMaxCells;
}

__host__ __device__ inline int32_t coord(float v, float lo, float cell, int32_t C) {
  const double t = ((static_cast<double>(v) - static_cast<double>(lo)) / static_cast<double>(cell)) * 65536.0;
  const int64_t top = (static_cast<int64_t>(C) << kFracBits) - 1;
  if (!(t > 0.0)) return 0;
  if (t >= static_cast<double>(top)) return static_cast<int32_t>(top);
  return static_cast<int32_t>(llrint(t));
}

// u[3] of vertex p; false (and zeros) where a coordinate is not finite
__host__ __device__ inline bool vertex_coord(const Lattice& L, const float (&p)[3], int32_t (&u)[3]) {
  const bool ok = finite(p[0]) && finite(p[1]) && finite(p[2]);
  for (int x = 0; x < 3; ++x) u[x] = ok ? coord(p[x], L.lo[x], L.cell[x], L.C[x]) : 0;
  return ok;
}

// the linear index of the cell of u: (cz * Cy + cy) * Cx + cx, below kMaxCells
__host__ __device__ inline int32_t cell_index(const Lattice& L, const int32_t (&u)[3]) {
  return ((u[2] >> kFracBits) * L.C[1] + (u[1] >> kFracBits)) * L.C[0] + (u[0] >> kFracBits);
}

// (float) sum over x, y, z in that order of ((double) u - (double) S / (double) n)^2, n >= 1: the division, the subtraction,
// the square and the two additions each rounded on their own, then one rounding to fp32.  Never negative, below 2^64.
__host__ __device__ inline float distance2(const int32_t (&u)[3], const int64_t (&S)[3], int32_t n) {
  double d = 0.0;
  for (int x = 0; x < 3; ++x) {
    const double mean = static_cast<double>(S[x]) / static_cast<double>(n);
    const double diff = static_cast<double>(u[x]) - mean;
    const double sq = diff * diff;
    d = x == 0 ? sq : d + sq;
  }
  return static_cast<float>(d);
}

}  // namespace ns_cluster
