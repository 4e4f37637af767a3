// The field's isosurface on the device (ns_mesh_extract): marching tetrahedra on the Kuhn split of every lattice cell, as an
// ordered stream compaction -- the sibling of ns_cloud_append.  fp32, HBM-bound: 4 B in per lattice point, 60 B out per triangle.
// Built with -ffp-contract=off: a vertex is p_a + tt * (p_b - p_a) with p = lo + (float)idx * h, every operation rounded on its
// own, and tt one correctly rounded division (the `/` operator, hipcc's default for HIP, as ns_map_to8b's) -- a function of the
// lattice edge alone, so the cells that share an edge compute the same bits for the same key.
//
// Cell e = (k * (Gy - 1) + j) * (Gx - 1) + i.  Workgroup g owns cells [g * kShare, (g + 1) * kShare); thread t takes
// g * kShare + s * kBlock + t, s = 0 .. kSteps - 1 (consecutive lanes read consecutive floats of a packed row: the eight corner
// loads of a wave are eight coalesced rows, and the rows two neighbouring cells share come from L1 / L2 -- no LDS staging: a row
// of cells is Gx - 1 long, so a tile of it would start at any dword and the staged copy saves no HBM traffic the caches do not
// save already), so within a share the order of e is (s, wave, lane).  Three launches on one stream:
//   count  workgroup g -> the triangles and the skipped cells of its share;
//   scan   ONE workgroup turns the triangle counts into absolute triangle indices in place and writes both totals;
//   emit   every workgroup evaluates its cells again and writes the triangles of a cell from the share's index + the triangles of
//          the earlier (s, wave) groups of its share (through LDS) + those of the lanes below (a cell has 0 .. 12 triangles: an
//          integer exclusive scan over the wave on shuffles, not a ballot).
// No atomics and nothing that waits on another workgroup's memory: the triangle order depends on the lattice alone.
#include <cmath>

#include "ns_block.h"
#include "ns_common.h"
#include "ns_mesh_table.h"

namespace {

using ns::kBlock;
using ns::kWaves;
constexpr int kShare = NS_MESH_SHARE;
constexpr int kSteps = ns::ShareOf<kShare>::steps;

__constant__ ns_mesh::CaseTable kCases = ns_mesh::make_case_table();

struct Lattice {
  const float* sigma;
  int64_t step[3];          // floats between neighbouring lattice points along x, y, z
  uint32_t Gx, Gxy;         // points per row and per slab
  uint32_t cx, cxy;         // cells per row and per slab
  uint32_t cx_inv, cxy_inv; // floor(2^32 / cx), floor(2^32 / cxy) (2^32 - 1 for a divisor of 1): div_small
  uint32_t cells;           // below 2^31
  float iso;
};

// e / d and e % d from d_inv = floor(2^32 / d): the estimate umulhi(e, d_inv) is the quotient or one less (e d_inv / 2^32 lies in
// (e / d - 1, e / d] for e < 2^32), so one correction is enough -- a dozen instructions less than the 32-bit division, twice per cell
__device__ __forceinline__ uint32_t div_small(uint32_t e, uint32_t d, uint32_t d_inv, uint32_t& rem) {
  uint32_t q = __umulhi(e, d_inv);
  rem = e - q * d;
  if (rem >= d) ++q, rem -= d;
  return q;
}

struct Frame {              // lattice point (i, j, k) lies at lo + (float)idx * h
  float lo[3], h[3];
};

struct Cell {
  uint32_t idx[3];          // i, j, k
  uint32_t lin;             // the lattice index of corner 000
  float v[8];               // corner values by corner code dx + 2 dy + 4 dz
  uint32_t inside;          // bit code set iff v[code] >= iso; 0 for a skipped cell
  bool skipped;             // a corner is NaN or +-inf
};

// the lattice offset of the corner with this code
__device__ __forceinline__ uint32_t corner_offset(const Lattice& L, uint32_t code) {
  return (code & 1u) + ((code >> 1) & 1u) * L.Gx + (code >> 2) * L.Gxy;
}

// bit q set iff corner q of tetrahedron t is inside
template <int T>
__device__ __forceinline__ uint32_t tet_mask(uint32_t inside) {
  constexpr int c1 = ns_mesh::tet_code(T, 1), c2 = ns_mesh::tet_code(T, 2);
  return (inside & 1u) | (((inside >> c1) & 1u) << 1) | (((inside >> c2) & 1u) << 2) | ((inside >> 7) << 3);
}

// loads cell e < L.cells and returns the number of its triangles
__device__ __forceinline__ int cell_load(const Lattice& L, uint32_t e, Cell& c) {
  uint32_t r, i;
  const uint32_t k = div_small(e, L.cxy, L.cxy_inv, r), j = div_small(r, L.cx, L.cx_inv, i);
  c.idx[0] = i, c.idx[1] = j, c.idx[2] = k;
  c.lin = k * L.Gxy + j * L.Gx + i;
  const float* p = L.sigma + static_cast<int64_t>(c.lin) * L.step[0];   // the corners lie at wave-uniform offsets from it
  bool finite = true;
  uint32_t inside = 0;
#pragma unroll
  for (uint32_t code = 0; code < 8; ++code) {
    const float v = p[(code & 1u) * L.step[0] + ((code >> 1) & 1u) * L.step[1] + (code >> 2) * L.step[2]];
    c.v[code] = v;
    finite = finite && (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
    if (v >= L.iso) inside |= 1u << code;            // NaN is outside (and the cell is skipped)
  }
  c.skipped = !finite;
  c.inside = finite ? inside : 0u;
  return kCases.cell_triangles[c.inside];            // the sum of its six tetrahedra's entries
}

// the triangles of tetrahedron T of the cell, from triangle index n on; returns the index after them
template <int T>
__device__ __forceinline__ int64_t tet_emit(const Lattice& L, const Frame& F, const Cell& c, int64_t n, int64_t capacity,
                                            float* __restrict__ tri_out, int64_t* __restrict__ key_out) {
  const uint32_t mask = tet_mask<T>(c.inside);
  if (mask == 0u || mask == 15u) return n;
  constexpr uint32_t c1 = ns_mesh::tet_code(T, 1), c2 = ns_mesh::tet_code(T, 2);
  const float w0 = c.v[0], w1 = c.v[c1], w2 = c.v[c2], w3 = c.v[7];
  const uint32_t entry = kCases.entry[T][mask];
  const int n_tri = static_cast<int>(entry & 3u);
  for (int tri = 0; tri < n_tri; ++tri, ++n) {
    if (n >= capacity) continue;                     // counted, not written
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const uint32_t edge = (entry >> (2 + 4 * (3 * tri + v))) & 15u, qa = edge & 3u, qb = edge >> 2;    // qa < qb
      const float sa = qa == 0u ? w0 : qa == 1u ? w1 : w2, sb = qb == 1u ? w1 : qb == 2u ? w2 : w3;
      const uint32_t ca = qa == 0u ? 0u : qa == 1u ? c1 : c2, cb = qb == 1u ? c1 : qb == 2u ? c2 : 7u;
      const float tt = (L.iso - sa) / (sb - sa);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float pa = F.lo[a] + static_cast<float>(c.idx[a] + ((ca >> a) & 1u)) * F.h[a];
        const float pb = F.lo[a] + static_cast<float>(c.idx[a] + ((cb >> a) & 1u)) * F.h[a];
        tri_out[n * 9 + v * 3 + a] = pa + tt * (pb - pa);
      }
      key_out[n * 3 + v] = static_cast<int64_t>(c.lin + corner_offset(L, ca)) * 8 + static_cast<int64_t>(cb ^ ca);
    }
  }
  return n;
}

// counts[g] = the triangles of share g, counts[groups + g] = its skipped cells
__global__ void __launch_bounds__(kBlock)
mesh_count_kernel(Lattice L, int64_t* __restrict__ counts, int groups) {
  __shared__ int wave_counts[2][kWaves];
  const uint32_t base = blockIdx.x * static_cast<uint32_t>(kShare) + threadIdx.x;   // below 2^31 + kShare
  int n = 0, skipped = 0;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const uint32_t e = base + s * kBlock;
    if (e < L.cells) {
      Cell c;
      n += cell_load(L, e, c);
      skipped += c.skipped ? 1 : 0;
    }
  }
  ns::wave_sum_to(n, wave_counts[0], skipped, wave_counts[1]);
  __syncthreads();                                         // one barrier for both sums
  if (threadIdx.x < 2) counts[static_cast<int64_t>(threadIdx.x) * groups + blockIdx.x] = ns::slots_sum(wave_counts[threadIdx.x]);
}

// counts[g] <- counts[0] + ... + counts[g - 1] (ns::share_scan, one workgroup); totals[0] = the sum of all, totals[1] = the sum
// of counts[groups ..], which every thread adds up for its own entries beside the scan's loads
__global__ void __launch_bounds__(kBlock)
mesh_scan_kernel(int64_t* __restrict__ counts, int groups, int64_t* __restrict__ totals) {
  __shared__ int64_t wave_skipped[kWaves];
  const int64_t* skipped_counts = counts + groups;
  int64_t skipped = 0;
  const int64_t triangles = ns::share_scan(counts, groups, 0, [&](int g, bool in_range) {
    skipped += in_range ? skipped_counts[g] : 0;
  });
  skipped = ns::block_sum(skipped, wave_skipped);
  if (threadIdx.x == 0) {
    totals[0] = triangles;
    totals[1] = skipped;
  }
}

// ns::share_place's placement, written out: a step's scan follows its eight loads, and the 7 300-instruction schedule hangs on it
__global__ void __launch_bounds__(kBlock)
mesh_emit_kernel(Lattice L, Frame F, const int64_t* __restrict__ bases, float* __restrict__ tri_out,
                 int64_t* __restrict__ key_out, int64_t capacity) {
  __shared__ int group_counts[kSteps][kWaves];
  const int64_t base = bases[blockIdx.x];
  if (base >= capacity) return;                            // every triangle of this share lies at or beyond the capacity
  const int wave = threadIdx.x >> 6;
  const uint32_t e0 = blockIdx.x * static_cast<uint32_t>(kShare) + threadIdx.x;
  Cell c[kSteps];
  int below[kSteps];                                       // triangles of the lanes of this wave below this one, per step
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const uint32_t e = e0 + s * kBlock;
    c[s].inside = 0u;
    const int n = e < L.cells ? cell_load(L, e, c[s]) : 0;
    below[s] = ns::wave_place(n, &group_counts[s][wave]);
  }
  __syncthreads();
  int groups_before = 0;                                   // triangles of the earlier (s, wave) groups
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    int mine = groups_before;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
      const int n = group_counts[s][v];
      if (v < wave) mine += n;
      groups_before += n;
    }
    if (c[s].inside == 0u || c[s].inside == 255u) continue;      // no crossing, skipped or out of range
    int64_t n = base + mine + below[s];
    n = tet_emit<0>(L, F, c[s], n, capacity, tri_out, key_out);
    n = tet_emit<1>(L, F, c[s], n, capacity, tri_out, key_out);
    n = tet_emit<2>(L, F, c[s], n, capacity, tri_out, key_out);
    n = tet_emit<3>(L, F, c[s], n, capacity, tri_out, key_out);
    n = tet_emit<4>(L, F, c[s], n, capacity, tri_out, key_out);
    tet_emit<5>(L, F, c[s], n, capacity, tri_out, key_out);
  }
}

// every dimension at least 2 and Gx * Gy * Gz in [8, 2^31): lattice and cell indices are 32-bit in the kernels
bool mesh_shape_ok(int Gx, int Gy, int Gz) {
  if (Gx < 2 || Gy < 2 || Gz < 2) return false;
  const int64_t xy = static_cast<int64_t>(Gx) * Gy;
  return ns::below_2_31(xy) && ns::below_2_31(xy * Gz);
}

int64_t mesh_cells(int Gx, int Gy, int Gz) { return static_cast<int64_t>(Gx - 1) * (Gy - 1) * (Gz - 1); }

int64_t mesh_groups(int Gx, int Gy, int Gz) { return ns::cdiv(mesh_cells(Gx, Gy, Gz), kShare); }

}  // namespace

extern "C" {

int64_t ns_mesh_workspace_bytes(int Gx, int Gy, int Gz) {
  if (!mesh_shape_ok(Gx, Gy, Gz)) return 0;
  return ns::round_256(mesh_groups(Gx, Gy, Gz) * 2 * static_cast<int64_t>(sizeof(int64_t)));
}

int ns_mesh_extract(const float* sigma_dev, int64_t sigma_stride, int Gx, int Gy, int Gz, float iso, float lo_x, float lo_y,
                    float lo_z, float h_x, float h_y, float h_z, float* tri_out, int64_t* key_out, int64_t capacity,
                    int64_t* count_dev, void* workspace_dev, void* stream) {
  NS_REQUIRE(Gx >= 2 && Gy >= 2 && Gz >= 2, "every lattice dimension must be at least 2");
  NS_REQUIRE(mesh_shape_ok(Gx, Gy, Gz), "Gx * Gy * Gz must be below 2^31");
  NS_REQUIRE(sigma_stride >= 0, "negative sigma_stride");
  NS_REQUIRE(capacity >= 0, "negative capacity");
  NS_REQUIRE(capacity == 0 || (tri_out && key_out), "tri_out and key_out are required when capacity > 0");
  NS_REQUIRE(count_dev && sigma_dev && workspace_dev, "null pointer");
  NS_REQUIRE(ns::aligned(count_dev, 8) && ns::aligned(key_out, 8) && ns::aligned(workspace_dev, 8),
             "count_dev, key_out and workspace_dev are 8-byte aligned");
  NS_REQUIRE(std::isfinite(iso) && std::isfinite(lo_x) && std::isfinite(lo_y) && std::isfinite(lo_z), "iso and lo must be finite");
  NS_REQUIRE(std::isfinite(h_x) && std::isfinite(h_y) && std::isfinite(h_z) && h_x > 0.0f && h_y > 0.0f && h_z > 0.0f,
             "h must be finite and positive");
  Lattice L;
  L.sigma = sigma_dev;
  L.Gx = static_cast<uint32_t>(Gx);
  L.Gxy = static_cast<uint32_t>(Gx) * static_cast<uint32_t>(Gy);
  L.step[0] = sigma_stride == 0 ? 1 : sigma_stride;
  L.step[1] = L.step[0] * L.Gx;
  L.step[2] = L.step[0] * L.Gxy;
  L.cx = static_cast<uint32_t>(Gx - 1);
  L.cxy = static_cast<uint32_t>(Gx - 1) * static_cast<uint32_t>(Gy - 1);
  L.cx_inv = L.cx == 1 ? UINT32_MAX : static_cast<uint32_t>((uint64_t(1) << 32) / L.cx);
  L.cxy_inv = L.cxy == 1 ? UINT32_MAX : static_cast<uint32_t>((uint64_t(1) << 32) / L.cxy);
  L.cells = static_cast<uint32_t>(mesh_cells(Gx, Gy, Gz));
  L.iso = iso;
  const Frame F{{lo_x, lo_y, lo_z}, {h_x, h_y, h_z}};
  const int groups = static_cast<int>(mesh_groups(Gx, Gy, Gz));        // at most 2^31 / NS_MESH_SHARE
  int64_t* counts = static_cast<int64_t*>(workspace_dev);
  hipStream_t s = ns::as_stream(stream);
  mesh_count_kernel<<<groups, kBlock, 0, s>>>(L, counts, groups);
  NS_LAUNCH_CHECK();
  mesh_scan_kernel<<<1, kBlock, 0, s>>>(counts, groups, count_dev);
  NS_LAUNCH_CHECK();
  if (capacity == 0) return NS_OK;                                     // a pure count: there is no triangle to place
  mesh_emit_kernel<<<groups, kBlock, 0, s>>>(L, F, counts, tri_out, key_out, capacity);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
