// Per-vertex normals of the device mesh (ns_mesh_normals): the finite-difference gradient of the density lattice, interpolated
// along the vertex's own lattice edge -- a function of the edge alone, as the position is: no atomics, no adjacency, no dependence
// on the triangulation.  Built with -ffp-contract=off: every fp32 and fp64 operation is rounded on its own, the divisions and the
// square root are the correctly rounded ones (`/` and sqrt, hipcc's default for HIP), so numpy restates the bits.
//
// A gather: one thread per key reads s_a, s_b and the twelve stencil neighbours of the two ends as 4-byte loads at sigma_stride
// (clamped indices, never a branch on the boundary; all fourteen are issued before the first use).  scene_mesh passes ascending
// keys, so neighbouring threads read neighbouring lattice rows and L2 / the Infinity Cache carry the reuse -- no LDS staging.
// Workgroup g owns keys [g * kShare, (g + 1) * kShare); thread t takes g * kShare + s * kBlock + t.  Two launches on one stream:
//   normals  workgroup g -> the normals of its keys, and its two partial counts (degenerate, invalid) into the workspace;
//   totals   ONE workgroup adds the partials and writes count_dev.
#include <cmath>

#include "ns_block.h"
#include "ns_common.h"
#include "ns_mesh_key.h"

namespace {

using ns::kBlock;
using ns::kWaves;
constexpr int kShare = NS_MESH_NORMALS_SHARE;
constexpr int kSteps = ns::ShareOf<kShare>::steps;

struct Lattice {
  const float* sigma;
  int64_t step;             // floats between neighbouring lattice points along x
  int32_t G[3];             // Gx, Gy, Gz
  int32_t row[3];           // lattice points between neighbours along x, y, z: 1, Gx, Gx * Gy
  float h[3];
  float iso;
};

__device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the normal of the vertex on edge e; false (and zeros) for a degenerate one
__device__ __forceinline__ bool edge_normal(const Lattice& L, const ns_mesh::Edge& e, float (&n)[3]) {
  const int32_t lin[2] = {e.lin_a, e.lin_b};
  float centre[2], minus[2][3], plus[2][3], span[2][3];
#pragma unroll
  for (int q = 0; q < 2; ++q) {                                       // fourteen loads, no use between them
    centre[q] = L.sigma[static_cast<int64_t>(lin[q]) * L.step];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const int32_t at = q == 0 ? e.a[x] : e.b[x];
      const int32_t xm = max(at - 1, 0), xp = min(at + 1, L.G[x] - 1);            // G >= 2: xp - xm is 1 or 2
      minus[q][x] = L.sigma[static_cast<int64_t>(lin[q] + (xm - at) * L.row[x]) * L.step];
      plus[q][x] = L.sigma[static_cast<int64_t>(lin[q] + (xp - at) * L.row[x]) * L.step];
      span[q][x] = static_cast<float>(xp - xm);
    }
  }
  const float sa = centre[0], sb = centre[1];
  const float tt = (L.iso - sa) / (sb - sa);
  bool ok = finite(sa) && finite(sb) && finite(tt);
  double G[3];
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const float ga = (plus[0][x] - minus[0][x]) / (span[0][x] * L.h[x]);
    const float gb = (plus[1][x] - minus[1][x]) / (span[1][x] * L.h[x]);
    const float g = ga + tt * (gb - ga);
    ok = ok && finite(g);
    G[x] = static_cast<double>(g);
  }
  const double len = sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2]);
  ok = ok && len != 0.0;
#pragma unroll
  for (int x = 0; x < 3; ++x) n[x] = ok ? static_cast<float>(-G[x] / len) : 0.0f;
  return ok;
}

// partials[g] = the degenerate vertices of share g, partials[groups + g] = its invalid keys
__global__ void __launch_bounds__(kBlock)
mesh_normals_kernel(Lattice L, const int64_t* __restrict__ keys, int64_t V, float* __restrict__ normal_out,
                    int64_t* __restrict__ partials, int groups) {
  __shared__ int wave_counts[2][kWaves];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kShare + threadIdx.x;
  int degenerate = 0, invalid = 0;
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    const int64_t v = base + s * kBlock;
    if (v >= V) continue;
    ns_mesh::Edge e;
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (ns_mesh::key_decode(keys[v], L.G[0], L.G[1], L.G[2], e)) degenerate += edge_normal(L, e, n) ? 0 : 1;
    else ++invalid;
    normal_out[v * 3] = n[0];
    normal_out[v * 3 + 1] = n[1];
    normal_out[v * 3 + 2] = n[2];
  }
  ns::wave_sum_to(degenerate, wave_counts[0], invalid, wave_counts[1]);
  __syncthreads();                                         // one barrier for both sums
  if (threadIdx.x < 2) partials[static_cast<int64_t>(threadIdx.x) * groups + blockIdx.x] = ns::slots_sum(wave_counts[threadIdx.x]);
}

// totals[c] = partials[c * groups] + ... + partials[c * groups + groups - 1], c = 0, 1: thread t adds the shares t, t + kBlock, ..
// in the order of g, the workgroup adds the threads (integers: the order changes nothing).  groups == 0 writes the two zeros.
__global__ void __launch_bounds__(kBlock)
mesh_normals_totals_kernel(const int64_t* __restrict__ partials, int groups, int64_t* __restrict__ totals) {
  __shared__ int64_t wave_totals[2][kWaves];
  int64_t degenerate = 0, invalid = 0;
  for (int g = threadIdx.x; g < groups; g += kBlock) {
    degenerate += partials[g];
    invalid += partials[static_cast<int64_t>(groups) + g];
  }
  ns::wave_sum_to(degenerate, wave_totals[0], invalid, wave_totals[1]);
  __syncthreads();
  if (threadIdx.x < 2) totals[threadIdx.x] = ns::slots_sum(wave_totals[threadIdx.x]);
}

// ns_mesh_extract's lattice conditions: every dimension at least 2 and Gx * Gy * Gz below 2^31
bool lattice_ok(int Gx, int Gy, int Gz) {
  if (Gx < 2 || Gy < 2 || Gz < 2) return false;
  const int64_t xy = static_cast<int64_t>(Gx) * Gy;
  return ns::below_2_31(xy) && ns::below_2_31(xy * Gz);
}

bool count_ok(int64_t V) { return V >= 0 && ns::below_2_31(V); }

}  // namespace

extern "C" {

int64_t ns_mesh_normals_workspace_bytes(int64_t V) {
  if (!count_ok(V)) return 0;
  return ns::round_256(ns::cdiv(V, kShare) * 2 * static_cast<int64_t>(sizeof(int64_t)));
}

int ns_mesh_normals(const float* sigma_dev, int64_t sigma_stride, int Gx, int Gy, int Gz, float iso, float h_x, float h_y,
                    float h_z, const int64_t* key_dev, int64_t V, float* normal_out, int64_t* count_dev, void* workspace_dev,
                    void* stream) {
  NS_REQUIRE(Gx >= 2 && Gy >= 2 && Gz >= 2, "every lattice dimension must be at least 2");
  NS_REQUIRE(lattice_ok(Gx, Gy, Gz), "Gx * Gy * Gz must be below 2^31");
  NS_REQUIRE(sigma_stride >= 0, "negative sigma_stride");
  NS_REQUIRE(std::isfinite(iso), "iso must be finite");
  NS_REQUIRE(std::isfinite(h_x) && std::isfinite(h_y) && std::isfinite(h_z) && h_x > 0.0f && h_y > 0.0f && h_z > 0.0f,
             "h must be finite and positive");
  NS_REQUIRE(count_ok(V), "V must lie in [0, 2^31)");
  NS_REQUIRE(count_dev, "count_dev is required");
  NS_REQUIRE(V == 0 || (sigma_dev && key_dev && normal_out && workspace_dev),
             "sigma_dev, key_dev, normal_out and workspace_dev are required when V > 0");
  NS_REQUIRE(ns::aligned(key_dev, 8) && ns::aligned(count_dev, 8) && ns::aligned(workspace_dev, 8),
             "key_dev, count_dev and workspace_dev are 8-byte aligned");
  NS_REQUIRE(ns::aligned(normal_out, 4), "normal_out is 4-byte aligned");
  Lattice L;
  L.sigma = sigma_dev;
  L.step = sigma_stride == 0 ? 1 : sigma_stride;
  L.G[0] = Gx, L.G[1] = Gy, L.G[2] = Gz;
  L.row[0] = 1, L.row[1] = Gx, L.row[2] = Gx * Gy;
  L.h[0] = h_x, L.h[1] = h_y, L.h[2] = h_z;
  L.iso = iso;
  const int groups = static_cast<int>(ns::cdiv(V, kShare));           // at most 2^31 / NS_MESH_NORMALS_SHARE
  int64_t* partials = static_cast<int64_t*>(workspace_dev);
  hipStream_t s = ns::as_stream(stream);
  if (groups > 0) {
    mesh_normals_kernel<<<groups, kBlock, 0, s>>>(L, key_dev, V, normal_out, partials, groups);
    NS_LAUNCH_CHECK();
  }
  mesh_normals_totals_kernel<<<1, kBlock, 0, s>>>(partials, groups, count_dev);
  NS_LAUNCH_CHECK();
  return NS_OK;
}

}  // extern "C"
