// The lattice-edge key of a mesh vertex (ns_mesh_extract's key_out, read back by ns_mesh_normals): key = lin(a) * 8 + code,
// code = dx + 2 dy + 4 dz the offset of the edge's far end b = a + d.  One function decodes and judges a key, for the kernel and
// for the CPU alike (tools/mesh_normals_hostcheck.cpp runs it under a host sanitizer): nothing is ever addressed through a key
// it refuses.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ns_mesh {

struct Edge {
  int32_t a[3], b[3];       // the lattice indices (i, j, k) of the two ends; b[x] - a[x] is 0 or 1
  int32_t lin_a, lin_b;     // their lattice indices (k * Gy + j) * Gx + i
};

// true iff `key` names a lattice edge of the Gx x Gy x Gz lattice (every dimension at least 1, Gx * Gy * Gz below 2^31); then
// `e` is that edge.  Refused: a negative key, lin(a) at or beyond the lattice size, code 0 (no edge), b outside the lattice.
__host__ __device__ inline bool key_decode(int64_t key, int32_t Gx, int32_t Gy, int32_t Gz, Edge& e) {
  const int64_t points = static_cast<int64_t>(Gx) * Gy * Gz;
  if (key < 0 || (key >> 3) >= points) return false;
  const uint32_t code = static_cast<uint32_t>(key & 7), lin = static_cast<uint32_t>(key >> 3);   // lin < 2^31
  if (code == 0u) return false;
  const uint32_t row = lin / static_cast<uint32_t>(Gx);
  e.a[0] = static_cast<int32_t>(lin - row * static_cast<uint32_t>(Gx));
  e.a[2] = static_cast<int32_t>(row / static_cast<uint32_t>(Gy));
  e.a[1] = static_cast<int32_t>(row - static_cast<uint32_t>(e.a[2]) * static_cast<uint32_t>(Gy));
  e.b[0] = e.a[0] + static_cast<int32_t>(code & 1u);
  e.b[1] = e.a[1] + static_cast<int32_t>((code >> 1) & 1u);
  e.b[2] = e.a[2] + static_cast<int32_t>(code >> 2);
  if (e.b[0] >= Gx || e.b[1] >= Gy || e.b[2] >= Gz) return false;
  e.lin_a = static_cast<int32_t>(lin);
  e.lin_b = (e.b[2] * Gy + e.b[1]) * Gx + e.b[0];            // a lattice point: below 2^31
  return true;
}

}  // namespace ns_mesh
