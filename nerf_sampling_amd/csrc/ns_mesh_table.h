// The case table of marching tetrahedra on the Kuhn split (ns_mesh_extract), derived at compile time from the geometric rule of
// include/nerf_sampling_hip.h.  Plain C++17, no HIP: ns_mesh.hip places it in constant memory, tools/mesh_hostcheck.cpp checks
// it on the CPU against the rule restated in floating point.
//
// Tetrahedron t = 0 .. 5 belongs to the permutation pi of the axes (x, y, z) in lexicographic order; its corners in the unit
// cell are w0 = 000, w1 = w0 + e_pi0, w2 = w1 + e_pi1, w3 = 111, named by their corner code dx + 2 dy + 4 dz.  `mask` has bit q
// set iff w_q is inside.  An entry:
//   bits 0-1        the number of triangles, 0 .. 2
//   bits 2 + 4 v .. vertex v = 0 .. 5 (three per triangle): the lattice edge it lies on as (qa, qb), two bits each, qa < qb the
//                   tetrahedron's corner numbers -- the codes grow along w0 .. w3, so w_qa is the end with the smaller lattice index.
// The winding is already applied: the normal of the triangle through the MIDPOINTS of its three edges has a positive dot product
// with (mean of the outside corners - mean of the inside corners).  Integer arithmetic on doubled coordinates, so no rounding.
#pragma once
#include <cstdint>

namespace ns_mesh {

constexpr int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// the corner code of corner q of tetrahedron t
constexpr int tet_code(int t, int q) {
  return q == 0 ? 0 : q == 1 ? (1 << kPerm[t][0]) : q == 2 ? ((1 << kPerm[t][0]) | (1 << kPerm[t][1])) : 7;
}

constexpr uint32_t tet_case(int t, int mask) {
  int in[4] = {}, out[4] = {}, n_in = 0, n_out = 0;
  for (int q = 0; q < 4; ++q) {
    if ((mask >> q) & 1) in[n_in++] = q;
    else out[n_out++] = q;
  }
  if (n_in == 0 || n_in == 4) return 0;
  // the crossed edges as (inside corner, outside corner), in the header's order
  int ea[6] = {}, eb[6] = {}, n_tri = 1;
  if (n_in == 1) {
    for (int v = 0; v < 3; ++v) ea[v] = in[0], eb[v] = out[v];
  } else if (n_in == 3) {
    for (int v = 0; v < 3; ++v) ea[v] = in[v], eb[v] = out[0];
  } else {                                   // the quad (a0 b0, a0 b1, a1 b1, a1 b0) as (0, 1, 2) and (0, 2, 3)
    const int qa[4] = {in[0], in[0], in[1], in[1]}, qb[4] = {out[0], out[1], out[1], out[0]};
    const int pick[6] = {0, 1, 2, 0, 2, 3};
    for (int v = 0; v < 6; ++v) ea[v] = qa[pick[v]], eb[v] = qb[pick[v]];
    n_tri = 2;
  }
  int w[4][3] = {};                          // corner coordinates
  for (int q = 0; q < 4; ++q)
    for (int c = 0; c < 3; ++c) w[q][c] = (tet_code(t, q) >> c) & 1;
  int dir[3] = {};                           // n_in * n_out * (mean outside - mean inside)
  for (int c = 0; c < 3; ++c) {
    for (int i = 0; i < n_out; ++i) dir[c] += n_in * w[out[i]][c];
    for (int i = 0; i < n_in; ++i) dir[c] -= n_out * w[in[i]][c];
  }
  uint32_t entry = static_cast<uint32_t>(n_tri);
  for (int tri = 0; tri < n_tri; ++tri) {
    int m[3][3] = {};                        // twice the midpoints
    for (int v = 0; v < 3; ++v)
      for (int c = 0; c < 3; ++c) m[v][c] = w[ea[3 * tri + v]][c] + w[eb[3 * tri + v]][c];
    int u[3] = {}, s[3] = {};
    for (int c = 0; c < 3; ++c) u[c] = m[1][c] - m[0][c], s[c] = m[2][c] - m[0][c];
    const int dot = (u[1] * s[2] - u[2] * s[1]) * dir[0] + (u[2] * s[0] - u[0] * s[2]) * dir[1] +
                    (u[0] * s[1] - u[1] * s[0]) * dir[2];
    const int order[3] = {0, dot < 0 ? 2 : 1, dot < 0 ? 1 : 2};
    for (int v = 0; v < 3; ++v) {
      const int a = ea[3 * tri + order[v]], b = eb[3 * tri + order[v]];
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      entry |= static_cast<uint32_t>(lo | (hi << 2)) << (2 + 4 * (3 * tri + v));
    }
  }
  return entry;
}

struct CaseTable {
  uint32_t entry[6][16];
  int32_t code[6][4];
  uint8_t cell_triangles[256];               // by the cell's inside corners (bit = corner code): its 0 .. 12 triangles
};

constexpr CaseTable make_case_table() {
  CaseTable T{};
  for (int t = 0; t < 6; ++t) {
    for (int mask = 0; mask < 16; ++mask) T.entry[t][mask] = tet_case(t, mask);
    for (int q = 0; q < 4; ++q) T.code[t][q] = tet_code(t, q);
  }
  for (int inside = 0; inside < 256; ++inside) {
    int n = 0;
    for (int t = 0; t < 6; ++t) {
      int mask = 0;
      for (int q = 0; q < 4; ++q) mask |= ((inside >> tet_code(t, q)) & 1) << q;
      n += static_cast<int>(T.entry[t][mask] & 3u);
    }
    T.cell_triangles[inside] = static_cast<uint8_t>(n);
  }
  return T;
}

}  // namespace ns_mesh
