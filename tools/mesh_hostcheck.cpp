// The host side of ns_mesh_extract -- every argument check and ns_mesh_workspace_bytes, all of which return ahead of any HIP call --
// and the library's case table (csrc/ns_mesh_table.h) judged on the CPU, as a stand-alone program for a host sanitizer run on a
// machine without a GPU (the pointers are never dereferenced):
//
//   cd nerf_sampling_amd/csrc
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c ns_mesh.hip -o /tmp/mesh.o && hipcc $F -x hip -c ns_core.cpp -o /tmp/core.o
//   hipcc $F -x hip -c ../../tools/mesh_hostcheck.cpp -o /tmp/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/mesh.o /tmp/core.o /tmp/main.o -o /tmp/hostcheck
//   /tmp/hostcheck
//
// The table: (1) every entry against the header's rule restated in double -- the crossed edges in the stated order, the winding
// by the normal through the edge midpoints --; (2) a ball of radius 0.7 on a 12^3 lattice over [-1, 1]^3 marched with the table
// on the CPU: every directed edge (by key) once and its reverse once, V - E + F = 2, 1824 triangles, and an enclosed volume 3.4 %
// below 4/3 pi r^3 -- the numbers of tests/test_device_mesh_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../include/nerf_sampling_hip.h"
#include "../nerf_sampling_amd/csrc/ns_mesh_table.h"

static int check_arguments() {
  float* sigma = reinterpret_cast<float*>(0x1000);
  float* tri = reinterpret_cast<float*>(0x2000);
  int64_t* keys = reinterpret_cast<int64_t*>(0x3000);
  int64_t* count = reinterpret_cast<int64_t*>(0x4000);
  void* ws = reinterpret_cast<void*>(0x5000);
  int bad = 0, n = 0;
  auto expect = [&](int64_t rc, int64_t want) {
    ++n;
    if (rc != want) {
      ++bad;
      std::printf("case %d: rc %lld, want %lld\n", n, static_cast<long long>(rc), static_cast<long long>(want));
    }
  };
  const int big = INT32_MAX;
  expect(ns_mesh_workspace_bytes(2, 2, 2), 256);
  expect(ns_mesh_workspace_bytes(16 * NS_MESH_SHARE + 1, 2, 2), 256);
  expect(ns_mesh_workspace_bytes(16 * NS_MESH_SHARE + 2, 2, 2), 512);
  expect(ns_mesh_workspace_bytes(2047, 1024, 1024), ((int64_t(2046) * 1023 * 1023 + NS_MESH_SHARE - 1) / NS_MESH_SHARE * 16 + 255) / 256 * 256);
  for (int g : {1, 0, -1, INT32_MIN}) {
    expect(ns_mesh_workspace_bytes(g, 4, 4), 0);
    expect(ns_mesh_workspace_bytes(4, g, 4), 0);
    expect(ns_mesh_workspace_bytes(4, 4, g), 0);
    expect(ns_mesh_extract(sigma, 1, g, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_extract(sigma, 1, 4, g, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_extract(sigma, 1, 4, 4, g, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
  }
  expect(ns_mesh_workspace_bytes(2048, 1024, 1024), 0);
  expect(ns_mesh_workspace_bytes(big, big, big), 0);
  expect(ns_mesh_workspace_bytes(big, big, 2), 0);
  expect(ns_mesh_extract(sigma, 1, 2048, 1024, 1024, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, big, big, big, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
  for (int64_t s : {int64_t(-1), int64_t(-4), INT64_MIN})
    expect(ns_mesh_extract(sigma, s, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
  for (int64_t c : {int64_t(-1), INT64_MIN})
    expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, c, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, nullptr, keys, 8, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, nullptr, 8, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_extract(nullptr, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, nullptr, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, nullptr, nullptr), NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, nullptr, nullptr, 0, count, nullptr, nullptr), NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, reinterpret_cast<int64_t*>(0x4004), ws, nullptr),
         NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, reinterpret_cast<int64_t*>(0x3004), 8, count, ws, nullptr),
         NS_E_INVALID);
  expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, reinterpret_cast<void*>(0x5004), nullptr),
         NS_E_INVALID);
  for (float v : {NAN, INFINITY, -INFINITY}) {
    expect(ns_mesh_extract(sigma, 1, 4, 4, 4, v, 0, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, v, 0, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, v, 0, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, v, 1, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
  }
  for (float v : {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, -1.0f}) {
    expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, v, 1, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, v, 1, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_extract(sigma, 1, 4, 4, 4, 0.f, 0, 0, 0, 1, 1, v, tri, keys, 8, count, ws, nullptr), NS_E_INVALID);
  }
  std::printf("%d argument cases, %d wrong; last error: %s\n", n, bad, ns_last_error());
  return bad;
}

// the header's rule in double: the triangles of tetrahedron t for `mask` as (qa, qb) corner pairs, qa < qb, wound
static std::vector<std::pair<int, int>> rule(int t, int mask) {
  std::vector<int> in, out;
  for (int q = 0; q < 4; ++q) (((mask >> q) & 1) ? in : out).push_back(q);
  std::vector<std::pair<int, int>> e;                      // (inside, outside)
  if (in.size() == 1) e = {{in[0], out[0]}, {in[0], out[1]}, {in[0], out[2]}};
  if (in.size() == 3) e = {{in[0], out[0]}, {in[1], out[0]}, {in[2], out[0]}};
  if (in.size() == 2) {
    const std::pair<int, int> q[4] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
    e = {q[0], q[1], q[2], q[0], q[2], q[3]};
  }
  double w[4][3], dir[3] = {0, 0, 0};
  for (int q = 0; q < 4; ++q)
    for (int c = 0; c < 3; ++c) w[q][c] = (ns_mesh::tet_code(t, q) >> c) & 1;
  for (int c = 0; c < 3; ++c) {
    for (int q : out) dir[c] += w[q][c] / static_cast<double>(out.size());
    for (int q : in) dir[c] -= w[q][c] / static_cast<double>(in.size());
  }
  for (size_t tri = 0; tri + 3 <= e.size(); tri += 3) {
    double m[3][3];
    for (int v = 0; v < 3; ++v)
      for (int c = 0; c < 3; ++c) m[v][c] = 0.5 * (w[e[tri + v].first][c] + w[e[tri + v].second][c]);
    const double u[3] = {m[1][0] - m[0][0], m[1][1] - m[0][1], m[1][2] - m[0][2]};
    const double s[3] = {m[2][0] - m[0][0], m[2][1] - m[0][1], m[2][2] - m[0][2]};
    const double dot = (u[1] * s[2] - u[2] * s[1]) * dir[0] + (u[2] * s[0] - u[0] * s[2]) * dir[1] + (u[0] * s[1] - u[1] * s[0]) * dir[2];
    if (dot < 0) std::swap(e[tri + 1], e[tri + 2]);
  }
  for (auto& p : e)
    if (p.first > p.second) std::swap(p.first, p.second);
  return e;
}

static int check_table() {
  const ns_mesh::CaseTable T = ns_mesh::make_case_table();
  int bad = 0;
  for (int t = 0; t < 6; ++t)
    for (int mask = 0; mask < 16; ++mask) {
      const auto want = rule(t, mask);
      const uint32_t entry = T.entry[t][mask];
      bool ok = (entry & 3u) * 3u == want.size();
      for (size_t v = 0; ok && v < want.size(); ++v) {
        const uint32_t f = (entry >> (2 + 4 * v)) & 15u;
        ok = static_cast<int>(f & 3u) == want[v].first && static_cast<int>(f >> 2) == want[v].second;
      }
      if (!ok) ++bad, std::printf("table entry t = %d, mask = %d differs from the rule\n", t, mask);
    }
  std::printf("96 table entries, %d wrong\n", bad);
  return bad;
}

// the ball on a G^3 lattice marched with the table, in double
static int check_ball() {
  const ns_mesh::CaseTable T = ns_mesh::make_case_table();
  const int G = 12;
  const double lo = -1.0, h = 2.0 / (G - 1), iso = 0.0, radius = 0.7;
  auto value = [&](int i, int j, int k) {
    const double x = lo + i * h, y = lo + j * h, z = lo + k * h;
    return radius - std::sqrt(x * x + y * y + z * z);
  };
  std::map<std::pair<int64_t, int64_t>, int> directed;
  std::set<int64_t> vertices;
  int64_t n_tri = 0;
  double volume = 0.0;
  for (int k = 0; k + 1 < G; ++k)
    for (int j = 0; j + 1 < G; ++j)
      for (int i = 0; i + 1 < G; ++i)
        for (int t = 0; t < 6; ++t) {
          int mask = 0;
          for (int q = 0; q < 4; ++q) {
            const int c = T.code[t][q];
            if (value(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)) >= iso) mask |= 1 << q;
          }
          const uint32_t entry = T.entry[t][mask];
          for (uint32_t tri = 0; tri < (entry & 3u); ++tri, ++n_tri) {
            int64_t key[3];
            double p[3][3];
            for (int v = 0; v < 3; ++v) {
              const uint32_t f = (entry >> (2 + 4 * (3 * tri + v))) & 15u;
              const int ca = T.code[t][f & 3u], cb = T.code[t][f >> 2];
              const int a[3] = {i + (ca & 1), j + ((ca >> 1) & 1), k + (ca >> 2)};
              const int b[3] = {i + (cb & 1), j + ((cb >> 1) & 1), k + (cb >> 2)};
              const double sa = value(a[0], a[1], a[2]), sb = value(b[0], b[1], b[2]), tt = (iso - sa) / (sb - sa);
              for (int c = 0; c < 3; ++c) p[v][c] = (lo + a[c] * h) + tt * ((lo + b[c] * h) - (lo + a[c] * h));
              key[v] = ((int64_t(a[2]) * G + a[1]) * G + a[0]) * 8 + (cb ^ ca);
              vertices.insert(key[v]);
            }
            for (int v = 0; v < 3; ++v) ++directed[{key[v], key[(v + 1) % 3]}];
            volume += (p[0][0] * (p[1][1] * p[2][2] - p[1][2] * p[2][1]) + p[0][1] * (p[1][2] * p[2][0] - p[1][0] * p[2][2]) +
                       p[0][2] * (p[1][0] * p[2][1] - p[1][1] * p[2][0])) / 6.0;
          }
        }
  bool paired = true;
  for (const auto& kv : directed) paired = paired && kv.second == 1 && directed.count({kv.first.second, kv.first.first}) == 1;
  const int64_t chi = static_cast<int64_t>(vertices.size()) - static_cast<int64_t>(directed.size()) / 2 + n_tri;
  const double error = volume / (4.0 / 3.0 * 3.14159265358979323846 * radius * radius * radius) - 1.0;
  std::printf("ball at 12^3: %lld triangles, edges paired: %s, chi = %lld, volume error %.4f %%\n", static_cast<long long>(n_tri),
              paired ? "yes" : "NO", static_cast<long long>(chi), 100.0 * error);
  return !(paired && chi == 2 && n_tri == 1824 && error < -0.033 && error > -0.035);
}

int main() {
  const int bad = check_arguments() + check_table() + check_ball();
  return bad != 0;
}
