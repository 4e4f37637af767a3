// The host side of ns_mesh_normals -- every argument check and ns_mesh_normals_workspace_bytes, all of which return ahead of any
// HIP call -- and the library's key decoding (csrc/ns_mesh_key.h, the one function the kernel runs per key) judged on the CPU, as
// a stand-alone program for a host sanitizer run on a machine without a GPU (the pointers are never dereferenced):
//
//   cd nerf_sampling_amd/csrc
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c ns_mesh_normals.hip -o /tmp/normals.o && hipcc $F -x hip -c ns_core.cpp -o /tmp/core.o
//   hipcc $F -x hip -c ../../tools/mesh_normals_hostcheck.cpp -o /tmp/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/normals.o /tmp/core.o /tmp/main.o -o /tmp/normals_hostcheck
//   /tmp/normals_hostcheck
//
// The keys: every key of three lattices -- (7, 6, 9), (2, 5, 3) and (3, 2, 2) -- from 8 below zero to 8 lattice points beyond the
// end against the header's rule restated with plain loops, and the extremes of int64.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../include/nerf_sampling_hip.h"
#include "../nerf_sampling_amd/csrc/ns_mesh_key.h"

static int check_arguments() {
  float* sigma = reinterpret_cast<float*>(0x1000);
  int64_t* keys = reinterpret_cast<int64_t*>(0x2000);
  float* normals = reinterpret_cast<float*>(0x3000);
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
  const int64_t limit = int64_t(1) << 31, S = NS_MESH_NORMALS_SHARE;
  expect(ns_mesh_normals_workspace_bytes(0), 0);
  expect(ns_mesh_normals_workspace_bytes(1), 256);
  expect(ns_mesh_normals_workspace_bytes(S), 256);
  expect(ns_mesh_normals_workspace_bytes(S + 1), 256);
  expect(ns_mesh_normals_workspace_bytes(16 * S), 256);
  expect(ns_mesh_normals_workspace_bytes(16 * S + 1), 512);
  expect(ns_mesh_normals_workspace_bytes(limit - 1), ((limit - 1 + S - 1) / S * 16 + 255) / 256 * 256);
  for (int64_t v : {int64_t(-1), INT64_MIN, limit, limit + 1, INT64_MAX}) {
    expect(ns_mesh_normals_workspace_bytes(v), 0);
    expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, keys, v, normals, count, ws, nullptr), NS_E_INVALID);
  }
  for (int g : {1, 0, -1, INT32_MIN}) {
    expect(ns_mesh_normals(sigma, 1, g, 4, 4, 0.f, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_normals(sigma, 1, 4, g, 4, 0.f, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_normals(sigma, 1, 4, 4, g, 0.f, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
  }
  expect(ns_mesh_normals(sigma, 1, 2048, 1024, 1024, 0.f, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_normals(sigma, 1, big, big, big, 0.f, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_normals(sigma, 1, big, big, 2, 0.f, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
  for (int64_t s : {int64_t(-1), int64_t(-4), INT64_MIN})
    expect(ns_mesh_normals(sigma, s, 4, 4, 4, 0.f, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
  for (float v : {NAN, INFINITY, -INFINITY})
    expect(ns_mesh_normals(sigma, 1, 4, 4, 4, v, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
  for (float v : {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, -1.0f}) {
    expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, v, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, v, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, v, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
  }
  // a NULL pointer where V > 0 needs it; count_dev always
  expect(ns_mesh_normals(nullptr, 1, 4, 4, 4, 0.f, 1, 1, 1, keys, 8, normals, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, nullptr, 8, normals, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, keys, 8, nullptr, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, keys, 8, normals, nullptr, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, keys, 8, normals, count, nullptr, nullptr), NS_E_INVALID);
  expect(ns_mesh_normals(nullptr, 1, 4, 4, 4, 0.f, 1, 1, 1, nullptr, 0, nullptr, nullptr, nullptr, nullptr), NS_E_INVALID);
  // alignment
  expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, reinterpret_cast<int64_t*>(0x2004), 8, normals, count, ws, nullptr),
         NS_E_INVALID);
  expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, keys, 8, normals, reinterpret_cast<int64_t*>(0x4004), ws, nullptr),
         NS_E_INVALID);
  expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, keys, 8, normals, count, reinterpret_cast<void*>(0x5004), nullptr),
         NS_E_INVALID);
  for (uintptr_t off : {1, 2, 3})
    expect(ns_mesh_normals(sigma, 1, 4, 4, 4, 0.f, 1, 1, 1, keys, 8, reinterpret_cast<float*>(0x3000 + off), count, ws, nullptr),
           NS_E_INVALID);
  std::printf("%d argument cases, %d wrong; last error: %s\n", n, bad, ns_last_error());
  return bad;
}

// the header's rule with plain loops: the edge of `key` on the lattice, or false
static bool rule(int64_t key, int Gx, int Gy, int Gz, int (&a)[3], int (&b)[3]) {
  if (key < 0) return false;
  const int64_t lin = key / 8;
  const int code = static_cast<int>(key % 8);
  if (lin >= int64_t(Gx) * Gy * Gz || code == 0) return false;
  int64_t at = 0;
  for (int k = 0; k < Gz; ++k)
    for (int j = 0; j < Gy; ++j)
      for (int i = 0; i < Gx; ++i, ++at)
        if (at == lin) a[0] = i, a[1] = j, a[2] = k;
  const int G[3] = {Gx, Gy, Gz};
  for (int x = 0; x < 3; ++x) {
    b[x] = a[x] + ((code >> x) & 1);
    if (b[x] >= G[x]) return false;
  }
  return true;
}

static int check_keys() {
  int bad = 0;
  int64_t n = 0, n_valid = 0;
  const int dims[3][3] = {{7, 6, 9}, {2, 5, 3}, {3, 2, 2}};
  for (const auto& d : dims) {
    const int Gx = d[0], Gy = d[1], Gz = d[2];
    const int64_t points = int64_t(Gx) * Gy * Gz;
    auto one = [&](int64_t key) {
      int a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
      ns_mesh::Edge e;
      const bool want = rule(key, Gx, Gy, Gz, a, b), got = ns_mesh::key_decode(key, Gx, Gy, Gz, e);
      bool ok = want == got;
      if (ok && got) {
        for (int x = 0; x < 3; ++x) ok = ok && e.a[x] == a[x] && e.b[x] == b[x];
        ok = ok && e.lin_a == (a[2] * Gy + a[1]) * Gx + a[0] && e.lin_b == (b[2] * Gy + b[1]) * Gx + b[0];
        ok = ok && e.lin_a < e.lin_b && e.lin_b < points;
        ++n_valid;
      }
      ++n;
      if (!ok) ++bad, std::printf("key %lld on (%d, %d, %d): decoded wrongly\n", static_cast<long long>(key), Gx, Gy, Gz);
    };
    for (int64_t key = -8; key < (points + 8) * 8; ++key) one(key);
    for (int64_t key : {INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 7, int64_t(1) << 34, (int64_t(1) << 34) + 1,
                        (int64_t(1) << 62) + 3})
      one(key);
  }
  // the largest lattice there is: its last point has no edge, the one before it has one along x
  ns_mesh::Edge e;
  const int64_t last = (int64_t(1) << 31) - 2;                        // 2047 x 1024 x 1024 = 2^31 - 2^20 points
  const int64_t points = int64_t(2047) * 1024 * 1024;
  bad += ns_mesh::key_decode((points - 1) * 8 + 1, 2047, 1024, 1024, e) ? 1 : 0;
  bad += ns_mesh::key_decode((points - 2) * 8 + 1, 2047, 1024, 1024, e) && e.lin_b == points - 1 && e.b[0] == 2046 ? 0 : 1;
  bad += ns_mesh::key_decode(last * 8 + 1, 2047, 1024, 1024, e) ? 1 : 0;
  std::printf("%lld keys, %lld of them valid, %d wrong\n", static_cast<long long>(n), static_cast<long long>(n_valid), bad);
  return bad;
}

int main() {
  const int bad = check_arguments() + check_keys();
  return bad != 0;
}
