// The host side of ns_mesh_components -- every argument check and ns_mesh_components_workspace_bytes, all of which return ahead of
// any HIP call -- as a stand-alone program for a host sanitizer run on a machine without a GPU (the pointers are never
// dereferenced):
//
//   cd nerf_sampling_amd/csrc
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c ns_mesh_components.hip -o /tmp/cc.o && hipcc $F -x hip -c ns_core.cpp -o /tmp/core.o
//   hipcc $F -x hip -c ../../tools/mesh_components_hostcheck.cpp -o /tmp/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/cc.o /tmp/core.o /tmp/main.o -o /tmp/cc_hostcheck
//   /tmp/cc_hostcheck
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../include/nerf_sampling_hip.h"

int main() {
  int64_t* faces = reinterpret_cast<int64_t*>(0x1000);
  int32_t* label = reinterpret_cast<int32_t*>(0x2000);
  int32_t* tri = reinterpret_cast<int32_t*>(0x3000);
  int32_t* vert = reinterpret_cast<int32_t*>(0x4000);
  int64_t* count = reinterpret_cast<int64_t*>(0x5000);
  void* ws = reinterpret_cast<void*>(0x6000);
  int bad = 0, n = 0;
  auto expect = [&](int64_t rc, int64_t want) {
    ++n;
    if (rc != want) {
      ++bad;
      std::printf("case %d: rc %lld, want %lld\n", n, static_cast<long long>(rc), static_cast<long long>(want));
    }
  };
  auto positive = [&](int64_t bytes) { expect(bytes > 0 && bytes % 8 == 0, 1); };
  const int64_t limit = int64_t(1) << 31;
  positive(ns_mesh_components_workspace_bytes(9, 8));
  positive(ns_mesh_components_workspace_bytes(1, 0));
  positive(ns_mesh_components_workspace_bytes(limit - 1, limit - 1));
  positive(ns_mesh_components_workspace_bytes(NS_MESH_COMPONENTS_SHARE + 1, 3 * NS_MESH_COMPONENTS_SHARE + 5));
  for (int64_t v : {int64_t(-1), INT64_MIN, limit, limit + 1, INT64_MAX}) {
    expect(ns_mesh_components_workspace_bytes(v, 8), 0);
    expect(ns_mesh_components_workspace_bytes(9, v), 0);
    expect(ns_mesh_components_workspace_bytes(v, v), 0);
    expect(ns_mesh_components(faces, 8, v, label, tri, vert, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_components(faces, v, 9, label, tri, vert, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_components(faces, v, v, label, tri, vert, count, ws, nullptr), NS_E_INVALID);
  }
  // a NULL pointer where V > 0 or F > 0 needs it
  expect(ns_mesh_components(nullptr, 8, 9, label, tri, vert, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(nullptr, 8, 0, label, tri, vert, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(faces, 8, 9, nullptr, tri, vert, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(faces, 8, 9, label, nullptr, vert, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(faces, 8, 9, label, tri, nullptr, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(faces, 8, 9, label, tri, vert, nullptr, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(faces, 8, 9, label, tri, vert, count, nullptr, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(nullptr, 0, 9, nullptr, tri, vert, count, ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(nullptr, 0, 9, label, tri, vert, count, nullptr, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), NS_E_INVALID);
  // alignment
  expect(ns_mesh_components(faces, 8, 9, label, tri, vert, reinterpret_cast<int64_t*>(0x5004), ws, nullptr), NS_E_INVALID);
  expect(ns_mesh_components(faces, 8, 9, label, tri, vert, count, reinterpret_cast<void*>(0x6004), nullptr), NS_E_INVALID);
  expect(ns_mesh_components(reinterpret_cast<int64_t*>(0x1004), 8, 9, label, tri, vert, count, ws, nullptr), NS_E_INVALID);
  for (uintptr_t off : {1, 2, 3}) {
    expect(ns_mesh_components(faces, 8, 9, reinterpret_cast<int32_t*>(0x2000 + off), tri, vert, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_components(faces, 8, 9, label, reinterpret_cast<int32_t*>(0x3000 + off), vert, count, ws, nullptr), NS_E_INVALID);
    expect(ns_mesh_components(faces, 8, 9, label, tri, reinterpret_cast<int32_t*>(0x4000 + off), count, ws, nullptr), NS_E_INVALID);
  }
  std::printf("%d argument cases, %d wrong; last error: %s\n", n, bad, ns_last_error());
  return bad != 0;
}
