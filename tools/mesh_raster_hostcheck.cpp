// The host side of ns_mesh_raster -- every argument check and ns_mesh_raster_workspace_bytes, all of which return ahead of any HIP
// call -- and the library's integer coverage (csrc/ns_mesh_raster_cover.h, the functions the kernels run per face and per
// pixel) judged on the CPU, as a stand-alone program for a host sanitizer run on a machine without a GPU (the pointers are never
// dereferenced):
//
//   cd nerf_sampling_amd/csrc
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c ns_mesh_raster.hip -o /tmp/raster.o && hipcc $F -x hip -c ns_core.cpp -o /tmp/core.o
//   hipcc $F -x hip -c ../../tools/mesh_raster_hostcheck.cpp -o /tmp/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/raster.o /tmp/core.o /tmp/main.o -o /tmp/raster_hostcheck
//   /tmp/raster_hostcheck
//
// The coverage: random and hand-made snapped triangles -- vertices on pixel centres, on the frame's border, at the +-2^28 ends of
// the band -- against the header's rule written with plain loops over the whole frame: the edge functions as the header spells
// them, the tie rule from the edge's end points, no bounding box.  Then the exactly-once properties: a quad split along a
// diagonal through pixel centres, and a fan around a pixel centre, under every winding.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "../include/nerf_sampling_hip.h"
#include "../nerf_sampling_amd/csrc/ns_mesh_raster_cover.h"

static int check_arguments(int* cases) {
  float* vertices = reinterpret_cast<float*>(0x1000);
  int64_t* faces = reinterpret_cast<int64_t*>(0x2000);
  float* attr = reinterpret_cast<float*>(0x3000);
  float* depth = reinterpret_cast<float*>(0x4000);
  int32_t* tri = reinterpret_cast<int32_t*>(0x5000);
  float* rgb = reinterpret_cast<float*>(0x6000);
  int64_t* count = reinterpret_cast<int64_t*>(0x7000);
  void* ws = reinterpret_cast<void*>(0x8000);
  const float good[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  int bad = 0, n = 0;
  auto expect = [&](int64_t rc, int64_t want) {
    ++n;
    if (rc != want) {
      ++bad;
      std::printf("case %d: rc %lld, want %lld\n", n, static_cast<long long>(rc), static_cast<long long>(want));
    }
  };
  auto r256 = [](int64_t b) { return (b + 255) / 256 * 256; };
  const int64_t limit = int64_t(1) << 31;
  struct Shape { int64_t V, F; int H, W; };
  for (const Shape& s : {Shape{8, 4, 8, 8}, Shape{0, 1, 1, 1}, Shape{1000, 2049, 37, 29}, Shape{1, NS_MESH_RASTER_SHARE, 64, 48},
                         Shape{limit - 1, limit - 1, 16384, 16384}})
    expect(ns_mesh_raster_workspace_bytes(s.V, s.F, s.H, s.W),
           r256(int64_t(8) * s.H * s.W) + r256(16 * s.V) + r256(4 * s.F) + 256);
  expect(ns_mesh_raster_workspace_bytes(8, 0, 8, 8), 0);
  for (const Shape& s : {Shape{-1, 4, 8, 8}, Shape{8, -1, 8, 8}, Shape{limit, 4, 8, 8}, Shape{8, limit, 8, 8}, Shape{8, 4, 0, 8},
                         Shape{8, 4, 8, 0}, Shape{8, 4, 16385, 8}, Shape{8, 4, 8, 16385}, Shape{8, 4, -1, 8},
                         Shape{INT64_MIN, 4, 8, 8}, Shape{8, INT64_MAX, 8, 8}})
    expect(ns_mesh_raster_workspace_bytes(s.V, s.F, s.H, s.W), 0);
  auto call = [&](int64_t V, int64_t F, const float* c2w, float fx, float fy, float cx, float cy, int H, int W, float near_,
                  int cull, float bg) {
    return ns_mesh_raster(vertices, V, faces, F, attr, c2w, fx, fy, cx, cy, H, W, near_, cull, bg, depth, tri, rgb, count, ws,
                          nullptr);
  };
  for (int h : {0, -1, 16385, INT32_MAX, INT32_MIN}) {
    expect(call(8, 4, good, 10, 10, 4, 4, h, 8, 0.5f, 0, 0), NS_E_INVALID);
    expect(call(8, 4, good, 10, 10, 4, 4, 8, h, 0.5f, 0, 0), NS_E_INVALID);
  }
  for (int64_t v : {int64_t(-1), limit, INT64_MIN, INT64_MAX}) {
    expect(call(v, 4, good, 10, 10, 4, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
    expect(call(8, v, good, 10, 10, 4, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
  }
  expect(call(8, 4, nullptr, 10, 10, 4, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
  for (int k = 0; k < 12; ++k)
    for (float v : {nan, inf, -inf}) {
      float m[12];
      for (int q = 0; q < 12; ++q) m[q] = good[q];
      m[k] = v;
      expect(call(8, 4, m, 10, 10, 4, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
    }
  for (float v : {nan, inf, -inf}) {
    expect(call(8, 4, good, v, 10, 4, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
    expect(call(8, 4, good, 10, v, 4, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
    expect(call(8, 4, good, 10, 10, v, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
    expect(call(8, 4, good, 10, 10, 4, v, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
    expect(call(8, 4, good, 10, 10, 4, 4, 8, 8, v, 0, 0), NS_E_INVALID);
    expect(call(8, 4, good, 10, 10, 4, 4, 8, 8, 0.5f, 0, v), NS_E_INVALID);
  }
  for (float v : {0.0f, -0.0f}) {
    expect(call(8, 4, good, v, 10, 4, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
    expect(call(8, 4, good, 10, v, 4, 4, 8, 8, 0.5f, 0, 0), NS_E_INVALID);
    expect(call(8, 4, good, 10, 10, 4, 4, 8, 8, v, 0, 0), NS_E_INVALID);
  }
  expect(call(8, 4, good, 10, 10, 4, 4, 8, 8, -1.0f, 0, 0), NS_E_INVALID);
  for (int c : {-1, 3, INT32_MAX, INT32_MIN}) expect(call(8, 4, good, 10, 10, 4, 4, 8, 8, 0.5f, c, 0), NS_E_INVALID);
  auto ptrs = [&](const float* v, const int64_t* f, int64_t F, const float* a, float* r, int64_t* c, void* w) {
    return ns_mesh_raster(v, 8, f, F, a, good, 10, 10, 4, 4, 8, 8, 0.5f, 0, 0, depth, tri, r, c, w, nullptr);
  };
  expect(ptrs(vertices, faces, 4, attr, rgb, nullptr, ws), NS_E_INVALID);
  expect(ptrs(vertices, faces, 0, attr, rgb, nullptr, ws), NS_E_INVALID);
  expect(ptrs(nullptr, faces, 4, attr, rgb, count, ws), NS_E_INVALID);
  expect(ptrs(vertices, nullptr, 4, attr, rgb, count, ws), NS_E_INVALID);
  expect(ptrs(vertices, faces, 4, attr, rgb, count, nullptr), NS_E_INVALID);
  expect(ptrs(vertices, faces, 4, nullptr, rgb, count, ws), NS_E_INVALID);
  expect(ptrs(vertices, faces, 0, nullptr, rgb, count, ws), NS_E_INVALID);
  expect(ptrs(vertices, reinterpret_cast<int64_t*>(0x2004), 4, attr, rgb, count, ws), NS_E_INVALID);
  expect(ptrs(vertices, reinterpret_cast<int64_t*>(0x2004), 0, attr, rgb, count, ws), NS_E_INVALID);
  expect(ptrs(vertices, faces, 4, attr, rgb, reinterpret_cast<int64_t*>(0x7004), ws), NS_E_INVALID);
  expect(ptrs(vertices, faces, 4, attr, rgb, count, reinterpret_cast<void*>(0x8004)), NS_E_INVALID);
  *cases = n;
  return bad;
}

// the header's coverage rule with plain arithmetic: whether pixel (i, j) is covered by the snapped triangle P
static bool rule(const int64_t (&X)[3], const int64_t (&Y)[3], int i, int j) {
  auto E = [](int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
  };
  const int64_t area2 = E(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
  if (area2 == 0) return false;
  const int64_t sg = area2 > 0 ? 1 : -1, px = int64_t(256) * i, py = int64_t(256) * j;
  int64_t sum = 0;
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const int64_t w = E(X[a], Y[a], X[b], Y[b], px, py), v = sg * w;
    sum += w;
    const int64_t dx = sg * (X[b] - X[a]), dy = sg * (Y[b] - Y[a]);
    const bool owned = dy < 0 || (dy == 0 && dx > 0);
    if (v < 0 || (v == 0 && !owned)) return false;
  }
  return sum == area2;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static int64_t draw(int64_t lo, int64_t hi) {               // [lo, hi], a xorshift generator: the same cases on every run
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return lo + static_cast<int64_t>(g_rng % static_cast<uint64_t>(hi - lo + 1));
}

// -> the number of pixels of the H x W frame the library's functions cover with the triangle; *wrong counts disagreements with the
// rule, pixels covered outside the clamped bounding box included
static int cover_count(const int64_t (&X)[3], const int64_t (&Y)[3], int H, int W, int* wrong, int* cover /* H*W or null */) {
  ns_raster::Proj v[3];
  for (int k = 0; k < 3; ++k) v[k] = ns_raster::Proj{static_cast<int32_t>(X[k]), static_cast<int32_t>(Y[k]), 1.0f + k, 1};
  ns_raster::Tri t;
  ns_raster::setup(v, H, W, t);
  int n = 0;
  for (int j = 0; j < H; ++j)
    for (int i = 0; i < W; ++i) {
      int64_t w[3];
      ns_raster::edge_values(t, i, j, w);
      const bool in_box = i >= t.i0 && i <= t.i1 && j >= t.j0 && j <= t.j1;
      const bool got = t.area2 != 0 && in_box && ns_raster::covered(t, w);
      const bool want = rule(X, Y, i, j);
      if (got != want || (t.area2 != 0 && w[0] + w[1] + w[2] != t.area2)) ++*wrong;
      if (got) {
        ++n;
        if (cover) ++cover[j * W + i];
      }
    }
  return n;
}

static int check_coverage(int64_t* triangles) {
  int wrong = 0;
  int64_t n = 0;
  const int H = 24, W = 29;
  for (int trial = 0; trial < 6000; ++trial) {
    int64_t X[3], Y[3];
    const int kind = trial % 6;
    for (int k = 0; k < 3; ++k) {
      if (kind == 0) X[k] = 256 * draw(-2, W + 1), Y[k] = 256 * draw(-2, H + 1);                // on pixel centres
      else if (kind == 1) X[k] = 128 * draw(-4, 2 * W + 4), Y[k] = 128 * draw(-4, 2 * H + 4);  // half pixels
      else if (kind == 2) X[k] = draw(-600, 256 * W + 600), Y[k] = draw(-600, 256 * H + 600);
      else if (kind == 3) X[k] = draw(0, 2048), Y[k] = draw(0, 2048);                           // small, many ties
      else if (kind == 4) X[k] = draw(-(1 << 28), 1 << 28), Y[k] = draw(-(1 << 28), 1 << 28);   // the whole band
      else X[k] = (k == 1 ? 1 : -1) * (int64_t(1) << 28), Y[k] = (k == 2 ? 1 : -1) * (int64_t(1) << 28);   // its corners
    }
    if (kind == 5 && trial % 12 == 5) X[0] = -X[0];
    cover_count(X, Y, H, W, &wrong, nullptr);
    ++n;
  }
  // a quad with corners on pixel centres, split along either diagonal: every winding of either triangle, each centre once
  const int64_t qx[4] = {256, 1280, 1280, 256}, qy[4] = {256, 256, 1280, 1280};
  const int order[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {2, 1, 0}, {1, 0, 2}};
  const int split[2][2][3] = {{{0, 1, 2}, {0, 2, 3}}, {{1, 2, 3}, {1, 3, 0}}};
  for (const auto& pair : split)
    for (const auto& oa : order)
      for (const auto& ob : order) {
        int cover[7 * 8] = {0};
        for (int side = 0; side < 2; ++side) {
          const int* o = side == 0 ? oa : ob;
          int64_t X[3], Y[3];
          for (int k = 0; k < 3; ++k) X[k] = qx[pair[side][o[k]]], Y[k] = qy[pair[side][o[k]]];
          cover_count(X, Y, 7, 8, &wrong, cover);
          ++n;
        }
        for (int j = 0; j < 7; ++j)
          for (int i = 0; i < 8; ++i)
            if (cover[j * 8 + i] != ((i >= 1 && i < 5 && j >= 1 && j < 5) ? 1 : 0)) ++wrong;
      }
  // a fan around the pixel centre (3, 3): the centre and every other covered centre exactly once, under 64 windings
  const int64_t fx[7] = {768, 0, 768, 1536, 1536, 768, 0}, fy[7] = {768, 256, 0, 256, 1280, 1536, 1280};
  int first[64] = {0};
  for (int mask = 0; mask < 64; ++mask) {
    int cover[64] = {0};
    for (int k = 0; k < 6; ++k) {
      const int a = 1 + k, b = 1 + (k + 1) % 6;
      const int idx[3] = {0, (mask >> k) & 1 ? b : a, (mask >> k) & 1 ? a : b};
      int64_t X[3], Y[3];
      for (int q = 0; q < 3; ++q) X[q] = fx[idx[q]], Y[q] = fy[idx[q]];
      cover_count(X, Y, 8, 8, &wrong, cover);
      ++n;
    }
    if (cover[3 * 8 + 3] != 1) ++wrong;
    for (int p = 0; p < 64; ++p) {
      if (cover[p] > 1) ++wrong;
      if (mask == 0) first[p] = cover[p];
      else if (cover[p] != first[p]) ++wrong;
    }
  }
  *triangles = n;
  return wrong;
}

int main() {
  int cases = 0;
  int64_t triangles = 0;
  const int bad_arguments = check_arguments(&cases);
  const int bad_coverage = check_coverage(&triangles);
  std::printf("%d argument and size cases, %d wrong; %lld triangles rasterised on the CPU against the rule, %d disagreements\n",
              cases, bad_arguments, static_cast<long long>(triangles), bad_coverage);
  return (bad_arguments + bad_coverage) != 0;
}
