// The host side of ns_frame_to8b -- every argument check and the empty frame, all of which return ahead of the launch --
// as a stand-alone program for a host sanitizer run on a machine without a GPU (the pointers are never dereferenced):
//
//   cd nerf_sampling_amd/csrc
//   F="--offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c ns_frames.hip -o /tmp/frames.o && hipcc $F -x hip -c ns_core.cpp -o /tmp/core.o
//   hipcc $F -x hip -c ../../tools/frame_to8b_hostcheck.cpp -o /tmp/main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/frames.o /tmp/core.o /tmp/main.o -o /tmp/hostcheck
//   /tmp/hostcheck
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../include/nerf_sampling_hip.h"

int main() {
  float* rgb = reinterpret_cast<float*>(0x1000);
  uint8_t* out = reinterpret_cast<uint8_t*>(0x2000);
  int bad = 0, n = 0;
  auto expect = [&](int rc, int want) {
    ++n;
    if (rc != want) {
      ++bad;
      std::printf("case %d: rc %d, want %d\n", n, rc, want);
    }
  };
  expect(ns_frame_to8b(rgb, 0, nullptr, 0, out, 3, nullptr), NS_OK);
  expect(ns_frame_to8b(nullptr, 4, nullptr, 0, nullptr, 4, nullptr), NS_OK);
  expect(ns_frame_to8b(nullptr, 0, nullptr, 5, out, 3, nullptr), NS_E_INVALID);
  expect(ns_frame_to8b(rgb, 0, nullptr, 5, nullptr, 3, nullptr), NS_E_INVALID);
  expect(ns_frame_to8b(rgb, 0, nullptr, -1, out, 3, nullptr), NS_E_INVALID);
  expect(ns_frame_to8b(rgb, 0, nullptr, INT64_MIN, out, 3, nullptr), NS_E_INVALID);
  expect(ns_frame_to8b(rgb, 0, nullptr, int64_t(1) << 29, out, 3, nullptr), NS_E_INVALID);
  expect(ns_frame_to8b(rgb, 3, nullptr, INT64_MAX, out, 4, nullptr), NS_E_INVALID);
  for (int64_t s : {int64_t(-1), int64_t(1), int64_t(2), int64_t(5), INT64_MAX, INT64_MIN})
    expect(ns_frame_to8b(rgb, s, nullptr, 5, out, 3, nullptr), NS_E_INVALID);
  for (int c : {-3, 0, 1, 2, 5, INT32_MAX, INT32_MIN}) expect(ns_frame_to8b(rgb, 0, nullptr, 5, out, c, nullptr), NS_E_INVALID);
  std::printf("%d cases, %d wrong; last error: %s\n", n, bad, ns_last_error());
  return bad != 0;
}
