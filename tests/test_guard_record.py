"""The selective PSNR guard's record of a flagged ray (csrc/ns_guard.h), no GPU needed: a host program that includes the header
prints every field offset and both record sizes, and they must be what the producers (the one-kernel renderer's epilogue), the
gather, the fix-up kernel and the workspace layout agree on."""

import os
import shutil
import subprocess

import pytest

from nerf_sampling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf_sampling_amd", "csrc")

SHORT = ("kSum", "kT", "kRaw", "kZ", "kDist", "kRayLo", "kRayHi", "kFloats")
LONG = ("kLongSum", "kLongT", "kLongRaw", "kLongZ", "kLongDist", "kLongRayLo", "kLongRayHi", "kLongOps", "kLongFloats")


def test_guard_record_layout_is_what_the_header_says(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    lines = ['#include <cstdio>', '#include "ns_guard.h"', "int main() {"]
    lines += [f'  std::printf("{n} %d\\n", static_cast<int>(nsfix::{n}));' for n in SHORT + LONG + ("kSums", "kOps")]
    lines += ['  std::printf("NS_FIX_LONG_FLOATS %d\\n", static_cast<int>(NS_FIX_LONG_FLOATS));',
              # the ray index through the header's own two halves and back, on a record of either length
              "  float rec[nsfix::kLongFloats] = {};",
              "  const long long r = 0x123456789abLL;",
              "  rec[nsfix::kRayLo] = nsfix::fix_ray_lo(r); rec[nsfix::kRayHi] = nsfix::fix_ray_hi(r);",
              '  std::printf("roundtrip %d\\n", nsfix::fix_ray_of(rec) == r ? 1 : 0);',
              "  return 0;", "}"]
    src = tmp_path / "guard_layout.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "guard_layout"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}

    assert got["kFloats"] == 16
    assert got["kLongFloats"] == 48 == got["NS_FIX_LONG_FLOATS"]
    # the single-chunk record: five sums, T, raw rgb, z, dist, ray index lo / hi
    assert [got[n] for n in SHORT[:-1]] == [0, 5, 6, 9, 10, 11, 12]
    assert got["kSums"] == 5 and got["kOps"] == 6
    # ray index and z (what fix_gather_kernel reads of either record) and the rest of floats 5 .. 12 sit where they do in both
    for s, l in zip(SHORT[:-1], LONG[:-2]):
        assert got[s] == got[l], (s, l)
    # the operand block: behind the shared fields, six operands of five sums, inside the record
    assert got["kLongOps"] == 16
    assert got["kLongOps"] + got["kOps"] * got["kSums"] <= got["kLongFloats"]
    assert got["kFloats"] % 4 == 0 and got["kLongFloats"] % 4 == 0
    assert got["roundtrip"] == 1

    # the long-guard workspace differs from the plain one by the records alone: kLongFloats floats per ray instead of kFloats
    # (R a multiple of 4: both record slices are whole 256-byte units)
    lib = _lib.load()
    for R in (4, 1000, 640000):
        extra = int(lib.ns_render_fused_guard_long_workspace_bytes(R)) - int(lib.ns_render_fused_workspace_bytes(R))
        assert extra == R * 4 * (got["kLongFloats"] - got["kFloats"]), R
    # ... and the plain one holds kFloats floats per ray: the rest of its layout at R = 1000 is 6 ray slices of 12 bytes per ray, mean
    # and z_last of 4, raw_last of 16 and the counter's 256
    rest = 6 * 12032 + 2 * 4096 + 16128 + 256
    assert int(lib.ns_render_fused_workspace_bytes(1000)) - rest == 1000 * 4 * got["kFloats"]
