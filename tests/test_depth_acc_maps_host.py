"""Host side of the renderers' depth / acc maps, no GPU needed: the new ns_render_args / ns_hier_args fields as the header lays
them out, the extras names ops accepts, and the compositing kernels' code objects (no scratch, no spill, registers within the
register file, no extra full DMA wait) with the map stores built in."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest

from nerf_sampling_amd import _lib, ops
from test_kernel_invariants import LIB, LLVM, _functions, _gfx950_code_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layout(tmp_path, struct, fields):
    src = tmp_path / "maps_layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nerf_sampling_hip.h"', "int main(void) {",
             f'  printf("sizeof %zu\\n", sizeof({struct}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "maps_layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


# (ns_hier_args keeps the max-weight sample's three pointers as its tail: the maps go in front of them)
@pytest.mark.parametrize("cls,struct,tail", [
    (_lib.RenderArgs, "ns_render_args", ["guard_threshold", "depth_dev", "acc_dev"]),
    (_lib.HierArgs, "ns_hier_args", ["ev_coarse_end", "depth_dev", "acc_dev", "max_z_dev", "max_w_dev", "max_rgb_dev"])])
def test_map_fields_are_declared_and_mirrored(tmp_path, cls, struct, tail):
    """depth_dev, acc_dev: where the header declares them, at the offsets and with the size ctypes uses"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = [f for f, _ in cls._fields_]
    assert names[-len(tail):] == tail, names[-len(tail):]
    fields = tuple(tail)
    got = _layout(tmp_path, struct, fields)
    assert got["sizeof"] == ctypes.sizeof(cls)
    ptr = ctypes.sizeof(ctypes.c_void_p)
    for f in fields:
        assert got[f] == getattr(cls, f).offset, f
    for f in ("depth_dev", "acc_dev"):
        assert getattr(cls, f).size == ptr
    assert got["acc_dev"] == got["depth_dev"] + ptr
    assert got["sizeof"] == got[tail[-1]] + ptr


def test_extras_names_are_checked_before_anything_runs():
    """unknown names raise ValueError before the library is touched (handles may be anything then)"""
    kw = dict(camera=(8, 8, [[8.0, 0, 4], [0, 8.0, 4], [0, 0, 1]], None, 0, 8), n_samples=16, mode="uniform", std=0.1)
    for bad in (("depth", "raw"), ("alphas",), ("disp",), ("z", "rgb")):
        with pytest.raises(ValueError, match="extras"):
            ops.render_rays_depthnet(None, None, extras=bad, **kw)
    for bad in (("pts",), ("depth", "alphas"), ("rgb",)):
        with pytest.raises(ValueError, match="extras"):
            ops.render_rays_hierarchical(None, None, camera=kw["camera"], extras=bad)


def test_extras_names_resolve():
    assert ops._extras_names(True, ("z", "weights", "pts")) == ("z", "weights", "pts")
    assert ops._extras_names(False, ("z", "weights", "pts")) == ()
    assert ops._extras_names(None, ("z", "weights", "raw")) == ()
    assert ops._extras_names(("acc", "z"), ("z", "weights", "pts")) == ("acc", "z")
    assert ops._extras_names(["depth"], ("z", "weights", "raw")) == ("depth",)
    assert ops._extras_names(1, ("z", "weights", "raw")) == ("z", "weights", "raw")


def _notes_and_isa(name_part: bytes):
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    import tempfile

    out = []
    for co in _gfx950_code_objects(LIB):
        if name_part not in co:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", f.name],
                                 capture_output=True, text=True, check=True).stdout
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name],
                                   capture_output=True, text=True, check=True).stdout
        out.append((dis, notes))
    assert out, name_part
    return out


def _kernel_notes(notes):
    """kernel name -> its metadata block (the AMDGPU notes list one block per kernel, .agpr_count first)"""
    res = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        m = re.search(r"\.name:\s*(\S+)", blk)
        if m:
            res[m.group(1)] = ".agpr_count: " + blk
    return res


def _field(blk, key):
    return int(re.search(r"\." + key + r":\s*(\d+)", blk).group(1))


def test_compositing_kernels_keep_no_scratch_and_fit_the_register_file():
    """Every kernel that composites and now stores depth / acc: the 16-bit MLP kernel on rays (four tiles and the five-tile
    production unit), the split-fp16 compositing kernel, the stand-alone raw2outputs kernels and the selective guard's fix-up --
    no private segment, no spilled VGPR, VGPRs + AGPRs within the 512 of a gfx950 SIMD lane, and (MLP kernels) no more full
    DMA waits than the existing invariants allow."""
    seen = set()
    for part, pat in ((b"nerf_mlp_ob16_kernel", r"nerf_mlp_ob16_kernel.*ELb0ELb[01]ELi[45]EEE"),
                      (b"nerf_mlp_x3_comp_kernel", r"nerf_mlp_x3_comp_kernel"),
                      (b"raw2outputs_kernel", r"18raw2outputs_kernel"),
                      (b"fix_last_sample_kernel", r"fix_last_sample_kernel")):
        for dis, notes in _notes_and_isa(part):
            blocks = {k: v for k, v in _kernel_notes(notes).items() if re.search(pat, k) and not k.endswith(".kd")}
            fns = _functions(dis)
            for name, blk in blocks.items():
                seen.add(name)
                assert _field(blk, "private_segment_fixed_size") == 0, name
                assert _field(blk, "vgpr_spill_count") == 0, name
                assert _field(blk, "vgpr_count") <= 512, name
                ins = fns.get(name, [])
                assert ins, name
                assert not any(i.startswith("scratch_") for i in ins), name
                if b"nerf_mlp" in part:
                    full_waits = sum(bool(re.search(r"s_waitcnt vmcnt\(0\)(?! *lgkmcnt)|s_waitcnt vmcnt\(0\)$", i)) for i in ins)
                    assert full_waits <= 10, (name, full_waits)
    # bf16 / f16 x (W = 256 generic, W = 128 generic, production four tiles, production five tiles); three split-fp16 forms;
    # six segment widths of raw2outputs; the fix-up for records of rays of one chunk and of several
    assert sum("nerf_mlp_ob16_kernel" in k for k in seen) == 8, sorted(seen)
    assert sum("nerf_mlp_x3_comp_kernel" in k for k in seen) == 3, sorted(seen)
    assert sum("raw2outputs_kernel" in k for k in seen) == 6, sorted(seen)
    assert sum("fix_last_sample_kernel" in k for k in seen) == 2, sorted(seen)
