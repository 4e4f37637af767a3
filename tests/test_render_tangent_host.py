"""Host side of the one-kernel renderer's depth tangents (ns_render_rays_fused_tangent), no GPU needed: ns_tangent_args as the
header lays it out against its ctypes mirror, the new symbols in the binding table, the code objects of the tangent kernel on
f16x3 and on f16 fields (no scratch, no spill, registers within a gfx950 SIMD, LDS within a CU), and the Python argument checks,
which raise before the library is touched."""

import ctypes
import os
import re
import shutil

import pytest
import torch

from nerf_sampling_amd import _lib, autograd, ops
from test_depth_acc_maps_host import _field, _kernel_notes, _layout, _notes_and_isa
from test_kernel_invariants import _functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["mean_dev", "d_rgb_dev", "d_disp_dev", "d_depth_dev", "d_acc_dev"]


def test_tangent_args_layout_matches_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    assert [f for f, _ in _lib.TangentArgs._fields_] == FIELDS
    got = _layout(tmp_path, "ns_tangent_args", tuple(FIELDS))
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert got["sizeof"] == ctypes.sizeof(_lib.TangentArgs) == len(FIELDS) * ptr
    for f in FIELDS:
        assert got[f] == getattr(_lib.TangentArgs, f).offset, f


def test_tangent_symbols_are_bound():
    hdr = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
    for name in ("ns_render_tangent_supported", "ns_render_tangent_workspace_bytes", "ns_render_rays_fused_tangent"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["ns_render_rays_fused_tangent"]
    assert args[1]._type_ is _lib.TangentArgs


# the two instantiations of the tangent renderer (ns_tangent.h): kernel name, mangled template arguments of its instances by
# width (NKB = W / 32; bf16 is not instantiated: refused), bytes of one block in the embedding stash,
# samples per group
KERNELS = {
    "f16x3": ("nerf_mlp_x3_tan_kernel", {256: "ILi8E", 128: "ILi4E"}, 2048, 64),
    "f16": ("nerf_tan16_kernel", {256: "Mma16F16ELi8E", 128: "Mma16F16ELi4E"}, 1024, 128),
}


def _blocks(kernel):
    out = []
    for dis, notes in _notes_and_isa(kernel.encode()):
        fns = _functions(dis)
        for name, blk in _kernel_notes(notes).items():
            if kernel in name and not name.endswith(".kd"):
                out.append((name, blk, fns.get(name, [])))
    return out


@pytest.mark.parametrize("field", list(KERNELS))
def test_tangent_kernel_keeps_no_scratch_and_fits_the_cu(field):
    """Both widths of the tangent kernel (W = 256 and W = 128): no private segment, no spilled VGPR, VGPRs + AGPRs within the
    512 of a gfx950 SIMD lane, no scratch instruction, no more full DMA waits than the forward kernels are allowed."""
    kernel, instances, _stash, _gs = KERNELS[field]
    seen = set()
    for name, blk, ins in _blocks(kernel):
        key = [w for w, tag in instances.items() if tag in name]
        assert len(key) == 1, name
        seen.add(key[0])
        assert _field(blk, "private_segment_fixed_size") == 0, name
        assert _field(blk, "vgpr_spill_count") == 0, name
        assert _field(blk, "vgpr_count") <= 512, name
        assert ins, name
        assert not any(i.startswith("scratch_") for i in ins), name
        full_waits = sum(bool(re.search(r"s_waitcnt vmcnt\(0\)(?! *lgkmcnt)|s_waitcnt vmcnt\(0\)$", i)) for i in ins)
        assert full_waits <= 10, (name, full_waits)
    assert seen == set(instances), sorted(seen)


# dynamic LDS of the tangent launch: this MIRRORS tan_lds_bytes (ns_tangent.h) -- the library exposes it nowhere, so a change
# there must be repeated here; launch_tan refuses at run time what exceeds 160 KiB.  For a group of gs samples (gs / 64 primal
# tiles per wave and as many tangent tiles): weight ring (4 slabs x 16 KiB) | bias image | embedding stash (4 waves x 2 gs / 64
# register tiles x 3 blocks of `stash` bytes) | input staging (4 waves x 11 slots x 256 B) | compositing records of the group
# (gs x 36 B + 512 B, ns_comp_epilogue.h) | tangent records (gs x 16 B of d raw, two parities of gs x 8 B of {dz, d dist}, 64 B
# of walk state)
def _dynamic_lds(bias_floats, stash, gs):
    ring, staging = 4 * 16384, 4 * 11 * 256
    return (ring + (bias_floats * 4 + 15) // 16 * 16 + 4 * (2 * gs // 64) * 3 * stash + staging + (gs * 36 + 512) +
            (gs * 16 + 2 * gs * 8 + 64))


@pytest.mark.parametrize("W,D", [(256, 8), (128, 8), (128, 4)])
@pytest.mark.parametrize("field", list(KERNELS))
def test_tangent_kernel_fits_the_cu_lds(field, W, D):
    kernel, instances, stash, gs = KERNELS[field]
    bias_floats = D * W + (W // 2 + 16) + 16     # D hidden layers, the view layer + sigma sub-block, the rgb sub-block
    dynamic = _dynamic_lds(bias_floats, stash, gs)
    checked = 0
    for name, blk, _ins in _blocks(kernel):
        if instances[W] not in name:
            continue
        checked += 1
        assert _field(blk, "group_segment_fixed_size") + dynamic <= 160 * 1024, (name, dynamic)
    assert checked == 1


def _packed(kind="nerf", dtype="f16x3"):
    return ops.PackedWeights(0, kind, dtype, "cpu")


CAM = (8, 8, [[8.0, 0, 4], [0, 8.0, 4], [0, 0, 1]], None, 0, 8)


def test_argument_checks_raise_before_the_library(monkeypatch):
    """Every check of ops.render_rays_depthnet_tangent / autograd.render_depthnet_differentiable fires before _lib.load()"""
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    dn = _packed("depthnet", "f16x3")
    kw = dict(camera=CAM, n_samples=16, std=0.1)
    with pytest.raises(NotImplementedError, match="f16x3"):
        ops.render_rays_depthnet_tangent(dn, _packed(dtype="bf16"), **kw)
    with pytest.raises(NotImplementedError, match="f16x3"):
        ops.render_rays_depthnet_tangent(dn, None, **kw)
    for n in (1, 3, 96, 576, 1024):
        with pytest.raises(NotImplementedError, match="n_samples"):
            ops.render_rays_depthnet_tangent(dn, _packed(), camera=CAM, n_samples=n, std=0.1)
    with pytest.raises(ValueError, match="exactly one"):
        ops.render_rays_depthnet_tangent(dn, _packed(), n_samples=16, std=0.1)
    with pytest.raises(ValueError, match="extras"):
        ops.render_rays_depthnet_tangent(dn, _packed(), extras=("z",), **kw)
    with pytest.raises(TypeError):
        ops.render_rays_depthnet_tangent(_packed("nerf"), _packed(), **kw)
    with pytest.raises(TypeError):
        ops.render_rays_depthnet_tangent([2.0] * 64, _packed(), **kw)
    with pytest.raises(RuntimeError, match="GPU"):            # a CPU depth tensor: this path has no CPU fallback
        ops.render_rays_depthnet_tangent(torch.full((64,), 3.0), _packed(), **kw)
    with pytest.raises(NotImplementedError, match="f16x3"):
        autograd.render_depthnet_differentiable(None, _packed(dtype="f32"), **kw)
    with pytest.raises(NotImplementedError, match="n_samples"):
        autograd.render_depthnet_differentiable(None, _packed(), camera=CAM, n_samples=100, std=0.1)
    with pytest.raises(ValueError, match="exactly one"):
        autograd.render_depthnet_differentiable(None, _packed(), n_samples=16, std=0.1)
    with pytest.raises(ValueError, match="chunk"):
        autograd.render_depthnet_differentiable(None, _packed(), chunk=0, **kw)
