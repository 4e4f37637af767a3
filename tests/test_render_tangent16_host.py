"""Host side of the depth tangents on an f16 field (ns_nerf_mlp_ob16_tan.hip), no GPU needed: the kernel's code objects at both
widths (no scratch, no spill, registers within a gfx950 SIMD lane, LDS within a CU), and the opt-in of the Python
entry points, whose checks fire before the library is touched."""

import inspect
import re

import pytest

from nerf_sampling_amd import _lib, autograd, ops
from test_depth_acc_maps_host import _field, _kernel_notes, _notes_and_isa
from test_kernel_invariants import _functions

KERNEL = "nerf_tan16_kernel"
# mangled template arguments of the instances: operand type, NKB = W / 32 (bf16 is not instantiated: refused)
INSTANCES = {("Mma16F16", 256): "Mma16F16ELi8E", ("Mma16F16", 128): "Mma16F16ELi4E"}


def _blocks():
    out = []
    for dis, notes in _notes_and_isa(KERNEL.encode()):
        fns = _functions(dis)
        for name, blk in _kernel_notes(notes).items():
            if KERNEL in name and not name.endswith(".kd"):
                out.append((name, blk, fns.get(name, [])))
    return out


def test_tangent16_kernels_keep_no_scratch_and_fit_the_simd():
    """W = 256 and W = 128: no private segment, no spilled VGPR, VGPRs + AGPRs within the 512 of a gfx950 SIMD
    lane, no scratch instruction, no more full DMA waits than the forward kernels are allowed"""
    seen = set()
    for name, blk, ins in _blocks():
        key = [k for k, v in INSTANCES.items() if v in name]
        assert len(key) == 1, name
        seen.add(key[0])
        assert _field(blk, "private_segment_fixed_size") == 0, name
        assert _field(blk, "vgpr_spill_count") == 0, name
        assert _field(blk, "vgpr_count") <= 512, name
        assert ins, name
        assert not any(i.startswith("scratch_") for i in ins), name
        full_waits = sum(bool(re.search(r"s_waitcnt vmcnt\(0\)(?! *lgkmcnt)|s_waitcnt vmcnt\(0\)$", i)) for i in ins)
        assert full_waits <= 10, (name, full_waits)
    assert seen == set(INSTANCES), sorted(seen)


# dynamic LDS of the launch: these constants MIRROR tan16_lds_bytes (ns_nerf_mlp_ob16_tan.hip) -- the library exposes it nowhere,
# so a change there must be repeated here; launch_tan16 refuses at run time what exceeds 160 KiB.  Weight ring (4 slabs x 16 KiB)
# | bias image | embedding stash (4 waves x 4 register tiles x 3 blocks x 1 KiB) | input staging (4 waves x 11 slots x 256 B) |
# compositing records of a 128-sample group (128 x 36 B + 512 B, ns_comp_epilogue.h) | tangent records (128 x 16 B of d raw, two
# parities of 128 x 8 B of {dz, d dist}, 64 B of walk state)
RING, STASH, STAGING = 4 * 16384, 4 * 4 * 3 * 1024, 4 * 11 * 256
RECORDS, TAN_RECORDS = 128 * 36 + 512, 128 * 16 + 2 * 128 * 8 + 64


@pytest.mark.parametrize("W,D", [(256, 8), (128, 8), (128, 4)])
def test_tangent16_kernels_fit_the_cu_lds(W, D):
    bias_floats = D * W + (W // 2 + 16) + 16     # D hidden layers, the view layer + sigma sub-block, the rgb sub-block
    dynamic = RING + (bias_floats * 4 + 15) // 16 * 16 + STASH + STAGING + RECORDS + TAN_RECORDS
    checked = 0
    for name, blk, _ins in _blocks():
        if ("ELi8E" in name) != (W == 256):
            continue
        checked += 1
        assert _field(blk, "group_segment_fixed_size") + dynamic <= 160 * 1024, (name, dynamic)
    assert checked == 1


def _packed(kind="nerf", dtype="f16x3"):
    return ops.PackedWeights(0, kind, dtype, "cpu")


CAM = (8, 8, [[8.0, 0, 4], [0, 8.0, 4], [0, 0, 1]], None, 0, 8)


class _Reached(Exception):
    pass


def test_approximate_admits_an_f16_field_and_nothing_else(monkeypatch):
    """approximate=True lets an f16 handle through every check to the library; bf16 and f32 stay refused, and without the
    opt-in an f16 handle is refused as before"""
    def reached():
        raise _Reached()
    monkeypatch.setattr(_lib, "load", reached)
    dn = _packed("depthnet", "f16x3")
    kw = dict(camera=CAM, n_samples=16, std=0.1)
    with pytest.raises(_Reached):
        ops.render_rays_depthnet_tangent(dn, _packed(dtype="f16"), approximate=True, **kw)
    for dtype in ("bf16", "f16"):
        with pytest.raises(NotImplementedError, match="f16x3"):
            ops.render_rays_depthnet_tangent(dn, _packed(dtype=dtype), **kw)
        with pytest.raises(NotImplementedError, match="f16x3"):
            autograd.render_depthnet_differentiable(None, _packed(dtype=dtype), **kw)
    with pytest.raises(NotImplementedError, match="n_samples"):
        ops.render_rays_depthnet_tangent(dn, _packed(dtype="f16"), camera=CAM, n_samples=96, std=0.1, approximate=True)
    for dtype in ("bf16", "f32"):
        for approximate in (False, True):
            with pytest.raises(NotImplementedError, match=dtype):
                ops.render_rays_depthnet_tangent(dn, _packed(dtype=dtype), approximate=approximate, **kw)
            with pytest.raises(NotImplementedError, match=dtype):
                autograd.render_depthnet_differentiable(None, _packed(dtype=dtype), approximate=approximate, **kw)
    for fn in (ops.render_rays_depthnet_tangent, autograd.render_depthnet_differentiable):
        p = inspect.signature(fn).parameters["approximate"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, fn.__name__
