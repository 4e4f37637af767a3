"""Static invariants of the split-fp16 (f16x3) NeRF kernel's compositing form, nerf_mlp_x3_comp_kernel (the one-kernel renderer
on an f16x3 field: placement, MLP and compositing in one kernel), on the built gfx950 code objects -- no GPU needed.  The same
properties test_kernel_invariants.py holds the other MLP kernels to: no scratch, no compiler-inserted full DMA wait per slab
step, the production program still straight-line generated code, and the LDS the launch asks for within the CU's 160 KiB."""
import re

import pytest

from test_kernel_invariants import _functions, _isa_of

# dynamic LDS of the compositing launch: these constants MIRROR comp_lds_bytes (ns_nerf_mlp_x3.hip) and the bias layout of
# ns_pack.hip -- the library exposes neither, so a change there must be repeated here; launch_comp refuses at run time what
# exceeds 160 KiB.  Weight ring (4 slabs x 16 KiB) | bias image | embedding stash (4 waves x 2 tiles x 3 blocks x hi / lo
# 1 KiB) | input staging (4 waves x 11 slots x 256 B) | compositing records (128 samples x 36 B + 512 B of chunk scalars,
# ns_comp_epilogue.h)
RING, STASH, STAGING, RECORDS = 4 * 16384, 4 * 2 * 3 * 2048, 4 * 11 * 256, 128 * 36 + 512


def _bias_floats(W, D):
    """the bias image of a NeRF with view directions: D hidden layers of W rows, the view layer's W/2 rows + the sigma
    sub-block, the rgb sub-block, each padded to 16-row sub-blocks"""
    return D * W + (W // 2 + 16) + 16


@pytest.fixture(scope="module")
def comp_kernels():
    dis, notes = _isa_of(b"nerf_mlp_x3_kernel")
    fns = {k: [i.split("//")[0].strip() for i in v] for k, v in _functions(dis).items() if "nerf_mlp_x3_comp_kernel" in k}
    return fns, notes


def test_three_compositing_instantiations(comp_kernels):
    fns, _ = comp_kernels
    # production (W = 256, generated layers), generic W = 256, generic W = 128
    assert sorted(re.search(r"kernelI(.*?)EEE", k).group(1) for k in fns) == ["Li4ELb0", "Li8ELb0", "Li8ELb1"], sorted(fns)


def test_compositing_kernels_use_no_scratch_and_no_full_dma_wait(comp_kernels):
    fns, notes = comp_kernels
    for name, ins in fns.items():
        assert not any(i.startswith("scratch_") for i in ins), f"{name}: scratch access in the kernel"
        full_waits = sum(bool(re.search(r"s_waitcnt vmcnt\(0\)(?! *lgkmcnt)|s_waitcnt vmcnt\(0\)$", i)) for i in ins)
        assert full_waits <= 10, f"{name}: {full_waits} s_waitcnt vmcnt(0)"
        m = re.search(re.escape(name) + r".*?\.private_segment_fixed_size:\s*(\d+)", notes, re.S)
        assert m and int(m.group(1)) == 0, name


def test_production_compositing_kernel_is_straight_line(comp_kernels):
    fns, _ = comp_kernels
    prod = [v for k, v in fns.items() if "ILi8ELb1EEE" in k]
    assert len(prod) == 1
    # three MFMAs per product term, two tiles per wave: the layer statements of the rays -> raw kernel, unchanged
    assert sum("v_mfma_f32_16x16x32_f16" in i for i in prod[0]) == 3 * 4180 // 2


@pytest.mark.parametrize("W,D", [(256, 8), (128, 8)])
def test_compositing_kernels_fit_the_cu_lds(comp_kernels, W, D):
    fns, notes = comp_kernels
    dynamic = RING + (_bias_floats(W, D) * 4 + 15) // 16 * 16 + STASH + STAGING + RECORDS
    for name in fns:
        if ("ILi8E" in name) != (W == 256):
            continue
        m = re.search(re.escape(name) + r".*?\.group_segment_fixed_size:\s*(\d+)", notes, re.S)
        assert m, name
        assert int(m.group(1)) + dynamic <= 160 * 1024, (name, int(m.group(1)), dynamic)
