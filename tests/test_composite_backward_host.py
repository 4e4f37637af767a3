"""Host-side checks of the compositing / placement backward (no GPU): the C entries are declared in the header with the
argument counts _lib binds, the built library holds their kernels, and those kernels use no scratch and stay within their LDS
budget -- read from the gfx950 code object as tests/test_x3_composite_invariants.py does."""
import os
import re

import pytest

from test_kernel_invariants import _functions, _isa_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ns_raw2outputs_backward", "ns_place_samples_backward")
# the chunked kernel keeps the transmittance entering each of up to 64 chunks per wave, four waves: 1 KiB
CHUNK_LDS = 4 * 64 * 4


def _header_arg_count(name):
    hdr = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in the header"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_declared_and_bound(name):
    from nerf_sampling_amd import _lib

    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert len(args) == _header_arg_count(name)


@pytest.fixture(scope="module")
def bwd_kernels():
    dis, notes = _isa_of(b"raw2outputs_backward_kernel")
    fns = {k: v for k, v in _functions(dis).items() if "backward" in k}
    return fns, notes


def test_backward_kernels_are_built(bwd_kernels):
    fns, _ = bwd_kernels
    one = sorted(int(re.search(r"raw2outputs_backward_kernelILi(\d+)E", k).group(1)) for k in fns
                 if "raw2outputs_backward_kernelI" in k)
    assert one == [2, 4, 8, 16, 32, 64], sorted(fns)
    for part in ("raw2outputs_backward_chunks_kernel", "raw2outputs_backward_single_kernel", "place_backward_kernel"):
        assert any(part in k for k in fns), (part, sorted(fns))


def _kernel_metadata(notes):
    """kernel symbol -> its metadata block of the code object's notes (one YAML map per kernel, .name inside it)"""
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        m = re.search(r"\.name:\s*(\S+)", block)
        if m:
            out[m.group(1)] = block
    return out


def test_backward_kernels_use_no_scratch_and_fit_their_lds(bwd_kernels):
    fns, notes = bwd_kernels
    meta = _kernel_metadata(notes)
    for name, ins in fns.items():
        assert not any(i.split("//")[0].strip().startswith("scratch_") for i in ins), f"{name}: scratch access"
        block = meta[name]
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", block).group(1)) == 0, name
        lds = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", block).group(1))
        assert lds <= (CHUNK_LDS if "chunks" in name else 0), (name, lds)


def test_backward_refuses_more_than_4096_samples_before_any_launch():
    from nerf_sampling_amd import _lib

    lib = _lib.load()
    rc = lib.ns_raw2outputs_backward(None, None, None, None, 1, 4097, 0, None, None, None, None, None, None, None, None,
                                     None, None)
    assert rc == -1 and b"4096" in lib.ns_last_error()
