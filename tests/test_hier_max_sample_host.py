"""Host side of the hierarchical renderer's max-weight sample (not gpu): the workspace size function and the ABI fields."""

import os
import re

import pytest

from nerf_sampling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def align256(x):
    return (x + 255) // 256 * 256


def test_max_workspace_is_the_layout_plus_one_fine_slice():
    lib = _lib.load()
    for R in (0, 1, 7, 256, 1081, 640000):
        for nc, nf in ((64, 128), (64, 64), (32, 32), (8, 8), (4, 4), (64, 448), (64, 32), (3, 0), (64, 0)):
            old = int(lib.ns_hier_workspace_bytes(R, nc, nf))
            new = int(lib.ns_hier_max_workspace_bytes(R, nc, nf))
            assert new == old + align256(R * (nc + nf) * 4), (R, nc, nf, old, new)
    for args in ((-1, 64, 128), (10, 2, 8), (10, 64, -1)):
        assert int(lib.ns_hier_workspace_bytes(*args)) == 0
        assert int(lib.ns_hier_max_workspace_bytes(*args)) == 0


def test_max_fields_come_last_in_header_and_mirror():
    names = [f for f, _ in _lib.HierArgs._fields_]
    assert names[-3:] == ["max_z_dev", "max_w_dev", "max_rgb_dev"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct ns_hier_args \{(.*?)\} ns_hier_args;", text, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-3:] == ["float* max_z_dev", "float* max_w_dev", "float* max_rgb_dev"]
    assert "ns_hier_max_workspace_bytes" in _lib.SIGNATURES


def test_max_sample_refusals_before_any_launch():
    """Bad combinations are refused by the host checks, before a ray is generated (so on a CPU-only box as well)."""
    import ctypes as C

    lib = _lib.load()
    a = _lib.HierArgs()
    a.coarse = a.fine = None
    assert lib.ns_render_rays_hierarchical(C.byref(a), None) == -1      # (no network: the first check)
    # the argument checks that need a network handle run on the GPU tests; here the Python layer's refusal
    from nerf_sampling_amd import ops

    with pytest.raises(ValueError):
        ops.render_rays_hierarchical(None, None, rays=None, n_importance=0, max_sample=True)
    with pytest.raises(ValueError):
        ops.render_rays_hierarchical(None, None, rays=None, extras=("rgb",))
