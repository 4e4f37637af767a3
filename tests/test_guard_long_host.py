"""The selective PSNR guard for rays of several chunks: the Python interface and the struct mirror (not gpu)."""

import ctypes
import inspect

import pytest

from nerf_sampling_amd import _lib, ops, parallel


def test_render_args_mirror_has_the_new_fields_in_the_guard_block():
    """Inside the guard block, in front of guard_threshold: tests/test_depth_acc_maps_host.py pins guard_threshold, depth_dev and
    acc_dev as the struct's last three fields."""
    names = [n for n, _ in _lib.RenderArgs._fields_]
    i = names.index("nerf_guard")
    assert names[i:i + 4] == ["nerf_guard", "guard_long_selective", "guard_count_dev", "guard_threshold"]
    assert names[i + 4:] == ["depth_dev", "acc_dev"]                       # what followed the guard block still does
    types = dict(_lib.RenderArgs._fields_)
    assert types["guard_long_selective"] is ctypes.c_int and types["guard_count_dev"] is ctypes.c_void_p
    a = _lib.RenderArgs()
    assert a.guard_long_selective == 0 and a.guard_count_dev is None       # a zero-initialised struct: today's behaviour


def test_set_psnr_guard_long_rays_round_trip():
    assert ops.guard_long_rays() == "every"                                # the module default
    try:
        ops.set_psnr_guard(True, long_rays="selective")
        assert ops.guard_long_rays() == "selective" and ops.psnr_guard()
        ops.set_psnr_guard(True)                                           # None leaves it as it is
        assert ops.guard_long_rays() == "selective"
        ops.set_psnr_guard(False, threshold=2.0)
        assert ops.guard_long_rays() == "selective"
        with pytest.raises(ValueError):
            ops.set_psnr_guard(True, long_rays="some")
        assert ops.guard_long_rays() == "selective" and not ops.psnr_guard()   # a refused call changes nothing
        ops.set_psnr_guard(False, long_rays="every")
        assert ops.guard_long_rays() == "every"
    finally:
        ops.set_psnr_guard(False, threshold=16.0, long_rays="every")


def test_render_rays_depthnet_arguments():
    sig = inspect.signature(ops.render_rays_depthnet)
    assert sig.parameters["guard_long_rays"].default == "every"
    assert sig.parameters["guard_long_rays"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(ops.set_psnr_guard).parameters["long_rays"].default is None
    assert inspect.signature(parallel.hip_row_renderer).parameters["guard_long_rays"].default is None


class _Handle:
    handle = None
    dtype = "bf16"


@pytest.mark.parametrize("bad", ["all", "", None, 1, "Selective"])
def test_a_bad_guard_long_rays_raises_before_any_launch(bad):
    """The value is checked before the library is loaded, a workspace is taken or anything is launched: no GPU is needed to see
    the ValueError, and the ray tensors are never looked at."""
    with pytest.raises(ValueError, match="guard_long_rays"):
        ops.render_rays_depthnet(_Handle(), _Handle(), rays=None, camera=None, n_samples=192, mode="uniform", std=0.1,
                                 guard_long_rays=bad)
    if bad is not None:                                                    # (None: the module setting, for the row renderer)
        with pytest.raises(ValueError, match="guard_long_rays"):
            parallel.hip_row_renderer(_Handle(), _Handle(), 4, 4, None, 192, "uniform", 0.1, guard_long_rays=bad)


def test_guard_count_is_an_extra_of_render_rays_depthnet_only():
    assert ops._extras_names(("guard_count", "depth"), ("z", "weights", "pts"), ("guard_count",)) == ("guard_count", "depth")
    assert ops._extras_names(True, ("z", "weights", "pts"), ("guard_count",)) == ("z", "weights", "pts")   # only when asked for
    with pytest.raises(ValueError):
        ops._extras_names(("guard_count",), ())                            # the tangent / hierarchical renderers do not offer it
