"""Host side of the depth tangents on an f16 field (ns_nerf_mlp_ob16_tan.hip), no GPU needed: the opt-in of the Python entry
points, whose checks fire before the library is touched.  (The kernel's code objects: test_render_tangent_host.py.)"""

import inspect

import pytest

from nerf_sampling_amd import _lib, autograd, ops

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
