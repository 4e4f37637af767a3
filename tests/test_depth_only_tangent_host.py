"""Host side of the one-sample (depth_only) tangent render and of render_rays' ``fused_step`` option, no GPU needed: the Python
argument checks (which raise before the library is touched), the code objects of the new kernel instance (no scratch, no spill,
registers within a gfx950 SIMD, LDS within a CU), and that render_rays without the option builds the autograd path it always
built."""

import re

import pytest
import torch

from nerf_sampling_amd import _lib, autograd, nerf_utils, ops
from test_depth_acc_maps_host import _field
from test_render_tangent_host import CAM, _blocks, _dynamic_lds, _packed


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def test_depth_only_is_accepted_by_the_argument_checks(no_library):
    """mode="depth_only" passes every check whatever n_samples says (the first thing past them is the depth tensor's device, or
    the library); the default mode keeps refusing n_samples = 1 from both entry points."""
    dn = _packed("depthnet", "f16x3")
    for n in (1, 3, 16, 1000):
        with pytest.raises(RuntimeError, match="GPU"):            # a CPU depth tensor: every argument check lies before this
            ops.render_rays_depthnet_tangent(torch.full((64,), 3.0), _packed(), camera=CAM, n_samples=n, std=0.1, mode="depth_only")
        with pytest.raises(AssertionError, match="library was touched"):
            ops.render_rays_depthnet_tangent(dn, _packed(), camera=CAM, n_samples=n, std=0.1, mode="depth_only")
    with pytest.raises(NotImplementedError, match="n_samples"):
        ops.render_rays_depthnet_tangent(dn, _packed(), camera=CAM, n_samples=1, std=0.1)
    with pytest.raises(NotImplementedError, match="n_samples"):
        ops.render_rays_depthnet_tangent(dn, _packed(), camera=CAM, n_samples=1, std=0.1, mode="uniform")
    with pytest.raises(NotImplementedError, match="n_samples"):
        autograd.render_depthnet_differentiable(None, _packed(), camera=CAM, n_samples=1, std=0.1)
    with pytest.raises(ValueError, match="exactly one"):
        ops.render_rays_depthnet_tangent(dn, _packed(), n_samples=1, std=0.1, mode="depth_only")
    with pytest.raises(ValueError, match="exactly one"):
        autograd.render_depthnet_differentiable(None, _packed(), n_samples=1, std=0.1, mode="depth_only")


def test_unknown_mode_raises(no_library):
    dn = _packed("depthnet", "f16x3")
    for mode in ("gaussian", "depth-only", "", None):
        with pytest.raises(ValueError, match="mode"):
            ops.render_rays_depthnet_tangent(dn, _packed(), camera=CAM, n_samples=16, std=0.1, mode=mode)
        with pytest.raises(ValueError, match="mode"):
            autograd.render_depthnet_differentiable(None, _packed(), camera=CAM, n_samples=16, std=0.1, mode=mode)


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("approximate", [False, True])
def test_depth_only_needs_an_f16x3_field(no_library, dtype, approximate):
    dn = _packed("depthnet", "f16x3")
    with pytest.raises(NotImplementedError, match="f16x3"):
        ops.render_rays_depthnet_tangent(dn, _packed(dtype=dtype), camera=CAM, n_samples=1, std=0.1, mode="depth_only",
                                         approximate=approximate)
    with pytest.raises(NotImplementedError, match="f16x3"):
        autograd.render_depthnet_differentiable(None, _packed(dtype=dtype), camera=CAM, n_samples=1, std=0.1, mode="depth_only",
                                                approximate=approximate)
    with pytest.raises(NotImplementedError, match="f16x3"):
        autograd.render_single_sample(torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3),
                                      _packed(dtype=dtype))


def test_render_rays_without_the_option_builds_the_same_autograd_path(monkeypatch):
    """render_rays with fused_step absent or False: points_along_rays -> the query function -> the trainer's raw2outputs, with
    ``raw`` among the keys, and neither one-call renderer touched.  With the option on and an ineligible configuration (a
    query function that is not the standard one) the same."""
    calls = []
    monkeypatch.setattr(ops, "argmax_gather", lambda w, z, raw=None: (z[:, :1], w[:, :1], None))
    monkeypatch.setattr(ops, "points_along_rays", lambda o, d, z: o[:, None] + d[:, None] * z[..., None])
    monkeypatch.setattr(autograd, "points_along_rays", lambda o, d, z: (calls.append("points_ag"), o[:, None] + d[:, None] * z[..., None])[1])
    monkeypatch.setattr(nerf_utils, "sample_as_in_NeRF",
                        lambda ray_batch, **k: (None, torch.ones(ray_batch.shape[0], 4), None, None, torch.ones(ray_batch.shape[0], 4),
                                                None, None, None))

    def refuse(*a, **k):
        raise AssertionError("a fused_step renderer was called")
    monkeypatch.setattr(autograd, "render_single_sample", refuse)
    monkeypatch.setattr(nerf_utils, "_vanilla_one_call", refuse)

    class Tr:
        def raw2outputs(self, raw, z_vals, rays_d, **k):
            calls.append("raw2outputs")
            return (torch.sigmoid(raw[:, 0, :3]), torch.full((raw.shape[0],), 1e10), None, None, None, None, None)

    def query(pts, viewdirs, net):
        calls.append("query")
        return torch.cat([pts, pts[..., :1]], -1)

    w = torch.ones(1, requires_grad=True)
    depth_network = lambda o, d: (o[:, :1] * 0 + 3.0) * w      # noqa: E731
    rb = torch.rand(5, 11)
    expected = {"depth_net_rgb_map", "depth_net_disp_map", "depth_net_z_vals", "max_z_vals", "depth_net_pts", "max_pts", "raw"}
    for extra in ({}, {"fused_step": False}, {"fused_step": True}):
        calls.clear()
        ret = nerf_utils.render_rays(rb, None, query, 8, Tr(), depth_network=depth_network, _skip_host_copies=True, **extra)
        assert calls == ["points_ag", "query", "raw2outputs"], (extra, calls)
        assert set(ret) == expected, extra
        assert ret["depth_net_rgb_map"].requires_grad and ret["depth_net_z_vals"].requires_grad


def test_trainer_option_reaches_the_render_kwargs():
    import inspect

    from nerf_sampling_amd.trainers import DepthNetTrainer

    assert inspect.signature(DepthNetTrainer.__init__).parameters["fused_step"].default is False
    kw = dict(dataset_type="blender", basedir="/tmp", expname="x", no_batching=True, datadir="", half_res=True, white_bkgd=True)
    assert DepthNetTrainer(**kw).fused_step is False
    assert DepthNetTrainer(fused_step=True, **kw).fused_step is True


# the one-sample instances of the f16x3 tangent kernel (ns_nerf_mlp_x3_tan.hip), mangled template argument by width
ONE_KERNEL, ONE_INSTANCES = "nerf_mlp_x3_tan1_kernel", {256: "ILi8E", 128: "ILi4E"}


def test_one_sample_kernel_keeps_no_scratch_and_fits_the_cu():
    seen = set()
    for name, blk, ins in _blocks(ONE_KERNEL):
        key = [w for w, tag in ONE_INSTANCES.items() if tag in name]
        assert len(key) == 1, name
        seen.add(key[0])
        assert _field(blk, "private_segment_fixed_size") == 0, name
        assert _field(blk, "vgpr_spill_count") == 0, name
        assert _field(blk, "vgpr_count") <= 512, name
        assert ins, name
        assert not any(i.startswith("scratch_") for i in ins), name
        full_waits = sum(bool(re.search(r"s_waitcnt vmcnt\(0\)(?! *lgkmcnt)|s_waitcnt vmcnt\(0\)$", i)) for i in ins)
        assert full_waits <= 10, (name, full_waits)
        bias_floats = 8 * key[0] + (key[0] // 2 + 16) + 16
        assert _field(blk, "group_segment_fixed_size") + _dynamic_lds(bias_floats, 2048, 64) <= 160 * 1024, name
    assert seen == set(ONE_INSTANCES), sorted(seen)
