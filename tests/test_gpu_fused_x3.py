"""The one-kernel renderer and the hierarchical renderer's in-epilogue compositing on split-fp16 (f16x3) fields
(nerf_mlp_x3_comp_kernel, ns_nerf_mlp_x3.hip + ns_comp_epilogue.h): bit-identical to the operator chain / to the raw arrays
composited by the stand-alone kernel, and the one-kernel renderer's memory footprint does not grow with n_samples."""

import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

SPLIT_N = (2, 4, 8, 16, 32, 64, 128, 192)
LONG_N = (256, 320, 384, 448, 512)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _chain(ops, dn, nf, o, d, view, n):
    """depthnet_forward -> place_samples -> nerf_forward_rays -> raw2outputs"""
    mean = ops.depthnet_forward(dn, o, d)
    pts, z = ops.place_samples(o, d, mean, n, "uniform", 0.1)
    raw = ops.nerf_forward_rays(nf, o, d, z, view)
    rgb, disp, _acc, _depth, _alphas, weights = ops.raw2outputs(raw, z, d, None, True)
    return dict(rgb=rgb, disp=disp, z=z, pts=pts, weights=weights)


def _assert_same(out, ref, keys, tag):
    for k in keys:
        assert torch.equal(_bits(out[k]), _bits(ref[k])), (tag, k, float((out[k] - ref[k]).abs().nan_to_num().max()))


@pytest.mark.parametrize("dn_dtype", ["f16x3", "f16"])
@pytest.mark.parametrize("scene,rows", [("lego_synth", 23), ("tiny_synth", 5)])
def test_one_kernel_f16x3_matches_operator_chain(gpu_modules, dn_dtype, scene, rows):
    """Ragged ray counts (1081 / 235 rays), every sample count the kernel serves: N <= 64 (whole rays per 64-sample chunk; with
    two tiles per wave a chunk straddles two waves) and N = 64 m (a ray spans chunks on different waves and groups), on the
    production kernel and the generic one; with and without per-sample outputs."""
    from nerf_sampling_amd import ops

    m = gpu_modules(scene)
    H, W = rows, 47
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(40.0, -30.0, 4.0)[:3, :4]
    dn, nf = m["depth"].packed(dn_dtype), m["fine"].packed("f16x3")
    o, d, view = ops.get_rays(H, W, K, c2w)[:3]
    kw = dict(camera=(H, W, K, c2w, 0, H), mode="uniform", std=0.1)
    for n in SPLIT_N + (LONG_N if scene == "tiny_synth" else ()):
        for g in (0, 1):
            with ops.debug_switch(generic_kernels=g):
                ref = _chain(ops, dn, nf, o, d, view, n)
                out = ops.render_rays_depthnet(dn, nf, n_samples=n, extras=True, one_kernel=True, **kw)
                lean = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=True, **kw)
                default = ops.render_rays_depthnet(dn, nf, n_samples=n, **kw)       # one_kernel=None picks it too
                torch.cuda.synchronize()
            tag = (n, g)
            _assert_same(out, ref, ("rgb", "disp", "z", "pts", "weights"), tag)
            _assert_same(lean, ref, ("rgb", "disp"), tag)
            _assert_same(default, ref, ("rgb", "disp"), tag)


def test_one_kernel_f16x3_support_rule(gpu_modules):
    """ns_render_fused_supported: 1 for an f16x3 field at every supported N; 0 for N = 96, an fp32 field and gaussian placement.
    N = 96 with one_kernel=True still raises."""
    from nerf_sampling_amd import _lib, ops

    lib = _lib.load()
    m = gpu_modules("tiny_synth")
    nf, n32, dn = m["fine"].packed("f16x3"), m["fine"].packed("f32"), m["depth"].packed("f16x3")
    uni, gau = ops._MODES["uniform"], ops._MODES["gaussian"]
    for n in SPLIT_N + LONG_N:
        assert lib.ns_render_fused_supported(nf.handle, uni, n) == 1, n
        assert lib.ns_render_fused_supported(n32.handle, uni, n) == 0, n
        assert lib.ns_render_fused_supported(nf.handle, gau, n) == 0, n
    for n in (96, 1, 3, 576, 1024):
        assert lib.ns_render_fused_supported(nf.handle, uni, n) == 0, n
    _, K = O.blender_intrinsics(8, 8)
    c2w = O.pose_spherical(0.0, -30.0, 4.0)[:3, :4]
    with pytest.raises(NotImplementedError):
        ops.render_rays_depthnet(dn, nf, camera=(8, 8, K, c2w, 0, 8), n_samples=96, mode="uniform", std=0.1, one_kernel=True)
    a = ops.render_rays_depthnet(dn, nf, camera=(8, 8, K, c2w, 0, 8), n_samples=96, mode="uniform", std=0.1)   # the chain serves it
    b = ops.render_rays_depthnet(dn, nf, camera=(8, 8, K, c2w, 0, 8), n_samples=96, mode="uniform", std=0.1, one_kernel=False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a["rgb"]), _bits(b["rgb"]))


def test_one_kernel_f16x3_w128_network(gpu_modules):
    """A W = 128 field (the generic kernel at four K-blocks), seeded random weights."""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.run_nerf_helpers import NeRF

    torch.manual_seed(7)
    net = NeRF(D=8, W=128, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True).cuda()
    m = gpu_modules("tiny_synth")
    dn, nf = m["depth"].packed("f16x3"), net.packed("f16x3")
    H, W = 11, 29
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(-20.0, -30.0, 4.0)[:3, :4]
    o, d, view = ops.get_rays(H, W, K, c2w)[:3]
    for n in (2, 16, 64, 128, 192, 512):
        ref = _chain(ops, dn, nf, o, d, view, n)
        out = ops.render_rays_depthnet(dn, nf, camera=(H, W, K, c2w, 0, H), n_samples=n, mode="uniform", std=0.1, extras=True,
                                       one_kernel=True)
        torch.cuda.synchronize()
        _assert_same(out, ref, ("rgb", "disp", "z", "pts", "weights"), n)


def test_one_kernel_f16x3_explicit_rays_shard_and_misses(gpu_modules):
    """Explicit rays into an interleaved [R, 4] shard; rays that miss the DepthNet's sphere render NaN -- exactly those rays,
    bit for bit as the chain does."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    H, W = 13, 47
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(-63.0, -30.0, 4.0)[:3, :4]
    dn, nf = m["depth"].packed("f16x3"), m["fine"].packed("f16x3")
    o, d, view = ops.get_rays(H, W, K, c2w)[:3]
    for n in (64, 128):
        ref = _chain(ops, dn, nf, o, d, view, n)
        shard = torch.full((o.shape[0] + 5, 4), -7.0, dtype=torch.float32, device="cuda")
        out = ops.render_rays_depthnet(dn, nf, rays=(o, d, view), n_samples=n, mode="uniform", std=0.1, shard=shard, one_kernel=True)
        torch.cuda.synchronize()
        assert out["rgb"].data_ptr() == shard.data_ptr()
        assert torch.equal(_bits(shard[:o.shape[0], :3]), _bits(ref["rgb"])) and torch.equal(_bits(shard[:o.shape[0], 3]), _bits(ref["disp"]))
        assert bool((shard[o.shape[0]:] == -7.0).all())
    o2, d2 = o.clone(), d.clone()
    miss = torch.arange(0, o.shape[0], 7, device="cuda")
    d2[miss] = torch.tensor([0.0, 0.0, 1.0], device="cuda")          # pointing away from the scene
    for n in (64, 16, 192):
        a = ops.render_rays_depthnet(dn, nf, rays=(o2, d2, view), n_samples=n, mode="uniform", std=0.1, extras=True, one_kernel=True)
        b = ops.render_rays_depthnet(dn, nf, rays=(o2, d2, view), n_samples=n, mode="uniform", std=0.1, extras=True, one_kernel=False)
        torch.cuda.synchronize()
        if n <= 64:
            _assert_same(a, b, ("rgb", "disp", "z", "weights", "pts"), n)
        else:   # several chunks: a missed ray's composited NaN may come out with the other sign bit than the chain's; the rest,
            # and the placed depths and points, to the bit
            _assert_same(a, b, ("z", "pts"), n)
            for k in ("rgb", "disp", "weights"):
                nan_a, nan_b = torch.isnan(a[k]), torch.isnan(b[k])
                assert torch.equal(nan_a, nan_b) and torch.equal(_bits(a[k])[~nan_a], _bits(b[k])[~nan_b]), (n, k)
        expect = torch.isnan(ref["rgb"]).any(-1)         # (rays of the unmodified batch that miss already)
        expect[miss] = True
        assert torch.equal(torch.isnan(a["rgb"]).any(-1), expect), n


def test_one_kernel_f16x3_with_guard_equals_chain(gpu_modules):
    """An f16x3 field with a guard handle takes the every-ray guard (sigma of every ray's last sample from the guard pass, applied
    in the compositing pass) whatever the threshold says: the chain's bits."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    H, W = 17, 47
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(-25.0, -30.0, 4.0)[:3, :4]
    dn, nf = m["depth"].packed("f16x3"), m["fine"].packed("f16x3")
    for gw in (m["fine"].packed("f16x3"), m["fine"].packed("f32")):
        for n in (64, 8, 192):
            kw = dict(camera=(H, W, K, c2w, 0, H), n_samples=n, mode="uniform", std=0.1, extras=True, guard=gw)
            ref = ops.render_rays_depthnet(dn, nf, one_kernel=False, **kw)
            for thr in (0.0, None, 2.0):
                out = ops.render_rays_depthnet(dn, nf, one_kernel=True, guard_threshold=thr, **kw)
                torch.cuda.synchronize()
                _assert_same(out, ref, ("rgb", "disp", "z", "weights", "pts"), (getattr(gw, "dtype", "?"), n, thr))


@pytest.mark.parametrize("n_c,n_i", [(64, 128), (64, 192), (4, 4), (8, 8)])
def test_hierarchical_f16x3_in_kernel_compositing_matches_chain(gpu_modules, n_c, n_i):
    """ns_render_rays_hierarchical on f16x3 fields composites both passes in the MLP kernel's epilogue: the same bits as the
    raw arrays composited by the stand-alone kernel (debug switch hier_chain), raw itself included."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    H, W = 23, 47
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(-70.0, -30.0, 4.0)[:3, :4]
    nc, nf = m["coarse"].packed("f16x3"), m["fine"].packed("f16x3")
    kw = dict(camera=(H, W, K, c2w, 0, H), n_coarse=n_c, n_importance=n_i, lindisp=True, white_bkgd=True)
    for g in (0, 1):
        with ops.debug_switch(hier_chain=1, generic_kernels=g):
            ref = ops.render_rays_hierarchical(nc, nf, extras=True, **kw)
            torch.cuda.synchronize()
        with ops.debug_switch(generic_kernels=g):
            out = ops.render_rays_hierarchical(nc, nf, extras=True, **kw)
            lean = ops.render_rays_hierarchical(nc, nf, **kw)
            torch.cuda.synchronize()
        _assert_same(out, ref, ("rgb", "disp", "weights", "z", "raw"), (n_c, n_i, g))
        _assert_same(lean, ref, ("rgb", "disp"), (n_c, n_i, g))


def test_one_kernel_f16x3_footprint_does_not_grow_with_n(gpu_modules):
    """N = 512: the peak device memory of a one-kernel f16x3 render is its workspace (which does not depend on N) plus the
    outputs -- far below R N 16 B, the raw array alone of the chain."""
    from nerf_sampling_amd import _lib, ops

    lib = _lib.load()
    m = gpu_modules("tiny_synth")
    dn, nf = m["depth"].packed("f16x3"), m["fine"].packed("f16x3")
    H = W = 64
    R, N = H * W, 512
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(15.0, -30.0, 4.0)[:3, :4]
    kw = dict(camera=(H, W, K, c2w, 0, H), n_samples=N, mode="uniform", std=0.1)
    ops.render_rays_depthnet(dn, nf, one_kernel=True, workspace=ops.RenderWorkspace(), **kw)   # module / allocator warm-up

    def peak_of(one_kernel):
        """device memory the call allocates, its own fresh workspace included"""
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = ops.render_rays_depthnet(dn, nf, one_kernel=one_kernel, workspace=ops.RenderWorkspace(), **kw)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    peak, out = peak_of(True)
    ws = int(lib.ns_render_fused_workspace_bytes(R))
    outputs = R * 3 * 4 + R * 4
    assert ws <= peak <= ws + outputs + (1 << 20), (peak, ws, outputs)           # the workspace is what the call allocates
    assert peak < R * N * 16 // 8 and peak < int(lib.ns_render_workspace_bytes(R, N)) // 8, (peak, R * N * 16)
    assert out["rgb"].shape == (R, 3)
    # the same measurement sees the chain's z / raw arrays
    peak_chain, _ = peak_of(False)
    assert peak_chain >= int(lib.ns_render_workspace_bytes(R, N)) > R * N * 16, (peak_chain, R * N * 16)
