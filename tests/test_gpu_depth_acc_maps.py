"""The expected-depth and opacity maps of the one-call renderers (ns_render_args / ns_hier_args depth_dev, acc_dev; ops extras
"depth" / "acc"): depth = sum_i w_i z_i and acc = sum_i w_i of every ray, bit for bit what ns_raw2outputs writes for the call's
own raw, z and rays_d -- from the compositing epilogue of the MLP kernels (one chunk per ray and several), from the selective
guard's fix-up, and from the chain's stand-alone compositing -- and asking for them changes no other output."""

import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

SPLIT_N = (2, 4, 8, 16, 32, 64, 128, 192)
LONG_N = (256, 320, 384, 448, 512)
MAPS = ("depth", "acc")


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same(a, b, tag, nan_sign=False):
    """bit-identical; nan_sign: a NaN may carry the other sign bit (rays of several chunks, as the existing helpers allow for
    disp), but NaN positions and every other value match to the bit"""
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    if not nan_sign:
        assert torch.equal(bits(a), bits(b)), (tag, float((a - b).abs().nan_to_num().max()))
        return
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), tag
    assert torch.equal(bits(a)[~na], bits(b)[~nb]), (tag, float((a - b).abs().nan_to_num().max()))


def frame(H=23, W=47, theta=40.0):
    _, K = O.blender_intrinsics(H, W)
    return (H, W, K, O.pose_spherical(theta, -30.0, 4.0)[:3, :4], 0, H)


def maps_of(ops, raw, z, d):
    """depth / acc as ns_raw2outputs writes them"""
    _rgb, _disp, acc, depth, _al, _w = ops.raw2outputs(raw, z, d, None, True, want_per_sample=False)
    return {"depth": depth, "acc": acc}


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f16x3"])
@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
def test_one_kernel_maps_equal_the_chain(gpu_modules, dtype, scene):
    """Every sample count the one-kernel renderer serves: its depth / acc equal the chain's (one_kernel=False), and the chain's
    equal raw2outputs on the chain's own z; rgb / disp are those of a call that asks for no maps, and the per-sample outputs
    those of a call that asks for them without the maps."""
    from nerf_sampling_amd import ops

    m = gpu_modules(scene)
    dn, nf = m["depth"].packed("f16" if dtype != "f16x3" else "f16x3"), m["fine"].packed(dtype)
    cam = frame()
    o, d, view = ops.get_rays(*cam[:4])[:3]
    kw = dict(camera=cam, mode="uniform", std=0.1)
    for n in SPLIT_N + (LONG_N if scene == "tiny_synth" else ()):
        tag = (dtype, scene, n)
        chain = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=False, extras=("z",) + MAPS, **kw)
        one = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=True, extras=MAPS, **kw)
        full = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=True, extras=("z", "weights", "pts") + MAPS, **kw)
        plain = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=True, extras=True, **kw)
        lean = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=True, **kw)
        raw = ops.nerf_forward_rays(nf, o, d, chain["z"], view)
        ref = maps_of(ops, raw, chain["z"], d)
        torch.cuda.synchronize()
        assert set(one) == {"rgb", "disp", *MAPS} and set(full) == {"rgb", "disp", "z", "weights", "pts", *MAPS}
        for k in MAPS:
            assert one[k].shape == (o.shape[0],)
            assert_same(chain[k], ref[k], (tag, "chain", k))
            assert_same(one[k], chain[k], (tag, "one", k), nan_sign=n > 64)
            assert_same(full[k], one[k], (tag, "full", k))
        for k in ("rgb", "disp"):
            assert_same(one[k], lean[k], (tag, "lean", k))
            assert_same(full[k], lean[k], (tag, "full", k))
        for k in ("z", "weights", "pts"):
            assert_same(full[k], plain[k], (tag, "per-sample", k))
        assert bool((one["acc"][~torch.isnan(one["acc"])] <= 1.0 + 1e-4).all())


def test_maps_of_missed_rays_shard_and_generic_kernels(gpu_modules):
    """Explicit rays, some pointing away from the sphere (NaN depth and acc, exactly there), written beside an interleaved
    [R, 4] shard; the generic kernels and both tile counts of the production kernel give the same maps."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    cam = frame(13, 47, -63.0)
    dn, nf = m["depth"].packed("f16"), m["fine"].packed("bf16")
    o, d, view = ops.get_rays(*cam[:4])[:3]
    d = d.clone()
    miss = torch.arange(0, o.shape[0], 7, device="cuda")
    d[miss] = torch.tensor([0.0, 0.0, 1.0], device="cuda")
    kw = dict(rays=(o, d, view), mode="uniform", std=0.1)
    for n in (64, 16, 192):
        chain = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=False, extras=MAPS, **kw)
        for t, g in ((0, 0), (4, 0), (5, 0), (0, 1)):
            shard = torch.full((o.shape[0] + 3, 4), -7.0, dtype=torch.float32, device="cuda")
            with ops.debug_switch(prod_tiles=t, generic_kernels=g):
                one = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=True, extras=MAPS, shard=shard, **kw)
                lean = ops.render_rays_depthnet(dn, nf, n_samples=n, one_kernel=True, **kw)
                torch.cuda.synchronize()
            tag = (n, t, g)
            for k in MAPS:
                assert_same(one[k], chain[k], (tag, k), nan_sign=n > 64)
                assert torch.isnan(one[k])[miss].all(), (tag, k)
            assert_same(shard[:o.shape[0], :3], lean["rgb"], (tag, "shard rgb"))
            assert_same(shard[:o.shape[0], 3], lean["disp"], (tag, "shard disp"))
            assert bool((shard[o.shape[0]:] == -7.0).all())


def test_maps_under_the_psnr_guard(gpu_modules):
    """Every-ray guard (one kernel and chain) and the selective guard (thresholds 4, 16 and 1e6 -- the last flags every ray: the
    fix-up's capacity case): the maps are raw2outputs of the 16-bit raw with sigma of the last sample from the f16x3 handle,
    wherever the selective guard's rule says the bits agree; at 1e6 on every ray."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    cam = frame(37, 47, -25.0)
    dn, nf, gw = m["depth"].packed("f16x3"), m["fine"].packed("bf16"), m["fine"].packed("f16x3")
    o, d, view = ops.get_rays(*cam[:4])[:3]
    mean = ops.depthnet_forward(dn, o, d)
    for n in (64, 32, 8, 2, 192):
        _pts, z = ops.place_samples(o, d, mean, n, "uniform", 0.1)
        raw = ops.nerf_forward_rays(nf, o, d, z, view)
        raw_last = ops.nerf_forward_rays(gw, o, d, z[:, -1:].contiguous(), view)
        patched = raw.clone()
        patched[:, -1, 3] = raw_last[:, 0, 3]
        ref = maps_of(ops, patched, z, d)
        every = ops.render_rays_depthnet(dn, nf, camera=cam, n_samples=n, mode="uniform", std=0.1, extras=MAPS, one_kernel=True,
                                         guard=gw, guard_threshold=0.0)
        torch.cuda.synchronize()
        for k in MAPS:
            assert_same(every[k], ref[k], (n, "every", k), nan_sign=n > 64)
        for one, thr in ((False, 0.0), (True, 4.0), (True, 16.0), (True, 1e6)):
            kw = dict(camera=cam, n_samples=n, mode="uniform", std=0.1, one_kernel=one, guard=gw, guard_threshold=thr)
            out = ops.render_rays_depthnet(dn, nf, extras=MAPS, **kw)
            lean = ops.render_rays_depthnet(dn, nf, **kw)
            torch.cuda.synchronize()
            same = torch.ones(o.shape[0], dtype=torch.bool, device="cuda")
            if one and n <= 64 and thr < 1e6:
                s16, s32 = raw[:, -1, 3], raw_last[:, 0, 3]
                same = ((s16 > 0) == (s32 > 0)) | (s16.abs() < thr)
                assert float(same.float().mean()) > 0.98, (n, thr)
            tag = (n, one, thr)
            for k in MAPS:
                assert_same(out[k][same], every[k][same], (tag, k), nan_sign=n > 64)
            for k in ("rgb", "disp"):
                assert_same(out[k], lean[k], (tag, "lean", k))


def test_chain_only_modes(gpu_modules):
    """Placements the one-kernel renderer does not serve take the chain: depth_only (N = 1) gives zeros, as the reference's
    empty weights do; gaussian placement gives raw2outputs of its own z; an fp32 field likewise."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    cam = frame()
    dn, nf = m["depth"].packed("f16"), m["fine"].packed("bf16")
    o, d, view = ops.get_rays(*cam[:4])[:3]
    R = o.shape[0]
    out = ops.render_rays_depthnet(dn, nf, camera=cam, n_samples=8, mode="depth_only", std=0.1, extras=("z", "weights") + MAPS)
    lean = ops.render_rays_depthnet(dn, nf, camera=cam, n_samples=8, mode="depth_only", std=0.1)
    torch.cuda.synchronize()
    for k in MAPS:
        assert out[k].shape == (R,) and bool((bits(out[k]) == 0).all()), k
    assert_same(out["rgb"], lean["rgb"], "depth_only rgb")
    torch.manual_seed(3)
    noise = torch.randn(R, 15, device="cuda")
    out = ops.render_rays_depthnet(dn, nf, camera=cam, n_samples=16, mode="gaussian", std=0.1, noise=noise,
                                   extras=("z", "weights") + MAPS)
    lean = ops.render_rays_depthnet(dn, nf, camera=cam, n_samples=16, mode="gaussian", std=0.1, noise=noise)
    raw = ops.nerf_forward_rays(nf, o, d, out["z"], view)
    ref = maps_of(ops, raw, out["z"], d)
    torch.cuda.synchronize()
    for k in MAPS:
        assert_same(out[k], ref[k], ("gaussian", k))
    for k in ("rgb", "disp"):
        assert_same(out[k], lean[k], ("gaussian", k))
    d32, n32 = m["depth"].packed("f32"), m["fine"].packed("f32")
    out = ops.render_rays_depthnet(d32, n32, camera=cam, n_samples=32, mode="uniform", std=0.1, extras=("z",) + MAPS)
    ref = maps_of(ops, ops.nerf_forward_rays(n32, o, d, out["z"], view), out["z"], d)
    torch.cuda.synchronize()
    for k in MAPS:
        assert_same(out[k], ref[k], ("f32", k))


def test_empty_batch_and_refusals(gpu_modules):
    from nerf_sampling_amd import ops

    m = gpu_modules("tiny_synth")
    dn, nf = m["depth"].packed("f16"), m["fine"].packed("bf16")
    e = torch.empty((0, 3), device="cuda")
    out = ops.render_rays_depthnet(dn, nf, rays=(e, e, e), n_samples=16, mode="uniform", std=0.1, extras=("weights",) + MAPS)
    assert set(out) == {"rgb", "disp", "weights", *MAPS} and out["depth"].shape == (0,)
    for bad in (("depth", "raw"), ("alphas",)):
        with pytest.raises(ValueError):
            ops.render_rays_depthnet(dn, nf, camera=frame(), n_samples=16, mode="uniform", std=0.1, extras=bad)
    with pytest.raises(ValueError):
        ops.render_rays_hierarchical(nf, nf, camera=frame(), n_coarse=16, n_importance=16, extras=("pts",))


HIER_SHAPES = ((64, 128), (64, 64), (32, 32), (8, 8), (64, 448), (64, 32))


@pytest.mark.parametrize("dtype", ["bf16", "f16x3", "f32"])
def test_hierarchical_maps_equal_raw2outputs(gpu_modules, dtype):
    """The fine pass's maps: in the compositing epilogue (bf16 / f16x3 at the sample counts it serves), through the chain
    (hier_chain=1, fp32 fields, 64 + 32 samples), with and without the max-weight sample -- raw2outputs of the call's own z /
    raw, bit for bit; rgb / disp / max_* as a call that asks for no maps."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    nc, nf = m["coarse"].packed(dtype), m["fine"].packed(dtype)
    cam = frame(theta=-70.0)
    d = ops.get_rays(*cam[:4])[1]
    for n_c, n_i in HIER_SHAPES:
        kw = dict(camera=cam, n_coarse=n_c, n_importance=n_i, lindisp=True, white_bkgd=True)
        for chain in (0, 1):
            for mx in (False, True):
                tag = (dtype, n_c, n_i, chain, mx)
                with ops.debug_switch(hier_chain=chain):
                    out = ops.render_rays_hierarchical(nc, nf, extras=("z", "raw") + MAPS, max_sample=mx, **kw)
                    only = ops.render_rays_hierarchical(nc, nf, extras=MAPS, max_sample=mx, **kw)
                    lean = ops.render_rays_hierarchical(nc, nf, max_sample=mx, **kw)
                    torch.cuda.synchronize()
                ref = maps_of(ops, out["raw"], out["z"], d)
                for k in MAPS:
                    assert_same(out[k], ref[k], (tag, k))
                    assert_same(only[k], ref[k], (tag, "only", k))
                for k in lean:
                    assert_same(only[k], lean[k], (tag, "lean", k))
                    assert_same(out[k], lean[k], (tag, "extras", k))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_hierarchical_maps_without_a_fine_pass(gpu_modules, dtype):
    """n_importance == 0: the coarse pass is the result, and so are its maps -- raw2outputs of the coarse z / raw, rebuilt here
    from the operators (their rgb / disp equal the call's, which shows they are the call's own arrays)."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    nc = m["coarse"].packed(dtype)
    cam = frame(theta=15.0)
    o, d, view = ops.get_rays(*cam[:4])[:3]
    R = o.shape[0]
    for n_c in (64, 16):
        out = ops.render_rays_hierarchical(nc, None, camera=cam, n_coarse=n_c, n_importance=0, extras=MAPS)
        lean = ops.render_rays_hierarchical(nc, None, camera=cam, n_coarse=n_c, n_importance=0)
        near = torch.full((R,), 2.0, device="cuda")
        far = torch.full((R,), 6.0, device="cuda")
        z = ops.coarse_z(near, far, n_c, True)
        raw = ops.nerf_forward_rays(nc, o, d, z, view)
        rgb, disp, acc, depth, _al, _w = ops.raw2outputs(raw, z, d, None, True, want_per_sample=False)
        torch.cuda.synchronize()
        assert_same(lean["rgb"], rgb, (dtype, n_c, "rebuilt rgb"))
        assert_same(lean["disp"], disp, (dtype, n_c, "rebuilt disp"))
        assert_same(out["depth"], depth, (dtype, n_c, "depth"))
        assert_same(out["acc"], acc, (dtype, n_c, "acc"))
        assert_same(out["rgb"], lean["rgb"], (dtype, n_c, "rgb"))


@pytest.mark.parametrize("dtype", ["f32", "f16x3"])
def test_maps_against_the_oracle(gpu_modules, dtype):
    """The fp32-grade paths (exact-fp32 chain; f16x3 one-kernel renderer with an f16x3 DepthNet) against the CPU oracle's
    depth_map / acc_map: within 1e-4 (depth relative above 1) on every ray whose oracle maps do not move by more than that
    under a sigma shift of 1e-5 max|sigma| -- the last sample's alpha = step(sigma_last) rule."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    p = m["params"]
    H = W = 32
    cam = frame(H, W, 30.0)
    _, K, c2w = cam[0], cam[2], cam[3]
    dn, nf = m["depth"].packed(dtype), m["fine"].packed(dtype)
    out = ops.render_rays_depthnet(dn, nf, camera=cam, n_samples=32, mode="uniform", std=0.1, extras=MAPS,
                                   one_kernel=dtype != "f32")
    torch.cuda.synchronize()
    batch, o, d, _ = O.ray_batch_from_camera(H, W, K, torch.as_tensor(c2w, dtype=torch.float32), 2.0, 6.0)
    with torch.no_grad():
        mean = O.depthnet_forward(p["depth"], o, d)
        pts, z = O.place_samples(o, d, mean, 32, "uniform", 0.1)
        raw = O.run_network(p["fine"], pts, batch[:, -3:])
        base = O.raw2outputs(raw, z, d, 0.0, True)
        eps = 1e-5 * float(raw[..., 3].abs().max())
        ill = torch.zeros(raw.shape[0], dtype=torch.bool)
        for sgn in (-1.0, 1.0):
            pert = raw.clone()
            pert[..., 3] += sgn * eps
            got = O.raw2outputs(pert, z, d, 0.0, True)
            ill |= (got[2] - base[2]).abs() > 1e-4
            ill |= (got[3] - base[3]).abs() / base[3].abs().clamp(min=1.0) > 1e-4
    acc_ref, depth_ref = base[2], base[3]
    ok = ~ill & torch.isfinite(depth_ref) & torch.isfinite(acc_ref)
    assert float(ok.float().mean()) > 0.9, float(ok.float().mean())
    err_acc = (out["acc"].cpu() - acc_ref).abs()
    err_depth = (out["depth"].cpu() - depth_ref).abs() / depth_ref.abs().clamp(min=1.0)
    print(f"maps vs oracle [{dtype}]: ill-conditioned {float(ill.float().mean()):.4f}, max acc err {float(err_acc[ok].max()):.2e}, "
          f"max depth err {float(err_depth[ok].max()):.2e}")
    assert float(err_acc[ok].max()) <= 1e-4
    assert float(err_depth[ok].max()) <= 1e-4
    assert torch.equal(torch.isnan(out["depth"].cpu()), torch.isnan(depth_ref))
