"""The hierarchical renderer's max-weight fine sample (nerf_utils.py:813-819: top_indices = fine_weights.argmax(1), then z, weight
and sigmoid(raw rgb) at that index).  On bf16 / f16 / f16x3 fields the argmax runs in the compositing epilogue of the fine pass's
MLP kernel; on f32 fields, or sample counts the kernel does not composite, ns_argmax_gather runs on the fine arrays.  Either way
the bits are those of ops.argmax_gather on the same call's weights / z / raw, and render_rays_test's NeRF modes (-nm / -nc /
-nf) return through the one call exactly what the operator chain returns."""

import ctypes as C

import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = ((64, 128), (64, 64), (32, 32), (8, 8), (4, 4), (64, 448))
VARIANTS = ((0, 0), (4, 0), (5, 0), (0, 1))       # (prod_tiles, generic_kernels)
MAX_KEYS = ("max_z", "max_weights", "max_rgb")


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same_bits(a, b, tag):
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    assert torch.equal(bits(a), bits(b)), tag


def check_against_gather(out, tag):
    """max_* of the call == ops.argmax_gather on the call's own extras, bit for bit"""
    from nerf_sampling_amd import ops

    ref = ops.argmax_gather(out["weights"], out["z"], out["raw"])
    for k, r in zip(MAX_KEYS, ref):
        assert_same_bits(out[k], r, (tag, k))


def frame(H=23, W=47, theta=-70.0):
    _, K = O.blender_intrinsics(H, W)
    return (H, W, K, O.pose_spherical(theta, -30.0, 4.0)[:3, :4], 0, H)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f16x3", "f32"])
def test_max_sample_matches_argmax_gather(gpu_modules, dtype):
    """Every (Nc, Nf) the epilogue serves (a fine ray of one chunk, or of 2 .. 8 chunks that straddle groups), a ragged frame, every
    kernel variant: max_* equal argmax_gather of the same call's extras; the lean call (no extras), the hier_chain route and the
    call without max_sample agree with it."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    nc, nf = m["coarse"].packed(dtype), m["fine"].packed(dtype)
    variants = VARIANTS if dtype != "f32" else ((0, 0),)
    for n_c, n_i in SHAPES:
        kw = dict(camera=frame(), n_coarse=n_c, n_importance=n_i, lindisp=True, white_bkgd=True)
        chain = {}
        for g in sorted({g for _, g in variants}):
            with ops.debug_switch(hier_chain=1, generic_kernels=g):
                chain[g] = ops.render_rays_hierarchical(nc, nf, extras=True, max_sample=True, **kw)
                torch.cuda.synchronize()
            check_against_gather(chain[g], (dtype, n_c, n_i, "hier_chain", g))
        for t, g in variants:
            tag = (dtype, n_c, n_i, t, g)
            with ops.debug_switch(prod_tiles=t, generic_kernels=g):
                out = ops.render_rays_hierarchical(nc, nf, extras=True, max_sample=True, **kw)
                lean = ops.render_rays_hierarchical(nc, nf, max_sample=True, **kw)
                plain = ops.render_rays_hierarchical(nc, nf, extras=True, **kw)
                torch.cuda.synchronize()
            assert set(lean) == {"rgb", "disp", *MAX_KEYS} and out["max_rgb"].shape == (23 * 47, 3)
            check_against_gather(out, tag)
            for k in MAX_KEYS:
                assert_same_bits(lean[k], out[k], (tag, "lean", k))
                assert_same_bits(chain[g][k], out[k], (tag, "hier_chain", k))
            for k in ("rgb", "disp", "z", "weights", "raw"):
                assert_same_bits(out[k], plain[k], (tag, "without max_sample", k))
            for k in ("rgb", "disp"):
                assert_same_bits(lean[k], plain[k], (tag, "lean", k))


def test_max_sample_chain_route(gpu_modules):
    """Fine passes the MLP kernel does not composite -- 64 + 32 samples on a bf16 field, any count on an f32 field -- take
    ns_argmax_gather after the chain; with weights given, with only some extras, and with none (weights then in the workspace)."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    for dtype, (n_c, n_i) in (("bf16", (64, 32)), ("f32", (64, 32)), ("f32", (64, 128))):
        nc, nf = m["coarse"].packed(dtype), m["fine"].packed(dtype)
        kw = dict(camera=frame(theta=33.0), n_coarse=n_c, n_importance=n_i, lindisp=False, white_bkgd=True, max_sample=True)
        out = ops.render_rays_hierarchical(nc, nf, extras=True, **kw)
        check_against_gather(out, (dtype, n_c, n_i))
        for extras in (False, ("z", "weights"), ("z",)):
            other = ops.render_rays_hierarchical(nc, nf, extras=extras, **kw)
            assert set(other) == {"rgb", "disp", *MAX_KEYS, *(extras or ())}
            for k in other:
                assert_same_bits(other[k], out[k], (dtype, n_c, n_i, extras, k))


def edge_rays(R, device="cuda"):
    """R explicit rays: camera rays with d = 0 rays (every weight 0: index 0 wins) and NaN-origin rays (NaN weights: the first
    NaN wins) mixed in"""
    H, W, K, c2w, _, _ = frame(17, 19, theta=12.0)
    from nerf_sampling_amd import ops

    o, d, v = ops.get_rays(H, W, K, c2w)
    idx = torch.arange(R, device=device) % o.shape[0]
    o, d, v = o[idx].clone(), d[idx].clone(), v[idx].clone()
    d[3::7] = 0.0
    o[5::11] = float("nan")
    return o.contiguous(), d.contiguous(), v.contiguous()


@pytest.mark.parametrize("dtype", ["bf16", "f16x3", "f32"])
def test_max_sample_edge_rays(gpu_modules, dtype):
    """d = 0 and NaN rays, and ray counts that leave a multi-chunk ray open across a group boundary (192 and 384 samples; the
    16-bit kernel's groups hold 256 or 320 samples, the f16x3 kernel's 128), or end in a partial group."""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    nc, nf = m["coarse"].packed(dtype), m["fine"].packed(dtype)
    for R in (1, 5, 67, 333):
        rays = edge_rays(R)
        for n_c, n_i in ((64, 128), (64, 320), (32, 32)):
            for t in ((0, 4, 5) if dtype == "bf16" else (0,)):
                with ops.debug_switch(prod_tiles=t):
                    out = ops.render_rays_hierarchical(nc, nf, rays=rays, n_coarse=n_c, n_importance=n_i, extras=True,
                                                       max_sample=True)
                    torch.cuda.synchronize()
                tag = (dtype, R, n_c, n_i, t)
                check_against_gather(out, tag)
                w = out["weights"]
                zero = torch.arange(R, device="cuda") % 7 == 3
                zero &= ~torch.isnan(w).any(-1)
                if zero.any():          # d = 0: no ray length, every weight 0 -> index 0
                    assert (w[zero] == 0).all(), tag
                    assert_same_bits(out["max_z"][zero, 0], out["z"][zero, 0], tag)
                nan = torch.isnan(w).any(-1)
                if R > 5:
                    assert nan[5], tag  # a NaN origin -> NaN weights -> the first NaN
                first_nan = torch.isnan(w).int().argmax(-1)
                assert torch.isnan(out["max_weights"][nan, 0]).all(), tag
                assert_same_bits(out["max_z"][nan, 0], out["z"][nan].gather(1, first_nan[nan, None])[:, 0], tag)


def test_max_sample_refusals(gpu_modules):
    """No fine pass, or only some of the three outputs: refused before anything is written."""
    from nerf_sampling_amd import _lib, ops

    m = gpu_modules("lego_synth")
    nc = m["coarse"].packed("bf16")
    shard = torch.full((23 * 47, 4), 7.0, device="cuda")
    with pytest.raises(ValueError):
        ops.render_rays_hierarchical(nc, nc, camera=frame(), n_coarse=64, n_importance=0, max_sample=True, shard=shard)
    torch.cuda.synchronize()
    assert (shard == 7.0).all()
    lib = _lib.load()
    R = 64
    o, d, v = edge_rays(R)
    outs = {k: torch.full((R, 4), 7.0, device="cuda") for k in ("rgb", "disp", "max_z", "max_w", "max_rgb")}
    ws = torch.empty(int(lib.ns_hier_max_workspace_bytes(R, 64, 128)) + 256, dtype=torch.uint8, device="cuda")
    for n_i, which in ((0, ("max_z", "max_w", "max_rgb")), (128, ("max_z",)), (128, ("max_w", "max_rgb"))):
        a = _lib.HierArgs()
        a.coarse, a.fine = nc.handle, nc.handle
        a.o_dev, a.d_dev, a.viewdirs_dev, a.R = o.data_ptr(), d.data_ptr(), v.data_ptr(), R
        a.Nc, a.Nf, a.lindisp, a.white_bkgd, a.near_, a.far_ = 64, n_i, 1, 1, 2.0, 6.0
        a.workspace_dev = (ws.data_ptr() + 255) & ~255
        a.rgb_dev, a.disp_dev = outs["rgb"].data_ptr(), outs["disp"].data_ptr()
        for k in which:
            setattr(a, k + "_dev", outs[k].data_ptr())
        assert lib.ns_render_rays_hierarchical(C.byref(a), None) == -1, (n_i, which)
        assert b"max" in lib.ns_last_error()
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert (t == 7.0).all(), k


# ---- render_rays_test's NeRF modes (-nm / -nc / -nf) through the one call ---------------------------------------------------

def make_trainer(**over):
    from nerf_sampling_amd.trainers import DepthNetTrainer

    kw = dict(dataset_type="blender", basedir="/tmp", expname="max", no_batching=True, datadir="/nonexistent", half_res=True,
              white_bkgd=True, N_importance=128, N_samples=64, use_viewdirs=True, input_dims_embed=3, device="cuda",
              n_depth_samples=32, sampling_mode="uniform", distance=0.1)
    kw.update(over)
    return DepthNetTrainer(**kw)


def render_kwargs(trainer, m, tagged, perturb):
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.run_nerf_helpers import get_embedder

    embed_fn, _ = get_embedder(trainer.multires, trainer.i_embed, 3)
    embeddirs_fn, _ = get_embedder(trainer.multires_views, trainer.i_embed, 3)
    query = lambda inputs, viewdirs, network_fn: trainer.run_network(  # noqa: E731
        inputs, viewdirs, network_fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, netchunk=trainer.netchunk)
    if tagged:
        query = nerf_utils.standard_query_fn(query)
    return dict(network_query_fn=query, perturb=perturb, N_importance=trainer.N_importance, network_fine=m["fine"],
                N_samples=trainer.N_samples, network_fn=m["coarse"], use_viewdirs=True, white_bkgd=trainer.white_bkgd,
                raw_noise_std=0.0, trainer=trainer, lindisp=trainer.lindisp, depth_network=m["depth"], model_mode="test",
                near=2.0, far=6.0, ndc=False)


def assert_same_frame(a, b, tag):
    assert_same_bits(a[0], b[0], (tag, "rgb"))
    assert a[0].is_cuda == b[0].is_cuda and a[1].is_cuda == b[1].is_cuda
    assert_same_bits(a[1].cpu(), b[1].cpu(), (tag, "disp"))
    assert set(a[2]) == set(b[2]), (tag, set(a[2]) ^ set(b[2]))
    for k in a[2]:
        x, y = a[2][k], b[2][k]
        assert x.shape == y.shape and x.dtype == y.dtype and x.is_cuda == y.is_cuda, (tag, k)
        assert_same_bits(x.cpu(), y.cpu(), (tag, k))


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
@pytest.mark.parametrize("flag", ["use_nerf_max_pts", "compare_nerf", "use_full_nerf"])
def test_render_test_nerf_modes_one_call(gpu_modules, scene, flag):
    """render_test with -nm / -nc / -nf: the one-call route (the standard query function) returns the keys, shapes, devices and
    bits of the operator chain (an untagged query function), deterministic and with perturb = 1 under the same seed; the
    one-call route really ran, once per chunk."""
    from nerf_sampling_amd import nerf_utils, ops

    m = gpu_modules(scene)
    tr = make_trainer(**{flag: True})
    H, W, K, c2w, _, _ = frame(13, 17, theta=41.0)           # 221 rays in chunks of 100: 3 calls
    for perturb in (0.0, 1.0):
        torch.manual_seed(1234)
        chain = nerf_utils.render_test(H, W, K, chunk=100, c2w=c2w, **render_kwargs(tr, m, False, perturb))
        calls = []
        orig = ops.render_rays_hierarchical
        ops.render_rays_hierarchical = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            torch.manual_seed(1234)
            one = nerf_utils.render_test(H, W, K, chunk=100, c2w=c2w, **render_kwargs(tr, m, True, perturb))
        finally:
            ops.render_rays_hierarchical = orig
        assert len(calls) == 3, (flag, perturb)
        assert_same_frame(chain, one, (scene, flag, perturb))
    if flag != "use_full_nerf":     # (the full pass returns the fine z; the max-weight modes return the argmax only)
        assert one[2]["max_z_vals"].shape == (H, W, 1) and one[2]["max_pts"].shape == (H, W, 1, 3)


def test_render_test_nerf_max_one_call_bf16(gpu_modules):
    """-nm on a bf16 field: the argmax runs in the fine pass's MLP epilogue, and still equals the operator chain bit for bit."""
    from nerf_sampling_amd import nerf_utils, ops

    ops.set_compute_dtype("bf16")
    m = gpu_modules("lego_synth")
    tr = make_trainer(use_nerf_max_pts=True)
    H, W, K, c2w, _, _ = frame(13, 17, theta=-41.0)
    chain = nerf_utils.render_test(H, W, K, chunk=1024, c2w=c2w, **render_kwargs(tr, m, False, 0.0))
    one = nerf_utils.render_test(H, W, K, chunk=1024, c2w=c2w, **render_kwargs(tr, m, True, 0.0))
    assert_same_frame(chain, one, "bf16")


def test_render_rays_test_without_bounds_keeps_the_chain(gpu_modules):
    """A direct render_rays_test call does not know the batch's scalar bounds: it keeps the operator chain."""
    from nerf_sampling_amd import nerf_utils, ops

    m = gpu_modules("tiny_synth")
    tr = make_trainer(use_nerf_max_pts=True)
    H, W, K, c2w, _, _ = frame(5, 7)
    batch = ops.get_rays(H, W, K, c2w, near=2.0, far=6.0, want_batch=True)[3]
    kw = render_kwargs(tr, m, True, 0.0)
    for k in ("near", "far", "ndc"):
        kw.pop(k)
    calls = []
    orig = ops.render_rays_hierarchical
    ops.render_rays_hierarchical = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        res = nerf_utils.render_rays_test(batch, **kw)
    finally:
        ops.render_rays_hierarchical = orig
    assert not calls and res["max_z_vals"].shape == (H * W, 1)
