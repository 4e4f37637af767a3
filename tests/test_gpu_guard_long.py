"""The selective PSNR guard for rays of several 64-sample chunks (ns_render_args::guard_long_selective, N = 128 .. 512): the
one-kernel renderer flags the finished rays whose own 16-bit sigma of the last sample lies within guard_threshold of zero, and the
fix-up repeats the last chunk's additions with the f16x3 sigma.  Expected results come from the operators, as in
tests/test_gpu_render.py::test_psnr_guard_replaces_sigma_of_the_last_sample.  Run with:  pytest -m gpu"""

import os
import subprocess
import sys

import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 47          # 1 739 rays: ragged against 256- and 320-sample groups and against the three-group runs of N = 192
POSE = (-25.0, -30.0, 4.0)
OUTS = ("rgb", "disp", "weights", "depth", "acc")
EXTRAS = ("z", "weights", "depth", "acc", "guard_count")


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def chain(gpu_modules):
    """(scene, dtype, n) -> what the operator chain gives on the camera's rays, computed once: the handles and rays, z, the
    16-bit sigma of every ray's last sample (s16) and the f16x3 one (s32), and the every-ray guard's outputs."""
    from nerf_sampling_amd import ops

    rays, cache = {}, {}

    def get(scene, dtype, n):
        m = gpu_modules(scene)
        if scene not in rays:
            _, K = O.blender_intrinsics(H, W)
            c2w = O.pose_spherical(*POSE)[:3, :4]
            dn, gw = m["depth"].packed("f16x3"), m["fine"].packed("f16x3")
            o, d, view = ops.get_rays(H, W, K, c2w)[:3]
            rays[scene] = dict(K=K, c2w=c2w, dn=dn, gw=gw, o=o, d=d, view=view, mean=ops.depthnet_forward(dn, o, d))
        if (scene, dtype, n) not in cache:
            r = rays[scene]
            nf = m["fine"].packed(dtype)
            _pts, z = ops.place_samples(r["o"], r["d"], r["mean"], n, "uniform", 0.1)
            raw = ops.nerf_forward_rays(nf, r["o"], r["d"], z, r["view"])
            raw_last = ops.nerf_forward_rays(r["gw"], r["o"], r["d"], z[:, -1:].contiguous(), r["view"])
            patched = raw.clone()
            patched[:, -1, 3] = raw_last[:, 0, 3]
            rgb, disp, acc, depth, _al, weights = ops.raw2outputs(patched, z, r["d"], None, True)
            cache[(scene, dtype, n)] = dict(r, nf=nf, z=z, s16=raw[:, -1, 3].clone(), s32=raw_last[:, 0, 3].clone(), rgb=rgb,
                                            disp=disp, weights=weights, depth=depth, acc=acc)
        return cache[(scene, dtype, n)]

    return get


def render(c, n, **kw):
    from nerf_sampling_amd import ops

    kw.setdefault("extras", EXTRAS)
    kw.setdefault("one_kernel", True)
    kw.setdefault("guard", c["gw"])
    if "rays" not in kw:
        kw["camera"] = (H, W, c["K"], c["c2w"], 0, H)
    return ops.render_rays_depthnet(c["dn"], c["nf"], n_samples=n, mode="uniform", std=0.1, **kw)


def assert_same_bits(a, b, keys, tag, rows=None):
    for k in keys:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert torch.equal(bits(x), bits(y)), (tag, k, float((x - y).abs().max()))


@pytest.mark.parametrize("n", [128, 192, 512])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("scene", ["lego_synth", "tiny_synth"])
def test_selective_long_guard_has_the_every_ray_guards_bits(chain, scene, dtype, n):
    """guard_long_rays="selective" at thresholds 16 and 2: rgb, disp, weights and the depth / acc maps carry the every-ray guard's
    bits on every ray of `same` -- the rays whose step does not flip between the 16-bit and the f16x3 sigma, or that are flagged
    -- and z on all rays; on the production network's four- and five-tile kernels (lego_synth) and the generic kernel
    (tiny_synth).  `same` covers >= 0.98 of the rays (the floor of the existing guard test at threshold 2); its shares on these
    scenes, measured from the operator chain, are printed below."""
    from nerf_sampling_amd import ops

    c = chain(scene, dtype, n)
    for thr in (16.0, 2.0):
        flagged = c["s16"].abs() < thr
        same = ((c["s16"] > 0) == (c["s32"] > 0)) | flagged
        share = float(same.float().mean())
        print(f"{scene} {dtype} N={n} thr={thr}: same {share:.5f}, flagged {float(flagged.float().mean()):.4f}")
        assert share >= 0.98, (scene, dtype, n, thr, share)
        for tiles in ((4, 5) if scene == "lego_synth" else (0,)):
            with ops.debug_switch(prod_tiles=tiles):
                out = render(c, n, guard_threshold=thr, guard_long_rays="selective")
            tag = (scene, dtype, n, thr, tiles)
            assert int(out["guard_count"]) == int(flagged.sum()), tag          # the selective path ran
            assert torch.equal(out["z"], c["z"]), tag
            assert_same_bits(out, c, OUTS, tag, rows=same)


def test_selective_long_guard_on_the_generic_kernel_of_the_production_network():
    """The same check with NS_OB16_GENERIC=1 (the production network on the generic compiled kernel), which is read once per
    process: a fresh child runs one case of the test above."""
    env = dict(os.environ, NS_OB16_GENERIC="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "every_ray_guards_bits and lego_synth and bf16 and 192"], cwd=ROOT, env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("n", [128, 192])
def test_the_selective_path_ran(chain, n):
    """extras "guard_count": the number of rays the kernel flagged equals the count from the operator chain's 16-bit raw -- a
    minority at threshold 2 -- and stays at its initial -1 when long rays take the every-ray form."""
    c = chain("lego_synth", "bf16", n)
    R = c["s16"].shape[0]
    for thr in (2.0, 16.0):
        want = int((c["s16"].abs() < thr).sum())
        out = render(c, n, guard_threshold=thr, guard_long_rays="selective", extras=("guard_count",))
        assert out["guard_count"].dtype == torch.int32 and out["guard_count"].shape == (1,) and out["guard_count"].is_cuda
        assert int(out["guard_count"]) == want, (n, thr)
        assert 0 < want and (thr != 2.0 or want < R // 2), (n, thr, want)
        every = render(c, n, guard_threshold=thr, guard_long_rays="every", extras=("guard_count",))
        assert int(every["guard_count"]) == -1, (n, thr)


def test_every_ray_flagged_and_no_ray_flagged(chain):
    """N = 192.  Threshold 1e6 flags every ray (the records' capacity): all outputs equal the every-ray guard's bit for bit on all
    rays, also through explicit rays into an interleaved [R, 4] shard.  Threshold 1e-30 flags none: the unguarded render."""
    n = 192
    c = chain("lego_synth", "bf16", n)
    R = c["s16"].shape[0]
    every = render(c, n, guard_threshold=0.0)
    assert_same_bits(every, c, OUTS, "every-ray guard vs the operators")
    out = render(c, n, guard_threshold=1e6, guard_long_rays="selective")
    assert int(out["guard_count"]) == R
    assert_same_bits(out, every, OUTS + ("z",), "thr 1e6")
    shard = torch.empty((R, 4), dtype=torch.float32, device="cuda")
    sel = render(c, n, rays=(c["o"], c["d"], c["view"]), guard_threshold=1e6, guard_long_rays="selective", shard=shard)
    assert sel["rgb"].data_ptr() == shard.data_ptr() and int(sel["guard_count"]) == R
    assert torch.equal(bits(shard[:, :3]), bits(every["rgb"])) and torch.equal(bits(shard[:, 3]), bits(every["disp"]))
    assert_same_bits(sel, every, ("weights", "depth", "acc", "z"), "thr 1e6, shard")
    plain = render(c, n, guard=None)
    none = render(c, n, guard_threshold=1e-30, guard_long_rays="selective")
    assert int(none["guard_count"]) == 0
    assert_same_bits(none, plain, OUTS + ("z",), "thr 1e-30")
    assert not torch.equal(bits(plain["rgb"]), bits(every["rgb"]))             # (the guard changes something on this frame)


@pytest.mark.parametrize("n", [192, 320])
@pytest.mark.parametrize("R", [1, 5, 7])
def test_rays_that_cross_groups_and_nan_rays(chain, R, n):
    """A handful of explicit rays on the five-tile kernel (groups of 320 samples): one run, the rays' ends in other groups than
    their starts, the open ray's carry handed on through LDS.  One ray misses the sphere (a NaN mean): it is never flagged, and
    NaN sits where the every-ray form has it."""
    from nerf_sampling_amd import ops

    c = chain("lego_synth", "bf16", 192)
    o, d, view = (c[k][200:200 + R].clone() for k in ("o", "d", "view"))
    if R > 1:
        d[R // 2] = torch.tensor([0.0, 0.0, 1.0], device="cuda")                # pointing away from the scene
    hit = torch.ones(R, dtype=torch.bool, device="cuda")
    hit[R // 2] = R == 1
    with ops.debug_switch(prod_tiles=5):
        every = render(c, n, rays=(o, d, view), guard_threshold=0.0)
        plain = render(c, n, rays=(o, d, view), guard=None)
        assert bool(torch.isnan(every["rgb"]).any(-1).eq(~hit).all())
        s16 = ops.nerf_forward_rays(c["nf"], o, d, every["z"], view)[:, -1, 3]   # (NaN on the ray that misses: never below thr)
        for thr in (1e6, 16.0):
            out = render(c, n, rays=(o, d, view), guard_threshold=thr, guard_long_rays="selective")
            flagged = s16.abs() < thr
            assert int(out["guard_count"]) == int(flagged.sum()) and not bool(flagged[~hit].any()), (R, n, thr)
            assert thr != 1e6 or int(flagged.sum()) == int(hit.sum())
            for k in OUTS + ("z",):
                assert torch.equal(torch.isnan(out[k]), torch.isnan(every[k])), (R, n, thr, k)
            assert_same_bits(out, every, OUTS + ("z",), (R, n, thr, "flagged"), rows=hit & flagged)
            assert_same_bits(out, plain, OUTS + ("z",), (R, n, thr, "not flagged: the 16-bit render"), rows=hit & ~flagged)


def test_defaults_are_untouched(chain):
    """Without the new argument a guarded N = 192 render takes the every-ray form at every threshold; at N = 64 the argument
    changes nothing (both are the single-chunk selective form)."""
    c = chain("lego_synth", "bf16", 192)
    every = render(c, 192, guard_threshold=0.0)
    for thr in (16.0, 2.0):
        out = render(c, 192, guard_threshold=thr)
        assert int(out["guard_count"]) == -1
        assert_same_bits(out, every, OUTS + ("z",), ("default", thr))
    for thr in (16.0, 2.0):
        a = render(c, 64, guard_threshold=thr, guard_long_rays="selective")
        b = render(c, 64, guard_threshold=thr, guard_long_rays="every")
        assert int(a["guard_count"]) == int(b["guard_count"]) >= 0               # (the single-chunk selective form reports it too)
        assert_same_bits(a, b, OUTS + ("z",), ("N = 64", thr))


def test_ignored_where_it_does_not_apply(chain, gpu_modules):
    """An f16x3 field, an fp32 guard handle and the five-launch chain: guard_long_rays="selective" gives the bits of "every", and
    the count tensor is left at -1."""
    c = chain("lego_synth", "bf16", 192)
    m = gpu_modules("lego_synth")
    cases = {"f16x3 field": dict(c, nf=m["fine"].packed("f16x3")), "fp32 guard": dict(c, gw=m["fine"].packed("f32")),
             "chain": c}
    for name, cc in cases.items():
        kw = dict(guard_threshold=16.0, one_kernel=name != "chain")
        a = render(cc, 192, guard_long_rays="selective", **kw)
        b = render(cc, 192, guard_long_rays="every", **kw)
        assert int(a["guard_count"]) == -1 and int(b["guard_count"]) == -1, name
        assert_same_bits(a, b, OUTS + ("z",), name)
