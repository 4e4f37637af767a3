"""The render kernel (nerf_render_ob16_kernel: the five-tile production program on the sigma-first stream, whose waves run
drain twins instead of the colour statements when none of their samples can contribute) against the production kernel, in one
process through ns_debug_set("no_colour_skip"), BIT FOR BIT on every output -- and the counter of skipping waves against the
number predicted from sigma, so that no case passes with the path never taken.

Every launch pins five tiles (prod_tiles=5): the dispatcher takes four below a few hundred thousand samples and whenever
per-sample outputs are asked for, and only five-tile launches qualify for the render kernel.

A "signed" field gives the tests a density they control: trunk units 0 / 1 carry relu(x) / relu(-x) of the point's first
coordinate through all eight layers exactly (weights 1, the numbers stay representable) and alpha_linear is 30 (h0 - h1), so
sigma = 30 x has the sign of x in bf16 and f16 alike; everything else is the seeded lego_synth field, so the colour layers see
ordinary activations.  Rays start near (0, 0, 4) and aim at (+-1, y, 0): every sample of a ray has the sign of d_x."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

EXTRAS = ("z", "weights", "pts", "depth", "acc")
KEYS = ("rgb", "disp", "depth", "acc", "weights", "z", "pts")
WAVE, GROUP = 80, 320            # samples of a five-tile wave and of a workgroup's group


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(a, b, what):
    for k in KEYS:
        x, y = a[k], b[k]
        assert x.shape == y.shape, (what, k)
        assert torch.equal(torch.isnan(x), torch.isnan(y)), (what, k, "NaN positions")
        assert torch.equal(_bits(x), _bits(y)), (what, k, int((_bits(x) != _bits(y)).sum()))


def _module(params, which="fine"):
    from nerf_sampling_amd.run_nerf_helpers import NeRF

    net = NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    net.load_state_dict(params[which])
    for p in net.parameters():
        p.requires_grad_(False)
    return net.to("cuda")


def _depthnet(params, cfg):
    from nerf_sampling_amd.depth_net import DepthNet

    n, w = cfg["depth"]["n_layers"], cfg["depth"]["width"]
    dn = DepthNet(hidden_sizes=[w] * n, cat_hidden_sizes=[w] * n, sphere_radius=2.0)
    dn.load_state_dict(params["depth"])
    return dn.to("cuda")


@torch.no_grad()
def _build_nets():
    from nerf_sampling_amd import synthetic

    lego, fit = synthetic.make_scene("lego_synth"), synthetic.make_scene("shapes_fit")
    out = {"fit": (_module(fit), _depthnet(fit, synthetic.SCENES["shapes_fit"]))}
    dn = _depthnet(lego, synthetic.SCENES["lego_synth"])
    base = _module(lego)
    for name, shift in (("lego-1e3", -1e3), ("lego+1e3", 1e3)):
        m = copy.deepcopy(base)
        m.alpha_linear.bias.data += shift
        out[name] = (m, dn)
    signed = copy.deepcopy(base)
    for l, lin in enumerate(signed.pts_linears):
        c0 = 63 if l == 5 else 0                      # the layer behind the skip sees cat[x(63), h]
        lin.weight[0:2] = 0.0
        lin.bias[0:2] = 0.0
        if l == 0:
            lin.weight[0, 0], lin.weight[1, 0] = 1.0, -1.0
        else:
            lin.weight[0, c0], lin.weight[1, c0 + 1] = 1.0, 1.0
    signed.alpha_linear.weight.zero_()
    signed.alpha_linear.weight[0, 0], signed.alpha_linear.weight[0, 1] = 30.0, -30.0
    signed.alpha_linear.bias.zero_()
    out["signed"] = (signed, dn)
    for name, b in (("zero+", 0.0), ("zero-", -0.0)):
        m = copy.deepcopy(base)
        m.alpha_linear.weight.zero_()
        m.alpha_linear.bias.fill_(b)
        out[name] = (m, dn)
    return out


@pytest.fixture(scope="module")
def nets():
    """name -> (field module, DepthNet module); packed handles are cached by the modules per dtype"""
    return _build_nets()


def _handles(nets, name, dtype):
    from nerf_sampling_amd import ops

    field, dn = nets[name]
    return dn.packed(ops.depthnet_dtype_for(dtype)), field.packed(dtype)


def _render(dw, nw, skip, *, n=64, white=True, rays=None, camera=None, **kw):
    from nerf_sampling_amd import ops

    sw = dict(prod_tiles=5, count_colour_skips=1)
    if not skip:
        sw["no_colour_skip"] = 1
    with ops.debug_switch(**sw):
        out = ops.render_rays_depthnet(dw, nw, rays=rays, camera=camera, n_samples=n, mode="uniform", std=0.1,
                                       white_bkgd=white, extras=EXTRAS, one_kernel=True, **kw)
        return out, ops.colour_skip_count()


def _n_waves(S):
    return 4 * (-(-S // GROUP))


def _predicted(nw, o, d, v, z):
    """Waves the kernel must skip, from the per-sample inputs it sees: every sample of the wave (the tail's waves hold clamped
    copies of the last sample) has sigma <= 0, finite inputs and a finite {z, dist |d|} record."""
    from nerf_sampling_amd import ops

    with ops.debug_switch(prod_tiles=5):
        sigma = ops.nerf_forward_rays(nw, o, d, z, v)[..., 3]
    R, N = z.shape
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, device=z.device)], 1)
    norm = torch.sqrt(d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0]))
    ray_ok = torch.isfinite(o).all(1) & torch.isfinite(d).all(1) & torch.isfinite(v).all(1)
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    ok = (sigma <= 0) & torch.isfinite(z) & torch.isfinite(dist * norm[:, None]) & ray_ok[:, None] & torch.isfinite(pts).all(-1)
    ok = ok.reshape(-1)
    S = ok.numel()
    idx = torch.arange(_n_waves(S) * WAVE, device=ok.device).clamp_(max=S - 1)
    return ok[idx].reshape(-1, WAVE).all(1)


def _camera_rays(H, W, K, c2w):
    from nerf_sampling_amd import ops

    o, d, v = ops.get_rays(H, W, K, c2w)[:3]
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), v.reshape(-1, 3).contiguous()


def _signed_rays(empty, seed=0):
    """one ray per entry of `empty` (bool): from near (0, 0, 4) towards (-1, y, 0) if empty else (+1, y, 0)"""
    g = torch.Generator().manual_seed(seed)
    R = len(empty)
    o = torch.tensor([0.0, 0.0, 4.0]) + 0.02 * torch.randn(R, 3, generator=g)
    tgt = torch.stack([torch.where(torch.as_tensor(empty), -1.0, 1.0) * (0.6 + 0.4 * torch.rand(R, generator=g)),
                       torch.rand(R, generator=g) - 0.5, torch.zeros(R)], 1)
    d = tgt - o
    d = d / d.norm(dim=1, keepdim=True)              # |d_x| >= 0.14, depths of 2 .. 6: |x| >= 0.28
    return o.cuda(), d.cuda(), d.clone().cuda()


def _check(nets, name, dtype, white, rays=None, camera=None, n=64, what=""):
    dw, nw = _handles(nets, name, dtype)
    new, count = _render(dw, nw, True, n=n, white=white, rays=rays, camera=camera)
    old, count_old = _render(dw, nw, False, n=n, white=white, rays=rays, camera=camera)
    assert count_old == 0, what
    _assert_same(new, old, what)
    return new, count, nw


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("white", [True, False])
def test_fitted_scene_frame_skips_what_sigma_predicts(nets, dtype, white):
    """40 x 40 rays of the fitted scene, from the camera and from the same rays as arrays: identical bits, and the counter
    equals the prediction and lies strictly between none and all of the waves"""
    from nerf_sampling_amd import synthetic

    H = W = 40
    _, K = synthetic.blender_intrinsics(H, W)
    c2w = synthetic.render_poses(40)[5, :3, :4]
    cam, count, nw = _check(nets, "fit", dtype, white, camera=(H, W, K, c2w, 0, H), what="camera")
    o, d, v = _camera_rays(H, W, K, c2w)
    arr, count_arr, _ = _check(nets, "fit", dtype, white, rays=(o, d, v), what="arrays")
    _assert_same(cam, arr, "camera vs arrays")
    want = int(_predicted(nw, o, d, v, cam["z"]).sum())
    waves = _n_waves(H * W * 64)
    print(f"fitted scene {dtype}: {count} of {waves} waves skip")
    assert count == count_arr == want
    assert 0 < count < waves


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("white", [True, False])
def test_every_wave_or_no_wave_skips_under_a_shifted_density_bias(nets, dtype, white):
    from nerf_sampling_amd import synthetic

    H = W = 24
    _, K = synthetic.blender_intrinsics(H, W)
    c2w = synthetic.render_poses(40)[15, :3, :4]
    for name, want in (("lego-1e3", _n_waves(H * W * 64)), ("lego+1e3", 0)):
        _, count, _ = _check(nets, name, dtype, white, camera=(H, W, K, c2w, 0, H), what=name)
        assert count == want, name
        o, d, v = _camera_rays(H, W, K, c2w)
        _, count, _ = _check(nets, name, dtype, white, rays=(o, d, v), what=name + " arrays")
        assert count == want, name


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("R", [1, 4, 5, 7, 13])
def test_ragged_tails(nets, dtype, R):
    """a one-ray launch, a wave of clamped duplicates only, partial groups: on the signed field with every other ray empty and
    with every ray empty"""
    for empty in ([r % 2 == 0 for r in range(R)], [True] * R):
        o, d, v = _signed_rays(empty, seed=R)
        new, count, nw = _check(nets, "signed", dtype, True, rays=(o, d, v), what=f"R={R}")
        want = _predicted(nw, o, d, v, new["z"])
        assert count == int(want.sum())
        if all(empty):
            assert count == _n_waves(R * 64)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("blocks", ["groups", "waves"])
def test_skipping_and_computing_passes_alternate_in_a_workgroup(nets, dtype, white, blocks):
    """R = 2600 = 520 groups of five rays: more than two rounds per workgroup on 256 CUs.  "groups": whole groups empty or
    solid, the parity flipping from round to round, so half of the workgroups go skip -> compute -> skip and the others the
    reverse.  "waves": two empty rays at the front of a group (its wave 0 skips alone) or at its back (wave 3), alternating
    likewise"""
    from nerf_sampling_amd import ops

    R = 2600
    empty = []
    for grp in range(R // 5):
        flip = ((grp & 1) ^ ((grp >> 8) & 1)) == 0
        if blocks == "groups":
            empty += [flip] * 5
        else:
            empty += [True, True, False, False, False] if flip else [False, False, False, True, True]
    o, d, v = _signed_rays(empty, seed=3)
    new, count, nw = _check(nets, "signed", dtype, white, rays=(o, d, v), what=blocks)
    want = _predicted(nw, o, d, v, new["z"])
    assert count == int(want.sum())
    per_group = want.reshape(-1, 4)
    if blocks == "groups":
        assert torch.equal(per_group.all(1).cpu(), torch.tensor(empty[::5])) and torch.equal(per_group.any(1), per_group.all(1))
    else:
        flips = torch.tensor(empty[::5])
        assert torch.equal(per_group[:, 0].cpu(), flips) and torch.equal(per_group[:, 3].cpu(), ~flips)
        assert not per_group[:, 1:3].any()
    # both orders occur inside one workgroup (groups b, b + CUs, b + 2 CUs), whatever the CU count of the device up to 519
    cus = int(ops._lib.load().ns_device_cu_count())
    first = per_group[:, 0].cpu()
    pairs = {(bool(first[b]), bool(first[b + cus])) for b in range(0, 520 - cus)} if 0 < cus < 520 else set()
    assert cus >= 520 or pairs == {(True, False), (False, True)}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n", [64, 32, 8, 2])
def test_sample_counts(nets, dtype, n):
    """N = 64 .. 2: rays per wave from 1.25 to 40; 41 rays, the first twenty and six more of them empty"""
    empty = [r < 20 or 30 <= r < 36 for r in range(41)]
    o, d, v = _signed_rays(empty, seed=n)
    new, count, nw = _check(nets, "signed", dtype, True, rays=(o, d, v), n=n, what=f"N={n}")
    want = _predicted(nw, o, d, v, new["z"])
    assert count == int(want.sum())
    if n >= 8:
        assert 0 < count < _n_waves(41 * n)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["zero+", "zero-"])
def test_sigma_of_exactly_zero_skips(nets, dtype, name):
    """alpha_linear with zero weights and a bias of +0 / -0: sigma is exactly zero everywhere, alpha is +0 and every wave skips
    (sigma <= 0 holds at 0: that such a wave skips is the skip condition itself).  The -0 bias does not reach the comparison as
    -0: it is the C operand of a chain of +0 products (zero weights, the zero-padded view K-block), and -0 + +0 = +0; both
    packings are kept because the two bias bit patterns are what a caller can hand in."""
    o, d, v = _signed_rays([True, False, True, True, False], seed=9)
    new, count, nw = _check(nets, name, dtype, True, rays=(o, d, v), what=name)
    assert count == _n_waves(5 * 64) == int(_predicted(nw, o, d, v, new["z"]).sum())
    assert not new["weights"].any() and not torch.signbit(new["weights"]).any()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("edge", ["nan_origin", "inf_direction", "huge_direction"])
def test_non_finite_rays_keep_their_waves_computing(nets, dtype, edge):
    """one ray of an empty-space group is not finite (or its |d| overflows): the waves that hold its samples (ray 2 of five:
    samples 128 .. 191, waves 1 and 2) run the colour statements, the other two skip; outputs equal the production kernel's"""
    o, d, v = _signed_rays([True] * 5, seed=11)
    if edge == "nan_origin":
        o[2, 1] = float("nan")
    elif edge == "inf_direction":
        d[2, 0] = float("-inf")
        v[2] = d[2] / d[2].norm()
    else:
        d[2] = d[2] * 1e20          # |d|^2 overflows fp32: dist |d| = inf
    new, count, nw = _check(nets, "signed", dtype, True, rays=(o, d, v), what=edge)
    want = _predicted(nw, o, d, v, new["z"]).cpu()
    assert count == int(want.sum())
    assert want.tolist() == [True, False, False, True]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_launches_that_read_raw_colour_keep_the_production_kernel(nets, dtype):
    """raw, the max-weight sample and the guards read the colour of samples whose weight may be zero: such launches do not
    qualify -- the counter stays 0 and the results do not depend on the switch"""
    from nerf_sampling_amd import ops

    dw, nw = _handles(nets, "signed", dtype)
    o, d, v = _signed_rays([True] * 10, seed=5)

    def both(fn):
        res = []
        for skip in (True, False):
            sw = dict(prod_tiles=5, count_colour_skips=1, **({} if skip else {"no_colour_skip": 1}))
            with ops.debug_switch(**sw):
                out = fn()
                res.append((out, ops.colour_skip_count()))
        (a, ca), (b, cb) = res
        assert ca == 0 and cb == 0
        for k in a:
            assert torch.equal(_bits(a[k].float()), _bits(b[k].float())), k
        return a

    z = torch.linspace(3.0, 4.0, 64, device="cuda").repeat(10, 1).contiguous()
    both(lambda: {"raw": ops.nerf_forward_rays(nw, o, d, z, v)})                                   # raw without compositing
    # The hierarchical renderer at 32 + 32 samples: its fine pass is a compositing launch of 64 samples per ray on all-empty rays,
    # which qualifies in every other respect -- on its own every wave skips -- so the max-weight pointers (the epilogue's argmax
    # reads raw rgb of a zero-weight sample: all weights are +0 here, the argmax is sample 0) and the raw pointer are what keeps it
    # on the production kernel.  (The coarse pass of each call does run the render kernel under the switch; the counter is the
    # last launch's, the fine pass's.)
    def hier(**kw):
        return ops.render_rays_hierarchical(nw, nw, rays=(o, d, v), n_coarse=32, n_importance=32, **kw)

    with ops.debug_switch(prod_tiles=5, count_colour_skips=1):
        plain = hier(extras=("z", "weights"))
        assert ops.colour_skip_count() == _n_waves(10 * 64)
    got = both(lambda: hier(max_sample=True, extras=("z", "weights")))                            # max-weight sample
    assert {"max_z", "max_weights", "max_rgb"} <= set(got) and not got["weights"].any()
    for k in ("rgb", "disp", "z", "weights"):
        assert torch.equal(_bits(got[k]), _bits(plain[k])), k
    got = both(lambda: hier(extras=("z", "weights", "raw")))                                      # raw beside compositing
    assert got["raw"].shape == (10, 64, 4) and bool((got["raw"][..., :3] != 0).any())
    for k in ("rgb", "disp", "z", "weights"):
        assert torch.equal(_bits(got[k]), _bits(plain[k])), k
    both(lambda: hier(max_sample=True, extras=("z", "weights", "raw")))
    gw = nets["signed"][0].packed("f16x3")
    dg = nets["signed"][1].packed("f16x3")
    for thr in (0.0, 16.0):                                                                         # every-ray / selective guard
        both(lambda: ops.render_rays_depthnet(dg, nw, rays=(o, d, v), n_samples=64, mode="uniform", std=0.1, extras=EXTRAS,
                                              one_kernel=True, guard=gw, guard_threshold=thr))
    # ... and the same call without a guard does qualify
    _, count = _render(dg, nw, True, rays=(o, d, v))
    assert count == _n_waves(10 * 64)
