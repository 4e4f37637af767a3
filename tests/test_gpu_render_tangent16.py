"""The one-kernel renderer with depth tangents on an f16 field (ns_render_rays_fused_tangent on an f16 handle,
ns_nerf_mlp_ob16_tan.hip, reached through approximate=True) on the GPU:
  * primal: rgb / disp / depth / acc are the f16 forward's bits -- ns_render_rays_fused on the same handle when the call runs the
    DepthNet itself, place_samples -> nerf_forward_rays -> raw2outputs of a supplied depth -- at every sample count, both ray
    sources, white and black backgrounds, both kernel widths;
  * exact zeros: rays without a depth tangent, and a field whose raw does not depend on position;
  * accuracy: J against the f16x3 tangent kernel on the same network (itself gated against autograd of the fp32 chain in
    test_gpu_render_tangent.py), per column on the rays not at a kink;
  * end to end: render_depthnet_differentiable(approximate=True)'s DepthNet gradients against the f16x3 path's."""

import copy

import pytest
import torch

from oracle import nerf_oracle as O
from test_gpu_render_tangent import _ill_conditioned, _scene_rays, _tangent_jacobian

pytestmark = pytest.mark.gpu

DTYPES = ("f16",)         # (bf16 stays refused: its DepthNet gradients missed their target)
ALL_N = (2, 4, 8, 16, 32, 64, 128, 192, 256, 320, 384, 448, 512)
JAC_N = (2, 8, 32, 64, 128, 192)
MAPS = ("rgb", "disp", "depth", "acc")
COLS = ("r", "g", "b", "disp", "depth", "acc")


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b, tag):
    assert torch.equal(_bits(a), _bits(b)), (tag, float((a - b).abs().nan_to_num().max()))


def _camera(H, W, az=40.0):
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(az, -30.0, 4.0)[:3, :4]
    return H, W, K, c2w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scene,rows", [("tiny_synth", 5), ("lego_synth", 7)])
def test_primal_is_the_forward_bit_for_bit(gpu_modules, scene, rows, dtype):
    """tiny_synth: W = 128 (NKB = 4); lego_synth: W = 256 (NKB = 8), whose forward runs the generated production layers"""
    from nerf_sampling_amd import ops

    m = gpu_modules(scene)
    H, W, K, c2w = _camera(rows, 47)
    dn, nf = m["depth"].packed("f16"), m["fine"].packed(dtype)
    o, d, view = ops.get_rays(H, W, K, c2w)[:3]
    mean = ops.depthnet_forward(dn, o, d).reshape(-1)
    for n in ALL_N:
        for white in (True, False):
            tag = (dtype, n, white)
            ref = ops.render_rays_depthnet(dn, nf, camera=(H, W, K, c2w, 0, H), n_samples=n, mode="uniform", std=0.1,
                                           one_kernel=True, white_bkgd=white, extras=("depth", "acc"))
            out, J = ops.render_rays_depthnet_tangent(dn, nf, camera=(H, W, K, c2w, 0, H), n_samples=n, std=0.1,
                                                      white_bkgd=white, extras=("depth", "acc"), approximate=True)
            for k in MAPS:
                _same(out[k], ref[k], tag + (k, "camera"))
            pts, z = ops.place_samples(o, d, mean, n, "uniform", 0.1)
            raw = ops.nerf_forward_rays(nf, o, d, z, view)
            rgb, disp, acc, depth, _alphas, _w = ops.raw2outputs(raw, z, d, None, white)
            out2, J2 = ops.render_rays_depthnet_tangent(mean, nf, rays=(o, d, view), n_samples=n, std=0.1, white_bkgd=white,
                                                        extras=("depth", "acc"), approximate=True)
            for k, v in (("rgb", rgb), ("disp", disp), ("depth", depth), ("acc", acc)):
                _same(out2[k], v, tag + (k, "mean"))
            fin = torch.isfinite(out["rgb"]).all(-1) & torch.isfinite(out["disp"])
            for k in MAPS:        # the same depth either way: the same Jacobian, finite where the forward is
                _same(J2[k], J[k], tag + (k, "J"))
                v = J[k] if J[k].dim() == 1 else J[k].amax(-1)
                assert torch.isfinite(v[fin]).all(), tag + (k,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rays_without_a_depth_tangent_give_zero(gpu_modules, dtype):
    """A NaN mean, and means whose every sample is clipped (to 2, or to 6 from a mean of 100): J == 0 exactly"""
    from nerf_sampling_amd import ops

    m = gpu_modules("lego_synth")
    H, W, K, c2w = _camera(4, 16)
    o, d, view = ops.get_rays(H, W, K, c2w)[:3]
    nf = m["fine"].packed(dtype)
    R = o.shape[0]
    for n in (8, 64, 128, 192):
        mean = torch.full((R,), 4.0, device="cuda")
        mean[0::4] = float("nan")
        mean[1::4] = 0.5
        mean[2::4] = 100.0
        _, J = ops.render_rays_depthnet_tangent(mean, nf, rays=(o, d, view), n_samples=n, std=0.1, approximate=True)
        for k in MAPS:
            for start in (0, 1, 2):
                v = J[k][start::4]
                assert torch.equal(v, torch.zeros_like(v)), (dtype, n, k, start)
            assert torch.isfinite(J[k][3::4]).all(), (dtype, n, k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [256, 128])
def test_a_field_constant_in_space_has_no_colour_or_opacity_tangent(dtype, W):
    """Every weight 0, every bias not: raw is the same at every point, so d rgb = d acc = 0 exactly, and with no sample clipped
    d depth = sum_j w_j dz_j = acc (up to the order of the fp32 sums)"""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.run_nerf_helpers import NeRF

    torch.manual_seed(0)
    net = NeRF(D=8, W=W, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.Linear):
                mod.weight.zero_()
                mod.bias.uniform_(0.05, 0.5)
    nf = net.cuda().packed(dtype)
    H, W_, K, c2w = _camera(6, 20)
    o, d, view = ops.get_rays(H, W_, K, c2w)[:3]
    R = o.shape[0]
    mean = 3.0 + 2.0 * torch.rand((R,), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    for n in (4, 64, 192):
        out, J = ops.render_rays_depthnet_tangent(mean, nf, rays=(o, d, view), n_samples=n, std=0.1, extras=("acc",),
                                                  approximate=True)
        assert torch.equal(J["rgb"], torch.zeros_like(J["rgb"])), (dtype, W, n)
        assert torch.equal(J["acc"], torch.zeros_like(J["acc"])), (dtype, W, n)
        assert float(out["acc"].min()) > 0.01, (dtype, W, n)
        torch.testing.assert_close(J["depth"], out["acc"], rtol=1e-6 * n, atol=0.0)


# Accuracy of the 16-bit Jacobian against the f16x3 kernel's, per column c over the rays not at a kink (_ill_conditioned) and
# finite on both sides: e = |J16 - J3| / rms(J3[:, c]); its median and 99th percentile, and the relative L2 error
# ||J16 - J3|| / ||J3|| of the column.  Gates: about 3x the largest value measured over N in JAC_N and the three columns of a
# kind (rgb: r, g, b), per dtype and scene.
# measured worst (median, p99, relative L2): tiny_synth rgb 0.0007 / 0.23 / 0.24, disp 0.0008 / 0.33 / 0.17, depth 0.0001 / 0.22 /
# 0.23, acc 0 / 0.22 / 0.22; lego_synth (N <= 32: at N >= 64 fewer than 20 of its rays are away from a kink) rgb 0 / 0.87 / 0.20,
# disp 0 / 0.60 / 0.15, depth 0 / 0.62 / 0.14, acc 0 / 0.45 / 0.31; the fitted band rgb 0.043 / 1.24 / 0.31, disp 0.011 / 0.35 /
# 0.085, depth 0.011 / 0.35 / 0.085, acc 0.97 / 6.0 / 1.33.  The tails are rays whose kinks the f16 field's rounding moves (a
# ReLU or the last sample's step within ~1e-3 of zero, the fp16 rounding, where the fp32 classification looks at 1e-5); on the
# fitted band d acc is such a quantity on most rays (0 where the last sample's sigma is > 0, not 0 where it is <= 0).
# Gates: 3 x measured (1e-3 where the measured median is 0).
ACC_GATE = {
    ("f16", "tiny_synth"): {"rgb": (0.0021, 0.69, 0.72), "disp": (0.0025, 1.0, 0.52), "depth": (0.001, 0.66, 0.69),
                            "acc": (0.001, 0.66, 0.68)},
    ("f16", "lego_synth"): {"rgb": (0.001, 2.6, 0.59), "disp": (0.001, 1.8, 0.44), "depth": (0.001, 1.9, 0.42),
                            "acc": (0.001, 1.4, 0.93)},
    ("f16", "shapes_fit"): {"rgb": (0.13, 3.7, 0.92), "disp": (0.032, 1.05, 0.26), "depth": (0.032, 1.05, 0.26),
                            "acc": (2.9, 18.0, 4.0)},
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth", "shapes_fit"])
def test_jacobian_against_the_f16x3_kernel(gpu_modules, scene, dtype):
    from nerf_sampling_amd import ops

    m = gpu_modules(scene)
    o, d, view = _scene_rays(scene)
    mean = ops.depthnet_forward(m["depth"].packed("f32"), o, d).reshape(-1)
    n3, n16 = m["fine"].packed("f16x3"), m["fine"].packed(dtype)
    stats = {}
    for n in JAC_N:
        out3, J3 = ops.render_rays_depthnet_tangent(mean, n3, rays=(o, d, view), n_samples=n, std=0.1)
        out16, J16 = ops.render_rays_depthnet_tangent(mean, n16, rays=(o, d, view), n_samples=n, std=0.1, approximate=True)
        A, B = _tangent_jacobian(J16), _tangent_jacobian(J3)
        fin = torch.isfinite(out16["rgb"]).all(-1) & torch.isfinite(out16["disp"])
        assert torch.isfinite(A[fin]).all(), (dtype, n)
        ill, _margin = _ill_conditioned(m["fine"], o, d, view, mean, n)
        well = ~(ill["relu"] | ill["step"] | ill["clip"]) & torch.isfinite(B).all(-1) & fin
        if int(well.sum()) < 20:      # (at N >= 64 nearly every ray of lego_synth has some visible unit at a kink)
            stats[n] = dict(rays=int(o.shape[0]), well=int(well.sum()))
            continue
        a, b = A[well], B[well]
        st = {}
        for c, name in enumerate(COLS):
            rms = float(b[:, c].square().mean().sqrt())
            if rms == 0.0:
                st[name] = (0.0, 0.0, 0.0)
                continue
            e = (a[:, c] - b[:, c]).abs() / rms
            st[name] = (float(e.median()), float(torch.quantile(e, 0.99)),
                        float((a[:, c] - b[:, c]).norm() / b[:, c].norm()))
        stats[n] = dict(rays=int(o.shape[0]), well=int(well.sum()), **{k: tuple(round(x, 5) for x in v) for k, v in st.items()})
    print(f"{dtype} {scene}: per N {stats}")
    worst = {}
    for st in stats.values():
        if "r" not in st:
            continue
        for kind, cols in (("rgb", ("r", "g", "b")), ("disp", ("disp",)), ("depth", ("depth",)), ("acc", ("acc",))):
            w = worst.setdefault(kind, [0.0, 0.0, 0.0])
            for col in cols:
                w[:] = [max(x, y) for x, y in zip(w, st[col])]
    print(f"{dtype} {scene}: worst (median, p99, rel L2) per kind {worst}")
    gate = ACC_GATE[(dtype, scene)]
    for kind, w in worst.items():
        for x, g, what in zip(w, gate[kind], ("median", "p99", "rel L2")):
            assert x <= g, (kind, what, x, g, stats)


def _q16(x):
    """x rounded to fp16 in value, the identity in its derivative: what an activation or operand of the f16 field is"""
    return x + (x.half().float() - x).detach()


def _posenc(x, L):
    """the reference's positional encoding (run_nerf_helpers.py:44-45 column order), differentiable"""
    return torch.cat([x] + [f(x * 2.0 ** k) for k in range(L) for f in (torch.sin, torch.cos)], -1)


def _f16_field_chain(net, o, d, view, mean, n, white):
    """An independent model of the f16 field, in fp32 torch with autograd: the packed network's operands (weights, the embedded
    inputs, every hidden activation) rounded to fp16, fp32 sums and biases, the view layer folded with feature_linear in fp64 as
    the packer does; placement and compositing by the fp32 chain (PlaceSamples -> Composite).  Its derivative carries no
    rounding, so against it the kernel's J differs by the fp16 rounding of the tangents (and the rare unit whose sign the two
    summation orders decide differently), not by the field."""
    from nerf_sampling_amd import autograd

    R = o.shape[0]
    pts, z = autograd.place_samples(o, d, mean, n, "uniform", 0.1)
    xe = _q16(_posenc(pts.reshape(-1, 3), 10))
    ve = _q16(_posenc(view[:, None].expand(R, n, 3).reshape(-1, 3), 4))
    W = net.W
    h = xe
    for i, L in enumerate(net.pts_linears):
        h = _q16(torch.relu(h @ _q16(L.weight).T + L.bias))
        if i in net._check_supported():
            h = torch.cat([xe, h], -1)
    sigma = h @ _q16(net.alpha_linear.weight).T + net.alpha_linear.bias
    Wf, bf = net.feature_linear.weight.double(), net.feature_linear.bias.double()
    Wv, bv = net.views_linears[0].weight.double(), net.views_linears[0].bias.double()
    w_fold = torch.cat([Wv[:, :W] @ Wf, Wv[:, W:]], -1).float()
    b_fold = (Wv[:, :W] @ bf + bv).float()
    hv = _q16(torch.relu(torch.cat([h, ve], -1) @ _q16(w_fold).T + b_fold))
    rgb = hv @ _q16(net.rgb_linear.weight).T + net.rgb_linear.bias
    raw = torch.cat([rgb, sigma], -1).reshape(R, n, 4)
    return autograd.composite(raw, z, d, None, white), raw.detach(), z.detach()


def _at_the_step(raw, z, d):
    """Rays whose last sample, composited with dist = 1e10 |d|, sits at the step of alpha: a visible last sample (T >= 1e-4)
    whose sigma is within 1e-4 of 0.  There alpha_last jumps between 0 and 1 with the sign of sigma, which the kernel and the
    model sum in different orders, and d alpha / d sigma is 1e10 |d|: the two Jacobians may differ without bound."""
    sig = raw[..., 3]
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * d.norm(dim=-1, keepdim=True)
    keep = 1.0 - (1.0 - torch.exp(-torch.relu(sig) * dist)) + 1e-10
    T_last = torch.prod(keep[:, :-1], -1)
    return (T_last >= 1e-4) & (sig[:, -1].abs() < 1e-4)


def _f16_field_jacobian(net, o, d, view, mean, n):
    mean = mean.detach().clone().requires_grad_(True)
    (rgb, disp, acc, depth, _a, _w), raw, z = _f16_field_chain(net, o, d, view, mean, n, True)
    cols = [rgb[:, 0], rgb[:, 1], rgb[:, 2], disp, depth, acc]
    J = []
    for i, c in enumerate(cols):
        (g,) = torch.autograd.grad(c.sum(), mean, retain_graph=i + 1 < len(cols))
        J.append(g)
    return torch.stack(J, -1), _at_the_step(raw, z, d)


# Gates of test_jacobian_against_the_same_f16_field, (median, p90, p99, rms) of e per kind, 3 x the worst measured over N in JAC_N
# (1e-5 where the measured value is 0: lego_synth's rays mostly hold no density, J = 0 on both sides).  Measured: tiny_synth rgb
# 4.2e-5 / 6.2e-4 / 3.1e-3 / 4.9e-3, disp 3.5e-5 / 3.4e-4 / 6.0e-3 / 0.068 (one ray, N = 64), depth 9e-6 / 6.0e-4 / 2.2e-3 /
# 4.5e-3, acc 0 / 6.1e-4 / 2.2e-3 / 4.6e-3; lego_synth rgb 0 / 3.9e-3 / 0.12 / 0.23, disp 0 / 2.1e-3 / 0.031 / 0.19, depth 0 /
# 2.0e-3 / 0.054 / 0.13, acc 0 / 2e-5 / 0.092 / 0.22; the fitted band rgb 3.1e-3 / 0.011 / 0.11 / 0.049, disp 1.5e-3 / 4.6e-3 /
# 0.034 / 0.013, depth 1.5e-3 / 4.8e-3 / 0.034 / 0.013, acc 1.5e-5 / 4e-5 / 1e-4 / 2e-5.  (Against the f16x3 kernel the same
# statistics are 10 .. 100 x larger: test_jacobian_against_the_f16x3_kernel.)
SAME_FIELD_GATE = {
    "tiny_synth": {"rgb": (1.3e-4, 1.9e-3, 9.3e-3, 0.015), "disp": (1.1e-4, 1.0e-3, 0.018, 0.2),
                   "depth": (3e-5, 1.8e-3, 6.6e-3, 0.014), "acc": (1e-5, 1.8e-3, 6.6e-3, 0.014)},
    "lego_synth": {"rgb": (1e-5, 0.012, 0.37, 0.68), "disp": (1e-5, 6.3e-3, 0.093, 0.58),
                   "depth": (1e-5, 6.0e-3, 0.16, 0.39), "acc": (1e-5, 6e-5, 0.28, 0.65)},
    "shapes_fit": {"rgb": (9.4e-3, 0.034, 0.33, 0.15), "disp": (4.5e-3, 0.014, 0.1, 0.04),
                   "depth": (4.6e-3, 0.014, 0.1, 0.04), "acc": (4.5e-5, 1.2e-4, 3e-4, 6e-5)},
}


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth", "shapes_fit"])
def test_jacobian_against_the_same_f16_field(gpu_modules, scene):
    """J of the kernel against autograd of _f16_field_chain on every finite ray not at the step (_at_the_step, counted): per
    column c, e = |J - J_field| / s_c with s_c = rms(J_field[:, c]), and for d acc the larger of its own and the colour columns'
    rms (same units; on rays that end opaque d acc is a cancellation of O(d rgb) terms to ~0 on both sides, no scale of its own)"""
    from nerf_sampling_amd import ops

    m = gpu_modules(scene)
    o, d, view = _scene_rays(scene)
    mean = ops.depthnet_forward(m["depth"].packed("f32"), o, d).reshape(-1)
    nf = m["fine"].packed("f16")
    stats = {}
    for n in JAC_N:
        out, J = ops.render_rays_depthnet_tangent(mean, nf, rays=(o, d, view), n_samples=n, std=0.1, approximate=True)
        A = _tangent_jacobian(J)
        B, step = _f16_field_jacobian(m["fine"], o, d, view, mean, n)
        assert bool((torch.isfinite(A).all(-1) & torch.isfinite(B).all(-1)).all()), (scene, n)
        a, b = A[~step], B[~step]
        rms = b.square().mean(0).sqrt()
        rms[5] = torch.maximum(rms[5], rms[:3].max())
        st = {"step": int(step.sum())}
        for c, name in enumerate(COLS):
            if float(rms[c]) == 0.0:
                continue
            e = (a[:, c] - b[:, c]).abs() / rms[c]
            st[name] = (round(float(e.median()), 6), round(float(torch.quantile(e, 0.9)), 5),
                        round(float(torch.quantile(e, 0.99)), 4), round(float((a[:, c] - b[:, c]).norm() / rms[c] / a.shape[0] ** 0.5), 5))
        stats[n] = st
    print(f"f16 {scene}: J against the same f16 field, (median, p90, p99, rms) per N {stats}")
    for n, st in stats.items():
        assert st["step"] <= 0.02 * o.shape[0], (n, stats)
        for col, v in st.items():
            if col == "step":
                continue
            gate = SAME_FIELD_GATE[scene]["rgb" if col in ("r", "g", "b") else col]
            for x, g, what in zip(v, gate, ("median", "p90", "p99", "rms")):
                assert x <= g, (n, col, what, x, g, stats)


@pytest.mark.parametrize("scene", ["lego_synth", "shapes_fit"])
def test_depthnet_gradients_against_the_same_f16_field(gpu_modules, scene):
    """The DepthNet gradient of render_depthnet_differentiable(approximate=True) against autograd through _f16_field_chain, and
    both against the f16x3 path's.  Measured cosines (lego_synth N = 32 / 128, the fitted band N = 32 / 128):
      kernel vs the same f16 field   1.000000 / 0.999983 / 0.999999 / 0.998931
      kernel vs f16x3                0.998017 / 0.999965 / 0.999894 / 0.978852
      the f16 field vs f16x3         0.998022 / 0.999934 / 0.999884 / 0.979927
    The f16 field itself, differentiated without any rounding of its tangents, is as far from the f16x3 path as the kernel is: the
    shortfall from the 0.999 first asked of f16 against f16x3 is the field's (its fp16 weights and activations), which no tangent
    arithmetic removes.  Gated: the kernel against the same field at 0.998 (the fitted band at N = 128 measures 0.99893, the rest
    >= 0.99998), and the kernel's distance from f16x3 within half of the field's own plus 1e-5."""
    from nerf_sampling_amd import autograd

    m = gpu_modules(scene)
    net = copy.deepcopy(m["depth"])
    for p in net.parameters():
        p.requires_grad_(True)
    params = [p for p in net.parameters() if p.requires_grad]
    o, d, view = _scene_rays(scene)
    target = torch.rand((o.shape[0], 3), device="cuda", generator=torch.Generator("cuda").manual_seed(3))

    def loss_of(out):
        return ((out["rgb"] - target) ** 2).mean() + 0.1 * out["depth"].mean()

    def cos(a, b):
        return float(a @ b / (a.norm() * b.norm()))

    res = {}
    for n in (32, 128):
        grads = {}
        for dt in ("f16x3", "f16"):
            out = autograd.render_depthnet_differentiable(net, m["fine"].packed(dt), rays=(o, d, view), n_samples=n, std=0.1,
                                                          chunk=200, approximate=dt != "f16x3")
            grads[dt] = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss_of(out), params)]).double()
        mean = autograd.depthnet_forward_train(net, o, d).reshape(-1)
        (rgb, disp, acc, depth, _a, _w), raw, z = _f16_field_chain(m["fine"], o, d, view, mean, n, True)
        g = torch.autograd.grad(loss_of({"rgb": rgb, "depth": depth}), params)
        grads["field"] = torch.cat([x.reshape(-1) for x in g]).double()
        step = _at_the_step(raw, z, d)
        assert torch.isfinite(grads["f16"]).all(), n
        res[n] = dict(kernel_vs_field=round(cos(grads["f16"], grads["field"]), 6),
                      kernel_vs_f16x3=round(cos(grads["f16"], grads["f16x3"]), 6),
                      field_vs_f16x3=round(cos(grads["field"], grads["f16x3"]), 6), step_rays=int(step.sum()))
    print(f"f16 {scene}: cosines of the DepthNet gradient per N {res}")
    for n, r in res.items():
        assert r["kernel_vs_field"] >= 0.998, (n, res)
        assert abs(r["kernel_vs_f16x3"] - r["field_vs_f16x3"]) <= 0.5 * (1.0 - r["field_vs_f16x3"]) + 1e-5, (n, res)
