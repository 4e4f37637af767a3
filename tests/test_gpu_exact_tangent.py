"""The depth-tangent render kernels (ns_tangent.h: nerf_mlp_x3_tan_kernel, nerf_mlp_x3_tan1_kernel, nerf_tan16_kernel) against
float64 on fields with one right answer (tests/exact_tangent.py; its conditions: tests/test_exact_tangent_host.py).

Every call is ops.render_rays_depthnet_tangent(mean, handle, rays=(o, d, view), ...) on an identity network whose `raw` and
d raw / d m are exact in the kernel's operand tiles: J may differ from the float64 reference by the fp32 arithmetic of
walk_samples / write_jacobian only, and EVERY finite-mean ray is held to the error model's bound in every column -- at every
supported sample count, with the window of unclipped samples at the ray's start, its end, across every 64-sample boundary and
inside every chunk, the merged mean inside, below and above [2, 6], samples exactly on 2 and 6, ray counts that leave the last
group partial, both backgrounds.  A NaN mean and an all-clipped ray ride in every batch of three rays or more: J == 0 exactly
for them.  The primal maps are held to composite_bounds.py's comparator (check_maps), and two calls give the same bits."""

import numpy as np
import pytest
import torch

import exact_field as E
import exact_tangent as X

pytestmark = pytest.mark.gpu

U = X.U
_packed = {}


def _handle(net, dtype):
    from nerf_sampling_amd import ops

    key = (net["name"], net["which"], dtype)
    if key not in _packed:
        w, b = E.tensors(net)
        _packed[key] = ops.pack_nerf(w, b, net["D"], net["W"], list(net["skips"]), dtype=dtype, use_viewdirs=True, output_ch=4)
    return _packed[key]


def _accepted(handle, mode, N):
    from nerf_sampling_amd import _lib, ops

    return bool(_lib.load().ns_render_tangent_supported(handle.handle, ops._MODES[mode], N))


def _dtype(instance):
    return "f16" if instance == "f16" else "f16x3"


def test_the_library_accepts_the_required_networks():
    """(so that a refusal cannot empty the table: every other network is skipped where the library refuses it)"""
    for name in X.REQUIRED:
        net = X.network(name, "A")
        for N in X.ALL_N:
            assert _accepted(_handle(net, "f16x3"), "uniform", N) and _accepted(_handle(net, "f16"), "uniform", N), (name, N)
        assert _accepted(_handle(net, "f16x3"), "depth_only", 1), name


def _render(net, case, instance):
    from nerf_sampling_amd import ops

    o, d, v, m = (torch.from_numpy(a).cuda() for a in X.case_inputs(net, case))
    kw = dict(rays=(o, d, v), n_samples=max(case["N"], 2), std=float(X.std_of(case["N"], net["step"])), white_bkgd=case["white"],
              extras=("depth", "acc"), approximate=instance == "f16", mode="depth_only" if instance == "single" else "uniform")
    out, J = ops.render_rays_depthnet_tangent(m, _handle(net, _dtype(instance)), **kw)
    _, J2 = ops.render_rays_depthnet_tangent(m, _handle(net, _dtype(instance)), **kw)
    cat = lambda t: torch.cat([t["rgb"], t["disp"][:, None], t["depth"][:, None], t["acc"][:, None]], -1)
    J, J2 = cat(J), cat(J2)
    assert torch.equal(J.view(torch.int32), J2.view(torch.int32)), "two calls give different Jacobians"
    return cat(out).double().cpu().numpy(), J.double().cpu().numpy()


@pytest.mark.parametrize("instance", X.INSTANCES)
@pytest.mark.parametrize("name,which", [pytest.param(n, w, id=f"{n}-{w}") for n, w in X.TABLE])
def test_jacobian_is_float64s_on_every_ray(name, which, instance):
    net = X.network(name, which)
    if not _accepted(_handle(net, "f16x3"), "uniform", 64):
        assert name not in X.REQUIRED
        pytest.skip(f"the library refuses {name}")
    worst, worst_primal, where = 0.0, 0.0, None
    for case in X.cases(net, instance):
        ref = X.jacobian64(net, case, instance=instance)
        out, J = _render(net, case, instance)
        tag = (name, which, instance, case["N"], len(case["mean"]), case["white"])
        rest = np.setdiff1d(np.arange(len(case["mean"])), ref["keep"])
        if case["N"] > 1:                                    # rays without a depth tangent: a NaN mean, every sample clipped
            assert (J[rest] == 0).all(), tag + ("NaN mean",)
            clipped = np.flatnonzero((ref["samples"]["dz"] == 0).all(axis=1))
            assert (J[ref["keep"][clipped]] == 0).all(), tag + ("all clipped",)
            assert len(rest) + len(clipped) >= (2 if len(case["mean"]) >= 3 else 0), tag
        else:
            assert (J[:, 3:] == 0).all(), tag
        ratio = np.abs(J[ref["keep"]] - ref["J"]) / ref["bound"]
        if ratio.max() > worst:
            worst, where = float(ratio.max()), tag + (X.COLS[int(ratio.max(axis=0).argmax())],)
        assert np.isfinite(J[ref["keep"]]).all(), tag
        assert ratio.max() <= 1.0, tag + (f"|J - J64| is {float(ratio.max()):.3g} of its bound, column "
                                          f"{X.COLS[int(ratio.max(axis=0).argmax())]}, ray {int(ratio.max(axis=1).argmax())}",)
        worst_primal = max(worst_primal, X.primal_check(out[ref["keep"]], ref, case["white"]))
    print(f"{instance} {name} on pool {which}: worst |J - J64| / bound {worst:.3f} at {where}; primal {worst_primal:.3f} of its bound")


@pytest.mark.parametrize("instance", ("f16x3", "f16"))
def test_d_mean_is_the_sum_over_the_kernels_jacobian(instance):
    """DepthNetTangentRender's backward down to the depth (autograd.tangent_d_mean) on the kernel's own J, integer upstream
    gradients in {-2 .. 2}: |d m - sum_k g_k J_k| <= 6u sum_k |g_k J_k|"""
    from nerf_sampling_amd import autograd, ops

    net = X.network("prod", "A")
    case = [c for c in X.cases(net, instance) if c["N"] == 192 and c["kind"] == "main"][0]
    o, d, v, m = (torch.from_numpy(a).cuda() for a in X.case_inputs(net, case))
    _, J = ops.render_rays_depthnet_tangent(m, _handle(net, _dtype(instance)), rays=(o, d, v), n_samples=192,
                                            std=float(X.std_of(192, net["step"])), approximate=instance == "f16")
    R = o.shape[0]
    gen = torch.Generator().manual_seed(5)
    g = {k: torch.randint(-2, 3, (R, 3) if k == "rgb" else (R,), generator=gen).float().cuda() for k in ("rgb", "disp", "depth", "acc")}
    got = autograd.tangent_d_mean(J, g["rgb"], g["disp"], g["depth"], g["acc"]).double().cpu()
    terms = torch.cat([(g["rgb"] * J["rgb"]).double(), *[(g[k] * J[k]).double()[:, None] for k in ("disp", "depth", "acc")]], -1).cpu()
    assert bool(((got - terms.sum(-1)).abs() <= 6 * U * terms.abs().sum(-1)).all())
    only = autograd.tangent_d_mean(J, None, None, g["depth"], None)
    assert torch.equal(only, g["depth"] * J["depth"])


@pytest.mark.parametrize("R", X.SINGLE_COUNTS)
def test_single_sample_render_backpropagates_the_kernels_jacobian(R):
    """SingleSampleTangentRender: rgb and J are those of the direct call, bit for bit, and d depth = sum_c g_c J_c"""
    from nerf_sampling_amd import autograd, ops

    net = X.network("d2w128", "A")
    case = [c for c in X.cases(net, "single") if len(c["mean"]) == R][0]
    o, d, v, m = (torch.from_numpy(a).cuda() for a in X.case_inputs(net, case))
    h = _handle(net, "f16x3")
    out, J = ops.render_rays_depthnet_tangent(m, h, rays=(o, d, v), n_samples=1, std=0.0, mode="depth_only")
    depth = m.clone()[:, None].requires_grad_(True)
    rgb, disp = autograd.render_single_sample(depth, o, d, v, h)
    assert torch.equal(rgb.detach().view(torch.int32), out["rgb"].view(torch.int32)) and torch.equal(disp, out["disp"])
    g = torch.randint(-2, 3, (R, 3), generator=torch.Generator().manual_seed(R)).float().cuda()
    (dm,) = torch.autograd.grad(rgb, depth, g)
    terms = (g * J["rgb"]).double()
    assert dm.shape == depth.shape
    assert bool(((dm.reshape(-1).double() - terms.sum(-1)).abs() <= 6 * U * terms.abs().sum(-1)).all())
