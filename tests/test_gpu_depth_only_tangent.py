"""The one-sample (NS_MODE_DEPTH_ONLY) instance of the tangent renderer (ns_tangent.h, nerf_mlp_x3_tan1_kernel) on the GPU:
  * primal: rgb / disp / depth / acc are the bits of the five-launch chain ns_render_rays_depthnet in depth_only mode on the same
    f16x3 handles, and of nerf_forward_rays -> raw2outputs at N = 1 for a supplied depth; J of disp / depth / acc is exactly 0;
  * Jacobian: J["rgb"] against torch autograd of the fp32 chain points_along_rays -> NerfInputGrad -> SingleSampleComposite under
    the per-ray bound of tests/test_gpu_render_tangent.py for its rgb columns;
  * a NaN depth gives a NaN rgb and a NaN J["rgb"] for its ray alone."""

import pytest
import torch

from test_gpu_render_tangent import KINK, MAPS, _camera, _same, _scene_rays

pytestmark = pytest.mark.gpu

RAY_COUNTS = (1, 3, 7, 63, 64, 65)


def _tangent(depthnet_or_mean, nf, **kw):
    from nerf_sampling_amd import ops

    return ops.render_rays_depthnet_tangent(depthnet_or_mean, nf, n_samples=1, std=0.1, mode="depth_only",
                                            extras=("depth", "acc"), **kw)


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
def test_primal_is_the_depth_only_chain_bit_for_bit(gpu_modules, scene):
    from nerf_sampling_amd import ops

    m = gpu_modules(scene)
    dn, nf = m["depth"].packed("f16x3"), m["fine"].packed("f16x3")
    cases = [(_camera(5, R), 2, 3) for R in RAY_COUNTS] + [(_camera(47, 67), 0, 47)]       # 3149 rays
    for (H, W, K, c2w), row0, row1 in cases:
        cam = (H, W, K, c2w, row0, row1)
        R = (row1 - row0) * W
        o, d, view = ops.get_rays(H, W, K, c2w, row0, row1)[:3]
        mean = ops.depthnet_forward(dn, o, d).reshape(-1)
        for white in (True, False):
            tag = (R, white)
            # the DepthNet inside the call, camera rays: == the five-launch chain in depth_only mode (n_samples is ignored)
            ref = ops.render_rays_depthnet(dn, nf, camera=cam, n_samples=5, mode="depth_only", std=0.1, one_kernel=False,
                                           white_bkgd=white, extras=("depth", "acc"))
            out, J = _tangent(dn, nf, camera=cam, white_bkgd=white)
            for k in MAPS:
                assert out[k].shape[0] == R and J[k].shape[0] == R
                _same(out[k], ref[k], tag + (k, "camera"))
            # explicit rays through the chain as well
            ref_x = ops.render_rays_depthnet(dn, nf, rays=(o, d, view), n_samples=1, mode="depth_only", std=0.1,
                                             one_kernel=False, white_bkgd=white, extras=("depth", "acc"))
            # a supplied depth, explicit rays: == nerf_forward_rays -> raw2outputs at N = 1
            z = mean[:, None].contiguous()
            raw = ops.nerf_forward_rays(nf, o, d, z, view)
            rgb, disp, acc, depth, _alphas, _w = ops.raw2outputs(raw, z, d, None, white)
            out2, J2 = _tangent(mean, nf, rays=(o, d, view), white_bkgd=white)
            for k, v in (("rgb", rgb), ("disp", disp), ("depth", depth), ("acc", acc)):
                _same(out2[k], v, tag + (k, "mean"))
                _same(out2[k], ref_x[k], tag + (k, "explicit rays"))
            assert torch.equal(out["disp"], torch.full_like(out["disp"], 1e10)), tag
            for k in ("depth", "acc"):
                assert torch.equal(out[k], torch.zeros_like(out[k])), tag + (k,)
            for k in ("disp", "depth", "acc"):        # constants of the single-sample rule: no tangent at all
                assert torch.equal(J[k], torch.zeros_like(J[k])) and torch.equal(J2[k], torch.zeros_like(J2[k])), tag + (k,)
            _same(J2["rgb"], J["rgb"], tag + ("J",))   # the same depth either way: the same Jacobian
            assert torch.isfinite(J["rgb"]).all(), tag
    # white_bkgd has no effect on a single sample
    a, Ja = _tangent(mean, nf, rays=(o, d, view), white_bkgd=True)
    b, Jb = _tangent(mean, nf, rays=(o, d, view), white_bkgd=False)
    _same(a["rgb"], b["rgb"], "white")
    _same(Ja["rgb"], Jb["rgb"], "white J")


def _chain_jacobian(m, o, d, view, mean):
    """d rgb / d mean [R,3] through the fp32 autograd chain of the training step, one backward per colour"""
    from nerf_sampling_amd import autograd

    mean = mean.detach().clone().requires_grad_(True)
    z = mean[:, None]
    pts = autograd.PointsAlongRays.apply(o, d, z)
    raw = autograd.NerfInputGrad.apply(pts, view, m["fine"])
    rgb = autograd.SingleSampleComposite.apply(raw, z, d, True)[0]
    cols = []
    for c in range(3):
        (g,) = torch.autograd.grad(rgb[:, c].sum(), mean, retain_graph=c < 2)
        cols.append(g)
    return torch.stack(cols, -1)


def _relu_kink(net, o, d, view, mean):
    """The ReLU-kink classifier of tests/test_gpu_render_tangent.py::_ill_conditioned at the ray's single sample: a hidden or
    view-layer pre-activation within KINK of 0, relative to its dot product's magnitude, from an fp32 recomputation of the field.
    (Sigma takes no part in a single sample's colour; the step and clip causes do not exist here.)"""
    from nerf_sampling_amd import ops

    with torch.no_grad():
        pts = o + d * mean[:, None]
        xe = ops.posenc(pts.contiguous(), 10)

        def lin(x, L):
            pre = x @ L.weight.T + L.bias
            rel = pre.abs() / (x.abs() @ L.weight.abs().T + L.bias.abs())
            return pre, (rel <= KINK).any(-1)

        near = torch.zeros(xe.shape[0], dtype=torch.bool, device=xe.device)
        h = xe
        skips = net._check_supported()
        for i, L in enumerate(net.pts_linears):
            pre, k = lin(h, L)
            near |= k
            h = torch.relu(pre)
            if i in skips:
                h = torch.cat([xe, h], -1)
        feat = h @ net.feature_linear.weight.T + net.feature_linear.bias
        _pre, k = lin(torch.cat([feat, ops.posenc(view.contiguous(), 4)], -1), net.views_linears[0])
        return near | k


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth", "shapes_fit"])
def test_jacobian_matches_autograd_of_the_fp32_chain(gpu_modules, scene):
    """Per ray |J - J_ref| <= 2^-12 (|J_ref| + 1) + 1e-6 (the rgb columns of test_gpu_render_tangent.py::_bound); rays at a ReLU
    kink are counted instead.  Measured on MI355X (rays / at a kink / past the bound / well-conditioned past the bound / worst
    well-conditioned ratio / median ratio):
        tiny_synth   480 / 13 / 0 / 0 / 0.038 / 0.0128
        lego_synth   480 / 65 / 0 / 0 / 0.064 / 0.0179
        shapes_fit   600 / 36 / 0 / 0 / 0.223 / 0.0089
    No ray of any set is past its bound, at a kink or not (the N = 2 test records at most 5 of 600)."""
    from nerf_sampling_amd import ops

    ops.set_compute_dtype("f32")
    m = gpu_modules(scene)
    o, d, view = _scene_rays(scene)
    mean = ops.depthnet_forward(m["depth"].packed("f32"), o, d).reshape(-1)
    Jref = _chain_jacobian(m, o, d, view, mean)
    _, J = _tangent(mean, m["fine"].packed("f16x3"), rays=(o, d, view))
    Jt = J["rgb"]
    finite_mean = torch.isfinite(mean)
    assert torch.isfinite(Jt[finite_mean]).all()
    ok = torch.isfinite(Jref).all(-1) & finite_mean
    ratio = ((Jt - Jref).abs() / (2.0 ** -12 * (Jref.abs() + 1.0) + 1e-6)).amax(-1)
    kink = _relu_kink(m["fine"], o, d, view, mean) & ok
    well = ratio[ok & ~kink]
    st = dict(rays=int(ratio.numel()), nonfinite=int((finite_mean & ~torch.isfinite(Jref).all(-1)).sum()), relu=int(kink.sum()), over=int((ratio[ok] > 1.0).sum()),
              well_over=int((well > 1.0).sum()), well_worst=round(float(well.max()), 3) if well.numel() else 0.0,
              median=round(float(ratio[ok].median()), 4))
    print(f"{scene}: {st}")
    assert st["nonfinite"] == 0, st
    assert st["well_over"] == 0, st                   # every ray past its bound sits at a kink
    assert st["over"] <= 0.02 * st["rays"], st        # ... and they are few
    assert st["median"] <= 0.2, st


def test_a_nan_depth_stays_in_its_ray(gpu_modules):
    from nerf_sampling_amd import ops

    m = gpu_modules("tiny_synth")
    H, W, K, c2w = _camera(5, 37)
    o, d, view = ops.get_rays(H, W, K, c2w)[:3]
    nf = m["fine"].packed("f16x3")
    R = o.shape[0]
    clean = torch.linspace(2.5, 5.5, R, device="cuda")
    bad = torch.zeros(R, dtype=torch.bool, device="cuda")
    bad[[0, 15, 16, 63, 64, 100, R - 1]] = True
    mean = torch.where(bad, torch.full_like(clean, float("nan")), clean)
    out0, J0 = _tangent(clean, nf, rays=(o, d, view))
    out1, J1 = _tangent(mean, nf, rays=(o, d, view))
    assert torch.isnan(out1["rgb"][bad]).all() and torch.isnan(J1["rgb"][bad]).all()
    for k in MAPS:
        _same(out1[k][~bad], out0[k][~bad], k)
        _same(J1[k][~bad], J0[k][~bad], ("J", k))
    for k in ("disp", "depth", "acc"):
        assert torch.equal(J1[k], torch.zeros_like(J1[k])), k
