"""render_rays' ``fused_step`` option on the GPU -- the DepthNet branch of the training step as one tangent-kernel call
(autograd.SingleSampleTangentRender) and the target pass as one hierarchical-renderer call -- against the default path: the
same targets and depths bit for bit, the same colours and DepthNet gradients within the f16x3 field's error, a captured step
that equals the eager one, and a loop that still learns."""

import copy

import pytest
import torch

from oracle import nerf_oracle as O
from test_gpu_training import _kwargs

pytestmark = pytest.mark.gpu

# relative L2 error of the whole DepthNet gradient against the default path's: 3 x the value measured on the first run
# (measured at perturb = 0 / 1: lego_synth 2.13e-5 / 2.09e-5, the fitted scene 3.05e-6 / 3.04e-6; max |rgb - rgb_default| 6.0e-7
# and 1.3e-6)
GRAD_GATE = {"lego_synth": 6.4e-5, "shapes_fit": 9.2e-6}


def _batch(scene):
    """1024 rays as _optimization_step takes them, [2, 1024, 3]: a 32 x 32 image of a synthetic scene, or a 32 x 32 window at the
    middle of one 800 x 800 spiral pose of the fitted scene (rays through the object)"""
    from nerf_sampling_amd import ops

    if scene != "shapes_fit":
        H = W = 32
        _, K = O.blender_intrinsics(H, W)
        o, d, _ = ops.get_rays(H, W, K, O.pose_spherical(25.0, -30.0, 4.0)[:3, :4])
        return H, W, K, torch.stack([o, d], 0)
    H = W = 800
    _, K = O.blender_intrinsics(H, W)
    o, d, _ = ops.get_rays(H, W, K, O.render_poses(40)[7][:3, :4], 384, 416)
    cols = torch.arange(384, 416, device="cuda")
    idx = (torch.arange(32, device="cuda")[:, None] * W + cols[None]).reshape(-1)
    return H, W, K, torch.stack([o[idx], d[idx]], 0)


def _setup(gpu_modules, scene, **over):
    from nerf_sampling_amd import nerf_utils, ops

    ops.set_compute_dtype("f32")
    m = dict(gpu_modules(scene))
    m["depth"] = copy.deepcopy(m["depth"])
    for p in m["depth"].parameters():
        p.requires_grad_(True)
    tr, kw = _kwargs(m, **over)
    nerf_utils.standard_query_fn(kw["network_query_fn"])
    kw.update(near=2.0, far=6.0, ndc=False)
    return m, tr, kw


@pytest.mark.parametrize("scene", ["lego_synth", "shapes_fit"])
def test_losses_and_depthnet_gradients_match_the_default_path(gpu_modules, scene):
    from nerf_sampling_amd import nerf_utils
    from nerf_sampling_amd.run_nerf_helpers import img2mse

    m, tr, kw = _setup(gpu_modules, scene)
    H, W, K, batch_rays = _batch(scene)
    target = torch.rand(1024, 3, generator=torch.Generator().manual_seed(5)).cuda()
    params = [p for p in m["depth"].parameters()]
    errs = {}
    for perturb in (0.0, 1.0):
        runs = {}
        for fused in (False, True):
            torch.manual_seed(11)
            rgb, _disp, extras = nerf_utils.render(H, W, K, chunk=1024 * 32, rays=batch_rays, retraw=True,
                                                   **dict(kw, perturb=perturb, fused_step=fused))
            assert ("raw" in extras) == (not fused)
            loss = img2mse(rgb, target) + torch.nn.functional.mse_loss(extras["depth_net_z_vals"], extras["max_z_vals"])
            runs[fused] = (rgb.detach(), extras, torch.autograd.grad(loss, params), float(loss.detach()))
        (rgb0, ex0, g0, l0), (rgb1, ex1, g1, l1) = runs[False], runs[True]
        for k in ("max_z_vals", "depth_net_z_vals"):
            assert ex0[k].shape == ex1[k].shape and torch.equal(ex0[k].view(torch.int32), ex1[k].view(torch.int32)), (perturb, k)
        for k in ("depth_net_pts", "max_pts"):
            assert torch.equal(ex0[k], ex1[k]), (perturb, k)
        rgb_err = float((rgb1 - rgb0).abs().max())
        num = sum(float(((a - b) ** 2).sum()) for a, b in zip(g1, g0)) ** 0.5
        den = sum(float((b ** 2).sum()) for b in g0) ** 0.5
        errs[perturb] = (rgb_err, num / den, l0, l1)
        assert all(torch.isfinite(g).all() for g in g1)
    print(f"{scene}: per perturb (max |rgb - rgb_default|, relative L2 error of the DepthNet gradient, losses) {errs}")
    for perturb, (rgb_err, rel, _l0, _l1) in errs.items():
        assert rgb_err < 1e-4, (perturb, errs)            # the project's fp32 gate: exact-fp32 field there, f16x3 here
        assert rel < GRAD_GATE[scene], (perturb, errs)


def test_graphed_fused_step_equals_eager_fused_step(gpu_modules):
    """Six steps with the option on (two eager warm-up steps, the capture, four replays; a learning-rate change before the
    fifth): losses and DepthNet weights of trainers.GraphedDepthNetStep bit-identical to six eager steps; ten further replays
    leave every loss and weight finite."""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.autograd import HipAdam

    H = W = 24
    _, K = O.blender_intrinsics(H, W)
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randint(0, H * W, (128,), generator=g).cuda(), torch.rand(128, 3, generator=g).cuda()) for _ in range(16)]
    results = {}
    for mode in ("eager", "graph"):
        m, tr, kw = _setup(gpu_modules, "tiny_synth")
        kw["fused_step"] = True
        tr.H, tr.W, tr.K = H, W, K
        o, d, _ = ops.get_rays(H, W, K, O.pose_spherical(20.0, -30.0, 4.0)[:3, :4])
        opt = HipAdam(list(m["depth"].parameters()), lr=1e-3)
        opt.use_device_step()
        step = (tr.graphed_optimization_loop(opt, kw) if mode == "graph"
                else (lambda rays, i, tgt: tr.core_optimization_loop(opt, kw, rays, i, tgt)))
        losses = []
        for i, (idx, tgt) in enumerate(batches[:6]):
            if i == 4:
                opt.param_groups[0]["lr"] = 5e-4
            loss, dn_loss, psnr, _ = step(torch.stack([o[idx], d[idx]], 0), i, tgt)
            losses.append((float(loss), float(dn_loss), float(psnr)))
        results[mode] = (losses, [p.detach().clone() for p in m["depth"].parameters()])
        if mode == "graph":
            assert step.graph is not None and step.calls == 6
            assert any(getattr(w, "dtype", None) == "f16x3" for w in step._keep)
            for i, (idx, tgt) in enumerate(batches[6:]):
                loss, dn_loss, _psnr, _ = step(torch.stack([o[idx], d[idx]], 0), 6 + i, tgt)
                assert torch.isfinite(loss).all() and torch.isfinite(dn_loss).all(), i
            assert step.calls == 16
            assert all(torch.isfinite(p).all() for p in m["depth"].parameters())
    (le, pe), (lg, pg) = results["eager"], results["graph"]
    assert le == lg, (le, lg)
    assert all(torch.equal(a, b) for a, b in zip(pe, pg))


def test_core_optimization_loop_reduces_loss_with_fused_step(gpu_modules):
    """tests/test_gpu_training.py::test_core_optimization_loop_reduces_loss with the option on, under that test's own criterion"""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.autograd import HipAdam

    m, tr, kw = _setup(gpu_modules, "tiny_synth")
    kw["fused_step"] = True
    H = W = 24
    _, K = O.blender_intrinsics(H, W)
    tr.H, tr.W, tr.K = H, W, K
    o, d, _ = ops.get_rays(H, W, K, O.pose_spherical(20.0, -30.0, 4.0)[:3, :4])
    batch_rays = torch.stack([o[100:356], d[100:356]], 0)
    target = torch.rand(256, 3, generator=torch.Generator().manual_seed(7)).cuda()
    opt = HipAdam(list(m["depth"].parameters()), lr=1e-3)
    fine_before = [p.clone() for p in m["fine"].parameters()]
    losses = []
    for i in range(8):
        loss, dn_loss, psnr, _ = tr.core_optimization_loop(opt, kw, batch_rays, i, target)
        losses.append(float(dn_loss))
    print("depth_net_loss (fused_step):", [round(x, 5) for x in losses])
    assert losses[-1] < losses[0]
    assert all(torch.equal(a, b) for a, b in zip(fine_before, m["fine"].parameters()))
