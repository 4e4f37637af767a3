"""Gradients through multi-sample compositing and sample placement on the GPU (ns_raw2outputs_backward,
ns_place_samples_backward): the autograd wiring of DepthNetTrainer.raw2outputs and utils.sample_points_around_mean, the
kernel against float64 torch autograd of the oracle under the error model of tests/composite_backward_bounds.py, and the
DepthNet branch of render_rays_test (nerf_utils.py:836-865) end to end against torch-CPU autograd of the oracle."""

import copy

import pytest
import torch

import composite_backward_bounds as CBB
import composite_bounds as CB
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(scope="module")
def ops():
    from nerf_sampling_amd import ops as _ops

    return _ops


def _trainer(**over):
    from test_gpu_render import make_trainer

    return make_trainer(**over)


# ---- the autograd wiring ------------------------------------------------------------------------------------------------
def test_raw2outputs_at_64_samples_has_a_graph():
    tr = _trainer()
    g = torch.Generator().manual_seed(0)
    raw = torch.randn(32, 64, 4, generator=g).cuda().requires_grad_(True)
    z = (2.0 + torch.cumsum(torch.rand(32, 64, generator=g) * 0.05, -1)).cuda()
    d = torch.randn(32, 3, generator=g).cuda()
    out = tr.raw2outputs(raw, z, d, white_bkgd=True)
    for k in (0, 1, 2, 3, 5, 6):
        assert out[k].grad_fn is not None, k
    (out[0].sum() + out[1].sum() * 1e-3).backward()
    assert raw.grad is not None and bool(torch.isfinite(raw.grad).all()) and float(raw.grad.abs().sum()) > 0
    # with the pytest noise draws (sampling_trainer.py:188-193) too
    raw.grad = None
    out = tr.raw2outputs(raw, z, d, raw_noise_std=1.0, white_bkgd=False, pytest=True)
    out[0].sum().backward()
    assert raw.grad is not None and float(raw.grad.abs().sum()) > 0


@pytest.mark.parametrize("mode", ["uniform", "gaussian", "depth_only"])
def test_sample_points_around_mean_has_a_graph(ops, mode):
    from nerf_sampling_amd import utils

    g = torch.Generator().manual_seed(1)
    o, d = torch.randn(40, 3, generator=g).cuda(), torch.randn(40, 3, generator=g).cuda()
    mean = (3.0 + torch.rand(40, 1, generator=g)).cuda().requires_grad_(True)
    torch.cuda.manual_seed(5)
    pts, z = utils.sample_points_around_mean(o, d, mean, 32, mode, 0.1)
    assert pts.grad_fn is not None and z.grad_fn is not None
    # the same values as the call without a gradient
    torch.cuda.manual_seed(5)
    with torch.no_grad():
        pts0, z0 = utils.sample_points_around_mean(o, d, mean, 32, mode, 0.1)
    assert torch.equal(pts, pts0) and torch.equal(z, z0)
    (pts.sum() + z.sum()).backward()
    n = z.shape[1]
    exp = (d.sum(-1) + 1.0) * n                       # every sample moves with the mean (none clipped here)
    assert torch.allclose(mean.grad.reshape(-1), exp, rtol=1e-5, atol=1e-4)
    with pytest.raises(NotImplementedError, match="rays_o / rays_d"):
        utils.sample_points_around_mean(o, d.clone().requires_grad_(True), mean, 32, mode, 0.1)


def test_place_samples_backward_against_autograd(ops):
    """d mean against torch autograd of the oracle's placement: the clip's inclusive bounds (means at 2 and 6, a grid point
    landing on 2), the merged mean, a NaN mean."""
    R = 64
    g = torch.Generator().manual_seed(2)
    mean = 1.5 + 5.0 * torch.rand(R, 1, generator=g)
    mean[0], mean[1], mean[2], mean[3] = 2.0, 6.0, 2.1, float("nan")
    o, d = torch.randn(R, 3, generator=g), torch.randn(R, 3, generator=g)
    for mode, n in (("uniform", 2), ("uniform", 3), ("uniform", 32), ("uniform", 128), ("gaussian", 64), ("depth_only", 1)):
        noise = torch.randn(R, n - 1, generator=g) if mode == "gaussian" else None
        m = mean.clone().requires_grad_(True)
        _, zo = O.place_samples(o, d, m, n, mode, 0.1, noise)
        dz = torch.randn(zo.shape, generator=g)
        (zo * dz).sum().backward()
        mine = ops.place_samples_backward(mean.cuda(), dz.cuda(), mode, 0.1).cpu()
        exp = m.grad.reshape(-1)
        assert torch.equal(torch.isnan(mine), torch.isnan(exp)), mode
        assert torch.allclose(mine, exp, rtol=1e-5, atol=1e-5 * n, equal_nan=True), (mode, n, (mine - exp).abs().max())


# ---- the kernel against float64 autograd ----------------------------------------------------------------------------------
BWD_SWEEP = list(range(1, 71)) + [96, 127, 128, 129, 200, 1000]
LAYOUTS = {}
for _n in BWD_SWEEP:
    LAYOUTS.setdefault(CB.layout_name(_n), []).append(_n)


# Measured on MI355X, worst |err| / bound over each layout's sweep (d_raw, d_z, d_rays_d): single 0.58 / 0 / 0, sw2
# 0.57 / 0.28 / 0.13, sw4 0.56 / 0.50 / 0.19, sw8 0.58 / 1.00 / 0.13, sw16 0.63 / 0.50 / 0.17, sw32 0.63 / 0.53 / 0.14,
# sw64 0.58 / 1.00 / 0.10, chunks 0.60 / 0.50 / 0.09.  The two 1.00 are entries whose exp(-s) lies below 2^-126: the kernel
# gets exactly 0 there, which is the model's charge for the flush itself.


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_raw2outputs_backward_against_float64(ops, layout):
    """Every N of the layout, R = 3 (256 / SW) + 1 rays, with and without noise, white and black background, the upstream
    gradient of each output alone and of all six together."""
    worst = {}
    for N in LAYOUTS[layout]:
        R = CB.rays_for(N) if N <= 64 else 13
        for with_noise in (False, True):
            raw, z, d, noise = CB.make_inputs(R, N, 3000 + N, with_noise)
            rd, zd, dd = raw.cuda(), z.cuda(), d.cuda()
            nd = None if noise is None else noise.cuda()
            for white in (False, True):
                for s, which in enumerate(CBB.GRAD_SETS):
                    G = CBB.upstream(R, N, which, seed=N * 100 + s)
                    grads = [None if G[k] is None else G[k].cuda() for k in CBB.GRADS]
                    got = ops.raw2outputs_backward(rd, zd, dd, nd, white, grads)
                    stats = CBB.check(got, raw, z, d, noise, white, G)
                    for k, v in stats.items():
                        w = worst.setdefault(k, [0.0, 0.0])
                        w[0], w[1] = max(w[0], v[0]), max(w[1], v[1])
    print(f"\nraw2outputs backward {layout} (N = {LAYOUTS[layout][0]}..{LAYOUTS[layout][-1]}): worst |err| / bound, max |err|: "
          + ", ".join(f"{k} {v[0]:.3f} {v[1]:.2e}" for k, v in worst.items()))


def test_raw2outputs_backward_outputs_are_independent(ops):
    """Each of d_raw / d_z / d_rays_d alone is the same bits as all three together; nothing requested, nothing launched."""
    R, N = 300, 64
    raw, z, d, noise = CB.make_inputs(R, N, 7, True)
    G = CBB.upstream(R, N, CBB.GRADS, seed=7)
    args = (raw.cuda(), z.cuda(), d.cuda(), noise.cuda(), True, [G[k].cuda() for k in CBB.GRADS])
    full = ops.raw2outputs_backward(*args)
    for i in range(3):
        want = [j == i for j in range(3)]
        one = ops.raw2outputs_backward(*args, want=want)
        assert torch.equal(torch.nan_to_num(one[i]), torch.nan_to_num(full[i]))
        assert all(one[j] is None for j in range(3) if j != i)


def test_composite_function_matches_the_kernel(ops):
    """The autograd.Function hands its upstream gradients to the kernel unchanged; a raw of five channels (output_ch = 5
    networks) gets zeros in the fifth."""
    from nerf_sampling_amd.autograd import composite

    R, N = 100, 33
    raw, z, d, _ = CB.make_inputs(R, N, 9, False)
    raw5 = torch.cat([raw, torch.randn(R, N, 1)], -1).cuda().requires_grad_(True)
    zc, dc = z.cuda().requires_grad_(True), d.cuda().requires_grad_(True)
    rgb, disp, acc, depth, alphas, weights = composite(raw5, zc, dc, None, True)
    G = CBB.upstream(R, N, ("rgb", "depth", "weights"), seed=3)
    ((rgb * G["rgb"].cuda()).sum() + (depth * G["depth"].cuda()).sum() + (weights * G["weights"].cuda()).sum()).backward()
    grads = [G[k].cuda() if G[k] is not None else None for k in CBB.GRADS]
    exp = ops.raw2outputs_backward(raw5.detach()[..., :4], zc.detach(), dc.detach(), None, True, grads)
    for got, want in ((raw5.grad[..., :4], exp[0]), (zc.grad, exp[1]), (dc.grad, exp[2])):
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(), want.nan_to_num())
    assert bool((raw5.grad[..., 4] == 0).all())


# ---- the DepthNet branch end to end ---------------------------------------------------------------------------------------
# worst relative error over the DepthNet gradient tensors (82 on lego_synth, 26 on tiny_synth), over n = 2, 32, 64, 128,
# measured on MI355X per (scene, mode); the gate is 3x of it.  The largest, lego_synth gaussian at n = 64, comes from rays
# whose last sample's sigma lies near 0: it is composited with dist = 1e10, alpha = step(sigma), and an fp32 rounding
# difference of the field between the MFMA kernel and the CPU flips that step (the PSNR guard's case, ops.py).
MEASURED_E2E = {("tiny_synth", "uniform"): 2.5e-5, ("lego_synth", "uniform"): 3.6e-4,
                ("tiny_synth", "gaussian"): 7.1e-5, ("lego_synth", "gaussian"): 3.4e-3}


def _oracle_grads(m, rb, n, mode, noise, target):
    p = {k: v.clone().requires_grad_(True) for k, v in m["params"]["depth"].items()}
    o, d, view = rb[:, 0:3], rb[:, 3:6], rb[:, 8:11]
    mean = O.depthnet_forward(p, o, d)
    pts, z = O.place_samples(o, d, mean, n, mode, 0.1, noise)
    raw = O.run_network(m["params"]["fine"], pts, view)
    rgb = O.raw2outputs(raw, z, d, 0.0, True)[0]
    loss = ((rgb - target) ** 2).mean()
    loss.backward()
    return float(loss.detach()), p


@pytest.mark.parametrize("scene", ["tiny_synth", "lego_synth"])
@pytest.mark.parametrize("mode", ["uniform", "gaussian"])
@pytest.mark.parametrize("n", [2, 32, 64, 128])
def test_depthnet_branch_gradients_match_oracle_autograd(golden, gpu_modules, scene, mode, n):
    """depth_network -> sample_points_around_mean -> run_network -> raw2outputs with an image loss under autograd: every
    DepthNet gradient tensor against torch-CPU autograd of the oracle (f32), and render_rays_test's DepthNet branch under
    autograd gives the same gradients as the chain."""
    from nerf_sampling_amd import nerf_utils, ops, utils

    ops.set_compute_dtype("f32")
    m = dict(gpu_modules(scene))
    dn = copy.deepcopy(m["depth"])
    for p in dn.parameters():
        p.requires_grad_(True)
    tr = _trainer(n_depth_samples=n, sampling_mode=mode, distance=0.1)
    from test_gpu_render import render_kwargs

    kw = render_kwargs(tr, dict(m, depth=dn))
    rb = T(golden("render_rays_train")["ray_batch"])[:48]
    target = torch.rand(48, 3, generator=torch.Generator().manual_seed(4))
    o, d, view = (rb[:, a:b].contiguous().cuda() for a, b in ((0, 3), (3, 6), (8, 11)))
    # the chain
    torch.cuda.manual_seed(11)
    mean = dn(o, d)
    pts, z = utils.sample_points_around_mean(o, d, mean, n, mode, 0.1)
    raw = kw["network_query_fn"](pts, view, m["fine"])
    rgb = tr.raw2outputs(raw, z, d, white_bkgd=True)[0]
    loss = ((rgb - target.cuda()) ** 2).mean()
    loss.backward()
    mine = {k: v.grad.detach().clone() for k, v in dn.named_parameters()}
    # the same draws for the oracle (ops.place_samples: torch.randn(R, n - 1) on the device)
    noise = None
    if mode == "gaussian":
        torch.cuda.manual_seed(11)
        noise = torch.randn(48, n - 1, device="cuda").cpu()
    loss_o, p = _oracle_grads(m, rb, n, mode, noise, target)
    assert abs(float(loss.detach()) - loss_o) < 1e-4 * max(1.0, abs(loss_o))
    gate = 3.0 * MEASURED_E2E[(scene, mode)]
    worst = 0.0
    for name, g in mine.items():
        go = p[name].grad
        assert go is not None, name
        rel = float((g.cpu() - go).norm() / (go.norm() + 1e-12))
        worst = max(worst, rel)
        assert rel < gate, (name, rel, float(go.norm()))
    assert len(mine) == len(p)
    # render_rays_test's DepthNet branch under autograd (nerf_utils.py:836-865)
    for q in dn.parameters():
        q.grad = None
    torch.cuda.manual_seed(11)
    ret = nerf_utils.render_rays_test(rb.cuda(), **kw)
    loss2 = ((ret["depth_net_rgb_map"] - target.cuda()) ** 2).mean()
    loss2.backward()
    same = 0.0
    for name, q in dn.named_parameters():
        assert q.grad is not None, name
        same = max(same, float((q.grad - mine[name]).norm() / (mine[name].norm() + 1e-12)))
    assert same < 1e-6, same
    print(f"{scene} {mode} n={n}: worst relative gradient error over {len(mine)} tensors = {worst:.2e} "
          f"(gate {gate:.1e}); render_rays_test vs chain {same:.1e}")
