"""The field fit on HIP: autograd.NerfFunction (forward and the gradients of every parameter tensor) and trainers.FieldFitter,
against torch-CPU autograd of the oracle.

Gate of every gradient tensor: relative L2 < 2e-3, the figure test_depthnet_training_gradients_match_oracle_autograd uses for
the same comparison (fp32 GEMMs in another summation order; a ReLU whose pre-activation is within rounding of zero may flip).
Each test prints its worst tensor's figure before it asserts.

The chain itself -- which columns, which mask, which operands each GEMM receives -- is pinned bit for bit by
tests/test_gpu_exact_field_backward.py on exactly representable networks; the gate here stays for real scenes, whose ReLUs sit
near zero."""

import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

GATE = 2e-3


def _net(params, D, W, skips=(4,), use_viewdirs=True, output_ch=4):
    from nerf_sampling_amd.run_nerf_helpers import NeRF

    net = NeRF(D=D, W=W, input_ch=63, input_ch_views=27, output_ch=output_ch, skips=list(skips), use_viewdirs=use_viewdirs)
    net.load_state_dict({k: v.clone() for k, v in params.items()})
    return net.to("cuda")


def _variants():
    from nerf_sampling_amd import synthetic as S

    out = {}
    for scene in ("tiny_synth", "lego_synth"):
        cfg = O.SCENES[scene]["fine"]
        out[scene] = (O.make_scene(scene)["fine"], dict(D=cfg["D"], W=cfg["W"], skips=(4,)))
    kw = dict(hidden_gain=6 ** 0.5, spectral_decay=True)
    out["skips025"] = (S.make_nerf_params(301, D=8, W=64, skips=(0, 2, 5), **kw), dict(D=8, W=64, skips=(0, 2, 5)))
    out["noview5"] = (S.make_nerf_params(302, D=4, W=64, use_viewdirs=False, output_ch=5, **kw),
                      dict(D=4, W=64, use_viewdirs=False, output_ch=5))
    out["noview4"] = (S.make_nerf_params(303, D=4, W=64, use_viewdirs=False, output_ch=4, **kw),
                      dict(D=4, W=64, use_viewdirs=False, output_ch=4))
    out["w97"] = (S.make_nerf_params(304, D=5, W=97, skips=(2,), **kw), dict(D=5, W=97, skips=(2,)))
    return out


_CACHE = {}


def _variant(name):
    if not _CACHE:
        _CACHE.update(_variants())
    return _CACHE[name]


def _inputs(R, N, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(R, N, 3, generator=g) * 4 - 2
    view = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    return pts, view


def _compare(named, oracle_p, tag):
    worst = 0.0
    for name, mod_p in named:
        g, go = mod_p.grad, oracle_p[name].grad
        if go is None:        # a tensor the forward never reads (views_linears of a network without view directions)
            assert g is None or not bool(g.abs().sum() > 0), (tag, name, "gradient of an unused tensor")
            continue
        assert g is not None, (tag, name)
        g = g.cpu()
        rel = float((g - go).norm() / (go.norm() + 1e-12))
        worst = max(worst, rel)
        assert rel < GATE, (tag, name, rel, float(go.norm()))
        assert bool(g.abs().sum() > 0) or not bool(go.abs().sum() > 0), (tag, name, "all-zero gradient")
    return worst


@pytest.mark.parametrize("R,N", [(37, 5), (64, 64)])
@pytest.mark.parametrize("name", ["tiny_synth", "lego_synth", "skips025", "noview5", "noview4", "w97"])
def test_forward_and_parameter_gradients(name, R, N):
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.autograd import nerf_forward_train

    params, kw = _variant(name)
    net = _net(params, **kw)
    use_view = kw.get("use_viewdirs", True)
    pts, view = _inputs(R, N, 7 * R + N)
    raw = nerf_forward_train(net, pts.cuda(), view.cuda() if use_view else None)
    # forward: against the inference kernel on an f32 handle of the same module, at that handle's own gate
    ref = ops.nerf_forward(net.packed("f32"), pts.cuda(), view.cuda() if use_view else None)
    assert raw.shape == ref.shape
    scale = ref.abs().reshape(-1, ref.shape[-1]).max(0).values
    err = ((raw.detach() - ref).abs().reshape(-1, ref.shape[-1]).max(0).values / scale).max()
    print(f"NerfFunction forward {name} {R}x{N}: max err / channel scale {float(err):.2e}")
    assert float(err) < 2e-5
    g = torch.randn(raw.shape, generator=torch.Generator().manual_seed(11))
    raw.backward(g.cuda())
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    raw_o = O.run_network(p, pts, view if use_view else None, skips=tuple(kw.get("skips", (4,))))
    assert float((raw.detach().cpu() - raw_o.detach()).abs().max()) < 1e-3 * float(raw_o.detach().abs().max())
    raw_o.backward(g)
    worst = _compare([(k, q) for k, q in net.named_parameters() if k in p], p, name)
    assert {k for k, _ in net.named_parameters()} >= set(p), "every oracle tensor has a module parameter"
    print(f"NerfFunction gradients {name} {R}x{N}: worst relative L2 over {len(p)} tensors = {worst:.2e}")


def test_points_gradient_only_on_request():
    from nerf_sampling_amd.autograd import NerfInputGrad, nerf_forward_train

    params, kw = _variant("tiny_synth")
    net = _net(params, **kw)
    pts, view = _inputs(37, 5, 3)
    g = torch.randn(37, 5, 4, generator=torch.Generator().manual_seed(5)).cuda()
    a = pts.cuda().requires_grad_(True)
    nerf_forward_train(net, a, view.cuda()).backward(g)
    b = pts.cuda().requires_grad_(True)
    NerfInputGrad.apply(b, view.cuda(), net).backward(g)
    assert torch.equal(a.grad, b.grad), "the same grad-input chain as NerfInputGrad"


# ---- the fit step ------------------------------------------------------------------------------------------------------------
def _batch(H=8, W=8):
    from nerf_sampling_amd import analytic_scene, ops

    poses = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poses.npz"))["render_poses"]
    _, K = O.blender_intrinsics(H, W)
    o, d, _ = ops.get_rays(H, W, K, torch.tensor(poses[3][:3, :4]))
    target, _, _ = analytic_scene.raycast(o.cpu(), d.cpu())
    return torch.stack([o, d], 0), target.cuda()


def _fitter(shared=False):
    from nerf_sampling_amd.trainers import FieldFitter

    scene, cfg = O.make_scene("tiny_synth"), O.SCENES["tiny_synth"]
    coarse = _net(scene["coarse"], cfg["coarse"]["D"], cfg["coarse"]["W"])
    fine = coarse if shared else _net(scene["fine"], cfg["fine"]["D"], cfg["fine"]["W"])
    ff = FieldFitter(coarse, fine, N_samples=8, N_importance=8, perturb=0.0, raw_noise_std=0.0, white_bkgd=True, lindisp=False)
    return ff, scene


def _oracle_loss(p_c, p_f, rays, target, info):
    o, d = rays[0].cpu(), rays[1].cpu()
    view = d / torch.norm(d, dim=-1, keepdim=True)
    loss = 0.0
    for p, z in ((p_c, info["z0"].cpu()), (p_f, info["z"].cpu())):
        raw = O.run_network(p, o[:, None] + d[:, None] * z[..., None], view)
        rgb = O.raw2outputs(raw, z, d, 0.0, True)[0]
        loss = loss + ((rgb - target.cpu()) ** 2).mean()
    return loss


@pytest.mark.parametrize("shared", [False, True])
def test_fit_step_gradients_match_the_oracle(shared):
    ff, scene = _fitter(shared)
    rays, target = _batch()
    loss, info = ff.forward_loss(rays, target)
    loss.backward()
    p_c = {k: v.clone().requires_grad_(True) for k, v in scene["coarse"].items()}
    p_f = p_c if shared else {k: v.clone().requires_grad_(True) for k, v in scene["fine"].items()}
    loss_o = _oracle_loss(p_c, p_f, rays, target, info)
    loss_o.backward()
    assert abs(float(loss) - float(loss_o)) < 1e-4 * max(1.0, abs(float(loss_o)))
    worst = _compare([(k, q) for k, q in ff.network_fn.named_parameters() if k in p_c], p_c, "coarse")
    if not shared:
        worst = max(worst, _compare([(k, q) for k, q in ff.network_fine.named_parameters() if k in p_f], p_f, "fine"))
    print(f"fit step (shared={shared}): loss {float(loss):.6f} vs oracle {float(loss_o):.6f}, worst relative L2 = {worst:.2e}")


def test_twenty_steps_on_a_fixed_batch_reduce_the_loss():
    ff, _ = _fitter()
    rays, target = _batch()
    losses = [float(ff.step(rays, target)[0]) for _ in range(20)]
    print("fit losses:", " ".join(f"{v:.5f}" for v in losses))
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < losses[0]
    assert ff.global_step == 20


def test_checkpoint_reloads_bit_for_bit_and_renders_fresh(tmp_path):
    from nerf_sampling_amd import ops

    ff, _ = _fitter()
    rays, target = _batch()
    H = W = 16
    _, K = O.blender_intrinsics(H, W)
    c2w = O.pose_spherical(30.0, -30.0, 4.0)[:3, :4]

    def frame(coarse, fine):
        out = ops.render_rays_hierarchical(coarse.packed("f32"), fine.packed("f32"), camera=(H, W, K, c2w, 0, H), n_coarse=8,
                                           n_importance=8, lindisp=False, white_bkgd=True)
        return out["rgb"].clone()

    before = frame(ff.network_fn, ff.network_fine)       # packs both networks: a stream that the fit must not leave in place
    ff.fit(lambda: (rays, target), 3, basedir=str(tmp_path), expname="fit", i_print=0)
    path = tmp_path / "fit" / "000003.tar"
    assert path.exists()
    ckpt = torch.load(str(path), weights_only=True, map_location="cuda")
    assert ckpt["global_step"] == 3 and "optimizer_state_dict" in ckpt
    cfg = O.SCENES["tiny_synth"]
    fresh = {}
    for which, key in (("coarse", "network_fn_state_dict"), ("fine", "network_fine_state_dict")):
        fresh[which] = _net(ckpt[key], cfg[which]["D"], cfg[which]["W"])
    for mod, new in ((ff.network_fn, fresh["coarse"]), (ff.network_fine, fresh["fine"])):
        sd, nd = mod.state_dict(), new.state_dict()
        assert set(sd) == set(nd)
        for k in sd:
            assert torch.equal(sd[k], nd[k]), k
    after = frame(ff.network_fn, ff.network_fine)
    assert torch.equal(after, frame(fresh["coarse"], fresh["fine"])), "a stale packed stream was rendered"
    assert not torch.equal(after, before), "three steps must change the frame"
