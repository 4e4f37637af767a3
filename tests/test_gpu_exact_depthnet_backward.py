"""The DepthNet's training pass against the float64 transposed chain on exactly representable networks (needs a GPU).

DepthNet.forward under autograd (autograd.DepthNetFunction: about forty ns_gemm_fused / ns_gemm_fused_batched launches, layer
outputs in column windows of shared buffers, `dact` epilogues on the layer below's saved output, bias gradients as row sums of a
transposed operand) and z.backward(dz) run on the networks, rays and integer dz of tests/exact_depthnet_backward.py.  Every forward
sum is exact there and no mask can differ (tests/test_exact_depthnet_backward_host.py proves it for every case used here), so z is
held to exact_depthnet's gate and every entry of every dW and db to its own derived bound around the float64 value: no norm over
a tensor, no other kernel on the other side, exact zeros where the reference has exact zeros, NaN nowhere.
"""
import numpy as np
import pytest
import torch

import exact_depthnet as X
import exact_depthnet_backward as B
from nerf_sampling_amd import ops
from nerf_sampling_amd.depth_net import DepthNet

pytestmark = pytest.mark.gpu

NAMES = list(B.TRAIN_NETWORKS)
_modules = {}
_device = {}


def _pool():
    if not _device:
        P = X.pool()
        _device.update(o=torch.from_numpy(P["o"]).float().cuda(), d=torch.from_numpy(P["d"]).float().cuda())
    return _device


def _module(name, head):
    """The package's DepthNet holding the network's weights and this head, on the device, every parameter trainable."""
    net = B.network(name)
    if name not in _modules:
        mod = DepthNet(hidden_sizes=net["hidden"], cat_hidden_sizes=net["cat"])
        mod.load_state_dict(X.state_dict(net, "main"))
        _modules[name] = [mod.cuda(), "main"]
    mod, loaded = _modules[name]
    if loaded != head:
        hw, hb = net["heads"][head]
        with torch.no_grad():
            mod.to_depth[0].weight.copy_(torch.from_numpy(hw).float())
            mod.to_depth[0].bias.copy_(torch.from_numpy(hb).float())
        _modules[name][1] = head
    assert all(p.requires_grad and p.is_cuda for p in mod.parameters())
    assert [k for k, _ in mod.named_parameters()] == B.param_names(net)
    return mod


def _rays(c):
    i = torch.from_numpy(c["rays"]).cuda()
    return _pool()["o"][i].contiguous(), _pool()["d"][i].contiguous()


def _run(name, c, o=None, d=None):
    """z = net(o, d), z.backward(dz): (z [R, 1], name -> gradient) as device tensors."""
    mod = _module(name, c["head"])
    mod.near, mod.far, mod.sphere_radius = c["near"], c["far"], torch.tensor([c["radius"]])
    if o is None:
        o, d = _rays(c)
    mod.zero_grad(set_to_none=True)
    z = mod(o, d)
    assert z.grad_fn is not None and z.shape == (c["R"], 1) and z.dtype == torch.float32
    z.backward(torch.from_numpy(c["dz"]).float().cuda())
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in mod.named_parameters()}
    mod.zero_grad(set_to_none=True)
    return z.detach(), grads


def _same_bits(a, b, what):
    za, ga = a
    zb, gb = b
    assert torch.equal(za.view(torch.int32), zb.view(torch.int32)), f"{what}: z"
    for k in ga:
        assert torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)), f"{what}: {k}"


@pytest.mark.parametrize("radius", X.RADII)
def test_sphere_intersect_returns_the_pools_coordinates(radius):
    """the precondition: ops.sphere_intersect, from which the training pass takes the six coordinates, is exact on the pool as
    the inference kernels' own formula is"""
    own = torch.from_numpy(np.flatnonzero(X.pool()["radius"] == radius)).cuda()
    _, pts = ops.sphere_intersect(_pool()["o"][own], _pool()["d"][own], radius)
    want = torch.from_numpy(X.pool()["x"][own.cpu().numpy()]).float().cuda()
    assert torch.equal(pts.reshape(-1, 6), want)


@pytest.mark.parametrize("name", NAMES)
def test_every_case(name):
    """z within the gate and every gradient entry within its bound, on every row of exact_depthnet_backward.cases"""
    worst_z = worst_g = 0.0
    for key in B.cases(name):
        c = B.case(name, key)
        z, grads = _run(name, c)
        verdicts, _ = B.compare(z.cpu().numpy(), {k: g.cpu().numpy() for k, g in grads.items()}, c["ref"])
        ratios = {k: v.worst for k, v in verdicts.items()}
        print(f"{name} {key}: worst |err| / bound: z {ratios['z']:.3f}, gradients {max(v for k, v in ratios.items() if k != 'z'):.3f}")
        bad = B.failures(verdicts, c["ref"])
        assert not bad, f"{name} {key}: {bad}"
        worst_z, worst_g = max(worst_z, ratios.pop("z")), max(worst_g, max(ratios.values()))
    print(f"{name}: worst |err| / bound over all cases: z {worst_z:.3f}, gradients {worst_g:.3f}")


def _picked(name):
    """A large case of the main head, a case of radius 2, and one of a chain head."""
    keys = B.cases(name)
    return [next(k for k in keys if k[0] == "main" and k[1] == 1300), next(k for k in keys if k[0] == "main" and k[2] == 2.0),
            next(k for k in keys if k[0] != "main" and k[1] >= 33)]


@pytest.mark.parametrize("name", NAMES)
def test_training_z_agrees_with_the_inference_kernel(name):
    """the same tensors packed for depthnet_kernel (f32): both paths agree on the parameter order and on near, far and radius"""
    net = B.network(name)
    for key in _picked(name):
        c = B.case(name, key)
        w, b = X.tensors(net, c["head"])
        handle = ops.pack_depthnet(w, b, net["hidden"], net["cat"], "f32")
        o, d = _rays(c)
        z_inf = ops.depthnet_forward(handle, o, d, c["near"], c["far"], c["radius"])
        z, _ = _run(name, c)
        assert z_inf.shape == z.shape and not torch.isnan(z_inf).any()
        assert float((z - z_inf).abs().max()) <= 2 * X.gate(c["near"], c["far"]), (name, key)


@pytest.mark.parametrize("name", NAMES)
def test_strided_rays_a_second_call_and_a_side_stream_give_the_same_bits(name):
    for key in _picked(name):
        c = B.case(name, key)
        first = _run(name, c)
        _same_bits(_run(name, c), first, f"{name} {key}: a second call")
        o, d = _rays(c)
        batch = torch.full((c["R"], 11), 7.0, dtype=torch.float32, device="cuda")      # rays as the trainer holds them
        batch[:, 0:3], batch[:, 3:6] = o, d
        assert not batch[:, 3:6].is_contiguous()
        _same_bits(_run(name, c, batch[:, 0:3], batch[:, 3:6]), first, f"{name} {key}: column slices of a ray batch")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = _run(name, c)
        torch.cuda.current_stream().wait_stream(side)
        _same_bits(got, first, f"{name} {key}: on a side stream")


@pytest.mark.parametrize("name", ["w40n3", "w24n1"])
def test_no_rays(name):
    """R = 0: z is [0, 1] and the backward gives zeros of every parameter's shape, as torch does, without a launch"""
    mod = _module(name, "main")
    mod.zero_grad(set_to_none=True)
    o = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    z = mod(o, o.clone())
    assert z.shape == (0, 1) and z.dtype == torch.float32 and z.grad_fn is not None
    z.backward(torch.empty((0, 1), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    for k, p in mod.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32 and not p.grad.any(), k
    mod.zero_grad(set_to_none=True)
