"""Every DepthNet kernel against the float64 chain on exactly representable networks (needs a GPU).

The networks of tests/exact_depthnet.py have weights, inputs and activations that every operand type holds exactly and sums
that are exact in fp32 in any order (tests/test_exact_depthnet_host.py proves it for every network and operand type used
here), and their rays are ones on which the kernels' own ray-sphere arithmetic never rounds.  So the head's sum is the
float64 value for the k-major fp32 kernel, the 16x16x32 bf16, f16 and split-f16 kernels, the generated production streams
and the mixed-operand kernel alike; only the sigmoid and the near/far mix remain, and z is held to
|z - z64| <= 8 U max(|near|, |far|), U = 2^-24, on every ray: no share is forgiven, and no other kernel stands on the other
side of the comparison.  A negative pre-activation occurs in the chain units only, whose every step the reference rounds
as the operand type's LeakyReLU rule says; the chains' heads read them one at a time.

Those networks give every sine and cosine weight zero.  The probes at the end hold the three in-kernel embeddings, column by
column, and the fold's products over them to the allowances derived in exact_depthnet's docstring.
"""
import numpy as np
import pytest
import torch

import exact_depthnet as X
from nerf_sampling_amd import ops

pytestmark = pytest.mark.gpu

_device = {}
_packed = {}


def _pool():
    if not _device:
        P = X.pool()
        _device.update(o=torch.from_numpy(np.concatenate([P["o"], P["miss_o"]])).float().cuda(),
                       d=torch.from_numpy(np.concatenate([P["d"], P["miss_d"]])).float().cuda(), n=len(P["o"]))
    return _device


def _handle(net, key, head, dtype):
    if (key, head, dtype) not in _packed:
        w, b = X.tensors(net, head)
        _packed[key, head, dtype] = ops.pack_depthnet(w, b, net["hidden"], net["cat"], dtype)
    return _packed[key, head, dtype]


_reference = {}


def _want(net, key, head, dtype, near, far):
    """z64 on every pool ray, and NaN on the eight rays behind them that miss (cached for the module)."""
    k = (key, head, dtype, near, far)
    if k not in _reference:
        if (key, dtype) not in _reference:
            _reference[key, dtype] = X.trunk(net, dtype, X.pool()["x12"])
        z = X.depth(X.head_sum(net, head, _reference[key, dtype]), near, far)
        _reference[k] = np.concatenate([z, np.full(8, np.nan)])
    return _reference[k]


def _run(net, key, head, dtype, idx, radius, near, far, what, runs=2):
    """the rays idx (pool rows; those past the pool's end miss) through ops.depthnet_forward, `runs` times; returns the worst
    |err| / gate"""
    P = _pool()
    i = torch.from_numpy(idx).cuda()
    o, d = P["o"][i].contiguous(), P["d"][i].contiguous()
    want = _want(net, key, head, dtype, near, far)[idx]
    worst = 0.0
    for run in range(runs):
        z = ops.depthnet_forward(_handle(net, key, head, dtype), o, d, near, far, radius)
        assert z.shape == (len(idx), 1) and z.dtype == torch.float32
        ratio, ray = X.worst_ratio(z.cpu().numpy(), want, near, far)
        print(f"{what} run {run}: worst |err| / gate = {ratio:.3f}")
        assert ratio <= 1.0, (f"{what} run {run}: ray {ray} of {len(idx)} (pool ray {idx[ray]}, ray % 16, 32, 64, 128, 256 = {ray % 16}, "
                              f"{ray % 32}, {ray % 64}, {ray % 128}, {ray % 256}): got {float(z[ray, 0])!r}, expected {want[ray]!r}, "
                              f"{ratio} gates")
        worst = max(worst, ratio)
    return worst


def _every_head_and_count(net, key, dtype, what=""):
    worst = 0.0
    for near, far in X.NEAR_FAR:
        for k, head in enumerate(net["heads"]):
            live = None
            if head != "main":      # a chain's few rays: ones on which it is not zero, so that it takes its negative branch in every other layer
                _want(net, key, head, dtype, near, far)
                live = X.head_sum(net, head, _reference[key, dtype]) != 0
            for R in X.RAY_COUNTS:
                idx = X.ray_indices(R, 3.0, seed=R + 16 * k, among=live if R < 100 else None)
                worst = max(worst, _run(net, key, head, dtype, idx, 3.0, near, far, f"{key} {dtype} {what}{head} R={R} near={near}"))
            # the production radius: its 36 rays, and the rays that miss scattered among them: NaN there and nowhere else
            idx = X.ray_indices(77, 2.0, seed=7 + k)
            idx[[0, 5, 16, 17, 33, 48, 63, 76]] = _pool()["n"] + np.arange(8)
            worst = max(worst, _run(net, key, head, dtype, idx, 2.0, near, far, f"{key} {dtype} {what}{head} radius 2 with misses near={near}"))
        idx = X.ray_indices(300, 3.0, seed=8)
        idx[::37] = _pool()["n"] + np.arange(len(idx[::37])) % 8
        worst = max(worst, _run(net, key, "main", dtype, idx, 3.0, near, far, f"{key} {dtype} {what}radius 3 with misses near={near}"))
    print(f"{key} {dtype} {what}: worst |err| / gate = {worst:.3f}")


CASES = [(name, dtype) for name in X.NETWORKS for dtype in X.dtypes_of(name)]


@pytest.mark.parametrize("name,dtype", CASES)
def test_every_network_head_and_ray_count(name, dtype):
    """ray counts around every tile, wave and workgroup size (16 and 32 rays a tile, 128 and 256 a group); every launch twice:
    the weight ring's phase must not depend on the launch before"""
    _every_head_and_count(X.network(name), name, dtype)


@pytest.mark.parametrize("dtype", ["f16", "f16x3"])
def test_production_network_on_the_generic_kernels(dtype):
    """the production shape through the compiled layers instead of the generated streams"""
    with ops.debug_switch(generic_kernels=1):
        _every_head_and_count(X.network(X.PROD), X.PROD, dtype, what="generic ")


@pytest.mark.parametrize("dtype", X.DTYPES)
def test_two_groups_per_workgroup(dtype):
    """more rays than one pass of every compute unit takes: some workgroup walks two groups of 128 or 256 rays"""
    net = X.network(X.PROD)
    R = 256 * int(ops._lib.load().ns_device_cu_count()) + 300
    assert 300 < R < 2 ** 20
    idx = X.ray_indices(R, 3.0, seed=5)
    idx[::997] = _pool()["n"]
    _run(net, X.PROD, "main", dtype, idx, 3.0, 2.0, 6.0, f"prod {dtype} R={R}")
    with ops.debug_switch(generic_kernels=1):
        _run(net, X.PROD, "main", dtype, idx, 3.0, 2.0, 6.0, f"prod {dtype} generic R={R}", runs=1)


REMAINDER_CASES = [(name, dtype, layer) for name in X.REMAINDER_NETWORKS for dtype in X.REMAINDER_DTYPES
                   if dtype in X.dtypes_of(name) for layer in X.remainder_layers(name, dtype)]


@pytest.mark.parametrize("name,dtype,layer", REMAINDER_CASES)
def test_split_operands(name, dtype, layer):
    """one layer's weights are w (1 + 2^-12) = hi + lo: that layer needs W_lo x_hi, every split layer behind it W_hi x_lo"""
    net = X.remainder_network(name, layer)
    key = (name, "remainder", layer)
    for near, far in X.NEAR_FAR:
        _run(net, key, "main", dtype, X.ray_indices(257, 3.0, seed=3), 3.0, near, far, f"{key} {dtype} near={near}")
        if name == X.PROD and dtype != "f16m":
            with ops.debug_switch(generic_kernels=1):
                _run(net, key, "main", dtype, X.ray_indices(257, 3.0, seed=3), 3.0, near, far, f"{key} {dtype} generic near={near}", runs=1)
    for k in [k for k in _packed if k[0] == key]:          # used once: not kept
        del _packed[k]


# ---- the sines and cosines, column by column ------------------------------------------------------------------------
_probe = {}


def _probe_inputs():
    if not _probe:
        o, d = X.probe_rays()
        e = X.embedding64(o, d, X.kernel_x6(o, d, X.PROBE_RADIUS))
        _probe.update(o=torch.from_numpy(o).cuda(), d=torch.from_numpy(d).cuda(), e=e)
    return _probe


def _probes(which, groups, dtype):
    P = _probe_inputs()
    worst = 0.0
    for g in groups:
        w, b, hidden, cat = X.probe_tensors(which, g)
        h = ops.pack_depthnet(w, b, hidden, cat, dtype)
        want, allow = X.probe_reference(P["e"], g, dtype)
        assert np.isnan(want[-3:]).all() and not np.isnan(want[:-3]).any()
        for run in range(2):
            z = ops.depthnet_forward(h, P["o"], P["d"], 0.0, 1.0, X.PROBE_RADIUS)
            ratio, ray = X.probe_worst(z.cpu().numpy(), want, allow)
            assert ratio <= 1.0, (f"probe {g} ({which}, {dtype}) run {run}: ray {ray}: got {float(z[ray, 0])!r}, expected {want[ray]!r}, "
                                  f"{ratio} gates; columns {X.probe_columns(g).tolist()}")
            worst = max(worst, ratio)
    print(f"probes {which} {dtype}: worst |err| / gate = {worst:.3f}")


@pytest.mark.parametrize("dtype", X.PROBE_DTYPES)
def test_trig_columns_at_width_256(dtype):
    """embed3 and embed6 (f32), embedN_16 with NC = 3 and 6 under Trig<false> (bf16, f16) and Trig<true> (f16x3): every column
    of the embedding in its slot, level, component and phase, through the fold and through the direct skip; misses stay NaN"""
    _probes("wide", range(X.PROBE_GROUPS), dtype)


@pytest.mark.parametrize("dtype", X.PROBE_NARROW_DTYPES)
def test_trig_columns_at_width_128(dtype):
    """the same groups on 42-unit trunks: the 128-wide kernels of both engines"""
    for n in range(6):
        _probes(n, range(7 * n, 7 * n + 7), dtype)
