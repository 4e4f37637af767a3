"""Every radiance-field kernel against the one correct answer, bit for bit (needs a GPU).

The networks of tests/exact_field.py have weights, inputs and activations that are bf16 and f16 numbers and sums that are
exact in fp32 in any order (tests/test_exact_field_host.py proves it for every network used here), so the float64 result of
the reference's literal layer chain, converted to fp32, is what every engine (k-major fp32, 16x16x32 bf16 / f16, split f16),
every schedule (generic, generated, four and five tiles) and every input form (embedded rows, points, rays) must return: no
tolerance, and no other kernel on the other side of the comparison.  Every comparison is torch.equal on values (-0.0 equals
0.0, a NaN equals nothing).

What this cannot show is said in DESIGN.md section 5: the rounding of operands that are not exactly representable,
compositing and the DepthNet.  The sines and cosines of the embedding, which these networks never read, are held column by
column in tests/exact_field_probes.py and tests/test_gpu_exact_field_probes.py.
"""
import numpy as np
import pytest
import torch

import exact_field as E
from nerf_sampling_amd import ops

pytestmark = pytest.mark.gpu

ALL_DTYPES = ("f32", "bf16", "f16", "f16x3")
_packed = {}
_device = {}


def _handle(net, key, dtype):
    """The packed handle of a network, cached for the module."""
    if (key, dtype) not in _packed:
        w, b = E.tensors(net)
        _packed[key, dtype] = ops.pack_nerf(w, b, net["D"], net["W"], list(net["skips"]), dtype=dtype,
                                            use_viewdirs=net["use_viewdirs"], output_ch=net["output_ch"])
    return _packed[key, dtype]


def _on_device(net, key):
    """(pool, raw64.float()) of a network on the device, cached for the module."""
    if key not in _device:
        assert E.is_f32(net["pool"]) and E.is_f32(net["raw"])
        _device[key] = (torch.from_numpy(net["pool"]).float().cuda(), torch.from_numpy(net["raw"]).float().cuda())
    return _device[key]


def _net(name, columns):
    return E.network(name, columns), (name, columns)


def _same(got, want, what):
    assert not torch.isnan(got).any(), f"{what}: NaN"
    diff = E.first_difference(got, want)
    assert not diff, f"{what}: {diff}"


def _embedded(net, key, dtype, M, seed=0, what=""):
    pool, raw = _on_device(net, key)
    idx = torch.from_numpy(E.row_indices(M, seed)).cuda()
    got = ops.nerf_forward_embedded(_handle(net, key, dtype), pool[idx].contiguous())
    _same(got, raw[idx], f"{key} {dtype} embedded M={M} {what}")


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("name", list(E.NETWORKS))
def test_embedded_rows(name, dtype):
    """row counts around every tile, wave and workgroup size of the three engines (16 rows a tile, 64 and 80 a wave, 320 a group)"""
    net, key = _net(name, "all")
    for M in E.ROW_COUNTS:
        _embedded(net, key, dtype, M, seed=M)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_production_network_on_the_generic_kernels(dtype):
    net, key = _net("prod", "all")
    with ops.debug_switch(generic_kernels=1):
        for M in E.ROW_COUNTS:
            _embedded(net, key, dtype, M, seed=M, what="generic")


@pytest.mark.parametrize("tiles", [4, 5])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_production_network_on_four_and_five_tiles(dtype, tiles):
    net, key = _net("prod", "all")
    with ops.debug_switch(prod_tiles=tiles):
        for M in E.ROW_COUNTS:
            _embedded(net, key, dtype, M, seed=M, what=f"tiles={tiles}")


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_several_groups_per_workgroup(dtype):
    """more rows than one pass of every compute unit takes: each workgroup walks several groups of 320; twice, the second
    launch on a device whose caches and LDS the first has left behind"""
    net, key = _net("prod", "all")
    M = 2 * 320 * int(ops._lib.load().ns_device_cu_count()) + 77
    assert 77 < M < 2 ** 20
    for run in range(2):
        _embedded(net, key, dtype, M, seed=5, what=f"run {run}")


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("name", list(E.NETWORKS))
def test_points_and_rays(name, dtype):
    """nerf_forward (points) and nerf_forward_rays (o + d z formed in the kernel) embed the points themselves: an "identity"
    network multiplies every sine and cosine by zero and reads the raw coordinates, which are dyadic; the same network once
    through the embedded form."""
    net, key = _net(name, "identity")
    pool, raw = _on_device(net, key)
    h = _handle(net, key, dtype)
    rays = {k: torch.from_numpy(v).float().cuda() for k, v in net["rays"].items()}
    for R, N in E.RAY_SHAPES:
        ray, rows = E.ray_indices(R, N, seed=R)
        ray_t, rows_t = torch.from_numpy(ray).cuda(), torch.from_numpy(rows).cuda()
        want = raw[rows_t]                                                     # [R, N, C]
        v = rays["viewdirs"][ray_t].contiguous() if net["use_viewdirs"] else None
        pts = pool[rows_t][..., :3].contiguous()
        _same(ops.nerf_forward(h, pts, v), want, f"{key} {dtype} points R={R} N={N}")
        z = rays["z"].reshape(-1)[rows_t].contiguous()
        o, d = rays["o"][ray_t].contiguous(), rays["d"][ray_t].contiguous()
        assert torch.equal(o[:, None, :] + d[:, None, :] * z[..., None], pts)
        _same(ops.nerf_forward_rays(h, o, d, z, v), want, f"{key} {dtype} rays R={R} N={N}")
    _embedded(net, key, dtype, 321, seed=1)


REMAINDER_CASES = [(name, layer) for name in E.REMAINDER_NETWORKS for layer in E.remainder_layers(name)]


@pytest.mark.parametrize("dtype", ["f16x3", "f32"])
@pytest.mark.parametrize("name,layer", REMAINDER_CASES)
def test_split_operands(name, layer, dtype):
    """one layer's weights are w (1 + 2^-12) = hi + lo: that layer needs W_lo x_hi, every later one W_hi x_lo, each in turn"""
    net = E.remainder_network(name, layer)
    key = (name, "all", layer)
    w, b = E.tensors(net)
    h = ops.pack_nerf(w, b, net["D"], net["W"], list(net["skips"]), dtype=dtype)      # used once: not cached
    pool, _ = _on_device(E.network(name), (name, "all"))
    idx = E.row_indices(321, seed=3)
    want = torch.from_numpy(net["raw"][idx]).float().cuda()
    assert not torch.equal(want, _on_device(E.network(name), (name, "all"))[1][torch.from_numpy(idx).cuda()])
    got = ops.nerf_forward_embedded(h, pool[torch.from_numpy(idx).cuda()].contiguous())
    _same(got, want, f"{key} {dtype} remainders M=321")
