"""The exactly representable radiance fields of tests/exact_field.py, on the CPU (no GPU needed): the conditions that make
`raw64.float()` the only correct answer of every kernel (C1 - C5, the remainder family's), the packer's fold on these weights,
and the weight stream as a multiset.  tests/test_gpu_exact_field.py runs the kernels on the same table of networks."""
import ctypes as C

import numpy as np
import pytest

import exact_field as E
from nerf_sampling_amd import _lib

CASES = [(name, columns) for name in E.NETWORKS for columns in E.COLUMNS]
REMAINDER_CASES = [(name, layer) for name in E.REMAINDER_NETWORKS for layer in E.remainder_layers(name)]
DTYPES = {"f32": _lib.DTYPE_F32, "bf16": _lib.DTYPE_BF16, "f16": _lib.DTYPE_F16, "f16x3": _lib.DTYPE_F16X3}


@pytest.mark.parametrize("name,columns", CASES)
def test_conditions(name, columns):
    net = E.network(name, columns)
    cfg = E.NETWORKS[name]
    assert (net["D"], net["W"], net["skips"], net["use_viewdirs"]) == (cfg["D"], cfg["W"], tuple(cfg["skips"]), cfg["use_viewdirs"])
    assert net["pool"].shape == (E.POOL_ROWS, 90 if net["use_viewdirs"] else 63)
    assert net["raw"].shape == (E.POOL_ROWS, net["output_ch"]) and np.isfinite(net["raw"]).all()
    E.check_c1(net)
    E.check_c2(net)
    assert E.check_c3(net) < 2.0 ** 24
    E.check_c4(net)
    E.check_c5(net)
    if columns == "all":
        assert np.isin(net["pool"] * 2, np.arange(-4, 5)).all()
        # rows stay wide where they survive: a row of layer 0 carries at least 32 terms
        assert (net["weights"][0] != 0).sum(axis=1).max() >= 32
    else:
        r = net["rays"]
        pts = r["o"][:, None, :] + r["d"][:, None, :] * r["z"][:, :, None]
        assert (net["pool"][:, :3] == pts.reshape(-1, 3)).all() and np.abs(pts).max() < 8 and (pts * 8 == np.rint(pts * 8)).all()
        assert (r["o"] * 4 == np.rint(r["o"] * 4)).all() and (r["z"] * 4 == np.rint(r["z"] * 4)).all()
        assert np.isin(r["d"], [0.0, 0.5, -0.5, 1.0, -1.0]).all()
        if net["use_viewdirs"]:
            assert (net["pool"][:, 63:66] == np.repeat(r["viewdirs"], E.RAY_POOL[1], axis=0)).all()
    # every output channel takes both signs and many values: a kernel that returns a constant cannot pass
    assert all(len(np.unique(net["raw"][:, c])) > 50 for c in range(net["raw"].shape[1]))


@pytest.mark.parametrize("name,layer", REMAINDER_CASES)
def test_remainder_conditions(name, layer):
    net = E.remainder_network(name, layer)
    base = E.network(name)
    assert E.check_remainders(net) < 2.0 ** 24
    assert E.is_f32(net["raw"]) and (net["raw"] != base["raw"]).any()
    changed = [n for n, a, b in zip(net["names"], net["weights"], base["weights"]) if (a != b).any()]
    assert changed == [layer] and all((a == b).all() for a, b in zip(net["biases"], base["biases"]))


def _nets():
    for name, columns in CASES:
        yield f"{name}-{columns}", lambda name=name, columns=columns: E.network(name, columns)
    for name, layer in REMAINDER_CASES:
        yield f"{name}-remainder-{layer}", lambda name=name, layer=layer: E.remainder_network(name, layer)


NETS = dict(_nets())


@pytest.mark.parametrize("key", list(NETS))
def test_literal_chain_equals_folded_evaluation_and_the_packers_fold(key):
    net = NETS[key]()
    assert (E.folded_chain(net, net["pool"]) == net["raw"]).all()
    # the same layers in fp32, in the order the CPU's BLAS sums them: exact sums do not depend on it
    h32 = {}
    for lname, w, b, inp, relu in E.kernel_layers(net):
        h32[lname] = inp.astype(np.float32) @ w.astype(np.float32).T + b.astype(np.float32)
        want = inp @ w.T + b
        assert h32[lname].dtype == np.float32 and (h32[lname].astype(np.float64) == want).all(), lname
    if not net["use_viewdirs"]:
        return
    W = net["W"]
    w = dict(zip(net["names"], net["weights"]))
    b = dict(zip(net["names"], net["biases"]))
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (w["feature"], b["feature"], w["views"], b["views"])]
    assert all((a.astype(np.float64) == x).all() for a, x in zip(arrs, (w["feature"], b["feature"], w["views"], b["views"])))
    wo = np.zeros((W // 2, W + 27), np.float32)
    bo = np.zeros((W // 2,), np.float32)
    _lib.check(_lib.load().ns_fold_nerf_views(W, *[a.ctypes.data_as(C.c_void_p) for a in arrs], wo.ctypes.data_as(C.c_void_p),
                                              bo.ctypes.data_as(C.c_void_p)), "ns_fold_nerf_views")
    wf, bf = E.fold_views(net)
    assert (wo.astype(np.float64) == wf).all() and (bo.astype(np.float64) == bf).all()


def _host_image(net, dtype):
    lib = _lib.load()
    keep_w = [np.ascontiguousarray(a, dtype=np.float32) for a in net["weights"]]
    keep_b = [np.ascontiguousarray(a, dtype=np.float32) for a in net["biases"]]
    wa = (C.c_void_p * len(keep_w))(*[k.ctypes.data for k in keep_w])
    ba = (C.c_void_p * len(keep_b))(*[k.ctypes.data for k in keep_b])
    mask = 0
    for i in net["skips"]:
        mask |= 1 << i
    args = (net["D"], net["W"], mask, int(net["use_viewdirs"]), net["output_ch"], wa, ba, dtype, 0)
    nbytes, nbias = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.ns_pack_nerf_host_image(*args, None, 0, None, 0, C.byref(nbytes), C.byref(nbias)), "ns_pack_nerf_host_image")
    stream = np.zeros(nbytes.value, np.uint8)
    bias = np.zeros(nbias.value, np.float32)
    _lib.check(lib.ns_pack_nerf_host_image(*args, stream.ctypes.data_as(C.c_void_p), stream.size,
                                           bias.ctypes.data_as(C.c_void_p), bias.size, C.byref(nbytes), C.byref(nbias)),
               "ns_pack_nerf_host_image")
    return stream, bias


def _decode(stream, dtype):
    if dtype == "f32":
        return stream.view(np.float32).astype(np.float64)
    if dtype == "bf16":
        return (stream.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return stream.view(np.float16).astype(np.float64)


def _nonzero_sorted(parts):
    v = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts])
    return np.sort(v[v != 0])


# the remainder family is for f16x3 and f32 handles
STREAM_CASES = [(key, dtype) for key in NETS for dtype in DTYPES if "-remainder-" not in key or dtype in ("f32", "f16x3")]


@pytest.mark.parametrize("key,dtype", STREAM_CASES)
def test_stream_holds_every_weight_once_and_nothing_else(key, dtype):
    """Whatever the layout: the nonzero elements of the stream are the nonzero weights of the layers the kernels run (view layer
    folded, narrow networks padded with zeros), for f16x3 their hi and lo parts; the bias image holds the biases."""
    net = NETS[key]()
    stream, bias = _host_image(net, DTYPES[dtype])
    layers = E.kernel_layers(net)
    if dtype == "f16x3":
        want = [part for _, w, _, _, _ in layers for part in E.split(w)]
    else:
        want = [w for _, w, _, _, _ in layers]
    got = _decode(stream, dtype)
    assert np.isfinite(got).all()
    assert np.array_equal(_nonzero_sorted([got]), _nonzero_sorted(want))
    assert np.array_equal(_nonzero_sorted([bias]), _nonzero_sorted([b for _, _, b, _, _ in layers]))


def test_row_and_ray_indices_stay_in_the_pool():
    for M in E.ROW_COUNTS + (200000,):
        idx = E.row_indices(M, seed=M)
        assert idx.shape == (M,) and idx.min() >= 0 and idx.max() < E.POOL_ROWS
        assert len(np.unique(idx)) == min(M, E.POOL_ROWS)
    rays, samples = E.RAY_POOL
    for R, N in E.RAY_SHAPES:
        ray, rows = E.ray_indices(R, N, seed=R)
        assert ray.shape == (R,) and rows.shape == (R, N) and ray.min() >= 0 and ray.max() < rays
        assert (rows // samples == ray[:, None]).all()                  # every sample of a ray comes from that ray's pool rows
        assert all(len(np.unique(r)) == N for r in rows)


def test_first_difference_reports_the_row_and_its_tile_position():
    import torch

    want = torch.arange(400 * 4, dtype=torch.float32).reshape(400, 4)
    assert E.first_difference(want.clone(), want) == ""
    zero = torch.zeros(3, 4)
    assert E.first_difference(-zero, zero) == ""                        # -0.0 equals 0.0
    got = want.clone()
    got[337, 2] += 1
    got[399, 0] = float("nan")
    msg = E.first_difference(got, want)
    assert "2 of 1600 values differ" in msg and "row 337 channel 2" in msg and "= 1, 17, 17, 17)" in msg
    assert "got 1351.0, expected 1350.0" in msg
    assert E.first_difference(got.reshape(20, 20, 4), want.reshape(20, 20, 4)) == msg
