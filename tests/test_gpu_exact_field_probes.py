"""The radiance-field kernels' sines and cosines, column by column, against float64 (needs a GPU).

Every probe field of tests/exact_field_probes.py (its coverage, reference, gates and mutants: tests/
test_exact_field_probes_host.py) through ops.pack_nerf and ops.nerf_forward / ops.nerf_forward_rays, on every operand type:
embed3 (k-major fp32), embed3_16 on v_sin_f32 (bf16, f16: the point's ten levels and the view direction's four, the latter
behind the embed-once-per-run branch), embedN_16 on Trig<true> (f16x3), the skip layer's re-read of the embedded point from
the per-wave stash, and the packer's column maps.  Every row, head and ray is held to the derived gate; every call runs twice,
the second time on the caches and LDS the first left behind.

The tangent probes of tests/exact_tangent_probes.py run ops.render_rays_depthnet_tangent on its three instances.  Each test
prints its worst |err| / gate; the figures measured on an MI355X stand in the two modules' docstrings.
"""
import numpy as np
import pytest
import torch

import exact_field as E
import exact_field_probes as P
import exact_tangent as X
import exact_tangent_probes as T
from nerf_sampling_amd import ops

pytestmark = pytest.mark.gpu

PROBES = P.probes()
IDS = [f"{s}-{r}-{p}" for s, r, p in PROBES]
PROD = [p for p in PROBES if p[0] == "prod"]
PROD_IDS = [i for i, p in zip(IDS, PROBES) if p[0] == "prod"]
_packed, _inputs, _refs = {}, {}, {}


def _handle(probe, dtype):
    if (probe, dtype) not in _packed:
        net = P.make_probe(*probe)
        w, b = P.tensors(net)
        _packed[probe, dtype] = ops.pack_nerf(w, b, net["D"], net["W"], list(net["skips"]), dtype=dtype,
                                              use_viewdirs=net["use_viewdirs"], output_ch=net["output_ch"])
    return _packed[probe, dtype]


def _input(shape, name):
    """(the input set, its tensors on the device, embedding64): computed once and left unchanged."""
    if (shape, name) not in _inputs:
        s = P.input_sets(shape)[name]
        dev = {k: torch.from_numpy(v).cuda() for k, v in s.items() if k != "form"}
        _inputs[shape, name] = (s, dev, P.embedding64(s["pts"], s["dirs"], E.NETWORKS[shape]["use_viewdirs"]))
    return _inputs[shape, name]


def _reference(probe, name, dtype):
    if (probe, name, dtype) not in _refs:
        net = P.make_probe(*probe)
        e = _input(probe[0], name)[2]
        if (probe, name) not in _refs:
            _refs[probe, name] = P.reference(net, e)
        _refs[probe, name, dtype] = (_refs[probe, name], P.gate(net, e, dtype))
    return _refs[probe, name, dtype]


def _run(probe, dtype, what=""):
    """Every input set of the probe's shape, twice; returns the worst |err| / gate."""
    net = P.make_probe(*probe)
    h = _handle(probe, dtype)
    top, where = 0.0, None
    for name in P.input_sets(probe[0]):
        s, dev, _ = _input(probe[0], name)
        raw64, allow = _reference(probe, name, dtype)
        v = dev["dirs"] if net["use_viewdirs"] else None
        for run in range(2):
            if s["form"] == "points":
                got = ops.nerf_forward(h, dev["pts"], v)
            else:
                got = ops.nerf_forward_rays(h, dev["o"], dev["d"], dev["z"], v)
            ratio, at = P.worst(got.double().cpu().numpy(), raw64, allow)
            if ratio > top:
                top, where = ratio, (name, run) + at
            assert ratio <= 1.0, (f"{probe} {dtype} {what} {name} run {run}: |raw - raw64| is {ratio:.3g} of its gate at row {at[0]}, "
                                  f"channel {at[1]}: head {[hd for hd in net['heads'] if hd[0] == at[1]]}")
    return top, where


@pytest.mark.parametrize("dtype", P.PROBE_DTYPES)
@pytest.mark.parametrize("shape,route,part", PROBES, ids=IDS)
def test_every_column_is_float64s(shape, route, part, dtype):
    top, where = _run((shape, route, part), dtype)
    print(f"{shape} {route} {part} {dtype}: worst |raw - raw64| / gate {top:.3f} at {where}")


@pytest.mark.parametrize("dtype", P.PROBE_DTYPES)
@pytest.mark.parametrize("shape,route,part", PROD, ids=PROD_IDS)
def test_production_network_on_the_generic_kernels(shape, route, part, dtype):
    with ops.debug_switch(generic_kernels=1):
        top, where = _run((shape, route, part), dtype, "generic")
    print(f"{shape} {route} {part} {dtype} generic: worst |raw - raw64| / gate {top:.3f} at {where}")


@pytest.mark.parametrize("tiles", [4, 5])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape,route,part", PROD, ids=PROD_IDS)
def test_production_network_on_four_and_five_tiles(shape, route, part, dtype, tiles):
    with ops.debug_switch(prod_tiles=tiles):
        top, where = _run((shape, route, part), dtype, f"tiles={tiles}")
    print(f"{shape} {route} {part} {dtype} tiles={tiles}: worst |raw - raw64| / gate {top:.3f} at {where}")


# ---- the tangent probes (tests/exact_tangent_probes.py) -------------------------------------------------------------
TPROBES = T.probes()
TIDS = [f"{s}-{r}-{p}" for s, r, p in TPROBES]


def _tangent_handle(net, dtype):
    key = ("tangent", net["name"], dtype)
    if key not in _packed:
        w, b = E.tensors(net)
        _packed[key] = ops.pack_nerf(w, b, net["D"], net["W"], list(net["skips"]), dtype=dtype, use_viewdirs=True, output_ch=4)
    return _packed[key]


@pytest.mark.parametrize("instance", T.INSTANCES)
@pytest.mark.parametrize("shape,route,part", TPROBES, ids=TIDS)
def test_every_columns_tangent_is_float64s(shape, route, part, instance):
    """ops.render_rays_depthnet_tangent on a tangent probe field: every finite-mean ray within the error model's bound in every
    column, J == 0 exactly for the NaN mean and the all-clipped ray; twice, the same bits"""
    net = T.network(shape, route, part)
    h = _tangent_handle(net, T.DTYPE[instance])
    cat = lambda t: torch.cat([t["rgb"], t["disp"][:, None], t["depth"][:, None], t["acc"][:, None]], -1)
    worst, where = 0.0, None
    for case in T.cases(net, instance):
        ref = T.jacobian64(net, case, instance)
        o, d, v, m = (torch.from_numpy(a).cuda() for a in X.case_inputs(net, case))
        kw = dict(rays=(o, d, v), n_samples=max(case["N"], 2), std=float(X.std_of(case["N"], net["step"])), white_bkgd=case["white"],
                  extras=("depth", "acc"), approximate=instance == "f16", mode="depth_only" if instance == "single" else "uniform")
        _, J = ops.render_rays_depthnet_tangent(m, h, **kw)
        _, J2 = ops.render_rays_depthnet_tangent(m, h, **kw)
        J, J2 = cat(J), cat(J2)
        assert torch.equal(J.view(torch.int32), J2.view(torch.int32)), "two calls give different Jacobians"
        J = J.double().cpu().numpy()
        tag = (shape, route, part, instance, case["N"], case["white"])
        if case["N"] > 1:
            assert (J[T.NAN_AT] == 0).all() and (J[T.CLIPPED_AT] == 0).all(), tag
            assert T.NAN_AT not in ref["keep"] and (ref["samples"]["dz"][list(ref["keep"]).index(T.CLIPPED_AT)] == 0).all()
        else:
            assert (J[:, 3:] == 0).all(), tag
        assert np.isfinite(J[ref["keep"]]).all(), tag
        ratio = np.abs(J[ref["keep"]] - ref["J"]) / ref["bound"]
        if ratio.max() > worst:
            worst, where = float(ratio.max()), tag + (X.COLS[int(ratio.max(axis=0).argmax())],)
        assert ratio.max() <= 1.0, tag + (f"|J - J64| is {float(ratio.max()):.3g} of its bound, column "
                                          f"{X.COLS[int(ratio.max(axis=0).argmax())]}, ray {int(ratio.max(axis=1).argmax())}",)
    print(f"{shape} {route} {part} {instance}: worst |J - J64| / bound {worst:.3f} at {where}")
