"""The exactly representable DepthNets of tests/exact_depthnet.py, on the CPU (no GPU needed): the pool of rays, the
conditions D1 - D6 that make the float64 chain the only correct head sum of every kernel, the packer's fold on these weights,
the fp32 oracle's acceptance and the rejection of every mutant the comparison is there to catch; then the probe networks of
the sines and cosines.  tests/test_gpu_exact_depthnet.py runs the kernels on the same tables."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_depthnet as X
import exact_field as E
from nerf_sampling_amd import _lib
from oracle import nerf_oracle as O

NAMES = list(X.NETWORKS)
CASES = [(name, dtype) for name in NAMES for dtype in X.dtypes_of(name)]
REMAINDER_CASES = [(name, dtype, layer) for name in X.REMAINDER_NETWORKS for dtype in X.REMAINDER_DTYPES
                   if dtype in X.dtypes_of(name) for layer in X.remainder_layers(name, dtype)]


def test_the_pool_is_what_the_filter_leaves():
    P = X.pool()
    assert P["counts"] == (2964, 516, 124)                 # rays, distinct intersection tuples, distinct directions at radius 3
    assert (P["radius"] == 3).sum() == 516 and (P["radius"] == 2).sum() == 36
    assert len(np.unique(P["x"], axis=0)) == 552 and P["x12"].shape == (552, 12)
    for radius in X.RADII:
        own = P["radius"] == radius
        keep, miss, x = X.exact_rays(P["o"][own], P["d"][own], radius)
        assert keep.all() and not miss.any() and (x == P["x"][own]).all()
        assert (np.abs(x).max(axis=1) <= radius).all() and ((x[:, :3] ** 2).sum(axis=1) == radius ** 2).all()
        assert (x == np.rint(x)).all() and E.fits16(x).all()
        keep, miss, x = X.exact_rays(P["miss_o"], P["miss_d"], radius)
        assert miss.all() and not keep.any() and np.isnan(x).all()
    assert np.abs(P["o"]).max() == 6 and np.abs(P["d"]).max() == 2 and len(P["miss_o"]) == 8
    # a ray with an inexact root, and one with an inexact quotient, are not kept
    keep, _, _ = X.exact_rays(np.array([[0.0, 0, 4], [0.0, 0, 4]]), np.array([[1.0, 0, -2], [0.0, 1, -2]]), 3.0)
    assert not keep.any()
    for R in X.RAY_COUNTS:
        for radius in X.RADII:
            idx = X.ray_indices(R, radius, seed=R)
            assert idx.shape == (R,) and (P["radius"][idx] == radius).all()
            assert len(np.unique(idx)) == min(R, int((P["radius"] == radius).sum()))


def test_the_activation_rules():
    assert np.float16(0.01).view(np.uint16) == 0x211F and X.SLOPE16 != X.SLOPE32
    v = np.array([3.0, 0.0, -1.0, -7552.0, -3.0])
    assert (X.leaky(v, "f32")[:2] == v[:2]).all() and X.leaky(v, "f32")[2] == -X.SLOPE32
    assert X.leaky(v, "f16")[2] == -X.SLOPE16 and X.leaky(v, "f16")[2] != X.leaky(v, "f32")[2]
    assert (X.leaky(v, "f16") == X.f16r(X.leaky(v, "f16"))).all() and (X.leaky(v, "bf16") == X.bf16r(X.leaky(v, "f32"))).all()
    hi = X.leaky(v, "x3hi")
    assert (hi == X.f16r(X.leaky(v, "f32"))).all() and (X.leaky(v, "x3") == hi + X.f16r(X.leaky(v, "f32") - hi)).all()
    assert (X.leaky(v, "x3") != hi).any() and (X.leaky(v, "x3") != X.leaky(v, "f32")).any()
    assert X.layer_rules("f16m", 10) == ["x3", "x3", "x3hi"] + ["f16"] * 7 and X.layer_rules("f16x3", 2) == ["x3", "x3"]
    r = np.random.default_rng(0).standard_normal(4096) * np.exp2(np.random.default_rng(1).integers(-20, 20, 4096))
    r = np.concatenate([r, [0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3.3895e38]])
    assert (X.bf16r(r) == torch.from_numpy(r).float().to(torch.bfloat16).double().numpy()).all()
    for rule in ("f32", "bf16", "f16", "x3", "x3hi"):
        assert np.isnan(X.leaky(np.array([np.nan]), rule)).all()


@pytest.mark.parametrize("name", NAMES)
def test_shape_and_structure(name):
    net = X.network(name)
    hidden, cat, _ = X.NETWORKS[name]
    assert (net["hidden"], net["cat"]) == (hidden, cat)
    assert [w.shape for w in net["cat_w"]] == [(cat[0], 3 * hidden[-1] + 252)] + [(b, a) for a, b in zip(cat, cat[1:])]
    for b, dim in enumerate(X.BRANCH_DIM):
        assert [w.shape for w in net["branch_w"][b]] == [(s, p + dim) for p, s in zip([dim] + hidden, hidden)]
    X.check_d1(net)
    X.check_d2(net)
    X.check_d4(net)
    # the rows are wide: an ordinary unit reads at least two columns, and eight on average wherever the layer before has them
    for l, w in enumerate(net["cat_w"]):
        rows = net["ordinary"][l]
        n = (w[rows] != 0).sum(axis=1)
        fed = l == 0 or net["cat"][l - 1] >= 32           # (behind a 16-wide layer there are its basis units to read and no other)
        assert n.min() >= (2 if fed else 1) and n.mean() >= (8 if fed else 2), (l, n.mean(), n.min())
    # a chain unit in every 16-row sub-block of every layer, relays of one term, a head of one term at two scales per chain
    last = len(cat) - 1
    for l, width in enumerate(cat):
        units = X.chain_units(net, l)
        assert all(any(lo <= u < hi for u in units) for lo, hi in X._blocks(width)), f"layer {l}"
        assert not set(units) & set(net["ordinary"][l]) and len(set(units)) == len(units)
        if l > 0:
            assert not net["cat_w"][l][net["ordinary"][l]][:, X.chain_units(net, l - 1)].any(), "an ordinary unit reads a chain unit"
    assert not net["heads"]["main"][0][0, X.chain_units(net, last)].any()
    for c, units in enumerate(net["chain"]):
        assert sorted(units) == list(range(min(units), len(cat)))
        for l in sorted(units)[1:]:
            row = net["cat_w"][l][units[l]]
            assert np.flatnonzero(row).tolist() == [units[l - 1]] and row[units[l - 1]] < 0 and net["cat_b"][l][units[l]] == 0
            assert np.log2(-row[units[l - 1]]) == np.rint(np.log2(-row[units[l - 1]]))
        for tag in ("", "s"):
            hw, hb = net["heads"][f"chain{c}{tag}"]
            assert np.flatnonzero(hw[0]).tolist() == [units[last]] and hb[0] == 0
    assert len(net["heads"]) == 1 + 2 * len(net["chain"]) and len(net["chain"]) == max(len(X._blocks(w)) for w in cat)


@pytest.mark.parametrize("name,dtype", CASES)
def test_conditions(name, dtype):
    net = X.network(name)
    assert X.check_d3(net, dtype) < 2.0 ** 24
    assert X.check_chain_range(net, dtype) == 0.0          # every split remainder is zero or a normal f16 number
    for near, far in X.NEAR_FAR:
        X.check_d6(net, dtype, near, far)
    # the chain heads' few-ray launches take rays on which the chain is not zero: there are enough for the largest of them
    a = X.trunk(net, dtype, X.pool()["x12"])
    for head in net["heads"]:
        if head != "main":
            live = (X.head_sum(net, head, a) != 0) & (X.pool()["radius"] == 3)
            assert live.sum() >= 33 and len(np.unique(X.ray_indices(33, 3.0, seed=1, among=live))) == 33
    z = X.reference(net, "main", dtype, X.pool()["x12"], 2.0, 6.0)
    assert np.isfinite(z).all() and len(np.unique(z)) > 100 and 2.0 < z.min() < 3.0 and 5.0 < z.max() < 6.0


@pytest.mark.parametrize("name,dtype", CASES)
def test_the_comparison_rejects_the_mutants(name, dtype):
    """a zeroed 32-column or 16-row block, two exchanged blocks of biases (D5); a negative branch that is missing, or has the
    other engine's slope, in one sub-block of one layer.  (hi + lo handed to f16m's first plain layer shows in no row of one
    term, whose fp16 rounding takes the lo part away again: the remainder family below rejects it.)"""
    net = X.network(name)
    X.check_d5(net, dtype)
    X.check_chains_cover(net, dtype, "zero")
    X.check_chains_cover(net, dtype, "slope")


def _library_fold(net, head="main"):
    ws, bs = X.tensors(net, head)
    n = len(net["hidden"])
    keep_w = [np.ascontiguousarray(w.numpy(), dtype=np.float32) for w in ws[:3 * n + 1]]
    keep_b = [np.ascontiguousarray(b.numpy(), dtype=np.float32) for b in bs[:3 * n + 1]]
    wa = (C.c_void_p * len(keep_w))(*[k.ctypes.data for k in keep_w])
    ba = (C.c_void_p * len(keep_b))(*[k.ctypes.data for k in keep_b])
    c0 = net["cat"][0]
    F, fb = np.zeros((c0, 252), np.float32), np.zeros((c0,), np.float32)
    _lib.check(_lib.load().ns_fold_depthnet_front(n, (C.c_int * n)(*net["hidden"]), c0, wa, ba, F.ctypes.data_as(C.c_void_p),
                                                  fb.ctypes.data_as(C.c_void_p)), "ns_fold_depthnet_front")
    return F.astype(np.float64), fb.astype(np.float64)


@pytest.mark.parametrize("name", NAMES)
def test_the_packers_fold_is_the_float64_fold(name):
    net = X.network(name)
    F, fb = _library_fold(net)
    F64, fb64 = X.fold64(net)
    assert (F == F64).all() and (fb == fb64).all()
    assert (X.literal_pre0(net, X.pool()["x12"]) == X.pool()["x12"] @ F64[:, X.ID_COLS].T + fb64).all()


def _oracle(net, head, idx, near, far, radius, extra=None):
    P = X.pool()
    o, d = P["o"][idx], P["d"][idx]
    if extra is not None:
        o, d = np.concatenate([o, extra[0]]), np.concatenate([d, extra[1]])
    z = O.depthnet_forward(X.state_dict(net, head), torch.from_numpy(o).float(), torch.from_numpy(d).float(),
                           sphere_radius=radius, near=near, far=far)
    assert z.dtype == torch.float32
    return z.double().numpy().reshape(-1)


@pytest.mark.parametrize("name", NAMES)
def test_the_fp32_oracle_passes_on_every_ray(name):
    """The reference's literal fp32 chain, branches unfolded, every head: within the gate on every pool ray at both radii and
    both (near, far); NaN on the rays that miss and on no other.  The worst ratio stays within the 4 U that the gate's
    derivation counts, half the gate (the measured figure is in exact_depthnet's docstring: it moves with torch's expf)."""
    net = X.network(name)
    P = X.pool()
    worst = 0.0
    for head in net["heads"]:
        for radius in X.RADII:
            idx = np.flatnonzero(P["radius"] == radius)
            for near, far in X.NEAR_FAR:
                z = _oracle(net, head, idx, near, far, radius, extra=(P["miss_o"], P["miss_d"]))
                assert np.isnan(z[len(idx):]).all() and not np.isnan(z[:len(idx)]).any()
                want = X.reference(net, head, "f32", P["x12"][idx], near, far)
                ratio, ray = X.worst_ratio(z[:len(idx)], want, near, far)
                assert ratio <= 1.0, f"{name} {head} radius {radius} near {near} far {far}: {ratio} gates at ray {ray}"
                worst = max(worst, ratio)
    print(f"fp32 oracle, {name}: worst |err| / gate = {worst:.3f}")
    assert worst <= X.ORACLE_BOUND


def test_the_comparison_counts_a_stray_nan():
    z = np.array([2.0, np.nan, 3.0])
    assert X.worst_ratio(z, z, 2.0, 6.0)[0] == 0.0
    assert X.worst_ratio(z, np.array([2.0, 2.5, 3.0]), 2.0, 6.0) == (np.inf, 1)
    assert X.worst_ratio(np.array([2.0, 2.5, 3.0]), z, 2.0, 6.0) == (np.inf, 1)
    assert X.worst_ratio(np.array([2.0, 2.0 + 1.5 * X.gate(2.0, 6.0)]), np.array([2.0, 2.0]), 2.0, 6.0)[0] == pytest.approx(1.5)
    assert X.gate(2.0, 6.0) == 48 * X.U and X.gate(0.0, 1.0) == 8 * X.U


# ---- the remainder family -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", X.REMAINDER_NETWORKS)
def test_remainder_base_networks(name):
    base = X.remainder_base(name)
    assert base["margin"] == X.MARGIN and not base["chain"] and list(base["heads"]) == ["main"]
    for dtype in X.REMAINDER_DTYPES:
        if dtype in X.dtypes_of(name):
            assert X.check_d3(base, dtype) < 2.0 ** 12
            for near, far in X.NEAR_FAR:
                X.check_d6(base, dtype, near, far)
    X.check_d4(base)
    F, fb = _library_fold(base)
    F64, fb64 = X.fold64(base)
    assert (F == F64).all() and (fb == fb64).all()


@pytest.mark.parametrize("name,dtype,layer", REMAINDER_CASES)
def test_remainder_conditions_and_mutants(name, dtype, layer):
    """the conditions of the family; the fp32 oracle's and the packer's fold's agreement; and the comparison rejects W_lo x_hi
    dropped in the layer with the remainders, W_hi x_lo dropped in the layer behind it, and for f16m hi + lo handed to the
    first plain layer"""
    net, base = X.remainder_network(name, layer), X.remainder_base(name)
    assert X.check_remainders(net, dtype) < 2.0 ** 24
    x12 = X.pool()["x12"]
    n = len(net["cat"])
    F, fb = _library_fold(net)
    F64, fb64 = X.fold64(net)
    assert (F == F64).all() and (fb == fb64).all()
    _, seen = X.trunk(net, dtype, x12, keep=True)
    rules = X.layer_rules(dtype, n)
    for near, far in X.NEAR_FAR:
        want = X.reference(net, "main", dtype, x12, near, far)
        two = 2 * X.gate(near, far)
        if dtype == "f32":
            z = _oracle(net, "main", np.arange(len(x12))[X.pool()["radius"] == 3], near, far, 3.0)
            assert X.worst_ratio(z, want[X.pool()["radius"] == 3], near, far)[0] <= 1.0
        # W_lo x_hi dropped: the layer runs on hi = w alone
        if layer == n:
            dropped = X.depth(X.head_sum(base, "main", seen[-1][2]), near, far)
        else:
            layers = X.kernel_layers(net)
            layers[layer] = X.kernel_layers(base)[layer]
            dropped = X.reference(net, "main", dtype, x12, near, far, layers=layers)
        assert np.abs(dropped - want).max() > two, f"W_lo x_hi dropped in layer {layer}"
        # W_hi x_lo dropped behind it: the next layer sees hi alone
        if layer < n and rules[layer] == "x3":
            lost = X.reference(net, "main", dtype, x12, near, far, act=lambda l, pre, rule: X.leaky(pre, "x3hi" if l == layer else rule))
            assert np.abs(lost - want).max() > two, f"W_hi x_lo dropped behind layer {layer}"
        if dtype == "f16m":
            kx = X.F16M_SPLIT_LAYERS
            both = X.reference(net, "main", dtype, x12, near, far, act=lambda l, pre, rule: X.leaky(pre, "x3" if l == kx - 1 else rule))
            assert np.abs(both - want).max() > two, "hi + lo handed to the first plain layer"


# ---- part B: the probes of the sines and cosines --------------------------------------------------------------------
def test_probe_networks_hold_every_column_once():
    assert sorted(np.concatenate([X.probe_columns(g) for g in range(X.PROBE_GROUPS)]).tolist()) == list(range(252))
    assert set(X.PROBE_HEAD) == {1.0, -1.0, 0.5, -0.5} and all(a != b for a, b in zip(X.PROBE_HEAD, X.PROBE_HEAD[1:]))
    for which in ["wide"] + list(range(6)):
        ws, bs, units = X.make_probe(which)
        net = dict(hidden=[64], cat=[len(units)], branch_w=[[ws[0]], [ws[1]], [ws[2]]], branch_b=[[bs[0]], [bs[1]], [bs[2]]],
                   cat_w=[ws[3]], cat_b=[bs[3]])
        F, fb = X.fold64(net)
        want = np.zeros_like(F)
        want[np.arange(len(units)), units] = [X.probe_sign(j) for j in units]
        assert (F == want).all() and not fb.any()                      # F is the signed one-hot matrix
        Fl, fbl = _library_fold(dict(net, heads={"main": (np.zeros((1, len(units))), np.zeros(1))}))
        assert (Fl == F).all() and (fbl == fb).all()
        routed = (ws[3][:, :192] != 0).any(axis=1)
        assert 0.4 < routed.mean() < 0.6                               # half through the branches and the fold's product
    o, d = X.probe_rays()
    x6 = X.kernel_x6(o, d, X.PROBE_RADIUS)
    assert np.isnan(x6[-3:]).all() and not np.isnan(x6[:-3]).any()
    assert (o == 0).any() and (o < 0).any() and (np.abs(o) == 8).any() and (o == np.float32(2.0 ** -20)).any()
    assert (d == 0).any() and (d < 0).any() and (np.abs(d) == 8).any() and (d == np.float32(2.0 ** -20)).any()


@pytest.mark.parametrize("g", range(X.PROBE_GROUPS))
def test_probes_accept_the_fp32_oracle_and_reject_the_mutants(g):
    """the oracle's fp32 chain on its own intersection coordinates passes the f32 gate; two columns of different levels
    exchanged, the sine and cosine of one level exchanged, one column negated, one argument off by 1e-5: each rejected"""
    o, d = X.probe_rays()
    ws, bs, hidden, cat = X.probe_tensors("wide", g)
    names = ["origin_layers.0", "direction_layers.0", "intersection_layers.0", "cat_layers.0", "to_depth.0"]
    p = {}
    for k, w, b in zip(names, ws, bs):
        p[k + ".weight"], p[k + ".bias"] = w, b
    z, parts = O.depthnet_forward(p, torch.from_numpy(o), torch.from_numpy(d), sphere_radius=X.PROBE_RADIUS, near=0.0, far=1.0,
                                  return_parts=True)
    x6 = parts["e_x"][:, :6].numpy()
    e = X.embedding64(o, d, x6)
    want, allow = X.probe_reference(e, g, "f32")
    ratio, ray = X.probe_worst(z.numpy(), want, allow)
    print(f"fp32 oracle, probe {g}: worst |err| / gate = {ratio:.3f}")
    assert ratio <= 1.0, (g, ratio, ray)
    cols = X.probe_columns(g)
    trig = [c for c in cols if c % 63 >= 3 and c < 126 or c >= 126 and (c - 126) >= 6]
    for dtype in X.PROBE_DTYPES:
        want, allow = X.probe_reference(e, g, dtype)
        for c in trig[:2]:
            at = 0 if c < 63 else 63 if c < 126 else 126
            n = 3 if c < 126 else 6
            level, phase, comp = (c - at - n) // (2 * n), (c - at - n) // n % 2, (c - at - n) % n
            other_level = at + n + 2 * n * ((level + 1) % 10) + n * phase + comp
            other_phase = at + n + 2 * n * level + n * (1 - phase) + comp
            for what, e2 in (("levels exchanged", _swap(e, c, other_level)), ("sine and cosine exchanged", _swap(e, c, other_phase)),
                             ("negated", _scale(e, c, -1.0)), ("argument off by 1e-5", _shift(e, c, 1e-5, other_phase, phase))):
                got, _ = X.probe_reference(e2, g, dtype)
                if what != "argument off by 1e-5":
                    assert X.probe_worst(got, want, allow)[0] > 2.0, (g, dtype, c, what)
                elif dtype in ("f32", "f16x3"):           # (1e-5 is below the 16-bit operands' rounding)
                    assert X.probe_worst(got, want, allow)[0] > 1.0, (g, dtype, c, what)


def _swap(e, a, b):
    e2 = e.copy()
    e2[:, [a, b]] = e[:, [b, a]]
    return e2


def _scale(e, c, s):
    e2 = e.copy()
    e2[:, c] *= s
    return e2


def _shift(e, c, delta, partner, phase):
    """column c with its argument moved by delta: sin(x + delta) = sin x cos delta + cos x sin delta, cos likewise"""
    e2 = e.copy()
    e2[:, c] = e[:, c] * np.cos(delta) + (1 if phase == 0 else -1) * e[:, partner] * np.sin(delta)
    return e2
