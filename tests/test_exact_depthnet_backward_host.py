"""The DepthNet training pass's reference of tests/exact_depthnet_backward.py on the CPU (no GPU needed): D1 - D4 on the
uniform networks, V1 - V3 on every case tests/test_gpu_exact_depthnet_backward.py walks, `reference64` against torch float64
autograd of the oracle's literal chain, the oracle's fp32 autograd inside the bound on every entry, and every mutant rejected."""
import numpy as np
import pytest
import torch

import exact_depthnet as X
import exact_depthnet_backward as B
import ray_front_reference as RF
from oracle import nerf_oracle as O

NAMES = list(B.TRAIN_NETWORKS)


def _all(name):
    return [(key, B.case(name, key)) for key in B.cases(name)]


@pytest.mark.parametrize("name", NAMES)
def test_networks_meet_d1_to_d4(name):
    net = B.network(name)
    X.check_d1(net)
    X.check_d2(net)
    X.check_d3(net, "f32")                 # with the literal unfolded chain
    X.check_d4(net)
    n = len(net["cat"])
    assert B.param_names(net) == [k for k in X.state_dict(net, "main")]
    assert len(net["chain"]) == (net["cat"][0] + 15) // 16 and all(min(u) == 0 for u in net["chain"])
    assert set(net["heads"]) == {"main"} | {f"chain{c}{t}" for c in range(len(net["chain"])) for t in ("", "s")}
    # a sign unit reads the direct columns alone: under a chain head nothing reaches the branches
    for c, units in enumerate(net["chain"]):
        assert not net["cat_w"][0][units[0], :3 * net["cat"][0]].any()
    assert n == len(net["hidden"])


@pytest.mark.parametrize("name", NAMES)
def test_the_table_of_cases(name):
    net = B.network(name)
    keys = B.cases(name)
    assert len(set(keys)) == len(keys)
    rows = B.PROD_ROWS if name == X.PROD else B.ROWS
    assert {k[1] for k in keys if k[0] == "main" and k[2] == 3.0} == set(rows)
    assert {k[0] for k in keys} == set(net["heads"])
    for radius in X.RADII:
        assert {(k[3], k[4]) for k in keys if k[2] == radius} == set(X.NEAR_FAR)
    for key, c in _all(name):
        head, R, radius = key[:3]
        dz = c["dz"]
        assert dz.shape == (R, 1) and np.isin(dz, np.arange(-2, 3)).all() and dz[-1, 0] != 0 and (R < 3 or (dz == 0).any())
        assert (X.pool()["radius"][c["rays"]] == radius).all()
        if head != "main" and R < 100:
            v = B.pool_head_sum(net, head)[c["rays"]]
            assert (v != 0).all() and (np.abs(v) <= B.UNSATURATED).all()
        assert (c["ref"]["z"] == X.reference(net, head, "f32", X.pool()["x12"][c["rays"]], c["near"], c["far"]).reshape(-1, 1)).all()


@pytest.mark.parametrize("radius", X.RADII)
def test_the_sphere_kernels_formula_is_exact_on_the_pool(radius):
    """ns_sphere_intersect's statement (ray_front_reference.sphere32) returns the pool's six coordinates exactly: the training
    pass takes them from that kernel, the inference kernels form them themselves"""
    P = X.pool()
    own = P["radius"] == radius
    _, pts = RF.sphere32(P["o"][own], P["d"][own], radius)
    assert pts.dtype == np.float32 and (pts.reshape(-1, 6).astype(np.float64) == P["x"][own]).all()


@pytest.mark.parametrize("name", NAMES)
def test_conditions(name):
    net = B.network(name)
    n = len(net["cat"])
    seen = np.zeros((len(net["chain"]), n, 2), dtype=bool)
    least, largest = {}, {}
    for key, c in _all(name):
        B.check_v1(c)
        B.check_zeros(c)
        if c["head"] == "main":
            B.check_v3(c)
            if c["R"] >= B.BLOCK_ROWS:
                for k, (lo, hi) in B.block_sharpness(c).items():
                    least[k], largest[k] = min(least.get(k, np.inf), lo), max(largest.get(k, 0.0), hi)
        else:
            chain = int(c["head"][5:].rstrip("s"))
            if not seen[chain].all():                  # (V2 asks for some case: the chain's later cases are not needed then)
                seen[chain] |= B.slope_rejections(c)
    for chain, layer, which in zip(*np.nonzero(~seen)):
        raise AssertionError(f"V2: {name}: no case of chain {chain} sees layer {layer}'s slope set to {(1, 0)[which]}")
    for k in (least if name not in B.LOOSE else ()):
        print(f"sharpness {name} {k}: max |ref| / bound per 16-row block from {least[k]:.3g} to {largest[k]:.3g}")
    trunk = [k for k in least if k.startswith(("cat_layers", "to_depth"))]
    print(f"sharpness {name}: over all tensors, the least block {min(least.values()):.3g}, the largest {max(largest.values()):.3g}; "
          f"trunk and head alone, the least block {min(least[k] for k in trunk):.3g}")


@pytest.mark.parametrize("name", NAMES)
def test_mutants(name):
    applied, unseen = set(), 0
    for key, c in _all(name):
        assert not B.differs(c["ref"], B.mutant_of(c)), "the reference is no mutant"
        for m in B.MUTANTS:
            other = B.mutant_of(c, mutant=m)
            if B.differs(c["ref"], other):
                applied.add(m)
                seen = B.rejected(c["ref"], other)
                if name in B.LOOSE and m in B.LOOSE_MUTANTS:
                    unseen += not seen
                    continue
                assert seen, f"{name} {key}: the comparison does not see {m}"
            else:
                assert not B.must_apply(m, c), f"{name} {key}: {m} is the chain itself"
    n = len(B.network(name)["cat"])
    expect = set(B.MUTANTS) - ({"dact_from_above", "dact_from_below", "branch_e_columns_missing", "branch_slot_below"} if n == 1 else set())
    assert applied == expect, (name, sorted(expect ^ applied))
    if name in B.LOOSE:
        print(f"{name}: {B.LOOSE_MUTANTS} go unseen on {unseen} cases (the bound outgrows the branch gradients there)")


class _LeakyF32Rule(torch.autograd.Function):
    """LeakyReLU as the f32 kernels state it, on float64 tensors: v > 0 ? v : fl32(fl32(0.01) v); the derivative from the output."""

    @staticmethod
    def forward(ctx, v):
        y = torch.where(v > 0, v, (B.SLOPE32 * v).float().double())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * torch.where(y > 0, 1.0, B.SLOPE32)


def _oracle_autograd(c, dtype, monkeypatch=None):
    """torch-CPU autograd of oracle.nerf_oracle.depthnet_forward in `dtype`: (z, name -> gradient) as float64 numpy."""
    P = X.pool()
    p = {k: v.to(dtype).requires_grad_() for k, v in X.state_dict(c["net"], c["head"]).items()}
    o, d = torch.from_numpy(P["o"][c["rays"]]).to(dtype), torch.from_numpy(P["d"][c["rays"]]).to(dtype)
    if monkeypatch is not None:
        monkeypatch.setattr(torch.nn.functional, "leaky_relu", lambda v, slope: _LeakyF32Rule.apply(v))
    z = O.depthnet_forward(p, o, d, sphere_radius=c["radius"], near=c["near"], far=c["far"])
    if monkeypatch is not None:
        monkeypatch.undo()
    assert z.dtype == dtype and z.shape == (c["R"], 1)
    z.backward(torch.from_numpy(c["dz"]).to(dtype))
    return z.detach().double().numpy(), {k: v.grad.double().numpy() for k, v in p.items()}


@pytest.mark.parametrize("name", NAMES)
def test_reference64_is_torch_float64_autograd_of_the_oracle(name, monkeypatch):
    """within 1e-12 of each entry's sum of magnitudes; exact zeros are zeros"""
    for key, c in _all(name):
        z, grads = _oracle_autograd(c, torch.float64, monkeypatch)
        assert np.abs(z - c["ref"]["z"]).max() <= 1e-12 * max(abs(c["near"]), abs(c["far"]))
        for k, (v, _) in c["ref"]["grads"].items():
            assert grads[k].shape == v.shape and (np.abs(grads[k] - v) <= 1e-12 * c["ref"]["mags"][k]).all(), (name, key, k)


@pytest.mark.parametrize("name", NAMES)
def test_the_fp32_oracle_stays_inside_the_bound(name):
    """the oracle's fp32 chain under torch autograd, the stand-in for a correct fp32 implementation: every entry accepted"""
    worst_z = worst_g = 0.0
    for key, c in _all(name):
        z, grads = _oracle_autograd(c, torch.float32)
        verdicts, _ = B.compare(z, grads, c["ref"])
        assert not B.failures(verdicts, c["ref"]), f"{name} {key}: {B.failures(verdicts, c['ref'])}"
        worst_z = max(worst_z, verdicts["z"].worst)
        worst_g = max(worst_g, max(v.worst for k, v in verdicts.items() if k != "z"))
    print(f"fp32 oracle on the CPU, {name}: worst |err| / bound: z {worst_z:.3f}, gradients {worst_g:.3f}")
    assert max(worst_z, worst_g) <= 1.0


def test_compare_rejects_a_nan_a_lost_entry_and_a_nonzero_where_a_zero_belongs():
    c = B.case("w24n1", B.cases("w24n1")[3])
    good = {k: v.astype(np.float32) for k, (v, _) in c["ref"]["grads"].items()}
    z = c["ref"]["z"].astype(np.float32)
    assert not B.failures(B.compare(z, good, c["ref"])[0], c["ref"])
    k = "cat_layers.0.bias"
    at = int(np.argmax(np.abs(good[k])))
    for bad_value in (np.nan, 0.0):
        bad = dict(good)
        bad[k] = good[k].copy()
        bad[k][at] = bad_value
        msg = B.failures(B.compare(z, bad, c["ref"])[0], c["ref"])
        assert msg.startswith(f"{k}: 1 of {good[k].size} entries outside the bound, first at ({at},)"), msg
    chain = next(B.case("w24n1", key) for key in B.cases("w24n1") if key[0] != "main")
    good = {k: v.astype(np.float32) for k, (v, _) in chain["ref"]["grads"].items()}
    bad = dict(good)
    bad["origin_layers.0.weight"] = good["origin_layers.0.weight"].copy()
    bad["origin_layers.0.weight"][3, 5] = 1e-30
    assert "origin_layers.0.weight: 1 of" in B.failures(B.compare(chain["ref"]["z"], bad, chain["ref"])[0], chain["ref"])
    bad["origin_layers.0.weight"][3, 5] = -0.0
    assert not B.failures(B.compare(chain["ref"]["z"], bad, chain["ref"])[0], chain["ref"])
