"""The depth-tangent check's own footing, on the CPU (tests/exact_tangent.py; the HIP kernels: tests/test_gpu_exact_tangent.py):
  * the conditions T1 - T4 and the caps, for every case the GPU test walks;
  * the float64 reference `jacobian64` against torch float64 autograd of the literal composition -- sort(cat[m + linspace, m]),
    clamp, the points, the chain with torch.relu, the oracle's raw2outputs -- one backward per output column;
  * an fp32 transcription of walk_samples / write_jacobian stays inside the error model's bound on every ray: the bound is not so
    tight that correct fp32 arithmetic fails it;
  * T5: the bound rejects every mutant on each N's full batch wherever it applies, and every mutant that can apply at all does
    somewhere."""

import numpy as np
import pytest
import torch

import exact_field as E
import exact_tangent as X
from oracle import nerf_oracle as O

PAIRS = [pytest.param(name, which, id=f"{name}-{which}") for name, which in X.TABLE]
_walked = {}


def _walk(name, which, instance):
    """[(case, reference)] of one network and instance, computed once"""
    key = (name, which, instance)
    if key not in _walked:
        net = X.network(name, which)
        _walked[key] = [(case, X.jacobian64(net, case, instance=instance)) for case in X.cases(net, instance)]
    return _walked[key]


@pytest.mark.parametrize("name,which", PAIRS)
def test_conditions_hold_for_every_case(name, which):
    net = X.network(name, which)
    every = [case for inst in X.INSTANCES for case, _ in _walk(name, which, inst)]
    c3 = X.check_t1(net, every)
    ok16 = X.check_t2(net)                                   # (asserts the f16x3 form and the quarter cap)
    t3 = X.check_t3(net)
    assert ok16.sum() >= 8
    for inst in X.INSTANCES:
        for case, ref in _walk(name, which, inst):
            assert np.isfinite(ref["J"]).all() and np.isfinite(ref["bound"]).all()
            if inst != "f16":                                # the f16x3 and one-sample cases draw on every pool ray
                assert len(X.allowed_rays(net, inst)) == X.POOL_RAYS
            else:
                assert ok16[case["ray"]].all()
            X.check_t4(ref)
    print(f"{name} on pool {which}: C3 2^{np.log2(c3):.1f}, T3 (tangent GEMMs) 2^{np.log2(t3):.1f}, "
          f"{int(ok16.sum())} of {X.POOL_RAYS} rays keep the f16 form")


def test_the_required_networks_are_in_the_table():
    assert all((name, "A") in X.TABLE for name in X.REQUIRED)
    assert ("prod", "B") in X.TABLE


def _autograd_jacobian(net, case):
    """d (r, g, b, disp, depth, acc) / d m of the finite-mean rays by torch float64 autograd of the literal composition"""
    keep = np.flatnonzero(np.isfinite(case["mean"]))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    rays, N = net["rays"], case["N"]
    o, d, v = (t(rays[k][case["ray"][keep]]) for k in ("o", "d", "viewdirs"))
    m = t(case["mean"][keep]).requires_grad_(True)
    R = len(keep)
    if N == 1:
        z = m[:, None]
    else:
        std = X.std_of(N, net["step"])
        grid = m[:, None] + torch.linspace(-std, std, N - 1, dtype=torch.float64)[None]
        z = torch.clamp(torch.sort(torch.cat([grid, m[:, None]], -1), -1)[0], X.NEAR, X.FAR)
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    x = torch.cat([pts, torch.zeros(R, z.shape[1], E.IN_PTS - 3, dtype=torch.float64)], -1)
    views = torch.cat([v, torch.zeros(R, E.IN_VIEWS - 3, dtype=torch.float64)], -1)[:, None, :].expand(R, z.shape[1], E.IN_VIEWS)
    w = {n: t(a) for n, a in zip(net["names"], net["weights"])}
    b = {n: t(a) for n, a in zip(net["names"], net["biases"])}
    lin = lambda n, h: h @ w[n].T + b[n]
    h = x
    for i in range(net["D"]):
        h = torch.relu(lin(f"pts{i}", h))
        if i in net["skips"]:
            h = torch.cat([x, h], -1)
    hv = torch.relu(lin("views", torch.cat([lin("feature", h), views], -1)))
    raw = torch.cat([lin("rgb", hv), lin("alpha", h)], -1)
    if N == 1:
        rgb = torch.sigmoid(raw[:, 0, :3])
        cols = [rgb[:, 0], rgb[:, 1], rgb[:, 2]]
    else:
        rgb, disp, acc, depth, *_ = O.raw2outputs(raw, z, d, 0.0, case["white"])
        cols = [rgb[:, 0], rgb[:, 1], rgb[:, 2], disp, depth, acc]
    J = np.zeros((R, 6))
    for c, col in enumerate(cols):
        (g,) = torch.autograd.grad(col.sum(), m, retain_graph=c + 1 < len(cols))
        J[:, c] = g.numpy()
    return J


@pytest.mark.parametrize("name,which", PAIRS)
def test_reference_is_float64_autograd_of_the_literal_composition(name, which):
    net = X.network(name, which)
    worst = 0.0
    for inst in ("f16x3", "single"):
        for case, ref in _walk(name, which, inst):
            if case["kind"] != "main":           # (the ray-count cases draw on the same depths and rays)
                continue
            Ja = _autograd_jacobian(net, case)
            # 1e-12 of the sum of magnitudes the entry is made of: d acc of an opaque ray is ~1e-10 left of terms of order 1
            err = np.abs(ref["J"] - Ja) / (np.abs(Ja) + ref["mag"] + 1e-300)
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-12, (name, which, case["N"], case["white"], float(err.max()))
    print(f"{name} on pool {which}: jacobian64 against float64 autograd, worst relative difference {worst:.2e}")


@pytest.mark.parametrize("name,which", PAIRS)
def test_fp32_transcription_of_the_walk_stays_inside_the_bound(name, which):
    net = X.network(name, which)
    worst = 0.0
    for inst in ("f16x3", "f16"):
        for case, ref in _walk(name, which, inst):
            ratio = np.abs(X.walk_fp32(net, case) - ref["J"]) / ref["bound"]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (name, which, inst, case["N"], len(case["mean"]), case["white"], float(ratio.max()))
    print(f"{name} on pool {which}: fp32 transcription of the walk, worst |J - J64| / bound {worst:.3f}")


@pytest.mark.parametrize("name,which", PAIRS)
def test_every_mutant_is_rejected(name, which):
    net = X.network(name, which)
    applied = {}
    for inst in X.INSTANCES:
        for case, ref in _walk(name, which, inst):
            # each N's full batch: it holds every depth of `means`, which is what puts the window where a mutant bites (across
            # sample 64, on a clip bound, ...); a ray-count batch draws a few of those depths and most mutants do not apply to it
            if case["kind"] != "main":
                continue
            for mutant, move in X.check_t5(net, case, ref, inst).items():
                applied[mutant] = min(applied.get(mutant, np.inf), move)
            if inst == "f16x3":
                for mutant in X.NEVER:               # what `applies` says of them: nothing an fp32 evaluation could show
                    got = X.jacobian64(net, case, mutant=mutant)["J"]
                    assert (np.abs(got - ref["J"]) <= 1e-3 * ref["bound"]).all(), mutant
    expect = set(X.MUTANTS) - set(X.NEVER) - {"relu_sigma0"} - (set() if net["skips"] else {"skip_d_dropped"})
    assert expect <= set(applied), sorted(expect - set(applied))
    print(f"{name} on pool {which}: smallest move / bound per mutant " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(applied.items())))
