"""The field fit's backward pass against the one correct answer, bit for bit (needs a GPU).

What joins ns_gemm_fused, ns_gemm_tall and ns_gemm_wgrad into a backward pass -- autograd._nerf_layers_forward,
_nerf_layers_backward, NerfFunction and NerfInputGrad: which columns of a skip layer's weight belong to the embedding, which
activation masks which gradient, the sigma head accumulated in place under the trunk's last ReLU, `d raw` read as two strided
views, the view layer's first W columns, and what each ns_gemm_wgrad call receives -- runs on the exactly representable networks
of tests/exact_field.py with an integer `d raw`.  tests/test_exact_field_backward_host.py proves for every case used here that
every sum of the backward is an fp32 number in any order (B1 - B4 of tests/exact_field_backward.py), so the float64 transposed
chain converted to fp32 is the only correct `raw`, `d xe`, `dW` and `db`: no tolerance, both engines, and no other kernel on the
other side of the comparison.  Every exact comparison is torch.equal on values (-0.0 equals 0.0, a NaN equals nothing); a
mismatch names the tensor, the first differing (row, column) and both values.

The public path (nerf_forward_train, NerfInputGrad) embeds the points itself, so it runs on the "identity" networks, whose sine
and cosine columns carry zero weights: `raw`, `d pts`, every `db` and the `dW` columns of identity and hidden inputs are exact;
the `dW` columns that multiply sines and cosines are held to exact_field_backward.ray_case's bound (rows * 2^-24 * sum |dy x|
plus train_kernels_reference.TRIG * sum |dy|) against float64.
"""
import pytest
import torch

import exact_field as E
import exact_field_backward as B
import train_kernels_reference as T

pytestmark = pytest.mark.gpu

NAMES = list(E.NETWORKS)
_modules = {}
_expected = {}


def _layers(mod, net):
    """The module's Linears in exact_field.layer_names' order."""
    lins = list(mod.pts_linears)
    lins += [mod.feature_linear, mod.alpha_linear, mod.views_linears[0], mod.rgb_linear] if net["use_viewdirs"] else [mod.output_linear]
    assert len(lins) == len(net["names"])
    return dict(zip(net["names"], lins))


def _module(name, columns):
    """run_nerf_helpers.NeRF holding the network's weights, on the device, cached for the module."""
    if (name, columns) not in _modules:
        from nerf_sampling_amd.run_nerf_helpers import NeRF

        net = E.network(name, columns)
        mod = NeRF(D=net["D"], W=net["W"], input_ch=E.IN_PTS, input_ch_views=E.IN_VIEWS, output_ch=net["output_ch"],
                   skips=list(net["skips"]), use_viewdirs=net["use_viewdirs"])
        w, b = E.tensors(net)
        with torch.no_grad():
            for lin, wt, bt in zip(_layers(mod, net).values(), w, b):
                assert lin.weight.shape == wt.shape and lin.bias.shape == bt.shape
                lin.weight.copy_(wt)
                lin.bias.copy_(bt)
        _modules[name, columns] = mod.to("cuda")
    return _modules[name, columns]


def _want(key, case):
    """The float64 reference of a case as fp32 device tensors, cached for the module."""
    if key not in _expected:
        _expected[key] = {k: torch.from_numpy(v).float().cuda() for k, v in B.compared(case["ref"]).items()}
    return _expected[key]


def _same(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        assert not torch.isnan(got[k]).any(), f"{what} {k}: NaN"
        diff = B.first_difference(got[k], want[k], f"{what}: {k}")
        assert not diff, diff


def _run_chain(name, case, engine, want_input=True, draw=None):
    """_nerf_layers_forward and _nerf_layers_backward on a case's rows, every Linear's (dW, db) from linear_backward_weight_splitk:
    dict with B.compared's keys ("d xe" left out without want_input)."""
    from nerf_sampling_amd import autograd as A

    net = case["net"]
    mod = _module(name, "all")
    names = {id(lin): n for n, lin in _layers(mod, net).items()}
    x = torch.from_numpy(case["x"]).float().cuda()
    xe = x[:, :E.IN_PTS].contiguous()
    ve = x[:, E.IN_PTS:].contiguous() if net["use_viewdirs"] else None
    if draw is None:
        draw = torch.from_numpy(case["draw"]).float().cuda()
    out = {}

    def collect(lin, dy, xin):
        n = names[id(lin)]
        assert f"dW {n}" not in out, f"{n}: a second weight gradient"
        out[f"dW {n}"], out[f"db {n}"] = A.linear_backward_weight_splitk(dy, xin)

    with torch.no_grad():
        raw, saved = A._nerf_layers_forward(mod, xe, ve, True, engine)
        dxe = A._nerf_layers_backward(mod, saved, draw, weight_grad=collect, want_input=want_input, engine=engine)
    torch.cuda.synchronize()
    out["raw"] = raw
    if want_input:
        out["d xe"] = dxe
    else:
        assert dxe is None
    return out


@pytest.mark.parametrize("engine", ["tile", "tall"])
@pytest.mark.parametrize("name", NAMES)
def test_chain(name, engine):
    """raw, d xe and every dW and db of the chain itself, at row counts with partial tiles (17, 257) and on both sides of
    ns_gemm_wgrad's first split of the rows (1024 | 1025)"""
    for M in B.CHAIN_M:
        case = B.chain_case(name, M)
        _same(_run_chain(name, case, engine), _want((name, M), case), f"{name} {engine} M={M}")


@pytest.mark.parametrize("engine", ["tile", "tall"])
@pytest.mark.parametrize("name", NAMES)
def test_chain_without_input_gradient_and_with_a_strided_d_raw(name, engine):
    """want_input=False returns no d xe and leaves every weight gradient as it was; d raw as a column slice of a wider tensor
    changes nothing"""
    for M in B.CHAIN_M:
        case = B.chain_case(name, M)
        want = dict(_want((name, M), case))
        C = case["draw"].shape[1]
        wide = torch.full((M, C + 3), 7.0, dtype=torch.float32, device="cuda")
        wide[:, 2:2 + C] = torch.from_numpy(case["draw"]).float().cuda()
        view = wide[:, 2:2 + C]
        assert not view.is_contiguous() or M == 1
        _same(_run_chain(name, case, engine, draw=view), want, f"{name} {engine} M={M} strided d raw")
        del want["d xe"]
        _same(_run_chain(name, case, engine, want_input=False), want, f"{name} {engine} M={M} want_input=False")


def _ray_inputs(case):
    pts = torch.from_numpy(case["pts"]).float().cuda()
    v = None if case["viewdirs"] is None else torch.from_numpy(case["viewdirs"]).float().cuda()
    draw = torch.from_numpy(case["draw"]).float().cuda().reshape(pts.shape[0], pts.shape[1], -1)
    return pts, v, draw


def _run_public(name, case, engine):
    """nerf_forward_train and raw.backward(d raw): (raw, d pts, name -> dW, name -> db)."""
    from nerf_sampling_amd.autograd import nerf_forward_train

    mod = _module(name, "identity")
    mod.zero_grad(set_to_none=True)
    pts, v, draw = _ray_inputs(case)
    pts.requires_grad_(True)
    raw = nerf_forward_train(mod, pts, v, engine)
    raw.backward(draw)
    torch.cuda.synchronize()
    lins = _layers(mod, case["net"])
    dW = {n: lin.weight.grad.clone() for n, lin in lins.items()}
    db = {n: lin.bias.grad.clone() for n, lin in lins.items()}
    mod.zero_grad(set_to_none=True)
    return raw.detach(), pts.grad, dW, db


def _flat(run):
    raw, dpts, dW, db = run
    return {"raw": raw, "d pts": dpts, **{f"dW {n}": t for n, t in dW.items()}, **{f"db {n}": t for n, t in db.items()}}


def _check_public(name, case, engine, shape):
    net = case["net"]
    want = _want((name, shape), case)
    what = f"{name} {engine} rays {shape[0]}x{shape[1]}"
    raw, dpts, dW, db = _run_public(name, case, engine)
    got = {"raw": raw.reshape(-1, raw.shape[-1]), "d pts": dpts.reshape(-1, 3)}
    exp = {"raw": want["raw"], "d pts": want["d xe"][:, :3].contiguous()}
    assert not want["d xe"][:, 3:].any()
    worst = 0.0
    for n in net["names"]:
        keep = torch.from_numpy(B.exact_columns(net, n)).cuda()
        got[f"db {n}"], exp[f"db {n}"] = db[n], want[f"db {n}"]
        got[f"dW {n}"], exp[f"dW {n}"] = dW[n][:, keep], want[f"dW {n}"][:, keep]
        if n in case["trig"]:
            lo, hi, ref, bound = case["trig"][n]
            v = T.compare_bound(dW[n][:, lo:hi].cpu().numpy(), ref, bound)
            worst = max(worst, v.worst)
            first = (int(v.rejected[0]) // (hi - lo), lo + int(v.rejected[0]) % (hi - lo)) if v.rejected.size else None
            assert first is None, f"{what}: dW {n}: {v.rejected.size} sine / cosine entries outside the bound, first (row, column) {first}"
    print(f"{what}: sine / cosine columns of dW, worst |err| / bound = {worst:.3f}")
    _same(got, exp, what)


@pytest.mark.parametrize("engine", ["tile", "tall"])
@pytest.mark.parametrize("name", NAMES)
def test_public_path(name, engine):
    """nerf_forward_train(...).backward on points and view directions: NerfFunction with the embedding in front"""
    for R, N in E.RAY_SHAPES:
        _check_public(name, B.ray_case(name, R, N), engine, (R, N))


@pytest.mark.parametrize("name", NAMES)
def test_input_gradient_of_the_frozen_field(name):
    """NerfInputGrad: the packed kernel forward, the recomputed chain backward"""
    from nerf_sampling_amd import ops
    from nerf_sampling_amd.autograd import NerfInputGrad

    ops.set_compute_dtype("f32")
    mod = _module(name, "identity")
    for R, N in E.RAY_SHAPES:
        case = B.ray_case(name, R, N)
        want = _want((name, (R, N)), case)
        pts, v, draw = _ray_inputs(case)
        pts.requires_grad_(True)
        raw = NerfInputGrad.apply(pts, v, mod)
        raw.backward(draw)
        torch.cuda.synchronize()
        _same({"raw": raw.detach().reshape(-1, raw.shape[-1]), "d pts": pts.grad.reshape(-1, 3)},
              {"raw": want["raw"], "d pts": want["d xe"][:, :3].contiguous()}, f"{name} NerfInputGrad rays {R}x{N}")


@pytest.mark.parametrize("name", NAMES)
def test_engines_agree(name):
    """"tile" and "tall" return identical bits on every case above (the sine and cosine columns of dW included: both engines
    hand ns_gemm_wgrad the same operands)"""
    for M in B.CHAIN_M:
        case = B.chain_case(name, M)
        tile, tall = _run_chain(name, case, "tile"), _run_chain(name, case, "tall")
        assert set(tile) == set(tall)
        for k in tile:
            diff = B.first_difference(tall[k], tile[k], f"{name} M={M}: {k} of engine tall against engine tile")
            assert not diff, diff
    for R, N in E.RAY_SHAPES:
        case = B.ray_case(name, R, N)
        a, b = _flat(_run_public(name, case, "tile")), _flat(_run_public(name, case, "tall"))
        for k in a:
            diff = B.first_difference(b[k], a[k], f"{name} rays {R}x{N}: {k} of engine tall against engine tile")
            assert not diff, diff
