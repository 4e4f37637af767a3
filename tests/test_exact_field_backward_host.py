"""The exact backward of tests/exact_field_backward.py on the CPU (no GPU needed): the conditions B1 - B4 on every case of the
table tests/test_gpu_exact_field_backward.py walks, every mutant of the chain rejected by that test's comparison, and torch-CPU
autograd of the literal chain, in float64 and in fp32, equal to `backward64` bit for bit -- fp32 arithmetic reproduces the
reference on this machine, so a mismatch on the GPU is the library's."""
import numpy as np
import pytest
import torch

import exact_field as E
import exact_field_backward as B
import train_kernels_reference as T

NAMES = list(E.NETWORKS)


def _cases(name, columns):
    """(label, case dict) of every case of one network."""
    if columns == "all":
        return [(f"M={M}", B.chain_case(name, M)) for M in B.CHAIN_M]
    return [(f"rays {R}x{N}", B.ray_case(name, R, N)) for R, N in E.RAY_SHAPES]


@pytest.mark.parametrize("columns", E.COLUMNS)
@pytest.mark.parametrize("name", NAMES)
def test_conditions_and_mutants(name, columns):
    worst = {}
    for label, c in _cases(name, columns):
        net, x, draw = c["net"], c["x"], c["draw"]
        fwd = E.chain(net, x, keep=True)
        assert (fwd[0] == c["ref"]["raw"]).all()
        B.check_b1(net, x, draw, forward=fwd)
        B.check_b2(net, x, forward=fwd)
        worst[label] = B.check_b3(net, x, draw, forward=fwd)
        B.check_b4(net, x, draw, ref=c["ref"], forward=fwd)
    print(f"B3 {name} {columns}: " + ", ".join(f"{k}: 2^{np.log2(v):.2f} ({what})" for k, (v, what) in worst.items()))


def test_every_mutant_applies_somewhere_and_the_reference_is_no_mutant():
    seen = set()
    for name in NAMES:
        net = E.network(name, "all")
        seen |= {m for m in B.MUTANTS for M in B.CHAIN_M if B.applies(m, net, M)}
    assert seen == set(B.MUTANTS)
    c = B.chain_case("d5w128s03", 17)
    assert not B.rejected(c["ref"], B.backward64(c["net"], c["x"], c["draw"]))
    # a mutant that does not apply is the chain itself
    c = B.chain_case("d2w128", 1024)
    for m in ("skip_split_62", "dw_last_slice_missing", "output_ch_4"):
        assert not B.applies(m, c["net"], 1024) and not B.rejected(c["ref"], B.backward64(c["net"], c["x"], c["draw"], mutant=m))


def _torch_backward(net, x, draw, dtype):
    """torch-CPU autograd of the literal chain (run_nerf_helpers.py:114-133) in `dtype`: dict name -> numpy float64, B.compared's keys."""
    F = torch.nn.functional
    w = {n: torch.from_numpy(a).to(dtype).requires_grad_() for n, a in zip(net["names"], net["weights"])}
    b = {n: torch.from_numpy(a).to(dtype).requires_grad_() for n, a in zip(net["names"], net["biases"])}
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    xe = xt[:, :E.IN_PTS].clone().requires_grad_()
    h = xe
    for i in range(net["D"]):
        h = F.relu(F.linear(h, w[f"pts{i}"], b[f"pts{i}"]))
        if i in net["skips"]:
            h = torch.cat([xe, h], -1)
    if net["use_viewdirs"]:
        alpha = F.linear(h, w["alpha"], b["alpha"])
        feature = F.linear(h, w["feature"], b["feature"])
        hv = F.relu(F.linear(torch.cat([feature, xt[:, E.IN_PTS:]], -1), w["views"], b["views"]))
        raw = torch.cat([F.linear(hv, w["rgb"], b["rgb"]), alpha], -1)
    else:
        raw = F.linear(h, w["output"], b["output"])
    raw.backward(torch.from_numpy(draw).to(dtype))
    out = {"raw": raw.detach(), "d xe": xe.grad}
    for n in net["names"]:
        out[f"dW {n}"], out[f"db {n}"] = w[n].grad, b[n].grad
    return {k: v.double().numpy() for k, v in out.items()}


@pytest.mark.parametrize("columns", E.COLUMNS)
@pytest.mark.parametrize("name", NAMES)
def test_torch_autograd_in_float64_and_in_fp32_equals_backward64(name, columns):
    for label, c in _cases(name, columns):
        want = B.compared(c["ref"])
        for dtype in (torch.float64, torch.float32):
            got = _torch_backward(c["net"], c["x"], c["draw"], dtype)
            assert set(got) == set(want)
            for k in want:
                assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (name, columns, label, dtype, k)


@pytest.mark.parametrize("name", NAMES)
def test_draws(name):
    net = E.network(name, "all")
    C = net["output_ch"]
    for columns in E.COLUMNS:
        for label, c in _cases(name, columns):
            g, M = c["draw"], c["x"].shape[0]
            wide = columns == "all" and M == B.WIDE_M
            assert g.shape == (M, C) and np.isin(g, np.arange(-2, 3) if wide else np.arange(-1, 2)).all(), label
            assert wide == bool((np.abs(g) == 2).any())
            assert (g != 0).any(axis=0).all() and (g.sum(axis=0) != 0).all(), f"{label}: a channel without a gradient"
            assert all((g[lo:lo + 16] != 0).any() for lo in range(0, M, 16)), f"{label}: a block of 16 rows without a gradient"
    thin = B.make_draw(net, 4000, seed=1, one_channel=True)
    assert ((thin != 0).sum(axis=1) <= 1).all() and (thin != 0).sum() == 250
    assert ((B.make_draw(net, 4000, seed=1, density=0.0) != 0).any(axis=1).sum()) == 250
    assert set(B.THIN) <= {(n, "identity", R * N) for n in NAMES for R, N in E.RAY_SHAPES}


@pytest.mark.parametrize("name", NAMES)
def test_sine_and_cosine_columns_of_the_public_path(name):
    """The dW columns that multiply sines and cosines: the exact dy times an fp32 encoding (numpy's sinf and cosf) lies inside the
    bound in fp32 arithmetic, an encoding with sin and cos swapped in band 0 does not, and the exact part of the same tensors is
    the reference on the zeroed input."""
    for R, N in E.RAY_SHAPES:
        c = B.ray_case(name, R, N)
        net, ref = c["net"], c["ref"]
        assert set(c["trig"]) == set(B.trig_layers(net)) and c["pts"].shape == (R, N, 3)
        assert (c["x"][:, :3] == c["pts"].reshape(-1, 3)).all() and E.is_f32(c["pts"])
        dys = B.backward64(net, c["x"], c["draw"], keep_dy=tuple(c["trig"]))["dy"]
        worst = 0.0
        for lname, (lo, hi, want, bound) in c["trig"].items():
            assert want.shape == bound.shape == (ref["dW"][lname].shape[0], hi - lo)
            assert not ref["dW"][lname][:, lo:hi].any() and not B.exact_columns(net, lname)[lo:hi].any()
            assert B.exact_columns(net, lname).sum() == ref["dW"][lname].shape[1] - (hi - lo)
            src, L = (c["pts"].reshape(-1, 3), 10) if lo == 3 else (c["x"][:, E.IN_PTS:E.IN_PTS + 3], 4)
            dy32 = dys[lname].astype(np.float32)
            got = dy32.T @ T.posenc32(src.astype(np.float32), L)[:, 3:]
            v = T.compare_bound(got, want, bound)
            assert v.rejected.size == 0, (name, R, N, lname, v.rejected[:5])
            worst = max(worst, v.worst)
            bad = dy32.T @ T.posenc32(src.astype(np.float32), L, mutant="sin_cos_swapped")[:, 3:]
            assert T.compare_bound(bad, want, bound).rejected.size > 0, (name, R, N, lname)
        print(f"sine / cosine columns {name} {R}x{N}: worst |err| / bound of the fp32 CPU sum = {worst:.3f}")


def test_first_difference_names_the_tensor():
    want = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    assert B.first_difference(want.clone(), want, "dW pts0") == ""
    got = want.clone()
    got[2, 1] = -1
    msg = B.first_difference(got, want, "dW pts0")
    assert msg.startswith("dW pts0: 1 of 12 values differ; first at row 2 channel 1") and "got -1.0, expected 7.0" in msg
    assert "shape" in B.first_difference(want[:3], want, "db")
    vec = torch.arange(5, dtype=torch.float32)
    bad = vec.clone()
    bad[3] = 9
    assert "first at row 3 channel 0" in B.first_difference(bad, vec, "db rgb")
