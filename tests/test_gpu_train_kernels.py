"""The training step's small kernels on the GPU, entry by entry against float64 (tests/train_kernels_reference.py holds the
inputs, the references, the error models and the comparators; tests/test_train_kernels_host.py shows on the CPU that they reject
every mutant).  Called through the C ABI: ns_act_forward, ns_act_backward, ns_colsum (ld, M = 0), ns_posenc, ns_posenc_backward,
ns_points_along_rays, ns_points_backward, ns_adam_step, ns_adam_step_dev (lr_dev given and NULL), ns_adam_step_multi_dev (rows
with n = 0) and ns_add_i32.  Every buffer a kernel writes has a band of sentinels behind it that must survive, every read-only
input must come back unchanged, and no rejected entry is forgiven.  The float64 references run on the CPU."""

import ctypes as C

import numpy as np
import pytest
import torch

import train_kernels_reference as K
from nerf_sampling_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 7777.25
GUARD = 512                      # floats behind every buffer a kernel writes
LR_IGNORED = 0.5                 # the scalar learning rate passed beside an lr_dev: it must not be used


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(a):
    """A device copy of `a` (flattened) with GUARD sentinels behind it."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    buf = torch.full((a.size + GUARD,), SENTINEL, device="cuda")
    buf[:a.size] = torch.from_numpy(a)
    return buf


def _result(buf, n):
    """The first n floats on the host; the guard band must be intact."""
    host = buf.cpu().numpy()
    assert bool((host[n:] == np.float32(SENTINEL)).all()), "written behind the end of the buffer"
    return host[:n]


def _call(name, *args):
    lib = _lib.load()
    assert getattr(lib, name)(*args, _stream()) == 0, (name, lib.ns_last_error())


def _accept(verdict, what, unit=""):
    print(f"{what}: worst |err| / bound = {verdict.worst:.3f}{unit}")
    assert verdict.rejected.size == 0, (what, int(verdict.rejected.size), verdict.rejected[:8], verdict.worst)


# ---- activations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.ACT_SIZES)
def test_act_forward(n):
    x = K.gen_act(n, n)
    for act in (0, 1, 2, 3):
        buf = _guarded(x)
        _call("ns_act_forward", _ptr(buf), n, act)
        got = _result(buf, n)
        assert np.array_equal(np.isnan(got), np.isnan(x)), (n, act, "NaN in gives NaN out, and nothing else does")
        _accept(K.compare_act_forward(got, x, act), f"ns_act_forward act={act} n={n}")


@pytest.mark.parametrize("n", K.ACT_SIZES)
def test_act_backward(n):
    dy, y = K.gen_act_backward(n, n + 1)
    yd = _dev(y)
    for act in (0, 1, 2, 3):
        buf = _guarded(dy)
        _call("ns_act_backward", _ptr(buf), _ptr(yd), n, act)
        _accept(K.compare_act_backward(_result(buf, n), dy, y, act), f"ns_act_backward act={act} n={n}")
    assert K.compare_bits(yd.cpu().numpy(), y).rejected.size == 0, "the activation output is read-only"


# ---- column sums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integers", [True, False], ids=["int", "float"])
def test_colsum(integers):
    worst = 0.0
    for M in K.COLSUM_M:
        for N in K.COLSUM_N:
            for pad in K.COLSUM_PAD:
                X = K.gen_colsum(M, N, pad, 1000 * M + 10 * N + pad, integers)
                Xd = _dev(X) if M else torch.zeros(N + pad, device="cuda")          # M = 0: an address, never read
                out = torch.full((N + GUARD,), SENTINEL, device="cuda")
                _call("ns_colsum", _ptr(Xd), N + pad, M, N, _ptr(out))
                got = _result(out, N)
                if M == 0:
                    assert bool((got == 0).all()), (N, pad, "M = 0 gives zeros")
                v = K.compare_colsum(got, X, N, integers)
                assert v.rejected.size == 0, (M, N, pad, v.rejected[:8], v.worst)
                worst = max(worst, v.worst)
    print(f"ns_colsum integers={integers}: worst |err| / bound = {worst:.3f}")


# ---- positional encoding ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,d,L", K.POSENC_CASES + (K.POSENC_FWD_STRIDE,))
def test_posenc_forward(M, d, L):
    x, _ = K.gen_posenc(M, d, L, M + d + L)
    width = d * (1 + 2 * L)
    xd, out = _dev(x), torch.full((M * width + GUARD,), SENTINEL, device="cuda")
    _call("ns_posenc", _ptr(xd), M, d, L, _ptr(out))
    got = _result(out, M * width).reshape(M, width)
    v = K.compare_posenc(got, x, L)
    if L:
        err = np.abs(got[:, d:].astype(np.float64) - K.posenc64(x, L)[:, d:])
        at = np.unravel_index(int(err.argmax()), err.shape)
        print(f"ns_posenc {M}x{d} L={L}: worst trig error {err.max() / K.U:.3f} U at x = {x[at[0], at[1] % d]!r}, column {d + at[1]}")
    _accept(v, f"ns_posenc {M}x{d} L={L}")
    assert K.compare_bits(xd.cpu().numpy(), x).rejected.size == 0


@pytest.mark.parametrize("M,d,L", K.POSENC_CASES + (K.POSENC_BWD_STRIDE,))
def test_posenc_backward(M, d, L):
    x, de = K.gen_posenc(M, d, L, M + d + L)
    xd, ded, out = _dev(x), _dev(de), torch.full((M * d + GUARD,), SENTINEL, device="cuda")
    _call("ns_posenc_backward", _ptr(xd), _ptr(ded), M, d, L, _ptr(out))
    _accept(K.compare_posenc_backward(_result(out, M * d), x, de, L), f"ns_posenc_backward {M}x{d} L={L}")
    assert K.compare_bits(xd.cpu().numpy(), x).rejected.size == 0 and K.compare_bits(ded.cpu().numpy(), de).rejected.size == 0


# ---- points -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N", K.POINTS_CASES + (K.POINTS_FWD_STRIDE, K.POINTS_BWD_STRIDE))
def test_points_forward_and_backward(R, N):
    o, d, z, dpts = K.gen_points(R, N, R + N)
    od, dd, zd, dpd = _dev(o), _dev(d), _dev(z), _dev(dpts)
    pts = torch.full((R * N * 3 + GUARD,), SENTINEL, device="cuda")
    _call("ns_points_along_rays", _ptr(od), _ptr(dd), _ptr(zd), R, N, _ptr(pts))
    _accept(K.compare_points(_result(pts, R * N * 3), o, d, z), f"ns_points_along_rays {R}x{N}")
    dz = torch.full((R * N + GUARD,), SENTINEL, device="cuda")
    _call("ns_points_backward", _ptr(dpd), _ptr(dd), R, N, _ptr(dz))
    _accept(K.compare_points_backward(_result(dz, R * N), dpts, d), f"ns_points_backward {R}x{N}")
    for dev, host in ((od, o), (dd, d), (zd, z), (dpd, dpts)):
        assert K.compare_bits(dev.cpu().numpy(), host).rejected.size == 0, "inputs are read-only"


# ---- Adam -------------------------------------------------------------------------------------------------------------------
class AdamState:
    """p, m, v with guard bands and g on the device."""

    def __init__(self, s):
        self.n = s["p"].size
        self.p, self.m, self.v = (_guarded(s[k]) for k in "pmv")
        self.g = _dev(s["g"])

    def row(self):
        return [self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n]

    def result(self, s):
        assert K.compare_bits(self.g.cpu().numpy(), s["g"]).rejected.size == 0, "the gradient is read-only"
        return {k: _result(getattr(self, k), self.n) for k in "pmv"}


def _same_bits(a, b, what):
    for k in "pmv":
        assert K.compare_bits(a[k], b[k]).rejected.size == 0, (what, k)


@pytest.mark.parametrize("n,t", K.ADAM_CASES)
def test_adam_three_entries(n, t):
    """ns_adam_step (bias corrections on the host), ns_adam_step_dev with and without lr_dev, and a one-row
    ns_adam_step_multi_dev: each inside the bound, the device-step entries bit-identical to one another."""
    lr, b1, b2, eps = K.ADAM_HYPER["lr"], K.ADAM_HYPER["b1"], K.ADAM_HYPER["b2"], K.ADAM_HYPER["eps"]
    hyper = K.hyper32()
    s = K.gen_adam(n, n + t)
    step = torch.tensor([t], dtype=torch.int32, device="cuda")              # set directly: nothing steps there
    lr_dev = torch.tensor([lr], dtype=torch.float32, device="cuda")
    tag = f"n={n} t={t}"

    a = AdamState(s)
    _call("ns_adam_step", _ptr(a.p), _ptr(a.g), _ptr(a.m), _ptr(a.v), n, lr, b1, b2, eps, t)
    host_bc = a.result(s)
    _accept(K.compare_adam(host_bc, s, t, *hyper), f"ns_adam_step {tag}")

    results = {}
    for name, scalar, ptr in (("lr_dev NULL", lr, None), ("lr_dev given", LR_IGNORED, lr_dev)):
        a = AdamState(s)
        _call("ns_adam_step_dev", _ptr(a.p), _ptr(a.g), _ptr(a.m), _ptr(a.v), n, scalar, _ptr(ptr), b1, b2, eps, _ptr(step))
        results[name] = a.result(s)
        _accept(K.compare_adam(results[name], s, t, *hyper), f"ns_adam_step_dev {name} {tag}")
        a = AdamState(s)
        table = torch.tensor([a.row()], dtype=torch.int64).cuda()
        _call("ns_adam_step_multi_dev", _ptr(table), 1, n, scalar, _ptr(ptr), b1, b2, eps, _ptr(step))
        _same_bits(a.result(s), results[name], f"ns_adam_step_multi_dev against ns_adam_step_dev, {name} {tag}")
    _same_bits(results["lr_dev NULL"], results["lr_dev given"], "the learning rate from the device against the scalar " + tag)
    assert int(step) == t and float(lr_dev) == np.float32(lr)


@pytest.mark.parametrize("use_lr_dev", [False, True], ids=["lr-scalar", "lr-dev"])
def test_adam_multi_tensor_table(use_lr_dev):
    """70 tensors of mixed sizes in one launch (rows with n = 0 carry NULL pointers; the largest tensor, which takes the
    grid-stride loop, sits inside the table): every tensor inside the bound and bit-identical to its own ns_adam_step_dev."""
    lr, b1, b2, eps = K.ADAM_HYPER["lr"], K.ADAM_HYPER["b1"], K.ADAM_HYPER["b2"], K.ADAM_HYPER["eps"]
    hyper, t = K.hyper32(), 2
    sizes = K.gen_adam_table(70)
    assert 0 in sizes and sizes[-1] > 0 and max(sizes) not in (sizes[0], sizes[-1]) and max(sizes) > K.STRIDE_THRESHOLD
    step = torch.tensor([t], dtype=torch.int32, device="cuda")
    lr_dev = torch.tensor([lr], dtype=torch.float32, device="cuda") if use_lr_dev else None
    scalar = LR_IGNORED if use_lr_dev else lr
    states = [K.gen_adam(n, 7000 + i) for i, n in enumerate(sizes)]
    multi = [AdamState(s) if s["p"].size else None for s in states]
    table = torch.tensor([a.row() if a else [0, 0, 0, 0, 0] for a in multi], dtype=torch.int64).cuda()
    _call("ns_adam_step_multi_dev", _ptr(table), len(sizes), max(sizes), scalar, _ptr(lr_dev), b1, b2, eps, _ptr(step))
    worst = 0.0
    for i, (s, a) in enumerate(zip(states, multi)):
        if a is None:
            continue
        got = a.result(s)
        v = K.compare_adam(got, s, t, *hyper)
        assert v.rejected.size == 0, (i, sizes[i], v.rejected[:8], v.worst)
        worst = max(worst, v.worst)
        one = AdamState(s)
        _call("ns_adam_step_dev", _ptr(one.p), _ptr(one.g), _ptr(one.m), _ptr(one.v), one.n, scalar, _ptr(lr_dev), b1, b2, eps,
              _ptr(step))
        _same_bits(got, one.result(s), f"row {i} (n = {sizes[i]}) against ns_adam_step_dev")
    print(f"ns_adam_step_multi_dev, {len(sizes)} rows, lr_dev={use_lr_dev}: worst |err| / bound = {worst:.3f}")
    assert int(step) == t


def test_add_i32():
    x = torch.tensor([5, 77], dtype=torch.int32, device="cuda")
    for delta, want in ((3, 8), (-10, -2), (0, -2), (100000, 99998), (-100000, -2)):
        _call("ns_add_i32", _ptr(x), delta)
        assert x.tolist() == [want, 77], delta


def test_hip_adam_device_step_matches_torch_adam():
    """HipAdam in device-step mode (one multi-tensor launch per step) against torch.optim.Adam on the CPU: five parameters, one
    of them past the grid-stride threshold, one with a non-contiguous gradient, one that never has a gradient; eight steps, the
    learning rate changed at the fifth."""
    from nerf_sampling_amd.autograd import HipAdam

    g = torch.Generator().manual_seed(11)
    shapes = [(1,), (300, 17), (256, 319), (65537,), (40, 3)]
    init = [torch.randn(sh, generator=g) for sh in shapes]
    mine = [w.clone().cuda().requires_grad_(True) for w in init]
    ref = [w.clone().requires_grad_(True) for w in init]
    oa, ob = HipAdam(mine, lr=1e-3), torch.optim.Adam(ref, lr=1e-3)
    oa.use_device_step()
    for k in range(8):
        if k == 4:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 3e-4
        for i, sh in enumerate(shapes[:4]):
            grad = torch.randn(sh, generator=g)
            if i == 1:                                       # a transposed view: not contiguous
                grad_t = grad.t().contiguous().cuda()
                mine[i].grad = grad_t.t()
                assert not mine[i].grad.is_contiguous()
            else:
                mine[i].grad = grad.cuda()
            ref[i].grad = grad.clone()
        oa.step()
        ob.step()
    for a, b, w0 in zip(mine[:4], ref[:4], init[:4]):
        assert torch.allclose(a.detach().cpu(), b.detach(), rtol=1e-5, atol=1e-6)
        sa, sb = oa.state[a], ob.state[b]
        assert torch.allclose(sa["exp_avg"].cpu(), sb["exp_avg"], rtol=1e-5, atol=1e-6)
        assert torch.allclose(sa["exp_avg_sq"].cpu(), sb["exp_avg_sq"], rtol=1e-5, atol=1e-6)
        assert not torch.equal(a.detach().cpu(), w0)
    assert torch.equal(mine[4].detach().cpu(), init[4]), "a parameter without a gradient is bit-unchanged"
    assert len(oa.state.get(mine[4], {})) == 0 and len(ob.state.get(ref[4], {})) == 0, "and has no state"
    sd = oa.state_dict()["state"]
    assert all(float(sd[i]["step"]) == 8.0 for i in range(4))
