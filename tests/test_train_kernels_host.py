"""tests/train_kernels_reference.py on the CPU, at every case tests/test_gpu_train_kernels.py runs: the generators meet their
stated conditions, the float64 references agree with torch float64 autograd and a float64 torch.optim.Adam, the fp32 oracle is
accepted on every entry (the worst |err| / bound is printed), and every mutant is rejected."""

import numpy as np
import pytest
import torch

import train_kernels_reference as K

F32 = np.float32


def _accepted(verdict, what):
    assert verdict.rejected.size == 0, (what, verdict.rejected[:8], verdict.worst)
    assert verdict.worst <= 1.0, (what, verdict.worst)
    print(f"{what}: fp32 oracle worst |err| / bound = {verdict.worst:.3f}")
    return verdict.worst


def _rejected(verdict, what):
    assert verdict.rejected.size > 0, f"mutant not rejected: {what}"


# ---- activations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.ACT_SIZES)
def test_activations(n):
    x = K.gen_act(n, n)
    assert x.dtype == F32 and x.shape == (n,)
    planted = K.ACT_PLANTED
    if n >= len(planted):
        assert K.compare_bits(x[:len(planted)], planted).rejected.size == 0
        assert np.isnan(x).any() and np.isinf(x).any() and (x == 0).any() and np.signbit(x[x == 0]).any()
    if n >= 2 * len(planted):
        assert K.compare_bits(x[-len(planted):], planted).rejected.size == 0
        mags = np.abs(x[np.isfinite(x)])
        assert mags.max() > 200 and (mags[mags > 0] < 1e-3).any()
        assert ((x > -103) & (x < -89)).any(), "draws on the stretch where expf(-v) overflows"
    for act in (0, 1, 2, 3):
        y = K.act_forward32(x, act)
        assert np.array_equal(np.isnan(y), np.isnan(x)), "NaN in gives NaN out"
        _accepted(K.compare_act_forward(y, x, act), f"act_forward {act} n={n}")
    fin = np.isfinite(x)
    ref = torch.from_numpy(x[fin]).double()
    assert np.array_equal(K.act_forward32(x, 1)[fin], torch.relu(torch.from_numpy(x[fin])).numpy())
    assert np.allclose(K.sigmoid64(x[fin]), torch.sigmoid(ref).numpy(), rtol=1e-14, atol=1e-300)
    _rejected(K.compare_act_forward(K.act_forward32(x, 3, "sigmoid_no_negation"), x, 3), "sigmoid without the negation")
    _rejected(K.compare_act_forward(K.act_forward32(x, 2, "leaky_slope"), x, 2), "leaky slope 0.1")
    if np.isnan(x).any():
        dropped = np.where(np.isnan(x), F32(0), K.act_forward32(x, 1))
        _rejected(K.compare_act_forward(dropped, x, 1), "a relu that returns 0 for NaN, as fmaxf(v, 0) does")

    dy, y = K.gen_act_backward(n, n + 1)
    assert (y == 0).any() if n > 1 else y[0] == 0
    for act in (0, 1, 2, 3):
        _accepted(K.compare_act_backward(K.act_backward32(dy, y, act), dy, y, act), f"act_backward {act} n={n}")
    assert K.act_backward32(dy, y, 1)[0] == 0 and K.act_backward32(dy, y, 2)[0] == dy[0] * K.LEAKY      # y = 0
    _rejected(K.compare_act_backward(K.act_backward32(dy, y, 2, "leaky_slope"), dy, y, 2), "leaky' 0.1")
    # torch agrees about the derivative at y = 0 (relu' = 0, leaky' = 0.01) and everywhere else
    yt = torch.from_numpy(y[np.isfinite(y)]).clone().requires_grad_(True)
    dyt = torch.from_numpy(dy[np.isfinite(y)])
    for act, fn in ((1, torch.relu), (2, lambda t: torch.nn.functional.leaky_relu(t, 0.01))):
        yt.grad = None
        (fn(yt) * dyt).sum().backward()           # for relu and leaky the output has the sign of the input
        assert np.array_equal(yt.grad.numpy(), K.act_backward32(dyt.numpy(), yt.detach().numpy(), act))


# ---- column sums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integers", [True, False], ids=["int", "float"])
def test_column_sums(integers):
    worst = 0.0
    before = np.full(300, 7777.25, dtype=F32)
    for M in K.COLSUM_M:
        for N in K.COLSUM_N:
            for pad in K.COLSUM_PAD:
                X = K.gen_colsum(M, N, pad, 1000 * M + 10 * N + pad, integers)
                assert X.shape == (M, N + pad) and X.dtype == F32 and bool((X[:, N:] == K.COLSUM_POISON).all())
                if integers:
                    assert M <= 2 ** 17 and bool((np.abs(X[:, :N]) <= 64).all()) and bool((X[:, :N] == np.round(X[:, :N])).all())
                if M:
                    assert bool((np.abs(X[-1, :N]) >= 1).all())
                    assert float(K.colsum_bound(X, N).max()) < 1.0
                tag = f"colsum {M}x{N} ld={N + pad}"
                got = K.colsum32(X, N)
                if M == 0:
                    assert bool((got == 0).all())
                v = K.compare_colsum(got, X, N, integers)
                assert v.rejected.size == 0 and v.worst <= 1.0, (tag, v)
                worst = max(worst, v.worst)
                if M:
                    _rejected(K.compare_colsum(K.colsum32(X, N, mutant="last_row_dropped"), X, N, integers), tag + " last row dropped")
                _rejected(K.compare_colsum(K.colsum32(X, N, before, "last_column_not_written"), X, N, integers),
                          tag + " last column not written")
    print(f"colsum integers={integers}: fp32 oracle worst |err| / bound = {worst:.3f}")


# ---- positional encoding ----------------------------------------------------------------------------------------------------
def _torch_posenc(x, L):
    out = [x]
    for l in range(L):
        out += [torch.sin(x * 2.0 ** l), torch.cos(x * 2.0 ** l)]
    return torch.cat(out, -1)


@pytest.mark.parametrize("M,d,L", K.POSENC_CASES + (K.POSENC_FWD_STRIDE, K.POSENC_BWD_STRIDE))
def test_positional_encoding(M, d, L):
    x, de = K.gen_posenc(M, d, L, M + d + L)
    assert x.shape == (M, d) and de.shape == (M, d * (1 + 2 * L)) and float(np.abs(x).max()) <= 4.0
    flat = x.reshape(-1)
    if flat.size >= 5:
        assert flat[0] == 0 and flat[3] == 4 and flat[4] == -4 and flat[1] == -flat[2]
        assert abs(np.cos(float(flat[1]) * 2.0 ** (max(L, 1) - 1))) < 1e-7, "the top band sits at a zero of cos"
    if M * d * (1 + 2 * L) > K.EW_GRID:
        assert (M, d, L) in (K.POSENC_FWD_STRIDE, K.POSENC_BWD_STRIDE)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    enc = _torch_posenc(xt, L)
    (enc * torch.from_numpy(de).double()).sum().backward()
    ref, (dref, dbound) = K.posenc64(x, L), K.posenc_backward64(x, de, L)
    assert np.allclose(ref, enc.detach().numpy(), rtol=0, atol=1e-13)
    assert bool((np.abs(dref - xt.grad.numpy()) <= 1e-6 * dbound + 1e-300).all())
    tag = f"posenc {M}x{d} L={L}"
    _accepted(K.compare_posenc(K.posenc32(x, L), x, L), tag + " forward")
    _accepted(K.compare_posenc_backward(K.posenc_backward32(x, de, L), x, de, L), tag + " backward")
    if L >= 1:
        _rejected(K.compare_posenc(K.posenc32(x, L, "sin_cos_swapped"), x, L), tag + " sin and cos swapped")
        _rejected(K.compare_posenc(K.posenc32(x, L, "top_band_frequency"), x, L), tag + " top band frequency")
        _rejected(K.compare_posenc_backward(K.posenc_backward32(x, de, L, "reads_next_column"), x, de, L), tag + " next column")
    if L >= 2:
        _rejected(K.compare_posenc_backward(K.posenc_backward32(x, de, L, "no_frequency_factor"), x, de, L), tag + " no 2^l")
    if L == 10:
        assert float(np.median(dbound)) < 2e-3, "at L = 10 and unit gradients the bound is far below an atol of 1e-2"


# ---- points -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N", K.POINTS_CASES + (K.POINTS_FWD_STRIDE, K.POINTS_BWD_STRIDE))
def test_points(R, N):
    o, d, z, dpts = K.gen_points(R, N, R + N)
    assert o.shape == d.shape == (R, 3) and z.shape == (R, N) and dpts.shape == (R, N, 3)
    assert float(z.min()) >= 2 and float(z.max()) <= 6
    zt = torch.from_numpy(z).double().requires_grad_(True)
    pts = torch.from_numpy(o).double()[:, None] + torch.from_numpy(d).double()[:, None] * zt[..., None]
    (pts * torch.from_numpy(dpts).double()).sum().backward()
    assert np.allclose(K.points64(o, d, z)[0], pts.detach().numpy(), rtol=1e-15, atol=0)
    assert np.allclose(K.points_backward64(dpts, d)[0], zt.grad.numpy(), rtol=1e-13, atol=1e-15)
    tag = f"points {R}x{N}"
    _accepted(K.compare_points(K.points32(o, d, z), o, d, z), tag + " forward")
    _accepted(K.compare_points_backward(K.points_backward32(dpts, d), dpts, d), tag + " backward")
    fma = (o.astype(np.float64)[:, None] + d.astype(np.float64)[:, None] * z.astype(np.float64)[..., None]).astype(F32)
    assert K.compare_points(fma, o, d, z).rejected.size == 0, "a fused multiply-add is accepted too"
    if R >= 2:
        _rejected(K.compare_points(K.points32(o, d, z, "next_ray_d"), o, d, z), tag + " d of ray r + 1")
        _rejected(K.compare_points_backward(K.points_backward32(dpts, d, "next_ray_d"), dpts, d), tag + " backward, d of ray r + 1")


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def _torch_adam64(s, t, lr, b1, b2, eps):
    p = torch.from_numpy(s["p"]).double().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(s["m"]).double(),
                        exp_avg_sq=torch.from_numpy(s["v"]).double())
    p.grad = torch.from_numpy(s["g"]).double()
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == t
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def test_adam_bias_correction_error_is_a_function_of_t():
    lr, b1, b2, eps = K.hyper32()
    assert b1 == float(F32(0.9)) and b2 == float(F32(0.999)) and b1 != 0.9
    for b in (b1, b2):
        assert float(F32(1) - F32(b)) == 1.0 - b, "1 - b is exact in fp32"
    r = {t: K.bc_rel_error(b2, t) for t in K.ADAM_STEPS}
    assert 2.5e-5 < r[2] < 3.5e-5 and r[1] > r[2] > r[10] > r[1000] > r[100000] == pytest.approx(K.U, rel=1e-6)
    for t in K.ADAM_STEPS:                      # numpy's powf against float64: inside the modelled ulp
        for b in (b1, b2):
            bc32 = float(F32(1) - np.power(F32(b), F32(t)))
            assert abs(bc32 - (1.0 - b ** t)) <= K.bc_rel_error(b, t) * (1.0 - b ** t)


@pytest.mark.parametrize("n,t", K.ADAM_CASES)
def test_adam(n, t):
    hyper = K.hyper32()
    s = K.gen_adam(n, n + t)
    idx = np.arange(n)
    assert all(s[k].dtype == F32 and s[k].shape == (n,) for k in "pgmv")
    assert bool((s["g"][idx % 8 >= 6] == 0).all()) and bool((s["v"][idx % 8 == 7] == 0).all()) and bool((s["v"] >= 0).all())
    live = np.abs(s["g"][idx % 8 < 6])
    assert bool((live >= 0.99e-6).all()) and bool((live <= 1.01e4).all())
    if n >= 255:
        assert live.min() < 1e-5 and live.max() > 1e3
    r = K.adam64(s, t, *hyper)
    p64, m64, v64 = _torch_adam64(s, t, *hyper)
    assert np.allclose(r["m"], m64, rtol=1e-14, atol=0) and np.allclose(r["v"], v64, rtol=1e-14, atol=0)
    assert bool((np.abs(r["p"] - p64) <= 1e-6 * r["bd"]).all()), "the reference against a float64 torch.optim.Adam"
    tag = f"adam n={n} t={t}"
    _accepted(K.compare_adam(K.adam32(s, t, *hyper), s, t, *hyper), tag)
    mutants = ["betas_swapped"]
    if n >= 8:
        mutants.append("eps_inside_sqrt")          # shows only where v' = 0
    if t <= 1000:
        mutants += ["bc2_without_sqrt", "step_plus_one"]
    if n > K.STRIDE_THRESHOLD:
        mutants.append("stride_tail_unchanged")
    for mutant in mutants:
        _rejected(K.compare_adam(K.adam32(s, t, *hyper, mutant=mutant), s, t, *hyper), f"{tag} {mutant}")
    ignored = K.adam32(s, t, 0.5, *hyper[1:])      # lr_dev ignored: the scalar the tests pass beside it is 0.5
    _rejected(K.compare_adam(ignored, s, t, *hyper), tag + " lr_dev ignored")
    _rejected(K.compare_adam(dict(p=s["p"], m=s["m"], v=s["v"]), s, t, *hyper), tag + " row skipped")


def test_adam_table():
    sizes = K.gen_adam_table(70)
    big = max(K.ADAM_TABLE_SIZES)
    assert len(sizes) == K.ADAM_TABLE_ROWS and set(sizes) == set(K.ADAM_TABLE_SIZES)
    assert 0 in sizes and sizes[0] != big and sizes[-1] not in (big, 0) and big > K.STRIDE_THRESHOLD
    assert sizes == K.gen_adam_table(70)
