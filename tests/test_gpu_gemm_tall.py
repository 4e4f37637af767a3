"""ns_gemm_tall on the GPU: C (+)= A B^T (+ bias), act, dact with a workgroup per slab of 128 rows and all N columns.

Exact cases: integer inputs in [-4, 4] held in fp32 -- every partial sum is below 16 * 512 + 8 < 2^24, so every summation order
is exact and the result must equal the integer reference bit for bit (the reference product is taken in float64, which holds
these integers exactly, and converted to int64).  Rows sit around the slab size (127, 128, 129) and around the 32-row groups.
Random cases: the standard bound of any summation order, (K + 2) 2^-24 sum_k |A_ik B_jk|, against a float64 product."""

import ctypes as C
import itertools

import pytest
import torch

from nerf_sampling_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256), (256, 319), (128, 283), (4, 128), (3, 128), (1, 256), (256, 63), (63, 256), (512, 512)]
ROWS = [1, 31, 32, 33, 127, 128, 129, 1000, 4097]
SENTINEL = 7777.0
GUARD = 512          # floats behind the C buffer


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tall(A, B, sb0, sb1, bias, Cv, rows, N, K, acc=0, act=0, dact=0, ref=None):
    return _lib.load().ns_gemm_tall(_ptr(A), A.stride(0), _ptr(B), sb0, sb1, _ptr(bias), _ptr(Cv), Cv.stride(0), rows, N, K, acc,
                                    act, dact, _ptr(ref), 0 if ref is None else ref.stride(0), _stream())


def _ints(shape, g, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).float().cuda()


@pytest.mark.parametrize("N,K", SHAPES)
def test_integer_inputs_are_exact(N, K):
    g = torch.Generator().manual_seed(1000 * N + K)
    R = max(ROWS)
    a_buf = _ints((R, K + 5), g)
    A = a_buf[:, 3:3 + K]                                  # lda > K, 4-byte aligned only
    W = _ints((N, K), g)
    Wt = W.t().contiguous()                                # [K, N]: B[j, k] at j + k * N
    bias = _ints((N,), g)
    c0 = _ints((R, N), g)
    r_buf = _ints((R, N + 3), g, 0, 2)                     # an activation output with zeros
    ref = r_buf[:, 1:1 + N]
    prod = (A.double() @ W.double().t()).to(torch.int64)   # exact
    assert bool((ref == 0).any()) and bool((ref > 0).any())
    flat = torch.full((R * (N + 7) + GUARD,), SENTINEL, device="cuda")
    for rows in ROWS:
        for use_bias, act, dact, acc, transposed in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
            flat.fill_(SENTINEL)
            buf = flat[:rows * (N + 7)].view(rows, N + 7)
            Cv = buf[:, 2:2 + N]
            exp = prod[:rows].clone()
            if use_bias:
                exp += bias.long()
            if acc:
                Cv.copy_(c0[:rows])
                exp += c0[:rows].long()
            if act:
                exp.clamp_(min=0)
            if dact:
                exp *= (ref[:rows] > 0).long()
            B, sb0, sb1 = (Wt, 1, N) if transposed else (W, K, 1)
            rc = _tall(A, B, sb0, sb1, bias if use_bias else None, Cv, rows, N, K, acc, act, dact, ref if dact else None)
            assert rc == 0, _lib.load().ns_last_error()
            tag = (N, K, rows, use_bias, act, dact, acc, transposed)
            assert torch.equal(Cv, exp.float()), tag
            assert bool((buf[:, :2] == SENTINEL).all()) and bool((buf[:, 2 + N:] == SENTINEL).all()), tag
            assert bool((flat[rows * (N + 7):] == SENTINEL).all()), tag


@pytest.mark.parametrize("transposed", [0, 1])
def test_relu_epilogue_keeps_a_nan_row(transposed):
    """act = 1 with one NaN in row 37 of A (two slabs: 129 rows): every output of that row is NaN, as torch.relu and nn.Linear
    give it, and every other row holds the bits of the run without the NaN."""
    g = torch.Generator().manual_seed(43)
    rows, N, K, nan_row = 129, 256, 319, 37
    A, W, bias = _ints((rows, K), g), _ints((N, K), g), _ints((N,), g)
    bad = A.clone()
    bad[nan_row, 7] = float("nan")
    B, sb0, sb1 = (W.t().contiguous(), 1, N) if transposed else (W, K, 1)
    outs = []
    for a in (A, bad):
        flat = torch.full((rows * N + GUARD,), SENTINEL, device="cuda")
        assert _tall(a, B, sb0, sb1, bias, flat[:rows * N].view(rows, N), rows, N, K, act=1) == 0, _lib.load().ns_last_error()
        assert bool((flat[rows * N:] == SENTINEL).all())
        outs.append(flat[:rows * N].view(rows, N))
    clean, got = outs
    exp = torch.relu(torch.nn.functional.linear(bad.double(), W.double(), bias.double())).float()
    others = torch.arange(rows, device="cuda") != nan_row
    assert bool(torch.isnan(exp[nan_row]).all()) and not bool(torch.isnan(exp[others]).any()), "the reference itself"
    assert bool(torch.isnan(got[nan_row]).all()), "the NaN row must come out NaN in every column"
    assert torch.equal(got[others], exp[others]) and torch.equal(got[others], clean[others])
    assert torch.equal(clean, torch.relu(torch.nn.functional.linear(A.double(), W.double(), bias.double())).float())


def test_wrappers_take_column_slices_of_the_cat_buffer():
    from nerf_sampling_amd import autograd as ag

    g = torch.Generator().manual_seed(5)
    M, Wd = 333, 64
    cat = _ints((M, 63 + Wd), g)
    W, b = _ints((Wd, Wd), g), _ints((Wd,), g)
    before = cat.clone()
    x = before[:, 63:]                                      # input: a column slice
    y = ag.linear_forward_tall(x, W, b, ag.RELU, out=cat[:, 63:])        # output: a column slice
    exp = (x.double() @ W.double().t() + b.double()).clamp(min=0).float()
    assert torch.equal(cat[:, 63:], exp) and torch.equal(cat[:, :63], before[:, :63])
    assert y.data_ptr() == cat[:, 63:].data_ptr()
    dy = _ints((M, Wd), g)
    W2 = _ints((Wd, 63 + Wd), g)
    dx = ag.linear_backward_input_tall(dy, W2, n_cols=63)
    assert torch.equal(dx, (dy.double() @ W2.double()[:, :63]).float())
    dh = ag.linear_backward_input_tall(dy, W2, dact_ref=cat)
    assert torch.equal(dh, ((dy.double() @ W2.double()) * (cat > 0)).float())
    with pytest.raises(ValueError):
        ag.linear_forward_tall(x.t(), W, b)
    with pytest.raises(NotImplementedError):
        ag.linear_forward_tall(torch.zeros(4, 513, device="cuda"), torch.zeros(8, 513, device="cuda"), None)


@pytest.mark.parametrize("N,K,rows", [(256, 319, 4097), (128, 283, 1000)])
def test_random_inputs_within_the_summation_bound_and_reproducible(N, K, rows):
    g = torch.Generator().manual_seed(N + K + rows)
    A = torch.randn(rows, K + 1, generator=g).cuda()[:, 1:]
    W = torch.randn(N, K, generator=g).cuda()
    bias = torch.randn(N, generator=g).cuda()

    def run(transposed, stream=None):
        out = torch.full((rows, N), SENTINEL, device="cuda")
        B, sb0, sb1 = (W.t().contiguous(), 1, N) if transposed else (W, K, 1)
        if stream is None:
            assert _tall(A, B, sb0, sb1, bias, out, rows, N, K) == 0
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                assert _tall(A, B, sb0, sb1, bias, out, rows, N, K) == 0
            torch.cuda.current_stream().wait_stream(stream)
        return out

    c64 = A.double() @ W.double().t()
    bound = (K + 2) * 2.0 ** -24 * (A.double().abs() @ W.double().abs().t() + bias.double().abs())
    for transposed in (False, True):
        c = run(transposed)
        ratio = ((c.double() - (c64 + bias.double())).abs() / bound).max()
        print(f"ns_gemm_tall {N}x{K}x{rows} transposed={transposed}: max err / bound = {float(ratio):.3e}")
        assert float(ratio) <= 1.0
        assert torch.equal(c, run(transposed)), "two calls must return the same bits"
        assert torch.equal(c, run(transposed, torch.cuda.Stream())), "a second stream must return the same bits"


@pytest.mark.parametrize("N,K,rows,status", [(513, 64, 100, -2), (64, 513, 100, -2), (64, 64, 0, -1)])
def test_unsupported_shapes_return_their_status_without_a_launch(N, K, rows, status):
    A = torch.zeros(max(rows, 1), K, device="cuda")
    W = torch.zeros(N, K, device="cuda")
    out = torch.full((max(rows, 1), N), SENTINEL, device="cuda")
    assert _tall(A, W, K, 1, None, out, rows, N, K) == status
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
