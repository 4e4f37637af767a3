"""ns_gemm_fused, ns_gemm_fused_batched and the small kernels beside them (csrc/ns_train.hip) on the GPU, called through ctypes.

Exact cases: integer inputs in [-4, 4] held in fp32 -- every partial sum is below 16 * 1024 + 8 < 2^24 (asserted in
tests/test_gemm_tile_host.py and again on the data here), so every summation order is exact and the result must equal
tests/gemm_tile_reference.py bit for bit; what follows the sum is one IEEE operation per step on both sides.  Random cases: the
standard bound of any summation order, (K + 2) 2^-24 (|A| |B|^T + |bias|), against a float64 product.  Every output buffer is
pre-filled with a sentinel and everything outside the [M, N] view (pad columns of the strided C, a band behind it, a band
behind the row sums) must still hold it afterwards."""

import ctypes as C
import itertools

import pytest
import torch

import gemm_tile_reference as G
from nerf_sampling_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 7777.25
GUARD = 512           # floats behind every output buffer
PAD = 7               # ldc = N + PAD, the view starts at column 2
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]       # (A k-contiguous, B k-contiguous)
LAYOUT_IDS = ["AkBk", "AkBs", "AsBk", "AsBs"]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ints(shape, g, lo=-G.INT_RANGE, hi=G.INT_RANGE):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _dyadic(shape, g):
    return torch.tensor(G.DYADIC)[torch.randint(0, len(G.DYADIC), shape, generator=g)]


class Operand:
    """X [rows, K] on the GPU in one of the two layouts, as (address, row stride, k stride).  k-contiguous: a column slice of
    a wider buffer (row stride K + 5 > K).  Otherwise X^T [K, rows + 3], a column slice again (row stride 1, k stride
    rows + 3: what a grad-weight GEMM reads).  The address is taken from the non-empty buffer, so K = 0 has one too."""

    def __init__(self, X, kcontig):
        rows, K = X.shape
        if kcontig:
            self.buf = torch.zeros(rows, K + 5)
            self.buf[:, 3:3 + K] = X
            self.off, self.s0, self.s1 = 3, K + 5, 1
        else:
            self.buf = torch.zeros(K + 1, rows + 3)
            self.buf[:K, 1:1 + rows] = X.t()
            self.off, self.s0, self.s1 = 1, 1, rows + 3
        self.buf = self.buf.cuda()
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * self.off)
        self.address = self.buf.data_ptr() + 4 * self.off


class Output:
    """C [M, N] as columns 2 .. 2 + N of a [M, N + PAD] buffer with GUARD floats behind it, and a_rowsum [M] with GUARD floats
    behind it; both hold the sentinel wherever the kernel must not write."""

    def __init__(self, Mmax, Nmax):
        self.flat = torch.full((Mmax * (Nmax + PAD) + GUARD,), SENTINEL, device="cuda")
        self.rs = torch.full((Mmax + GUARD,), SENTINEL, device="cuda")

    def reset(self, M, N, seed=None):
        self.M, self.N = M, N
        self.flat.fill_(SENTINEL)
        self.rs.fill_(SENTINEL)
        self.buf = self.flat[:M * (N + PAD)].view(M, N + PAD)
        self.view = self.buf[:, 2:2 + N]
        if seed is not None:
            self.view.copy_(seed)
        return self

    def ok(self, exp, exp_rs):
        """One GPU boolean: the view and the row sums equal the expectation bit for bit (as values: -0 == +0) and everything
        around them is still the sentinel."""
        M, N = self.M, self.N
        ok = (self.view == exp.cuda()).all() & (self.buf[:, :2] == SENTINEL).all() & (self.buf[:, 2 + N:] == SENTINEL).all() \
            & (self.flat[M * (N + PAD):] == SENTINEL).all()
        if exp_rs is None:
            return ok & (self.rs == SENTINEL).all()
        return ok & (self.rs[:M] == exp_rs.cuda()).all() & (self.rs[M:] == SENTINEL).all()


def _fused(a, b, bias, out, M, N, K, acc=0, act=0, dact=0, ref=None, rowsum=False):
    return _lib.load().ns_gemm_fused(a.ptr, a.s0, a.s1, b.ptr, b.s0, b.s1, _ptr(bias), _ptr(out.view), out.view.stride(0), M, N, K,
                                     acc, act, dact, _ptr(ref), 0 if ref is None else ref.stride(0),
                                     _ptr(out.rs) if rowsum else None, _stream())


def _settle(pending):
    """One synchronisation for a run of cases: [(tag, GPU boolean)] -> the first failing tag, if any."""
    if pending:
        flags = torch.stack([ok for _, ok in pending]).cpu()
        bad = [tag for (tag, _), f in zip(pending, flags.tolist()) if not f]
        assert not bad, f"{len(bad)} of {len(pending)} cases differ from the reference or wrote outside their view; first: {bad[0]}"
    pending.clear()


class Problem:
    """Integer operands for every size of the sweep at one K: the sizes are the top-left corners of one A [100, K] and one
    B [257, K], so the strides are those of the largest."""

    def __init__(self, K, layout, seed):
        g = torch.Generator().manual_seed(seed)
        self.K = K
        Mx, Nx = max(m for m, _ in G.SIZES), max(n for _, n in G.SIZES)
        self.A, self.B = _ints((Mx, K), g), _ints((Nx, K), g)
        self.bias, self.c0 = _ints((Nx,), g), _ints((Mx, Nx), g)
        self.ref = _dyadic((Mx, Nx + 3), g)
        self.ref[:2, 1:3] = torch.tensor([[0.0, 1.0], [0.5, 0.0]])          # zeros and positives in every view, (1, 1) aside
        assert bool((self.ref == 0).any()) and bool((self.ref > 0).any())
        worst = self.A.abs().double() @ self.B.abs().double().t() + self.bias.abs().double() + self.c0.abs().double()
        assert float(worst.max()) < 2 ** 24 and float(worst.max()) <= G.max_partial_sum(K)
        self.prod = G.product(self.A, self.B)
        self.a, self.b = Operand(self.A, layout[0]), Operand(self.B, layout[1])
        self.bias_d, self.c0_d, self.ref_d = self.bias.cuda(), self.c0.cuda(), self.ref.cuda()
        self.out = Output(Mx, Nx)

    def run(self, M, N, use_bias, acc, act, dact, rowsum, pending, tag):
        out = self.out.reset(M, N, self.c0_d[:M, :N] if acc else None)
        ref_d = self.ref_d[:, 1:]                                           # ld_ref = Nmax + 3 > N, 4-byte aligned only
        rc = _fused(self.a, self.b, self.bias_d if use_bias else None, out, M, N, self.K, acc, act, dact,
                    ref_d if dact else None, rowsum)
        assert rc == 0, (_lib.load().ns_last_error(), tag)
        exp = G.epilogue(self.prod[:M, :N], self.bias[:N] if use_bias else None, self.c0[:M, :N], self.ref[:M, 1:1 + N],
                         act, dact, acc)          # (the corner of the product is the product of the corners)
        pending.append((tag, out.ok(exp, G.rowsum(self.A[:M]) if rowsum else None)))


# ---- a. exact, single launch -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_integer_inputs_are_exact_at_every_k(layout):
    """Every K of the sweep x every size: the plain call and the all-on call (bias, accumulate, relu, relu', row sums)."""
    pending = []
    for K in G.K_SWEEP:
        p = Problem(K, layout, 100 + K)
        for (M, N) in G.SIZES:
            p.run(M, N, 0, 0, 0, 0, False, pending, (layout, M, N, K, "plain"))
            p.run(M, N, 1, 1, 1, 1, True, pending, (layout, M, N, K, "bias acc act=1 dact=1 rowsum"))
        _settle(pending)


@pytest.mark.parametrize("K", G.K_PRODUCT)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_integer_inputs_are_exact_under_every_epilogue(layout, K):
    """bias x accumulate x act {0, 1, 2} x dact {0, 1, 2, 3} x row sums, every size."""
    pending = []
    p = Problem(K, layout, 200 + K)
    for (M, N) in G.SIZES:
        for use_bias, acc, act, dact, rowsum in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1, 2, 3), (False, True)):
            p.run(M, N, use_bias, acc, act, dact, rowsum, pending,
                  (layout, M, N, K, f"bias={use_bias} acc={acc} act={act} dact={dact} rowsum={rowsum}"))
        _settle(pending)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_relu_epilogue_keeps_a_nan_row(layout):
    """act = 1 with one NaN in row G.NAN_ROW of A: every output of that row is NaN, as torch.relu and nn.Linear give it (fmaxf
    would return the bias-free 0), and every other row holds the bits of the run without the NaN."""
    g = torch.Generator().manual_seed(41)
    M, N, K = 65, 100, 64
    A, B, bias = _ints((M, K), g), _ints((N, K), g), _ints((N,), g)
    bad = A.clone()
    bad[G.NAN_ROW, 7] = float("nan")
    b, bias_d = Operand(B, layout[1]), bias.cuda()
    clean, out = Output(M, N).reset(M, N), Output(M, N).reset(M, N)
    assert _fused(Operand(A, layout[0]), b, bias_d, clean, M, N, K, act=1) == 0
    assert bool(clean.ok(G.expected(A, B, bias, act=1), None))
    assert _fused(Operand(bad, layout[0]), b, bias_d, out, M, N, K, act=1) == 0
    got, exp = out.view.cpu(), G.expected(bad, B, bias, act=1)
    others = torch.arange(M) != G.NAN_ROW
    assert bool(torch.isnan(exp[G.NAN_ROW]).all()) and not bool(torch.isnan(exp[others]).any()), "the reference itself"
    assert bool(torch.isnan(got[G.NAN_ROW]).all()), "the NaN row must come out NaN in every column"
    assert torch.equal(got[others], exp[others]) and torch.equal(got[others], clean.view.cpu()[others])
    assert bool((out.buf[:, :2] == SENTINEL).all() & (out.buf[:, 2 + N:] == SENTINEL).all()
                & (out.flat[M * (N + PAD):] == SENTINEL).all() & (out.rs == SENTINEL).all()), "guard bands"


# ---- b. the sigmoid epilogue -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(64, 1, 256), (33, 33, 4)])
def test_sigmoid_epilogue_within_its_bound(M, N, K):
    """act = 3 on integer inputs in [-1, 1]: the pre-activation is exact, so the error is the sigmoid's alone:
    |err| <= 8 * 2^-24 * sigma + 2^-126 (expf within 2 ulp -- no figure for expf is given in the installed HIP documentation, so
    the 2 ulp stand --, one add, one IEEE divide; the absolute term covers the denormal range).  With dact the result takes one
    more IEEE multiply by the exact factor g = act'(y): |err| <= g * that bound + 2^-24 * g * sigma + 2^-149."""
    g = torch.Generator().manual_seed(M + K)
    A, B, bias = _ints((M, K), g, -1, 1), _ints((N, K), g, -1, 1), _ints((N,), g, -1, 1)
    if K == 256:                                            # both saturated ends: v = +-sum b^2 (+ bias)
        B[0, :200] = 1.0
        A[0], A[1] = B[0], -B[0]
    ref = _dyadic((M, N + 3), g)
    ref[:2, 1] = torch.tensor([0.5, 0.5])
    a, b, out = Operand(A, True), Operand(B, True), Output(M, N)
    v = G.expected(A, B, bias).double()                     # exact
    assert float(v.abs().max()) <= G.max_partial_sum(K, 1)
    sig = torch.sigmoid(v)
    for dact in (0, 1, 2, 3):
        out.reset(M, N)
        assert _fused(a, b, bias.cuda(), out, M, N, K, 0, 3, dact, ref.cuda()[:, 1:] if dact else None, True) == 0
        got = out.view.cpu().double()
        fac = G.dact_factor(ref[:, 1:1 + N], dact).double() if dact else torch.ones_like(sig)
        bound = G.sigmoid_bound(v) if dact == 0 else fac * G.sigmoid_bound(v) + G.U * fac * sig + 2.0 ** -149
        ratio = float(((got - sig * fac).abs() / bound).max())
        print(f"ns_gemm_fused sigmoid {M}x{N}x{K} dact={dact}: max err / bound = {ratio:.3e}")
        assert ratio <= 1.0, (M, N, K, dact)
        assert bool(out.ok(out.view.cpu(), G.rowsum(A))), "row sums or guard bands"
        if K == 256 and dact == 0:
            assert float(v.max()) >= 200 and float(v.min()) <= -200
            assert bool((got == 1.0).any()) and bool((got < 2.0 ** -126).any()), "both saturated ends occur"


# ---- c. random floats --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(100, 257, 319), (256, 64, 1024)])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_random_inputs_within_the_summation_bound_and_reproducible(layout, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    A, B, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    a, b, bias_d = Operand(A, layout[0]), Operand(B, layout[1]), bias.cuda()

    def run(stream=None):
        out = Output(M, N).reset(M, N)
        if stream is None:
            assert _fused(a, b, bias_d, out, M, N, K, rowsum=True) == 0
        else:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                assert _fused(a, b, bias_d, out, M, N, K, rowsum=True) == 0
            torch.cuda.current_stream().wait_stream(stream)
        assert bool(out.ok(out.view.cpu(), out.rs[:M].cpu())), "guard bands"
        return out.view.clone(), out.rs[:M].clone()

    c64 = A.double() @ B.double().t() + bias.double()
    bound = (K + 2) * G.U * (A.double().abs() @ B.double().abs().t() + bias.double().abs())
    c, rs = run()
    ratio = float(((c.cpu().double() - c64).abs() / bound).max())
    rs_ratio = float(((rs.cpu().double() - A.double().sum(1)).abs() / ((K + 2) * G.U * A.double().abs().sum(1))).max())
    print(f"ns_gemm_fused {M}x{N}x{K} {LAYOUT_IDS[LAYOUTS.index(layout)]}: max err / bound = {ratio:.3e}, row sums {rs_ratio:.3e}")
    assert ratio <= 1.0 and rs_ratio <= 1.0
    c2, rs2 = run()
    assert torch.equal(c, c2) and torch.equal(rs, rs2), "two calls must return the same bits"
    c3, rs3 = run(torch.cuda.Stream())
    assert torch.equal(c, c3) and torch.equal(rs, rs3), "a second stream must return the same bits"


# ---- d. batched --------------------------------------------------------------------------------------------------------

def _fill(q, a, b, bias, out, M, N, K, acc=0, act=0, dact=0, ref=None, rowsum=False):
    q.A_dev, q.sa0, q.sa1 = a.address, a.s0, a.s1
    q.B_dev, q.sb0, q.sb1 = b.address, b.s0, b.s1
    q.bias_dev = None if bias is None else bias.data_ptr()
    q.C_dev, q.ldc = out.view.data_ptr(), out.view.stride(0)
    q.M, q.N, q.K = M, N, K
    q.accumulate, q.act, q.dact = acc, act, dact
    q.dact_ref_dev, q.ld_ref = (None, 0) if ref is None else (ref.data_ptr(), ref.stride(0))
    q.a_rowsum_dev = out.rs.data_ptr() if rowsum else None


# (M, N, K), bias, accumulate, act, dact, row sums: every problem its own shape and epilogue; the grid covers (100, 257)
BATCH = [((65, 100, 64), 1, 0, 1, 0, True),
         ((33, 31, 300), 0, 1, 0, 1, False),
         ((100, 257, 7), 1, 1, 2, 2, True),
         ((1, 1, 129), 0, 0, 0, 3, False)]


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_batched_launch_keeps_each_problems_shape_and_epilogue(layout, count):
    g = torch.Generator().manual_seed(300 + count)
    arr = (_lib.GemmProblem * count)()
    keep, checks = [], []
    for q, ((M, N, K), use_bias, acc, act, dact, rowsum) in zip(arr, BATCH[:count]):
        A, B, bias, c0 = _ints((M, K), g), _ints((N, K), g), _ints((N,), g), _ints((M, N), g)
        ref = _dyadic((M, N + 3), g)
        ref[0, 1] = 0.0 if M * N > 1 else 0.5
        a, b, bias_d, ref_d = Operand(A, layout[0]), Operand(B, layout[1]), bias.cuda(), ref.cuda()[:, 1:]
        out = Output(M, N).reset(M, N, c0.cuda() if acc else None)
        _fill(q, a, b, bias_d if use_bias else None, out, M, N, K, acc, act, dact, ref_d if dact else None, rowsum)
        exp = G.expected(A, B, bias if use_bias else None, c0, ref[:, 1:1 + N], act, dact, acc)
        keep.append((a, b, bias_d, ref_d))
        checks.append((out, exp, G.rowsum(A) if rowsum else None, (M, N, K)))
    assert _lib.load().ns_gemm_fused_batched(arr, count, _stream()) == 0, _lib.load().ns_last_error()
    for out, exp, exp_rs, tag in checks:
        assert bool(out.ok(exp, exp_rs)), (layout, count, tag)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_results_do_not_depend_on_the_trip_length(layout):
    """A K = 100 problem beside a K = 300 partner runs with trips of 64; alone through ns_gemm_fused with trips of 32.  Random
    floats: the same bits, row sums included."""
    g = torch.Generator().manual_seed(17)
    M, N, K = 65, 100, 100
    A, B, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    A2, B2 = torch.randn(33, 300, generator=g), torch.randn(31, 300, generator=g)
    assert G.trip_length(K) == 32 and G.trip_length(300) == 64
    a, b, bias_d = Operand(A, layout[0]), Operand(B, layout[1]), bias.cuda()
    a2, b2 = Operand(A2, layout[0]), Operand(B2, layout[1])
    alone, batched, partner = Output(M, N).reset(M, N), Output(M, N).reset(M, N), Output(33, 31).reset(33, 31)
    assert _fused(a, b, bias_d, alone, M, N, K, act=2, rowsum=True) == 0
    arr = (_lib.GemmProblem * 2)()
    _fill(arr[0], a2, b2, None, partner, 33, 31, 300, rowsum=True)
    _fill(arr[1], a, b, bias_d, batched, M, N, K, act=2, rowsum=True)
    assert _lib.load().ns_gemm_fused_batched(arr, 2, _stream()) == 0, _lib.load().ns_last_error()
    assert bool(batched.ok(alone.view, alone.rs[:M])), "the K = 100 problem differs between trips of 32 and of 64"
    assert bool(alone.ok(alone.view, alone.rs[:M])), "guard bands"
    alone2 = Output(33, 31).reset(33, 31)
    assert _fused(a2, b2, None, alone2, 33, 31, 300, rowsum=True) == 0
    assert bool(partner.ok(alone2.view, alone2.rs[:33]))
    c64 = A.double() @ B.double().t() + bias.double()
    c64 = torch.where(c64 > 0, c64, 0.01 * c64)
    bound = (K + 3) * G.U * (A.double().abs() @ B.double().abs().t() + bias.double().abs())     # + the leaky multiply
    assert bool(((alone.view.cpu().double() - c64).abs() <= bound).all())


def test_batched_grad_weight_layout_as_the_backward_launches_it():
    """dW = dy^T x for three branches in one launch: A = dy^T (sa0 = 1), B = x^T (sb0 = 1), K = 1024 rays, the bias gradient
    as row sums."""
    g = torch.Generator().manual_seed(23)
    rays = 1024
    arr = (_lib.GemmProblem * 3)()
    keep, checks = [], []
    for q, (n_out, n_in) in zip(arr, [(256, 319), (256, 256), (33, 63)]):
        dy, x = _ints((rays, n_out), g).cuda(), _ints((rays, n_in), g).cuda()
        out = Output(n_out, n_in).reset(n_out, n_in)
        q.A_dev, q.sa0, q.sa1 = dy.data_ptr(), 1, n_out
        q.B_dev, q.sb0, q.sb1 = x.data_ptr(), 1, n_in
        q.C_dev, q.ldc = out.view.data_ptr(), out.view.stride(0)
        q.M, q.N, q.K = n_out, n_in, rays
        q.a_rowsum_dev = out.rs.data_ptr()
        keep.append((dy, x))
        checks.append((out, (dy.double().t() @ x.double()).float(), dy.double().sum(0).float(), (n_out, n_in)))
    assert _lib.load().ns_gemm_fused_batched(arr, 3, _stream()) == 0, _lib.load().ns_last_error()
    for out, exp, exp_rs, tag in checks:
        assert bool(out.ok(exp, exp_rs)), tag


def test_rejected_batches_launch_nothing():
    g = torch.Generator().manual_seed(29)
    M, N, K = 33, 31, 64
    A, B = _ints((M, K), g), _ints((N, K), g)
    outs = [Output(M, N).reset(M, N) for _ in range(5)]
    ak, bk, as_ = Operand(A, True), Operand(B, True), Operand(A, False)
    five = (_lib.GemmProblem * 5)()
    for q, out in zip(five, outs):
        _fill(q, ak, bk, None, out, M, N, K, rowsum=True)
    assert _lib.load().ns_gemm_fused_batched(five, 5, _stream()) == -1
    mixed = (_lib.GemmProblem * 2)()
    _fill(mixed[0], ak, bk, None, outs[0], M, N, K, rowsum=True)
    _fill(mixed[1], as_, bk, None, outs[1], M, N, K, rowsum=True)
    assert _lib.load().ns_gemm_fused_batched(mixed, 2, _stream()) == -1
    assert b"ns_gemm_fused_batched" in _lib.load().ns_last_error()
    torch.cuda.synchronize()
    for out in outs:
        assert bool((out.flat == SENTINEL).all()) and bool((out.rs == SENTINEL).all())
    assert _lib.load().ns_gemm_fused_batched(five, 4, _stream()) == 0          # the same table, four of them: accepted
    exp = G.expected(A, B)
    assert all(bool(out.ok(exp, G.rowsum(A))) for out in outs[:4]) and bool((outs[4].flat == SENTINEL).all())


# ---- e. the small kernels beside it ------------------------------------------------------------------------------------

def test_colsum_is_exact():
    g = torch.Generator().manual_seed(31)
    lib = _lib.load()
    pending = []
    for M, N in itertools.product((1, 31, 32, 33, 1000), (1, 31, 33, 256)):
        X = _ints((M, N + 3), g)
        Xd = X.cuda()
        out = torch.full((N + GUARD,), SENTINEL, device="cuda")
        assert lib.ns_colsum(_ptr(Xd), N + 3, M, N, _ptr(out), _stream()) == 0, lib.ns_last_error()
        exp = X[:, :N].double().sum(0).float().cuda()
        pending.append(((M, N), (out[:N] == exp).all() & (out[N:] == SENTINEL).all()))
    _settle(pending)


ACT_SIZES = [1, 255, 256, 257, 256 * 4096 + 5]           # the last: more blocks than the elementwise grid's cap, grid-stride


@pytest.mark.parametrize("n", ACT_SIZES)
def test_act_forward(n):
    g = torch.Generator().manual_seed(n)
    lib = _lib.load()
    x = torch.randn(n, generator=g) * 4
    x[0] = 0.0 if n > 1 else -3.0
    for act in (0, 1, 2, 3):
        buf = torch.full((n + GUARD,), SENTINEL, device="cuda")
        buf[:n] = x.cuda()
        assert lib.ns_act_forward(_ptr(buf), n, act, _stream()) == 0, lib.ns_last_error()
        got = buf[:n].cpu()
        assert bool((buf[n:] == SENTINEL).all()), (n, act)
        if act == 3:
            ratio = float(((got.double() - torch.sigmoid(x.double())).abs() / G.sigmoid_bound(x.double())).max())
            print(f"ns_act_forward sigmoid n={n}: max err / bound = {ratio:.3e}")
            assert ratio <= 1.0
        else:
            assert torch.equal(got, G.act_apply(x, act)), (n, act)


@pytest.mark.parametrize("n", ACT_SIZES)
def test_act_backward(n):
    g = torch.Generator().manual_seed(n + 1)
    lib = _lib.load()
    dy = torch.randn(n, generator=g)
    y = torch.randn(n, generator=g)
    y[torch.rand(n, generator=g) < 0.25] = 0.0
    if n == 1:
        y[0] = 0.0
    for act in (0, 1, 2, 3):
        if act == 3:                                     # exact on the dyadic outputs: y (1 - y) is exact, one multiply follows
            y, dy = _dyadic((n,), g), _ints((n,), g)
        buf = torch.full((n + GUARD,), SENTINEL, device="cuda")
        buf[:n] = dy.cuda()
        yd = y.cuda()
        assert lib.ns_act_backward(_ptr(buf), _ptr(yd), n, act, _stream()) == 0, lib.ns_last_error()
        exp = dy * G.dact_factor(y, act) if act else dy
        assert torch.equal(buf[:n].cpu(), exp), (n, act)
        assert bool((buf[n:] == SENTINEL).all()) and torch.equal(yd.cpu(), y), (n, act)


ADAM_SIZES = [1, 255, 65536, 65537, 200000]              # 65536 = 256 blocks x 256 threads: the grid-stride threshold


@pytest.mark.parametrize("use_lr_dev", [False, True])
def test_multi_tensor_adam_matches_the_per_tensor_kernel_and_torch(use_lr_dev):
    g = torch.Generator().manual_seed(37)
    lib = _lib.load()
    lr, b1, b2, eps, step0 = 1e-3, 0.9, 0.999, 1e-8, 4
    lr_dev = torch.tensor([lr], device="cuda") if use_lr_dev else None
    lr_arg = 0.5 if use_lr_dev else lr                    # with lr_dev the argument is not the learning rate

    def guarded(x):
        buf = torch.full((x.numel() + GUARD,), SENTINEL, device="cuda")
        buf[:x.numel()] = x.cuda()
        return buf

    host = [dict(p=torch.randn(n, generator=g), m=0.1 * torch.randn(n, generator=g), v=0.01 * torch.rand(n, generator=g))
            for n in ADAM_SIZES]
    multi = [{k: guarded(t[k]) for k in "pmv"} for t in host]
    single = [{k: guarded(t[k]) for k in "pmv"} for t in host]
    grads = [torch.empty(n, device="cuda") for n in ADAM_SIZES]
    table = torch.tensor([[t["p"].data_ptr(), gr.data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), n]
                          for t, gr, n in zip(multi, grads, ADAM_SIZES)], dtype=torch.int64).cuda()
    step = torch.tensor([step0], dtype=torch.int32, device="cuda")
    params = [t["p"].clone().requires_grad_(True) for t in host]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps)
    for q, t in zip(params, host):
        opt.state[q] = dict(step=torch.tensor(float(step0)), exp_avg=t["m"].clone(), exp_avg_sq=t["v"].clone())
    for _ in range(3):
        assert lib.ns_add_i32(_ptr(step), 1, _stream()) == 0
        for q, gr, n in zip(params, grads, ADAM_SIZES):
            q.grad = torch.randn(n, generator=g)
            gr.copy_(q.grad)
        assert lib.ns_adam_step_multi_dev(_ptr(table), len(ADAM_SIZES), max(ADAM_SIZES), lr_arg, _ptr(lr_dev), b1, b2, eps,
                                          _ptr(step), _stream()) == 0, lib.ns_last_error()
        for t, gr, n in zip(single, grads, ADAM_SIZES):
            assert lib.ns_adam_step_dev(_ptr(t["p"]), _ptr(gr), _ptr(t["m"]), _ptr(t["v"]), n, lr_arg, _ptr(lr_dev), b1, b2, eps,
                                        _ptr(step), _stream()) == 0, lib.ns_last_error()
        opt.step()
    assert int(step) == step0 + 3
    for t, s, q, n in zip(multi, single, params, ADAM_SIZES):
        for k in "pmv":
            assert torch.equal(t[k], s[k]), (n, k, "multi-tensor and per-tensor launches differ in bits")
            assert bool((t[k][n:] == SENTINEL).all()), (n, k, "guard band")
        st = opt.state[q]
        for got, want in ((t["p"], q.detach()), (t["m"], st["exp_avg"]), (t["v"], st["exp_avg_sq"])):
            assert torch.allclose(got[:n].cpu(), want, rtol=1e-5, atol=1e-6), n
        assert not torch.equal(t["p"][:n].cpu(), host[ADAM_SIZES.index(n)]["p"])


def test_multi_tensor_adam_with_nothing_to_do_touches_nothing():
    lib = _lib.load()
    n = 300
    bufs = [torch.full((n,), SENTINEL, device="cuda") for _ in range(4)]
    table = torch.tensor([[b.data_ptr() for b in bufs] + [n]], dtype=torch.int64).cuda()
    step = torch.tensor([1], dtype=torch.int32, device="cuda")
    assert lib.ns_adam_step_multi_dev(_ptr(table), 0, n, 1e-3, None, 0.9, 0.999, 1e-8, _ptr(step), _stream()) == 0
    assert lib.ns_adam_step_multi_dev(_ptr(table), 1, 0, 1e-3, None, 0.9, 0.999, 1e-8, _ptr(step), _stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs) and int(step) == 1
