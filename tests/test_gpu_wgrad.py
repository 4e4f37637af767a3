"""ns_gemm_wgrad on the GPU: dW = dy^T x and db = column sums of dy, rows split over workgroups, slices summed in a fixed order.

Exactness: integer inputs in [-4, 4] stored as fp32 make every partial sum an integer below 2^24 (rows <= 65 536: |sum| <= 16 rows
<= 2^20), so dW and db must equal an int64 reference bit for bit whatever the summation order -- a dropped, duplicated or misplaced
row or column is a wrong integer.  The outputs sit inside a guard band of a sentinel value that must survive.
Random floats: per element |dW - dW64| <= rows 2^-24 sum_m |dy x|, the order-independent worst-case bound of an fp32 sum."""

import pytest
import torch

from nerf_sampling_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
PAD = 5


def _ptr(t):
    return None if t is None else t.data_ptr()


def _guarded(n_rows, n_cols, fill=None):
    """an [n_rows, n_cols] view in the middle of a sentinel-filled buffer (PAD on every side); its leading dimension is wider"""
    buf = torch.full((n_rows + 2 * PAD, n_cols + 2 * PAD), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[PAD : PAD + n_rows, PAD : PAD + n_cols]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _band_intact(buf, n_rows, n_cols):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[PAD : PAD + n_rows, PAD : PAD + n_cols] = False
    return bool((buf[mask] == SENTINEL).all())


def _workspace(rows, N, K):
    lib = _lib.load()
    nbytes = lib.ns_gemm_wgrad_workspace_bytes(rows, N, K)
    if nbytes == 0:
        return None, None
    buf = torch.full((nbytes // 4 + 2 * 64,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[64 : 64 + nbytes // 4]


def _call(dy, x, dW, db, accumulate=0, ws=None):
    lib = _lib.load()
    rows, N = dy.shape
    K = x.shape[1]
    assert x.stride(1) == 1 or K == 1
    stream = torch.cuda.current_stream().cuda_stream
    return lib.ns_gemm_wgrad(_ptr(dy), dy.stride(0), dy.stride(1), _ptr(x), x.stride(0), rows, N, K, _ptr(dW), dW.stride(0),
                             accumulate, _ptr(db), _ptr(ws), stream)


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).float()


def _run_exact(N, K, rows, dy_layout="plain", x_wide=False, accumulate=False, want_db=True, seed=0):
    dy_h, x_h = _ints((rows, N), seed), _ints((rows, K), seed + 1)
    if dy_layout == "plain":
        dy = dy_h.cuda()
    else:                                   # columns 0..2 / column 3 of an [rows, 4] tensor
        assert N == (3 if dy_layout == "rgb" else 1)
        g4 = _ints((rows, 4), seed + 2)
        if dy_layout == "rgb":
            g4[:, :3] = dy_h
            dy = g4.cuda()[:, :3]
        else:
            g4[:, 3:4] = dy_h
            dy = g4.cuda()[:, 3:4]
    if x_wide:                              # a column slice of a wider buffer
        wide = _ints((rows, K + 9), seed + 3)
        wide[:, 4 : 4 + K] = x_h
        x = wide.cuda()[:, 4 : 4 + K]
    else:
        x = x_h.cuda()
    ref_W = dy_h.double().t() @ x_h.double()          # exact: integers far below 2^53
    ref_b = dy_h.double().sum(0)
    init = None
    if accumulate:
        init = _ints((N, K), seed + 4)
        ref_W = ref_W + init.double()
    wbuf, dW = _guarded(N, K, fill=None if init is None else init.cuda())
    bbuf, db = _guarded(1, N)
    wsbuf, ws = _workspace(rows, N, K)
    rc = _call(dy, x, dW, db[0] if want_db else None, int(accumulate), ws)
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().ns_last_error()
    assert torch.equal(dW.cpu().double(), ref_W), f"dW differs at {(dW.cpu().double() != ref_W).sum().item()} elements"
    if want_db:
        assert torch.equal(db[0].cpu().double(), ref_b)
    else:
        assert bool((db == SENTINEL).all())
    assert _band_intact(wbuf, N, K) and _band_intact(bbuf, 1, N)
    if wsbuf is not None:
        assert bool((wsbuf[:64] == SENTINEL).all()) and bool((wsbuf[64 + ws.numel():] == SENTINEL).all())


SHAPES = [(32, 32, 1), (1, 63, 5), (3, 128, 100), (128, 283, 1025), (256, 319, 4097), (97, 160, 20001), (256, 256, 65536)]


@pytest.mark.parametrize("N,K,rows", SHAPES)
def test_exact_integers(N, K, rows):
    _run_exact(N, K, rows)


def _split_changes(N, K, lo=1025, hi=65536):
    """rows r in [lo, hi] with splits(r) != splits(r - 1), found by bisection on the non-decreasing split count"""
    lib = _lib.load()
    f = lambda r: lib.ns_gemm_wgrad_splits(r, N, K)  # noqa: E731
    out = []

    def walk(a, b):                # f(a) != f(b), a < b
        if b - a == 1:
            out.append(b)
            return
        m = (a + b) // 2
        if f(a) != f(m):
            walk(a, m)
        if f(m) != f(b):
            walk(m, b)

    if f(lo - 1) != f(hi):
        walk(lo - 1, hi)
    return sorted(out)


@pytest.mark.parametrize("N,K", [(40, 72), (256, 256)])
def test_exact_on_both_sides_of_every_split_change(N, K):
    changes = _split_changes(N, K)
    assert changes and changes[0] == 1025, changes       # rows <= 1024 are never split, 1025 are
    lib = _lib.load()
    for r in changes:
        assert lib.ns_gemm_wgrad_splits(r - 1, N, K) < lib.ns_gemm_wgrad_splits(r, N, K)
        _run_exact(N, K, r - 1, seed=r)
        _run_exact(N, K, r, seed=r + 7)


@pytest.mark.parametrize("rows", [100, 4097])
@pytest.mark.parametrize("layout,N", [("rgb", 3), ("sigma", 1)])
def test_exact_strided_dy(layout, N, rows):
    _run_exact(N, 128, rows, dy_layout=layout)


@pytest.mark.parametrize("rows", [100, 4097])
def test_exact_x_column_slice_accumulate_and_no_db(rows):
    _run_exact(128, 283, rows, x_wide=True)
    _run_exact(128, 283, rows, accumulate=True)
    _run_exact(97, 160, rows, x_wide=True, accumulate=True, want_db=False)


@pytest.mark.parametrize("N,K,rows", [(256, 319, 4097), (128, 283, 20001)])
def test_random_floats_within_the_fp32_sum_bound_and_reproducible(N, K, rows):
    g = torch.Generator().manual_seed(1234)
    dy_h, x_h = torch.randn((rows, N), generator=g), torch.randn((rows, K), generator=g)
    dy, x = dy_h.cuda(), x_h.cuda()
    outs = []
    for _ in range(2):
        dW = torch.empty((N, K), dtype=torch.float32, device="cuda")
        db = torch.empty((N,), dtype=torch.float32, device="cuda")
        _, ws = _workspace(rows, N, K)
        assert _call(dy, x, dW, db, 0, ws) == 0
        torch.cuda.synchronize()
        outs.append((dW.cpu(), db.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls must give the same bits"
    ref_W = dy_h.double().t() @ x_h.double()
    bound_W = rows * 2.0 ** -24 * (dy_h.double().abs().t() @ x_h.double().abs())
    err_W = (outs[0][0].double() - ref_W).abs()
    print(f"wgrad {N}x{K}x{rows}: max err / bound = {float((err_W / bound_W).max()):.3e}")
    assert bool((err_W <= bound_W).all())
    ref_b = dy_h.double().sum(0)
    bound_b = rows * 2.0 ** -24 * dy_h.double().abs().sum(0)
    assert bool(((outs[0][1].double() - ref_b).abs() <= bound_b).all())


def test_error_returns_launch_nothing():
    """each bad argument gives its status and the outputs keep their sentinel (no launch was made)"""
    rows, N, K = 2048, 8, 16
    dy, x = _ints((rows, N), 1).cuda(), _ints((rows, K), 2).cuda()
    wbuf, dW = _guarded(N, K)
    db = torch.full((N,), SENTINEL, dtype=torch.float32, device="cuda")
    _, ws = _workspace(rows, N, K)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(dy=_ptr(dy), s0=N, s1=1, x=_ptr(x), sx=K, rows=rows, N=N, K=K, dW=_ptr(dW), ldw=dW.stride(0), acc=0, db=_ptr(db),
                 ws=_ptr(ws))
        a.update(kw)
        return lib.ns_gemm_wgrad(a["dy"], a["s0"], a["s1"], a["x"], a["sx"], a["rows"], a["N"], a["K"], a["dW"], a["ldw"], a["acc"],
                                 a["db"], a["ws"], stream)

    for bad in (dict(dy=None), dict(x=None), dict(dW=None), dict(rows=0), dict(rows=1 << 31), dict(N=0), dict(K=0),
                dict(ldw=K - 1), dict(s0=-1), dict(acc=3), dict(ws=None)):
        assert call(**bad) == -1, bad
    for bad in (dict(N=513), dict(K=513)):
        assert call(**bad) == -2, bad
    torch.cuda.synchronize()
    assert bool((wbuf == SENTINEL).all()) and bool((db == SENTINEL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(dW.cpu().double(), dy.cpu().double().t() @ x.cpu().double())
