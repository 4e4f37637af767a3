"""ns_depth_sqerr / ops.depth_sqerr: sum over rays and samples of (double)(fl32(z[r, k] - ref[r]))^2, in double on the device.
Yardstick: an int64 sum where every term is exact, the float64 sum of the squared fp32 differences on random floats.

S, the number of flat elements r * N + k one workgroup owns, is the header's NS_DEPTH_SQERR_SHARE, and what the library does
with it is checked through ns_depth_sqerr_workspace_bytes (one double per share).  The ray counts straddle 64 (a wave), 256 (a
workgroup's threads) and S: with N = 1 they put the last ray into the last lane of a share, the first lane of the next and one
beyond two shares; with the other N the share boundary falls inside a ray."""

import ctypes as C
import math
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0
N_SAMPLES = [1, 2, 3, 63, 64, 65, 192]


def _share():
    from nerf_sampling_amd import _lib

    text = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
    S = int(re.search(r"#define NS_DEPTH_SQERR_SHARE (\d+)", text).group(1))
    lib = _lib.load()
    assert lib.ns_depth_sqerr_workspace_bytes(32 * S, 1) == 256 and lib.ns_depth_sqerr_workspace_bytes(32 * S + 1, 1) == 512
    return S


S = _share()
RAYS = [1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S + 1]


def _grid(R, N, seed):
    """z [R,N] and ref [R] as integers k: the values are 2 + k / 64 in [2, 6], so every difference is a multiple of 1/64 below
    4, every square a multiple of 2^-12 below 16, and the whole sum at most R N 2^16 < 2^53 units of 2^-12 in any order"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 257, size=(R, N)), rng.integers(0, 257, size=(R,))


def _grid_reference(kz, kr):
    d = kz.astype(np.int64) - kr.astype(np.int64)[:, None]
    return float(np.sum(d * d, dtype=np.int64)) / 4096.0


def _depths(k):
    return (np.float32(2.0) + k.astype(np.float32) / np.float32(64.0)).astype(np.float32)


def _guarded_workspace(R, N):
    import torch

    from nerf_sampling_amd import ops

    need = ops.depth_sqerr_workspace_bytes(R, N)
    assert need >= 8 * ((R * N + S - 1) // S) and need % 256 == 0
    buf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[256:256 + need]


@pytest.mark.parametrize("N", N_SAMPLES)
@pytest.mark.parametrize("R", RAYS)
def test_exact_on_a_dyadic_grid(R, N):
    """Packed z (and the vector form for N = 1), z as a column slice of a wider buffer poisoned with NaN, ref as [R] and [R,1],
    the sum written into a slot of a longer array, a repeat on a second stream: all EQUAL the int64 reference, and the other
    slots and the guard bands around the workspace stay untouched."""
    import torch

    from nerf_sampling_amd import ops

    kz, kr = _grid(R, N, seed=R * 1000 + N)
    want = _grid_reference(kz, kr)
    z = torch.from_numpy(_depths(kz)).cuda()
    ref = torch.from_numpy(_depths(kr)).cuda()
    wide = torch.full((R, N + 5), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, 2:2 + N] = z
    forms = [(z, ref), (wide[:, 2:2 + N], ref.reshape(R, 1))]
    if N == 1:
        forms += [(z.reshape(R), ref), (wide[:, 2], ref)]
    out = torch.full((len(forms) + 3,), SENTINEL, dtype=torch.float64, device="cuda")
    buf, ws = _guarded_workspace(R, N)
    for i, (zf, rf) in enumerate(forms):
        assert ops.depth_sqerr(zf, rf, out=out, slot=i + 1, workspace=ws) is out
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.depth_sqerr(z, ref, out=out, slot=len(forms) + 1)
    side.synchronize()
    one = ops.depth_sqerr(z, ref)
    assert one.shape == (1,) and one.dtype == torch.float64 and one.is_cuda
    got = out.cpu().numpy()
    print(f"R={R} N={N}: got {got[1:-1].tolist()} and {float(one.cpu()[0])!r}, int64 reference {want!r}")
    assert got[0] == SENTINEL and got[-1] == SENTINEL
    assert (got[1:-1] == want).all() and float(one.cpu()[0]) == want
    b = buf.cpu().numpy()
    assert (b[:256] == 0xA5).all() and (b[-256:] == 0xA5).all()


@pytest.mark.parametrize("N", N_SAMPLES)
@pytest.mark.parametrize("R", RAYS)
def test_random_floats_within_the_summation_bound(R, N):
    """|got - ref| <= n 2^-52 ref, n = R N, ref the float64 numpy sum of the squared fp32 differences: each of the two sums of n
    non-negative terms is within (n - 1) 2^-53 of the true sum whatever its order.  The same bits on a second call."""
    import torch

    from nerf_sampling_amd import ops

    rng = np.random.default_rng(R * 77 + N)
    z_h = (rng.random((R, N), dtype=np.float32) * np.float32(4.0) + np.float32(2.0)).astype(np.float32)
    ref_h = (rng.random((R,), dtype=np.float32) * np.float32(4.0) + np.float32(2.0)).astype(np.float32)
    d = z_h - ref_h[:, None]
    assert d.dtype == np.float32
    d = d.astype(np.float64)
    want = float(np.sum(d * d))
    z, ref = torch.from_numpy(z_h).cuda(), torch.from_numpy(ref_h).cuda()
    one, again = ops.depth_sqerr(z, ref), ops.depth_sqerr(z, ref.reshape(R, 1))
    got = float(one.cpu()[0])
    bound = R * N * 2.0 ** -52 * want
    print(f"R={R} N={N}: got {got!r} ref {want!r} |diff| {abs(got - want):.3e} bound {bound:.3e}")
    assert abs(got - want) <= bound
    assert one.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    assert float(ops.mse_from_sqerr(one, R * N)[0]) == got / (R * N)


@pytest.mark.parametrize("R,N,at", [(1, 1, (0, 0)), (65, 3, (64, 2)), (S + 1, 1, (S, 0)), (2 * S + 1, 65, (S // 65, S % 65)),
                                    (257, 64, (0, 0)), (257, 64, (256, 63))])
def test_one_nan_anywhere_makes_the_sum_nan(R, N, at):
    """in z (a ray that misses the sphere has a NaN DepthNet depth) or in ref; the neighbouring slots keep their sums"""
    import torch

    from nerf_sampling_amd import ops

    kz, kr = _grid(R, N, seed=R + N)
    z_h, ref_h = _depths(kz), _depths(kr)
    out = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda")
    z_nan, ref_nan = z_h.copy(), ref_h.copy()
    z_nan[at] = np.nan
    ref_nan[at[0]] = np.nan
    dev = lambda a: torch.from_numpy(a).cuda()                                       # noqa: E731
    ops.depth_sqerr(dev(z_h), dev(ref_h), out=out, slot=0)
    ops.depth_sqerr(dev(z_nan), dev(ref_h), out=out, slot=1)
    ops.depth_sqerr(dev(z_h), dev(ref_nan), out=out, slot=2)
    ops.depth_sqerr(dev(z_h), dev(ref_h), out=out, slot=3)
    got = out.cpu().numpy()
    want = _grid_reference(kz, kr)
    assert got[0] == want and got[3] == want and got[4] == SENTINEL
    assert math.isnan(got[1]) and math.isnan(got[2])
    assert np.isnan(ops.mse_from_sqerr(out[1:3], R * N)).all()


def test_refusals_before_any_launch():
    """What the host knows is refused by the entry itself (NS_E_INVALID, which the loader's check turns into ValueError) and by
    the wrapper (ValueError); ``out`` and the workspace are never written."""
    import torch

    from nerf_sampling_amd import _lib, ops

    R, N = 65, 3
    kz, kr = _grid(R, N, seed=9)
    z, ref = torch.from_numpy(_depths(kz)).cuda(), torch.from_numpy(_depths(kr)).cuda()
    lib = _lib.load()
    out = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
    buf, ws = _guarded_workspace(R, N)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                          # noqa: E731

    def entry(z_p=p(z), stride=0, ref_p=p(ref), R_=R, N_=N, sum_p=p(out), ws_p=p(ws)):
        return lib.ns_depth_sqerr(z_p, stride, ref_p, R_, N_, sum_p, ws_p, stream)

    # R * N at and beyond 2^31: refused on the shape alone, before any pointer is followed
    for bad in (dict(z_p=None), dict(ref_p=None), dict(sum_p=None), dict(ws_p=None), dict(R_=0), dict(R_=-1), dict(N_=0),
                dict(N_=-2), dict(stride=1), dict(stride=N - 1), dict(stride=-N), dict(R_=2 ** 31, N_=1),
                dict(R_=2 ** 25, N_=64), dict(R_=2 ** 40, N_=3)):
        rc = entry(**bad)
        assert rc == -1, bad
        assert b"ns_depth_sqerr" in lib.ns_last_error()
        with pytest.raises(ValueError, match="ns_depth_sqerr"):
            _lib.check(rc, "ns_depth_sqerr")
    wide = torch.zeros((R, N + 2), dtype=torch.float32, device="cuda")
    for bad in (dict(z=z.double()), dict(z=z.cpu()), dict(z=z.reshape(R, N, 1)), dict(z=z[:0]), dict(z=z[:, :0]),
                dict(z=wide[:, ::2]), dict(z=z.t()), dict(z=z.as_strided((R, N), (N - 1, 1))),   # rows that overlap
                dict(ref=ref[:-1]), dict(ref=ref.double()), dict(ref=ref.cpu()), dict(ref=ref.reshape(1, R)),
                dict(ref=wide[:, 0]), dict(ref=z),
                dict(out=out.float()), dict(out=out.reshape(2, 1)), dict(out=out.cpu()), dict(slot=2), dict(slot=-1),
                dict(workspace=ws[:8].cpu()), dict(workspace=ws[:0]), dict(workspace=buf[257:257 + ws.numel()])):
        args = dict(z=z, ref=ref, out=out, slot=0, workspace=ws)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.depth_sqerr(**args)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (buf.cpu().numpy() == 0xA5).all()
    assert entry() == 0 and entry(stride=N) == 0                                     # and the call they vary is a good one
    assert float(out.cpu()[0]) == _grid_reference(kz, kr)
