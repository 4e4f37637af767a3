"""ns_map_to8b / ops.map_to8b against numpy's own arithmetic on the host copy of the same fp32 input, bit for bit:

    q = x / np.float32(m);  expected = np.where(np.isnan(q), 0, 255 * np.clip(q, 0, 1)).astype(np.uint8)

-- the reference's to8b(disps / np.max(disps)) (Trainer.py:371-376) with a NaN quotient defined as 0.  Every count around the
four-value group, the wave and the workgroup; packed maps that start 0 .. 3 floats into their allocation (the float4 and the
single-float loads) and the [:, 3] column of an [R,4] shard; outputs that start 0 .. 3 bytes into a fenced buffer (the dword
and the byte stores); the fp32 neighbours of k * m / 255, where a reciprocal and a multiply would round differently from the one
division; random bit patterns; divisors of 0, inf, NaN and -inf; no divisor at all."""

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099]
DIVISORS = [0.7, 1.0, 3.0, 1e-30, 1e10]
POISON = 0xA5
FENCE = 8
_cache = {}


def expected(x, m):
    with np.errstate(all="ignore"):
        q = x / np.float32(m)
        return np.where(np.isnan(q), 0, 255 * np.clip(q, 0, 1)).astype(np.uint8)


def _denom(m):
    """the divisor as one float of device memory that is 4-byte but not 8-byte aligned (the second of three)"""
    return torch.tensor([np.nan, m, np.nan], dtype=torch.float32, device="cuda")[1:2]


def _values():
    """fp32 [max count] on the host, shared by the layout tests: disparities in [-0.1, 0.9] against the divisor 0.7, with
    the edge values and some NaNs sprinkled in"""
    if "values" not in _cache:
        rng = np.random.default_rng(41)
        x = rng.random(max(COUNTS), dtype=np.float32) - np.float32(0.1)
        edge = np.array([0.0, -0.0, 0.7, np.inf, -np.inf, np.nan, 1e-40, 0.35, np.nextafter(np.float32(0.7), np.float32(0))],
                        np.float32)
        where = rng.integers(0, x.size, 400)
        x[where] = edge[rng.integers(0, edge.size, 400)]
        x[:4] = [0.35, np.nan, 0.7, 0.1]
        _cache["values"] = x
    return _cache["values"]


def _device_map(x, layout, in_off):
    """x on the device as a packed map that starts in_off floats into its allocation, or as the [:, 3] column of an [n,4]
    shard whose other columns hold values that would give other bytes"""
    n = x.size
    if layout == "packed":
        flat = torch.full((in_off + n + 4,), 0.5, dtype=torch.float32, device="cuda")
        m = flat[in_off:in_off + n]
        m.copy_(torch.from_numpy(x))
        assert m.is_contiguous()
        return m
    flat = torch.full((in_off + n * 4,), 0.5, dtype=torch.float32, device="cuda")
    shard = flat[in_off:].view(n, 4)
    shard[:, 3].copy_(torch.from_numpy(x))
    m = shard[:, 3]
    assert n == 1 or (int(m.stride(0)) == 4 and not m.is_contiguous())
    assert (m.data_ptr() - flat.data_ptr()) % 16 == (4 * in_off + 12) % 16
    return m


@pytest.mark.parametrize("layout", ["packed", "column"])
def test_every_layout_is_numpys_bytes_and_stays_inside_its_range(layout):
    from nerf_sampling_amd import ops

    x, denom = _values(), _denom(0.7)
    checked = 0
    for n in COUNTS:
        want = expected(x[:n], 0.7)
        for in_off in range(4):
            m = _device_map(x[:n], layout, in_off)
            for out_off in range(4):
                buf = torch.full((out_off + n + FENCE,), POISON, dtype=torch.uint8, device="cuda")
                out = buf[out_off:out_off + n]
                got = ops.map_to8b(m, denom=denom, out=out)
                assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n,) and got.dtype == torch.uint8
                host = buf.cpu().numpy()
                where = (layout, n, in_off, out_off)
                assert np.array_equal(host[out_off:out_off + n], want), where
                assert (host[:out_off] == POISON).all() and (host[out_off + n:] == POISON).all(), where
                checked += 1
    assert checked == len(COUNTS) * 16
    assert np.array_equal(ops.map_to8b(m, denom=denom).cpu().numpy(), want)          # allocated by the call


def _run(x, m, layout="packed"):
    from nerf_sampling_amd import ops

    x = np.ascontiguousarray(x, dtype=np.float32)
    return ops.map_to8b(_device_map(x, layout, 0), denom=None if m is None else _denom(m)).cpu().numpy()


@pytest.mark.parametrize("m", DIVISORS)
def test_the_neighbours_of_k_m_over_255(m):
    """the three fp32 neighbours of fl(k * m / 255) for every k: the quotient lands on or beside k / 255, where the last bit of
    the division decides the byte.  With the divisor 0.7 a reciprocal and a multiply give other bytes on some of them: the case
    tells the two apart."""
    vals = []
    for k in range(256):
        centre = np.float32(k) * np.float32(m) / np.float32(255)
        vals += [np.nextafter(centre, np.float32(-np.inf)), centre, np.nextafter(centre, np.float32(np.inf))]
    x = np.array(vals, dtype=np.float32)
    assert x.size == 768 and np.isfinite(x).all()
    want = expected(x, m)
    for layout in ("packed", "column"):
        got = _run(x, m, layout)
        assert np.array_equal(got, want), (layout, np.flatnonzero(got != want)[:8].tolist())
    assert len(set(want.tolist())) >= 255
    if m == 0.7:
        with np.errstate(all="ignore"):
            recip = (np.float32(255) * np.clip(x * (np.float32(1) / np.float32(m)), 0, 1)).astype(np.uint8)
        assert (recip != want).sum() > 0


def test_random_bit_patterns():
    """2^20 bit patterns, NaNs, infinities and denormals among them, under a tiny, an ordinary and a large divisor"""
    bits = np.random.default_rng(21).integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32).copy()
    x[:6] = [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40]
    nan = np.isnan(x)
    assert 1000 < nan.sum() < x.size // 50
    for m in (1e-30, 0.7, 1e10):
        got, want = _run(x, m), expected(x, m)
        assert np.array_equal(got, want), (m, np.flatnonzero(got != want)[:8].tolist())
        assert (got[nan] == 0).all() and got[0] == 255 and got[1] == 0


def test_divisors_that_make_nan_quotients():
    """m = 0, inf, NaN, -inf: numpy's NaN quotients (0 / 0, inf / inf, anything over NaN) are written as 0, the others as numpy
    writes them"""
    x = np.array([0.0, -0.0, 0.25, -0.25, np.inf, -np.inf, np.nan, 1e-40, 3.4e38, 0.5, 0.7], dtype=np.float32)
    for m in (0.0, -0.0, np.inf, np.nan, -np.inf):
        for layout in ("packed", "column"):
            got, want = _run(x, m, layout), expected(x, m)
            assert np.array_equal(got, want), (m, layout, got.tolist(), want.tolist())
    assert _run(x, 0.0).tolist() == [0, 0, 255, 0, 255, 0, 0, 255, 255, 255, 255]
    assert _run(x, np.inf).tolist() == [0] * 11 and _run(x, np.nan).tolist() == [0] * 11
    assert _run(x, -np.inf).tolist() == [0] * 11


def test_no_divisor_is_the_divisor_one():
    x = _values()
    for layout in ("packed", "column"):
        got = _run(x, None, layout)
        assert np.array_equal(got, _run(x, 1.0, layout)) and np.array_equal(got, expected(x, 1.0))


def test_refusals_leave_the_output_alone_and_an_empty_map_is_a_no_op():
    from nerf_sampling_amd import _lib, ops

    lib = _lib.load()
    x = torch.rand(16, device="cuda")
    den = _denom(0.7)
    out = torch.full((32,), POISON, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xp, dp, o = C.c_void_p(x.data_ptr()), C.c_void_p(den.data_ptr()), C.c_void_p(out.data_ptr())
    bad = [(None, 1, 16, dp, o), (xp, 1, 16, dp, None), (xp, 1, -1, dp, o), (xp, 1, 2 ** 31, dp, o),
           (xp, 1, 16, C.c_void_p(den.data_ptr() + 2), o)]
    bad += [(xp, st, 16, dp, o) for st in (-1, 0, 2, 3, 5)]
    for args in bad:
        assert lib.ns_map_to8b(*args, s) == -1, args
        assert b"ns_map_to8b" in lib.ns_last_error()
    assert lib.ns_map_to8b(xp, 1, 0, dp, o, s) == 0 and lib.ns_map_to8b(None, 4, 0, None, None, s) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
    assert tuple(ops.map_to8b(x[:0], denom=den).shape) == (0,)
    for kwargs in (dict(out=out[:15]), dict(out=out[:16].float()), dict(denom=torch.ones(2, device="cuda")),
                   dict(denom=torch.ones(1, device="cuda", dtype=torch.float64)), dict(denom=torch.ones(1)), dict(denom=0.7)):
        with pytest.raises(ValueError):
            ops.map_to8b(x, **kwargs)
    for bad_map in (torch.rand(16, 2, device="cuda"), torch.rand(48, device="cuda")[::3], x.double()):
        with pytest.raises(ValueError):
            ops.map_to8b(bad_map)
    with pytest.raises(RuntimeError):
        ops.map_to8b(x.cpu())
    assert (out.cpu().numpy() == POISON).all()
