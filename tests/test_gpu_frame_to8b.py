"""ns_frame_to8b against run_nerf_helpers.to8b -- (255 * np.clip(x, 0, 1)).astype(np.uint8) on the host copy of the same fp32
input -- bit for bit: every pixel count around the four-pixel group, the wave and the workgroup, both input layouts, both
channel counts, inputs that start 0 .. 3 floats and outputs that start 0 .. 3 bytes into their allocations (the dword and the
byte store paths, the float4 and the single-float load paths), with the bytes around the output checked; the fp32 values at
which the rounding of 255 * x decides the truncation; NaN -> 0; the refusals."""

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PIXELS = [1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 143, 2401]
POISON = 0xA5
FENCE = 8                                   # poison bytes kept after the written range (and 0 .. 3 before it)
_cache = {}


def _to8b(x):
    from nerf_sampling_amd.run_nerf_helpers import to8b

    with np.errstate(invalid="ignore"):
        return to8b(x)


def _pixels():
    """fp32 [max n, 4] on the host, shared by every layout test: colours and an alpha column in [-0.25, 1.25] with the
    edge values sprinkled in, no NaN"""
    if "pixels" not in _cache:
        rng = np.random.default_rng(8)
        x = (rng.random((max(N_PIXELS), 4), dtype=np.float32) * np.float32(1.5) - np.float32(0.25))
        edge = np.array([0.0, -0.0, 1.0, np.inf, -np.inf, 1e-40, 0.5, np.nextafter(np.float32(1), np.float32(0))], np.float32)
        where = rng.integers(0, x.size, 600)
        x.reshape(-1)[where] = edge[rng.integers(0, edge.size, 600)]
        _cache["pixels"] = x
    return _cache["pixels"]


@pytest.mark.parametrize("channels,with_alpha", [(3, False), (3, True), (4, False), (4, True)])
@pytest.mark.parametrize("stride", [3, 4])
def test_every_layout_is_numpys_to8b_and_stays_inside_its_range(stride, channels, with_alpha):
    from nerf_sampling_amd import ops

    px = _pixels()
    checked = 0
    for n in N_PIXELS:
        want = _to8b(px[:n, :3])
        if channels == 4:
            a8 = _to8b(px[:n, 3:]) if with_alpha else np.full((n, 1), 255, np.uint8)
            want = np.concatenate([want, a8], 1)
        for in_off in range(4):
            flat = torch.full((in_off + n * stride + 4,), float("nan"), dtype=torch.float32, device="cuda")
            if stride == 3:
                rgb = flat[in_off:in_off + n * 3].view(n, 3)
                rgb.copy_(torch.from_numpy(px[:n, :3]))
            else:                                                   # the [:, :3] view of [n,4]; the fourth float stays NaN
                rgb = flat[in_off:in_off + n * 4].view(n, 4)[:, :3]
                rgb.copy_(torch.from_numpy(px[:n, :3]))
                assert tuple(rgb.stride()) == (4, 1) and not rgb.is_contiguous() or n == 1
            alpha = torch.from_numpy(np.ascontiguousarray(px[:n, 3])).cuda() if with_alpha else None
            for out_off in range(4):
                buf = torch.full((out_off + n * channels + FENCE,), POISON, dtype=torch.uint8, device="cuda")
                out = buf[out_off:out_off + n * channels]
                got = ops.frame_to8b(rgb, alpha=alpha, out=out, channels=channels)
                assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, channels) and got.dtype == torch.uint8
                host = buf.cpu().numpy()
                where = (stride, channels, with_alpha, n, in_off, out_off)
                assert np.array_equal(host[out_off:out_off + n * channels].reshape(n, channels), want), where
                assert (host[:out_off] == POISON).all() and (host[out_off + n * channels:] == POISON).all(), where
                checked += 1
    assert checked == len(N_PIXELS) * 16
    fresh = ops.frame_to8b(rgb, alpha=alpha, channels=channels)       # allocated by the call
    assert np.array_equal(fresh.cpu().numpy(), want)


def _run(values):
    """to8b of a flat fp32 array through the kernel (padded to whole pixels) -> uint8 of the same length"""
    from nerf_sampling_amd import ops

    v = np.asarray(values, dtype=np.float32).reshape(-1)
    pad = (-v.size) % 3
    x = np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, 3)
    return ops.frame_to8b(torch.from_numpy(x).cuda()).cpu().numpy().reshape(-1)[:v.size]


def test_the_values_where_rounding_decides_the_truncation():
    """for k = 0 .. 255 the nine fp32 numbers from 4 ulps below to 4 ulps above fl(k / 255) (255 * x lands on or beside the
    integer k there; k = 0 and k = 255 are the neighbourhoods of 0 and 1), then denormals, signed zeros, values outside
    [0, 1] and the infinities"""
    vals = []
    for k in range(256):
        centre = np.float32(k) / np.float32(255)
        lo = hi = centre
        around = [centre]
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            around += [lo, hi]
        vals += sorted(around)
    vals = np.array(vals, dtype=np.float32)
    assert vals.size == 256 * 9 and np.isfinite(vals).all()
    got, want = _run(vals), _to8b(vals)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert set(want.tolist()) == set(range(256))                                     # every byte value is reached
    tiny = np.float32(1e-45)
    special = np.array([0.0, -0.0, tiny, -tiny, 1e-40, -1e-40, 1.1754942e-38, 1.17549435e-38, -1.17549435e-38, -1e-3, -1.0,
                        -3.4e38, 1.0000001, 1.5, 2.0, 256.0, 3.4e38, np.inf, -np.inf, 0.999999, 0.99999994, 0.5, 0.25,
                        1.0 / 255.0, 0.00392156, 0.00392157], dtype=np.float32)
    got, want = _run(special), _to8b(special)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert got[1] == 0 and got[17] == 255 and got[18] == 0 and got[16] == 255 and got[11] == 0


def test_random_bit_patterns_and_nans():
    bits = np.random.default_rng(20).integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    nan = np.isnan(x)
    assert 1000 < nan.sum() < x.size // 50
    got = _run(x)
    want = _to8b(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert (got[nan] == 0).all()                                                     # the kernel's rule, whatever numpy gave
    # NaNs of both signs, quiet and signalling, several payloads
    payloads = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA5A5A5, 0xFFD00D00,
                         0x7F800100, 0xFFBFFFFF], dtype=np.uint32)
    x = payloads.view(np.float32)
    assert np.isnan(x).all()
    assert (_run(x) == 0).all()
    # ... also in the alpha channel, and beside finite neighbours in one group
    from nerf_sampling_amd import ops

    rgb = torch.tensor([[0.5, float("nan"), 1.0], [float("nan"), 0.25, float("nan")]], device="cuda")
    alpha = torch.tensor([float("nan"), 1.0], device="cuda")
    assert ops.frame_to8b(rgb, alpha=alpha, channels=4).cpu().tolist() == [[127, 0, 255, 0], [0, 63, 0, 255]]


def test_refusals_leave_the_output_alone_and_an_empty_frame_is_a_no_op():
    from nerf_sampling_amd import _lib, ops

    lib = _lib.load()
    rgb = torch.rand(16, 3, device="cuda")
    out = torch.full((64,), POISON, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r, o = C.c_void_p(rgb.data_ptr()), C.c_void_p(out.data_ptr())
    bad = [(None, 0, None, 16, o, 3), (r, 0, None, 16, None, 3), (r, 0, None, -1, o, 3), (r, 0, None, 2 ** 29, o, 3)]
    bad += [(r, st, None, 16, o, 3) for st in (-1, 1, 2, 5)] + [(r, 0, None, 16, o, c) for c in (0, 1, 2, 5)]
    for args in bad:
        assert lib.ns_frame_to8b(*args, s) == -1, args
    assert lib.ns_frame_to8b(r, 0, None, 0, o, 3, s) == 0 and lib.ns_frame_to8b(None, 0, None, 0, None, 4, s) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
    # the wrapper: an empty frame, and what it refuses itself
    assert tuple(ops.frame_to8b(rgb[:0]).shape) == (0, 3)
    for kwargs in (dict(channels=2), dict(out=out[:47]), dict(out=out[:48].float()), dict(alpha=rgb[:, 0], channels=4),
                   dict(alpha=torch.zeros(15, device="cuda"), channels=4)):
        with pytest.raises(ValueError):
            ops.frame_to8b(rgb, **kwargs)
    with pytest.raises(ValueError):
        ops.frame_to8b(torch.rand(16, 6, device="cuda")[:, ::2])                     # neither packed nor the [R,4] view
    with pytest.raises(ValueError):
        ops.frame_to8b(rgb.double())
    with pytest.raises(RuntimeError):
        ops.frame_to8b(rgb.cpu())
    assert (out.cpu().numpy() == POISON).all()
