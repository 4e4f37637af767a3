"""ns_cloud_append / ops.cloud_append / ops.PointCloud: the samples whose weight passes a threshold, compacted on the device in
the order of the flat element r * N + k.  Yardstick (tests/cloud_reference.py, numpy): mask = w >= t with NaN false; the points
are ops.points_along_rays(o, d, z)[mask] compared as BITS, the weights w[mask], the colours the kept samples' ray colours.

S, the number of flat elements one workgroup owns, is the header's NS_CLOUD_SHARE; what the library does with it is checked
through ns_cloud_workspace_bytes (one int64 per share).  Every call here goes through the C ABI with a workspace of exactly that
size, poisoned with 0xA5 and fenced by guard bytes, and with outputs poisoned the same way."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import cloud_reference as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
PAD = 8                                                   # poisoned records behind the capacity


def _share():
    from nerf_sampling_amd import _lib

    text = open(os.path.join(ROOT, "include", "nerf_sampling_hip.h")).read()
    S = int(re.search(r"#define NS_CLOUD_SHARE (\d+)", text).group(1))
    lib = _lib.load()
    assert lib.ns_cloud_workspace_bytes(32 * S, 1) == 256 and lib.ns_cloud_workspace_bytes(32 * S + 1, 1) == 512
    return S


S = _share()
N_SAMPLES = [1, 2, 3, 64, 65, 192]
TOTALS = [1, S - 1, S, S + 1, 3 * S + 77]                 # R * N lands on these, or on the two multiples of N around them


def _shapes():
    out = []
    for N in N_SAMPLES:
        rays = set()
        for T in TOTALS:
            rays |= {max(1, T // N), -(-T // N)}
        if N == 1:
            rays |= {63, 64, 65}                          # a wave boundary
        out += [(R, N) for R in sorted(rays)]
    return out


SHAPES = _shapes()


def _rays(R, N, seed):
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((R, 3)).astype(np.float32)
    d = rng.standard_normal((R, 3)).astype(np.float32)
    z = (rng.random((R, N), dtype=np.float32) * np.float32(4.0) + np.float32(2.0)).astype(np.float32)
    rgb = rng.random((R, 3), dtype=np.float32)
    return o, d, z, rgb


def _weights_of(mask, rng):
    """weights in [0.5, 1) where the mask is set and in [0, 0.5) elsewhere: threshold 0.5"""
    u = rng.random(mask.shape, dtype=np.float32) * np.float32(0.49)
    return np.where(mask, np.float32(0.5) + u, u).astype(np.float32)


def _patterns(R, N, seed):
    """(name, w [R,N], t, z override or None)"""
    rng = np.random.default_rng(seed)
    n = R * N
    flat = lambda m: _weights_of(m.reshape(R, N), rng)    # noqa: E731
    idx = np.arange(n)
    out = [("none", flat(np.zeros(n, bool)), 0.5), ("all", flat(np.ones(n, bool)), 0.5),
           ("one percent", flat(rng.random(n) < 0.01), 0.5), ("every second", flat(idx % 2 == 0), 0.5),
           ("first only", flat(idx == 0), 0.5), ("last only", flat(idx == n - 1), 0.5),
           ("one share", flat((idx >= S) & (idx < 2 * S) if n > S else idx >= 0), 0.5)]
    special = rng.random((R, N), dtype=np.float32)
    pick = rng.integers(0, 8, size=(R, N))
    special[pick == 0] = np.nan
    special[pick == 1] = np.inf
    special[pick == 2] = -np.inf
    out.append(("nan and inf weights", special, 0.5))
    out.append(("inf threshold", special, np.inf))
    zeros = np.array([-0.0, 0.0, -1e-30, 1e-30, np.nan], dtype=np.float32)[rng.integers(0, 5, size=(R, N))]
    out.append(("minus zero", zeros, 0.0))
    return out


class Call:
    """One cloud through the C ABI: poisoned outputs of capacity + PAD records, the counter, and a fenced workspace per call."""

    def __init__(self, capacity, colours=True, null_outputs=False):
        import torch

        self.capacity, self.colours = capacity, colours
        rows = capacity + PAD
        byte = lambda n: torch.full((n,), POISON, dtype=torch.uint8, device="cuda")   # noqa: E731
        self.pts = None if null_outputs else byte(rows * 12)
        self.w = None if null_outputs else byte(rows * 4)
        self.rgb = byte(rows * 12) if colours and not null_outputs else None
        self.count = torch.zeros((1,), dtype=torch.int64, device="cuda")
        self.fences = []

    def append(self, o, d, z, w, rgb, t, strided=False):
        """o, d [R,3], z, w [R,N], rgb [R,3]: host arrays.  ``strided``: z and w are column slices of [R, N + 5] buffers and rgb
        the first three columns of an [R,4] one, everything around them NaN."""
        import torch

        from nerf_sampling_amd import _lib

        lib = _lib.load()
        R, N = w.shape
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()             # noqa: E731
        o_t, d_t = dev(o), dev(d)
        if strided:
            zw = torch.full((2, R, N + 5), float("nan"), dtype=torch.float32, device="cuda")
            zw[0, :, 2:2 + N], zw[1, :, 3:3 + N] = dev(z), dev(w)
            z_t, w_t, zs, ws_ = zw[0, :, 2:2 + N], zw[1, :, 3:3 + N], N + 5, N + 5
            shard = torch.full((R, 4), float("nan"), dtype=torch.float32, device="cuda")
            shard[:, :3] = dev(rgb)
            c_t, cs = shard[:, :3], 4
        else:
            z_t, w_t, zs, ws_, c_t, cs = dev(z), dev(w), 0, 0, dev(rgb), 0
        need = lib.ns_cloud_workspace_bytes(R, N)
        assert need == (8 * ((R * N + S - 1) // S) + 255) // 256 * 256
        buf = torch.full((need + 512,), POISON, dtype=torch.uint8, device="cuda")
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())                 # noqa: E731
        rc = lib.ns_cloud_append(p(o_t), p(d_t), p(z_t), zs, p(w_t), ws_, p(c_t) if self.colours else None, cs, R, N, float(t),
                                 p(self.pts), p(self.w), p(self.rgb), self.capacity, p(self.count),
                                 C.c_void_p(buf.data_ptr() + 256), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.ns_last_error()
        self.fences.append(buf)
        return self

    def result(self):
        """(pts [capacity,3] as int32 bits, w [capacity] as int32 bits, rgb likewise or None, count) after checking that the
        records behind the capacity and the workspaces' fences still hold the poison"""
        for buf in self.fences:
            b = buf.cpu().numpy()
            assert (b[:256] == POISON).all() and (b[-256:] == POISON).all()
        count = int(self.count.cpu()[0])
        if self.pts is None:
            return None, None, None, count
        out = []
        for t, width in ((self.pts, 3), (self.w, 1), (self.rgb, 3)):
            if t is None:
                out.append(None)
                continue
            b = t.cpu().numpy()
            assert (b[self.capacity * 4 * width:] == POISON).all(), "written at or beyond the capacity"
            out.append(b[:self.capacity * 4 * width].view(np.int32).reshape(self.capacity, width))
        return out[0], out[1].reshape(-1), out[2], count


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _points(o, d, z):
    import torch

    from nerf_sampling_amd import ops

    pts = ops.points_along_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(z).cuda())
    return pts.cpu().numpy()


def _assert_records(got, want, kept_rows=None):
    """the first ``kept_rows`` records (all, by default) equal the reference's bit for bit; whatever lies between them and the
    capacity is still poison"""
    pts, w, rgb, _ = got
    want_pts, want_w, want_rgb = want
    m = len(want_w) if kept_rows is None else kept_rows
    assert (pts[:m] == _bits(want_pts)[:m]).all() and (w[:m] == _bits(want_w)[:m]).all()
    poison = np.int32(np.frombuffer(bytes([POISON] * 4), dtype=np.int32)[0])
    assert (pts[m:] == poison).all() and (w[m:] == poison).all()
    if rgb is not None:
        assert (rgb[:m] == _bits(want_rgb)[:m]).all() and (rgb[m:] == poison).all()


@pytest.mark.parametrize("R,N", SHAPES)
def test_every_pattern_equals_the_reference(R, N):
    """Ten weight patterns per shape, packed and strided inputs: the same records, the same count, nothing beyond them."""
    o, d, z, rgb = _rays(R, N, seed=R * 1000 + N)
    pts = _points(o, d, z)
    for name, w, t in _patterns(R, N, seed=R * 7 + N):
        want = CR.select(pts, w, rgb, t)
        kept = len(want[1])
        for strided in (False, True):
            got = Call(R * N).append(o, d, z, w, rgb, t, strided=strided).result()
            assert got[3] == kept, (name, strided, got[3], kept)
            _assert_records(got, want)
    # a NaN depth on a kept sample: the record is there, its point the NaN ns_points_along_rays writes
    z_nan = z.copy()
    z_nan[R - 1, N - 1] = np.nan
    w = np.full((R, N), 0.75, dtype=np.float32)
    got = Call(R * N).append(o, d, z_nan, w, rgb, 0.5).result()
    assert got[3] == R * N
    _assert_records(got, CR.select(_points(o, d, z_nan), w, rgb, 0.5))
    assert np.isnan(got[0][-1].view(np.float32)).all()


def test_no_rays_is_a_no_op():
    import torch

    from nerf_sampling_amd import ops

    e3, e2 = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
    call = Call(4)
    call.count.fill_(7)
    got = call.append(e3, e3, e2, e2, e3, 0.0).result()
    assert got[3] == 7
    _assert_records(got, (e3, np.zeros((0,), np.float32), e3))
    cloud = ops.PointCloud(4, colours=True)
    z = torch.zeros((0, 2), device="cuda")
    assert cloud.append(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), device="cuda"), z, z,
                        rgb=torch.zeros((0, 3), device="cuda")) is cloud
    assert cloud.count() == 0 and cloud.tensors()[0].shape == (0, 3)
    assert ops.cloud_workspace_bytes(0, 2) == 0 and ops.cloud_workspace_bytes(-1, 2) == 0 and ops.cloud_workspace_bytes(5, 0) == 0
    assert ops.cloud_workspace_bytes(2 ** 31, 1) == 0 and ops.cloud_workspace_bytes(2 ** 25, 64) == 0
    assert ops.cloud_workspace_bytes(2 ** 31 - 1, 1) == 8 * 2 ** 20


def _batches(shapes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, (R, N) in enumerate(shapes):
        o, d, z, rgb = _rays(R, N, seed=seed + i)
        out.append((o, d, z, _weights_of(rng.random((R, N)) < 0.3, rng), rgb))
    return out


@pytest.mark.parametrize("shapes", [[(S + 3, 3), (70, 64)], [(65, 1), (2 * S // 64 + 1, 64), (40, 65)]])
@pytest.mark.parametrize("colours", [True, False])
def test_appending_call_after_call(shapes, colours):
    """Two and three calls of different N into one cloud equal the concatenated reference; a second run gives the same bytes."""
    batches = _batches(shapes, seed=11)
    want = CR.select_batches([(_points(o, d, z), w, rgb) for o, d, z, w, rgb in batches], 0.5)
    kept = len(want[1])
    assert 0 < kept < sum(R * N for R, N in shapes)
    runs = []
    for _ in range(2):
        call = Call(kept + 5, colours=colours)
        for i, (o, d, z, w, rgb) in enumerate(batches):
            call.append(o, d, z, w, rgb, 0.5, strided=bool(i % 2))
        runs.append(call.result())
        assert runs[-1][3] == kept
        assert (runs[-1][2] is None) == (not colours)
        _assert_records(runs[-1], want)
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert a is None or a.tobytes() == b.tobytes()


@pytest.mark.parametrize("R,N", [(3 * S + 77, 1), (S // 3 + 5, 3), (100, 65)])
def test_capacity_is_never_exceeded(R, N):
    """capacity = kept - 3: the first capacity records are right, the counter says kept, and the poisoned records behind the
    capacity are untouched in all three outputs; capacity = 0 with NULL outputs only counts; a second call into a full cloud
    keeps counting."""
    (o, d, z, w, rgb), = _batches([(R, N)], seed=R + N)
    want = CR.select(_points(o, d, z), w, rgb, 0.5)
    kept = len(want[1])
    assert kept > 3
    got = Call(kept - 3).append(o, d, z, w, rgb, 0.5).result()          # result() checks the bytes behind the capacity
    assert got[3] == kept
    _assert_records(got, want, kept_rows=kept - 3)
    assert Call(0, null_outputs=True).append(o, d, z, w, rgb, 0.5).result()[3] == kept
    assert Call(0, colours=False).append(o, d, z, w, rgb, 0.5).result()[3] == kept
    twice = Call(kept + 2).append(o, d, z, w, rgb, 0.5).append(o, d, z, w, rgb, 0.5).result()
    assert twice[3] == 2 * kept
    assert (twice[0][:kept] == _bits(want[0])).all() and (twice[0][kept:] == _bits(want[0])[:2]).all()
    assert (twice[1][kept:] == _bits(want[1])[:2]).all() and (twice[2][kept:] == _bits(want[2])[:2]).all()


@pytest.mark.parametrize("shares", [2047, 2048, 2049, 4097])
def test_the_scan_across_its_tiles(shares):
    """The scan of the per-share counts walks tiles of 2048 entries with a carry and two LDS buffers in turn: one tile short of
    full, full, one entry into the second, one entry into the third.  About 1 % of the weights pass, and so do the first and the
    last flat element and the two elements on either side of the first tile boundary (the last of share 2047, the first of
    share 2048); two appends into one cloud, so that the second scan starts from a counter that is not 0."""
    N = 64
    assert S % N == 0
    R = shares * S // N - (shares != 2048)                                 # the last share is 64 elements short; at 2048, full
    n = R * N
    assert (n + S - 1) // S == shares
    o, d, z, rgb = _rays(R, N, seed=shares)
    pts = _points(o, d, z)
    rng = np.random.default_rng(shares + 1)
    mask = rng.random(n) < 0.01
    edges = [e for e in (0, 2048 * S - 1, 2048 * S, n - 1) if e < n]
    mask[edges] = True
    w = _weights_of(mask.reshape(R, N), rng)
    w_again = np.ascontiguousarray(w[::-1, ::-1])                          # another pattern, its first and last element kept too
    want = CR.select_batches([(pts, w, rgb), (pts, w_again, rgb)], 0.5)
    kept = len(want[1])
    assert kept == 2 * int(mask.sum()) and 2 * len(edges) < kept < n // 25
    got = Call(kept + 5).append(o, d, z, w, rgb, 0.5).append(o, d, z, w_again, rgb, 0.5).result()
    assert got[3] == kept
    _assert_records(got, want)


def test_point_cloud_object():
    """ops.PointCloud / ops.cloud_append: the same records through the tensor interface, the overflow error and truncate"""
    import torch

    from nerf_sampling_amd import ops

    batches = _batches([(S + 3, 3), (70, 64)], seed=5)
    want = CR.select_batches([(_points(o, d, z), w, rgb) for o, d, z, w, rgb in batches], 0.5)
    kept = len(want[1])
    dev = lambda a: torch.from_numpy(a).cuda()                                        # noqa: E731
    for colours in (True, False):
        cloud = ops.PointCloud(kept, colours=colours)
        assert cloud.count() == 0 and cloud.capacity == kept and cloud.count_dev.dtype == torch.int64
        for o, d, z, w, rgb in batches:
            shard = torch.zeros((len(rgb), 4), device="cuda")
            shard[:, :3] = dev(rgb)
            assert cloud.append(dev(o), dev(d), dev(z), dev(w), rgb=shard[:, :3] if colours else None, min_weight=0.5) is cloud
        assert cloud.count() == kept
        pts, w_, rgb_ = cloud.tensors()
        assert (_bits(pts.cpu().numpy()) == _bits(want[0])).all() and (_bits(w_.cpu().numpy()) == _bits(want[1])).all()
        assert (rgb_ is None) if not colours else (_bits(rgb_.cpu().numpy()) == _bits(want[2])).all()
    small = ops.PointCloud(kept - 3)
    for o, d, z, w, rgb in batches:
        ops.cloud_append(small, dev(o), dev(d), dev(z), dev(w), min_weight=0.5)
    assert small.count() == kept
    with pytest.raises(RuntimeError, match=str(kept)):
        small.tensors()
    pts, w_, rgb_ = small.tensors(truncate=True)
    assert pts.shape == (kept - 3, 3) and rgb_ is None and (_bits(pts.cpu().numpy()) == _bits(want[0])[:kept - 3]).all()
    counter = ops.PointCloud(0)
    o, d, z, w, rgb = batches[0]
    assert counter.append(dev(o), dev(d), dev(z), dev(w), min_weight=0.5).count() == len(CR.select(np.zeros(w.shape + (3,)), w, None, 0.5)[1])


def test_refusals_before_any_launch():
    """What the host knows is refused by the entry itself (NS_E_INVALID, which the loader's check turns into ValueError) and by
    the wrapper (ValueError); nothing is written."""
    import torch

    from nerf_sampling_amd import _lib, ops

    R, N = 65, 3
    (o, d, z, w, rgb), = _batches([(R, N)], seed=3)
    dev = lambda a: torch.from_numpy(a).cuda()                                        # noqa: E731
    o, d, z, w, rgb = dev(o), dev(d), dev(z), dev(w), dev(rgb)
    lib = _lib.load()
    cap = R * N
    outs = torch.full((3, cap * 3), -7.0, device="cuda")
    count = torch.zeros((1,), dtype=torch.int64, device="cuda")
    ws = torch.full((256 + 8,), POISON, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                          # noqa: E731

    def entry(o_p=p(o), d_p=p(d), z_p=p(z), zs=0, w_p=p(w), ws_=0, c_p=p(rgb), cs=0, R_=R, N_=N, pts_p=p(outs[0]),
              w_out_p=p(outs[1]), rgb_p=p(outs[2]), cap_=cap, count_p=p(count), ws_p=p(ws)):
        return lib.ns_cloud_append(o_p, d_p, z_p, zs, w_p, ws_, c_p, cs, R_, N_, 0.5, pts_p, w_out_p, rgb_p, cap_, count_p, ws_p,
                                   stream)

    for bad in (dict(o_p=None), dict(d_p=None), dict(z_p=None), dict(w_p=None), dict(count_p=None), dict(ws_p=None),
                dict(pts_p=None), dict(w_out_p=None), dict(c_p=None), dict(R_=-1), dict(N_=0), dict(N_=-2), dict(zs=N - 1),
                dict(zs=-N), dict(ws_=1), dict(ws_=-1), dict(cs=2), dict(cs=-3), dict(cap_=-1), dict(R_=2 ** 31, N_=1),
                dict(R_=2 ** 25, N_=64), dict(R_=2 ** 40, N_=3), dict(count_p=C.c_void_p(count.data_ptr() + 4)),
                dict(ws_p=C.c_void_p(ws.data_ptr() + 4))):
        rc = entry(**bad)
        assert rc == -1, bad
        assert b"ns_cloud_append" in lib.ns_last_error()
        with pytest.raises(ValueError, match="ns_cloud_append"):
            _lib.check(rc, "ns_cloud_append")
    cloud = ops.PointCloud(cap, colours=True)
    plain = ops.PointCloud(cap)
    wide = torch.zeros((R, N + 2), device="cuda")
    for bad in (dict(cloud=None), dict(o=o.double()), dict(o=o.cpu()), dict(o=o[:-1]), dict(d=d[:, :2]), dict(d=d.t()),
                dict(z=z.double()), dict(z=z.cpu()), dict(z=z[:-1]), dict(z=z[:, :2]), dict(z=wide[:, ::2][:, :N]),
                dict(z=z.reshape(R, N, 1)), dict(w=w.t()), dict(w=w[:, :0]), dict(w=w.as_strided((R, N), (N - 1, 1))),
                dict(rgb=None), dict(rgb=rgb.double()), dict(rgb=rgb[:-1]), dict(rgb=wide[:, ::2][:, :3]), dict(rgb=rgb.cpu()),
                dict(cloud=plain)):
        args = dict(cloud=cloud, o=o, d=d, z=z, w=w, rgb=rgb)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.cloud_append(**args)
    with pytest.raises(ValueError):
        ops.PointCloud(-1)
    torch.cuda.synchronize()
    assert (outs.cpu().numpy() == -7.0).all() and int(count.cpu()[0]) == 0 and (ws.cpu().numpy() == POISON).all()
    assert cloud.count() == 0 and plain.count() == 0
    assert entry() == 0 and entry(zs=N, ws_=N, cs=3) == 0                             # and the call they vary is a good one
    assert int(count.cpu()[0]) == 2 * int((w >= 0.5).sum())
